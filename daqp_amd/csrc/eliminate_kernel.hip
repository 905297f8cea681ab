// eliminate_kernel.hip -- translation unit of the equality-elimination kernels (eliminate.hip.h) and of the two kernels around the
// adjoint of an eliminated batch (eliminate_adjoint.hip.h)
#include <hip/hip_runtime.h>
#include "eliminate.hip.h"
#include "eliminate_adjoint.hip.h"

namespace daqp_amd {
template __global__ void k_eliminate<1, 1>(ElimDev);      // n <= 64: one wavefront per problem
// 65 <= n <= 511: one workgroup per problem, 2 / 4 / 8 entries per lane
template __global__ void k_eliminate<2, 4>(ElimDev);
template __global__ void k_eliminate<4, 4>(ElimDev);
template __global__ void k_eliminate<8, 4>(ElimDev);
template __global__ void k_eliminate_update<1>(ElimDev);
template __global__ void k_eliminate_update<2>(ElimDev);
template __global__ void k_eliminate_update<4>(ElimDev);
template __global__ void k_eliminate_update<8>(ElimDev);
template __global__ void k_expand<1>(ElimDev, ExpandArgs);
template __global__ void k_expand<2>(ElimDev, ExpandArgs);
template __global__ void k_expand<4>(ElimDev, ExpandArgs);
template __global__ void k_expand<8>(ElimDev, ExpandArgs);
template __global__ void k_elim_basis<1>(ElimDev, double *);
template __global__ void k_elim_basis<2>(ElimDev, double *);
template __global__ void k_elim_basis<4>(ElimDev, double *);
template __global__ void k_elim_basis<8>(ElimDev, double *);
template __global__ void k_adjoint_reduce<1>(ElimDev, ElimAdjointArgs);
template __global__ void k_adjoint_reduce<2>(ElimDev, ElimAdjointArgs);
template __global__ void k_adjoint_reduce<4>(ElimDev, ElimAdjointArgs);
template __global__ void k_adjoint_reduce<8>(ElimDev, ElimAdjointArgs);
template __global__ void k_adjoint_expand<1>(ElimDev, ElimAdjointArgs);
template __global__ void k_adjoint_expand<2>(ElimDev, ElimAdjointArgs);
template __global__ void k_adjoint_expand<4>(ElimDev, ElimAdjointArgs);
template __global__ void k_adjoint_expand<8>(ElimDev, ElimAdjointArgs);
}
