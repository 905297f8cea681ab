// backward_kernel.hip -- translation unit of the adjoint kernels (backward.hip.h, nullspace.hip.h)
#include <hip/hip_runtime.h>
#include "backward.hip.h"
#include "nullspace.hip.h"

namespace daqp_amd {
template __global__ void k_backward<64, true, true, false>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, true, false>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, false, false>(BatchDev, BackwardArgs);
// batches created with ns_max > 0: soft rows in the (2,2) block, q_k and u_k emitted
template __global__ void k_backward<64, true, true, true>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, true, true>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, false, true>(BatchDev, BackwardArgs);
// a dual right-hand side (daqp_batch_backward_dual): g_lam on W in the second block
template __global__ void k_backward<64, true, true, false, true>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, true, false, true>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, false, false, true>(BatchDev, BackwardArgs);
// both (daqp_batch_backward_soft_dual): g_lam and the soft_slack term on W in the second block, -S in the (2,2) block
template __global__ void k_backward<64, true, true, true, true>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, true, true, true>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, false, true, true>(BatchDev, BackwardArgs);
// the null-space adjoint: the caller's H instead of the kept factor (singular H, LPs)
template __global__ void k_backward_nullspace<64>(BatchDev, NullspaceArgs);
template __global__ void k_backward_nullspace<64, true>(BatchDev, NullspaceArgs);
}
