// backward_kernel.hip -- translation unit of the adjoint kernel (backward.hip.h)
#include <hip/hip_runtime.h>
#include "backward.hip.h"

namespace daqp_amd {
template __global__ void k_backward<64, true, true>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, true>(BatchDev, BackwardArgs);
template __global__ void k_backward<256, false, false>(BatchDev, BackwardArgs);
}
