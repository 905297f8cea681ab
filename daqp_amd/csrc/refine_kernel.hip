// refine_kernel.hip -- translation unit of the refinement kernels (refine.hip.h, refine_nullspace.hip.h)
#include <hip/hip_runtime.h>
#include "refine.hip.h"
#include "refine_nullspace.hip.h"

namespace daqp_amd {
template __global__ void k_refine<64, true, true>(BatchDev, RefineArgs);       // n <= 64: one wavefront, everything in LDS
template __global__ void k_refine<256, false, true>(BatchDev, RefineArgs);     // beyond: R^-1 streamed, rows + Gram matrix in LDS
template __global__ void k_refine<256, false, false>(BatchDev, RefineArgs);    // ... or in the per-workgroup scratch
template __global__ void k_refine_nullspace<64>(BatchDev, RefineNullspaceArgs);  // no factor of H: the null-space method, one wavefront, n <= 64
}
