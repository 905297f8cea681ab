// certify_kernel.hip -- translation unit of the certificate kernels (certify.hip.h)
#include <hip/hip_runtime.h>
#include "certify.hip.h"

namespace daqp_amd {
template __global__ void k_certify_wave<kCertWaves>(CertifyArgs);      // n <= 64: one wavefront per problem
// 65 <= n <= 511: one workgroup per problem, 2 / 4 / 8 columns per lane
template __global__ void k_certify_wg<2>(CertifyArgs);
template __global__ void k_certify_wg<4>(CertifyArgs);
template __global__ void k_certify_wg<8>(CertifyArgs);
}
