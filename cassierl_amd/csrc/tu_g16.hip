// tu_g16.hip -- translation unit of the four-environments-per-wavefront PD / torque kernels (cassie_kernels_g16.hip).
#define CASSIE_TU_G16
#include "cassie_kernels.hip"
#include "cassie_kernels_g16.hip"
#include "cassie_launch.h"

namespace cassie {
namespace launch {

template void step_g16_tier<false>(int, int, hipStream_t, const VecParams&, int*);

void classify_pending(int n_envs, hipStream_t s, const VecParams& p, int* pending) {
  hipLaunchKernelGGL(g16::classify_pending_kernel, dim3((n_envs + 3) / 4), dim3(64), 0, s, p, pending);
}

}  // namespace launch
}  // namespace cassie
