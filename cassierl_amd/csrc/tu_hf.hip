// tu_hf.hip -- translation unit of the height-field instantiations: the PD / torque / record-command step kernels (the latter = the mj_step of StepOsc / StepJacobian) and the
// reset kernel with the terrain collision stage compiled in (each environment on its own field of the batch's terrain library), and the two small
// kernels that set the environments' field ids.  Separate from tu_base / tu_g16 so that the flat-floor
// kernels (the headline) are byte-for-byte what they were and everything builds in parallel.
#include "cassie_kernels.hip"
#include "cassie_kernels_g16.hip"
#define CASSIE_LEG_HF
#include "cassie_kernels_leg.hip"
#include "cassie_launch.h"

namespace cassie {
namespace launch {

template void step_k1_tier<true>(int, K1Variant, int, hipStream_t, const VecParams&, int);
template void step_g16_tier<true>(int, int, hipStream_t, const VecParams&, int*);
template void step_leg_tier<true>(int, int, hipStream_t, const VecParams&, int*);
template void reset_tier<true>(int, hipStream_t, const VecParams&, const uint8_t*, const double*, const double*);

// CassieVecSetTerrainIds: first every selected id is checked (bad[0] = 1 if one lies outside [0, n_fields)), then -- only if none
// does -- the selected ids are copied into the handle's array
__global__ void terrain_ids_check_kernel(const int* ids, const uint8_t* mask, int n, int n_fields, int* bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i]) && (unsigned)ids[i] >= (unsigned)n_fields) *bad = 1;
}
__global__ void terrain_ids_set_kernel(int* dst, const int* ids, const uint8_t* mask, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i])) dst[i] = ids[i];
}
void terrain_ids_check(int n, hipStream_t s, const int* ids, const uint8_t* mask, int n_fields, int* bad) {
  hipLaunchKernelGGL(terrain_ids_check_kernel, dim3((n + 255) / 256), dim3(256), 0, s, ids, mask, n, n_fields, bad);
}
void terrain_ids_set(int n, hipStream_t s, int* dst, const int* ids, const uint8_t* mask) {
  hipLaunchKernelGGL(terrain_ids_set_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, ids, mask, n);
}

}  // namespace launch
}  // namespace cassie
