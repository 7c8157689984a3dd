// tu_duo_hf.hip -- translation unit of the height-field instantiation of the 64-environments-per-wavefront kernels (cassie_kernels_duo.hip,
// env_step_duo_hf_kernel): its own unit, so that tu_duo.hip -- the headline kernel -- compiles to exactly what it was.
#define CASSIE_LEG_HF
#include "cassie_kernels_duo.hip"
#include "cassie_launch.h"

namespace cassie {
namespace launch {

template void step_duo_tier<true>(int, int, hipStream_t, const VecParams&, int*, double*, int, bool);

}  // namespace launch
}  // namespace cassie
