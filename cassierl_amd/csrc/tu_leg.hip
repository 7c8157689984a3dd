// tu_leg.hip -- translation unit of the two-lanes-per-environment PD / torque / record-command kernels (cassie_kernels_leg.hip).
#include "cassie_kernels_leg.hip"
#include "cassie_launch.h"

namespace cassie {
namespace launch {

template void step_leg_tier<false>(int, int, hipStream_t, const VecParams&, int*);

}  // namespace launch
}  // namespace cassie
