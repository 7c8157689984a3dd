// tu_duo.hip -- translation unit of the 64-environments-per-wavefront PD / torque / record-command kernels (cassie_kernels_duo.hip).
#include "cassie_kernels_duo.hip"
#include "cassie_launch.h"

namespace cassie {
namespace launch {

// Workspace of a handle: [slots][W_N][64] doubles + the claim table (slots words, zero = free; zeroed once by the owner, every launch leaves
// it zero).  Up to DuoSlots::DIRECT_MAX tasks: one slot per task, no table.  Above: a table of a power of two >= 2 x simds slots.
int duo_table_slots(int n_envs, int simds) {
  const int tasks = ((n_envs + 63) / 64 + leg::DUO_WAVES - 1) / leg::DUO_WAVES * leg::DUO_WAVES;
  if (tasks <= leg::DuoSlots::DIRECT_MAX) return 0;
  int t = 64;
  while (t < 2 * simds) t *= 2;
  return t;
}
int duo_workspace_slots_per_wave() { return leg::DDuo::W_N; }
size_t duo_workspace_bytes(int n_envs, int table_slots) {
  const int tasks = ((n_envs + 63) / 64 + leg::DUO_WAVES - 1) / leg::DUO_WAVES * leg::DUO_WAVES;
  const size_t slots = table_slots ? (size_t)table_slots : (size_t)tasks;
  return slots * leg::duo_workspace_doubles_per_wave * sizeof(double) + (size_t)table_slots * sizeof(unsigned);
}
template void step_duo_tier<false>(int, int, hipStream_t, const VecParams&, int*, double*, int, bool);

}  // namespace launch
}  // namespace cassie
