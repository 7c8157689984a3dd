// cassie_tier_plan.h -- which kernel carries the first physics tier of a Cassie2d batch, and how a step is cut into segments: the policy of
// the C-ABI's host side as pure functions of sizes, flags and overrides.  No HIP here: the header compiles with a plain C++ compiler, and
// oracle/tier_plan_host.cpp (tests/test_tier_plan_host.py) checks it, and bench.py's mirror of it, on a machine without a GPU.
#ifndef CASSIE_TIER_PLAN_H_
#define CASSIE_TIER_PLAN_H_
#include "../../include/cassie_vec.h"
#include "cassie_vec_layout.h"

namespace cassie {
namespace plan {

constexpr int DUO_MIN_ENVS = 32768;  // 64 environments per wavefront: never below one full round of the pair form (plan_tiers weighs whole rounds above it)
constexpr int LEG_MIN_ENVS = 6144;   // measured crossover (r03, bench workload): 4096 envs 0.63 ms (g16 tier) vs 0.75 ms (leg tier), 8192 envs 0.83 vs 0.74 ms

// what the environment says (env_switch): -1 unset, 0 / 1 the switch
struct TierOverrides {
  int g16 = -1;   // CASSIE2D_G16=0 selects the wave-per-environment kernel only (A/B)
  int leg = -1;   // CASSIE2D_LEG=0/1 overrides the size rule of the two-lanes-per-environment kernel
  int duo = -1;   // CASSIE2D_DUO=0/1 overrides the size rule of its 64-environments-per-wavefront form
};

struct TierPlan {
  bool g16;       // the packed kernels at all
  bool leg;       // first tier = the two-lanes-per-environment kernel
  int duo_envs;   // environments [0, duo_envs) take its 64-environments-per-wavefront form, the rest the two-lanes kernel (0 or n unless the size rule splits the batch)
};

// simds: SIMDs of the chip (4 per compute unit); flags: CassieVecConfig::flags.  Per tier: the size rule, then the environment, then the flag bits.
inline TierPlan plan_tiers(int n_envs, int simds, int flags, const TierOverrides& env) {
  TierPlan t{true, false, 0};
  if (env.g16 == 0) t.g16 = false;
  if (flags & CASSIE_WAVE_PER_ENV) t.g16 = false;
  // Two lanes per environment = 32 environments per wavefront, one wavefront per SIMD: a launch of up to 32 768 environments takes
  // one wavefront's time (0.74 ms per Env.step of ten substeps).  Below LEG_MIN_ENVS the 4-environments-per-wavefront kernel (8x
  // more wavefronts, two per SIMD, 0.45-0.6 ms for a lone pair of wavefronts) is faster.
  t.leg = t.g16 && n_envs >= LEG_MIN_ENVS;
  if (env.leg >= 0) t.leg = t.g16 && env.leg == 1;
  if (flags & CASSIE_LEG_TIER_OFF) t.leg = false;
  if (flags & CASSIE_LEG_TIER_ON) t.leg = t.g16;
  // the joint-sweep form of that tier (64 environments per wavefront) where the batch fills the chip with it: one wavefront per SIMD is
  // 65 536 environments; below DUO_MIN_ENVS the 32-environment wavefronts of the pair form finish earlier (twice as many SIMDs busy).
  // both forms run one wavefront per SIMD, so a launch takes whole ROUNDS of the chip's SIMDs: per round the pair form's wavefront
  // (32 environments) lives ~0.62 ms, the joint form's (64 environments) ~1.0 ms (r06 sweep, MI355X: profiles/r06_size_sweep.jsonl).  Three
  // candidates: the pair form for everyone; the joint form for everyone; the joint form for the whole rounds of the batch and the pair form for the
  // remainder (r06).  32 768 envs: one round either way, the pair form's is shorter; 65 536: 1 x 1.0 against 2 x 0.62; 98 304: 1.0 + 0.62 against
  // 3 x 0.62 or 2 x 1.0; 131 072: 2 x 1.0.
  const double T_PAIR = 0.62, T_JOINT = 1.0;
  const int round_pair = 32 * simds, round_joint = 64 * simds;
  auto rounds = [](int n, int per) { return (n + per - 1) / per; };
  const double cost_pair = T_PAIR * rounds(n_envs, round_pair), cost_joint = T_JOINT * rounds(n_envs, round_joint);
  const int whole = n_envs / round_joint * round_joint, rest = n_envs - whole;
  const double cost_split = T_JOINT * (whole / round_joint) + T_PAIR * rounds(rest, round_pair);
  if (t.leg && n_envs > DUO_MIN_ENVS) {
    if (whole > 0 && rest > 0 && cost_split < cost_pair && cost_split < cost_joint) t.duo_envs = whole;
    else if (1.05 * cost_joint < cost_pair) t.duo_envs = n_envs;
  }
  if (env.duo >= 0) t.duo_envs = (t.leg && env.duo == 1) ? n_envs : 0;
  if (flags & CASSIE_DUO_TIER_OFF) t.duo_envs = 0;
  if (flags & CASSIE_DUO_TIER_ON) t.duo_envs = t.leg ? n_envs : 0;
  // that kernel addresses the batch arrays with 32-bit byte offsets (cassie_kernels_duo.hip: duo_io); a batch whose records exceed 4 GiB (6.1 M envs) stays in the pair form
  if ((unsigned long long)n_envs * ENV_STRIDE * sizeof(double) > 0xFFFFFFFFull) t.duo_envs = 0;
  return t;
}

constexpr int SEG2D_MAX = 4, SEG3D = 3;   // segments of a Cassie2d Env.step / a Cassie3d step while environments are handed down

// Cassie2d (launch_physics_tiers): a first segment of ONE substep, then up to max_seg - 1 more of near-equal length, the longer ones first.
// len[max_seg]; returns the number of segments.
inline int segment_lengths_2d(int n_sub, int max_seg, int* len) {
  int nseg = 0, left = n_sub - 1;
  len[nseg++] = 1;
  for (int parts = max_seg - 1; parts > 0; parts--) {
    const int l = (left + parts - 1) / parts;
    if (l > 0) { len[nseg++] = l; left -= l; }
  }
  return nseg;
}

// Cassie3d (launch3d): n_seg near-equal parts, the longer ones first (the caller asks for segments from 2 n_seg substeps on: none is empty).
inline int segment_lengths_3d(int n_sub, int n_seg, int* len) {
  int left = n_sub;
  for (int j = 0; j < n_seg; j++) { len[j] = (left + (n_seg - j) - 1) / (n_seg - j); left -= len[j]; }
  return n_seg;
}

}  // namespace plan
}  // namespace cassie
#endif
