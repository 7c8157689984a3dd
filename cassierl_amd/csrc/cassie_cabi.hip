// cassie_cabi.hip -- host side of libcassie2d.so: the C-ABI of include/cassie2d.h (legacy, batch-of-one) and include/cassie_vec.h
// (batched Cassie2d) on top of the kernel launchers declared in cassie_launch.h (one translation unit per kernel family, tu_*.hip).
// The batched Cassie3d ABI is cassie3d_cabi.hip; what the two share is cassie_host.h, the tier policy is cassie_tier_plan.h.
// There is no CPU code path here: every entry point launches HIP kernels or fails.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/cassie2d.h"
#include "cassie2d_planar.h"
#include "cassie_host.h"
#include "cassie_launch.h"
#include "cassie_tier_plan.h"

// words of the phase-clock buffer: the 64-environments-per-wavefront kernel has 24 buckets (leg::DUO_PHASES), the other kernels use the first 16
constexpr int CASSIE_PHASE_WORDS = 24;
namespace cassie {
namespace launch {
// the physics launchers (cassie_launch.h): the tier's height-field instantiation when the parameters carry a terrain library
void step_k1(int mode, K1Variant variant, int n_envs, hipStream_t s, const VecParams& p, int split) {
  (p.hf.fields ? step_k1_tier<true> : step_k1_tier<false>)(mode, variant, n_envs, s, p, split);
}
void reset(int n_envs, hipStream_t s, const VecParams& p, const uint8_t* mask, const double* qpos, const double* qvel) {
  (p.hf.fields ? reset_tier<true> : reset_tier<false>)(n_envs, s, p, mask, qpos, qvel);
}
void step_g16(int mode, int n_envs, hipStream_t s, const VecParams& p, int* pending) {
  (p.hf.fields ? step_g16_tier<true> : step_g16_tier<false>)(mode, n_envs, s, p, pending);
}
void step_leg(int mode, int n_envs, hipStream_t s, const VecParams& p, int* pending) {
  (p.hf.fields ? step_leg_tier<true> : step_leg_tier<false>)(mode, n_envs, s, p, pending);
}
void step_duo(int mode, int n_envs, hipStream_t s, const VecParams& p, int* pending, double* workspace, int table_slots, bool flat_hint) {
  (p.hf.fields ? step_duo_tier<true> : step_duo_tier<false>)(mode, n_envs, s, p, pending, workspace, table_slots, flat_hint);
}
}  // namespace launch
}  // namespace cassie

using namespace cassie_host;
namespace L2 = cassie::launch;

static_assert(CASSIE_STATE_STRIDE == cassie::ENV_STRIDE, "public stride must match the kernel layout");
static_assert(sizeof(StateGeneral) == 208 && sizeof(StateOperationalSpace) == 144 && sizeof(ControllerOsc) == 56 &&
                  sizeof(ControllerPd) == 48 && sizeof(ControllerTorque) == 48 && sizeof(ControllerForce) == 48,
              "ABI struct sizes (RobotInterface.h:14-50)");

// Buffers first, events and streams last: the members are released in reverse order (cassie_host.h).
CASSIE_HOST_PRIVATE_BEGIN
struct CassieVec : Handle {
  static constexpr int NSEG = cassie::plan::SEG2D_MAX;
  CassieVecConfig cfg{};
  DeviceBuffer<double> state;
  DeviceBuffer<double> traj_qpos;
  double traj_tmax = 0.0;
  int traj_n = 0;
  // terrain library (N4): the fields' heights back to back, one descriptor per field, the field of every environment; hf_n == 0: the flat floor
  DeviceBuffer<double> hf_heights;
  DeviceBuffer<cassie::Terrain> hf_fields;
  int hf_n = 0;
  DeviceBuffer<int> hf_ids;                  // [n] device, in [0, hf_n) (allocated with the first library; CassieVecSetTerrainIds checks before it writes)
  DeviceBuffer<int> hf_bad;                  // device word of that check
  // scratch for the host-pointer conveniences
  DeviceBuffer<double> d_act, d_obs, d_rew, d_q, d_v, d_dbg;
  DeviceBuffer<double> ovf, ovf_dbg;         // workspace for constraint columns beyond the register-resident ones
  DeviceBuffer<int> pending;                 // substeps left per env after the 4-envs-per-wave kernel
  DeviceBuffer<int> pending_leg;             // substeps left per env after the two-lanes-per-env kernel (input of the 4-envs-per-wave kernel)
  bool leg = true;                           // first tier = the two-lanes-per-environment kernel (CASSIE2D_LEG=0/1 overrides the size rule)
  DeviceBuffer<uint8_t> duo_ws;              // workspace of the 64-environments-per-wavefront kernel (L2::duo_workspace_bytes)
  int duo_table = 0;                         // claim-table slots of its workspace (L2::duo_table_slots; 0: one slot per task).  CASSIE2D_DUO_TABLE=<slots> forces a table (tests)
  bool duo_flat_hint = false;                // CASSIE2D_DUO_FLAT_HINT=1 (tests): every wavefront's first probe is word 0
  size_t duo_ws_bytes = 0;
  int duo_envs = 0;                          // environments [0, duo_envs) take that form, the rest the two-lanes kernel (0 or n unless the size rule splits the batch)
  bool duo = false;                          // ... in its 64-environments-per-wavefront form (cassie_kernels_duo.hip; CASSIE2D_DUO=0/1 overrides the size rule)
  DeviceBuffer<unsigned long long> phase;    // profiling builds (-DCASSIE_PHASE_TIMING): CASSIE_PHASE_WORDS cycle accumulators
  DeviceBuffer<unsigned long long> stats;    // device event counters (cassie::STAT_*)
  bool g16 = true;                           // CASSIE2D_G16=0 selects the wave-per-environment kernel only (A/B)
  DeviceBuffer<uint8_t> d_done;
  MappedHost<int> deep_hint;                 // pinned host word the first tier writes (launch serial of the last deep hand-over), with its device address
  unsigned serial = 64;                      // launches of the physics tiers so far (starts past the hint window); wraps (compared modulo 2^32)
  int side_mode = -1;                        // CASSIE2D_SIDE_BY_SIDE=0/1 (tests): never / always run the lower tiers side by side; -1: by the hint
  // the Env.step in segments while robots are down (launch_physics_tiers): per segment the hand-over lists, two streams, three events
  int seg_mode = -1;                         // CASSIE2D_SEGMENTS=0/1 (A/B, tests): never / always in segments while robots are down; -1: by the count below
  MappedHost<unsigned> pend_hint;            // pinned host words [64]: estimated environments that left the first tier in launch serial & 63 (classify_pending_kernel)
  DeviceBuffer<unsigned> qp_stats;           // [3 n]: OSC QP iteration statistics (allocated by the first CassieVecQpIterations call: the controllers only count when someone reads)
  DeviceBuffer<unsigned> pend_count;         // device [130]: the launch's running sum and arrival ticket, per-serial sums and tags (classify_pending_kernel)
  unsigned pend_rate = 0;                    // hand-overs per launch, estimated from the last 48 launches' words
  bool reset_packed = true;                  // CASSIE2D_RESET_PACKED=0: CassieVecReset with one wavefront per environment only (A/B, tests)
  DeviceBuffer<uint8_t> need_slow;           // [n] written by the packed reset kernel: environments the wave-per-environment reset takes
  bool seg_ready = false, seg_failed = false;
  DeviceBuffer<int> seg_pend[NSEG];          // [n] substeps left per env after segment j of the two-lanes-per-env kernel
  DeviceBuffer<int> seg_pend2[NSEG];         // [n] ... after the 4-envs-per-wave kernel took segment j's environments
  DeviceBuffer<int> gone;                    // [n] the environment left the first tier in an earlier segment of this Env.step
  Event ev0, ev1, ev_fork, ev_join, seg_fork[NSEG], seg_join_a[NSEG], seg_join_b[NSEG];
  Stream side;                               // second stream: the two lower physics tiers run side by side behind the first
  Stream seg_deep[NSEG], seg_shal[NSEG];
};
CASSIE_HOST_PRIVATE_END

namespace {

int adim_of(int mode) { return mode == CASSIE_CTRL_OSC ? 7 : 6; }

constexpr unsigned SEG_MIN_HANDOVERS = 96;   // hand-overs per launch from which the Env.step runs in segments (launch_physics_tiers)
// doubles per env in the overflow workspace: the constraint columns beyond the register-resident ones (K1_MAXACT per row lane; K1_MAXACT_DBG in
// the debug build of the substep, which forces the overflow path in tests)
constexpr int OVF_STRIDE = (CP_NSLOT - L2::K1_MAXACT) * 64, OVF_STRIDE_DBG = (CP_NSLOT - L2::K1_MAXACT_DBG) * 64;

cassie::VecParams make_params(CassieVec* h) {
  cassie::VecParams p{};
  p.state = h->state.get(); p.n_envs = h->n;
  p.adim = adim_of(h->cfg.control_mode); p.n_sub = h->cfg.n_substeps; p.flags = h->cfg.flags; p.env_kind = h->cfg.env_kind; p.auto_reset = h->cfg.auto_reset;
  p.traj_qpos = h->traj_qpos.get(); p.traj_tmax = h->traj_tmax; p.traj_n = h->traj_n;
  p.ovf = h->ovf.get(); p.ovf_stride = OVF_STRIDE;
  p.stats = h->stats.get(); p.qp_stats = h->qp_stats.get(); p.phase = h->phase.get();
  p.hf.fields = h->hf_n ? h->hf_fields.get() : nullptr; p.hf.ids = h->hf_ids.get(); p.hf.n_fields = h->hf_n;
  return p;
}

// lists, streams and events of the segmented Env.step (first use; false: not available, the one-launch order is used)
bool seg_resources(CassieVec* h) {
  if (h->seg_ready) return true;
  if (h->seg_failed) return false;
  const size_t n = (size_t)h->n;
  bool ok = h->gone.alloc(n) == hipSuccess;
  for (int j = 0; j < CassieVec::NSEG && ok; j++)
    ok = h->seg_pend[j].alloc(n) == hipSuccess && h->seg_pend2[j].alloc(n) == hipSuccess &&
         h->seg_deep[j].create(hipStreamNonBlocking) == hipSuccess && h->seg_shal[j].create(hipStreamNonBlocking) == hipSuccess &&
         h->seg_fork[j].create(hipEventDisableTiming) == hipSuccess && h->seg_join_a[j].create(hipEventDisableTiming) == hipSuccess &&
         h->seg_join_b[j].create(hipEventDisableTiming) == hipSuccess;
  if (!ok) { h->seg_failed = true; (void)hipGetLastError(); return false; }
  h->seg_ready = true;
  return true;
}

// The first tier of a launch (flat floor or height field): the first `duo_envs` environments in the 64-environments-per-wavefront kernel, the rest in
// the two-lanes kernel (r06: a batch of whole rounds of the chip plus a remainder of at most one short round takes BOTH -- 65 537 .. 98 304 envs: 1.0 + 0.62 ms
// instead of three short rounds; the two kernels are bit-identical, so which environment runs where is invisible in the results).
void launch_first_tier(CassieVec* h, int mode, const cassie::VecParams& p) {
  const int nd = h->duo_envs;
  if (nd > 0) L2::step_duo(mode, nd, h->stream, p, h->pending_leg.get(), (double*)h->duo_ws.get(), h->duo_table, h->duo_flat_hint);
  if (nd < h->n) {
    cassie::VecParams q = p;
    if (nd > 0) {   // the remainder: every per-environment array moved on by nd environments
      const size_t o = (size_t)nd;
      q.n_envs = h->n - nd;
      q.state = p.state + o * cassie::ENV_STRIDE;
      if (p.actions) q.actions = p.actions + o * (size_t)p.adim;
      if (p.obs) q.obs = p.obs + o * 26;
      if (p.terminal_obs) q.terminal_obs = p.terminal_obs + o * 26;
      if (p.reward) q.reward = p.reward + o;
      if (p.done) q.done = p.done + o;
      if (p.hf.ids) q.hf.ids = p.hf.ids + o;
    }
    L2::step_leg(mode, h->n - nd, h->stream, q, h->pending_leg.get() + nd);
  }
}

// The tiers below the first, for the environments a first-tier launch left in `pend`: the deep ones (PENDING_DEEP, classify_pending) on stream
// `sd` in the wave-per-environment kernel, the others on stream `ss` in the 4-environments-per-wavefront kernel and the wave-per-environment
// pass behind it (what that passed on in `pend2`).  sd == ss: one after the other, the same kernels on the same data.
void launch_lower_tiers(CassieVec* h, int mode, const cassie::VecParams& p, hipStream_t sd, hipStream_t ss, int* pend, int* pend2) {
  cassie::VecParams pd = p, pa = p, pb = p;
  pd.pending = pend; pd.pending_pick = cassie::PICK_DEEP;
  L2::step_k1(mode, L2::K1_DEEP, h->n, sd, pd, L2::K1_HANDOVER_SPLIT);
  pa.pending = pend; pa.pending_pick = cassie::PICK_SHALLOW;
  L2::step_g16(mode, h->n, ss, pa, pend2);
  pb.pending = pend2; pb.pending_pick = cassie::PICK_ALL;
  L2::step_k1(mode, L2::K1_DEEP, h->n, ss, pb, L2::K1_HANDOVER_SPLIT);
}

// Physics tiers (mode 0 PD, 1 torque, 2 commands from the record).  Each tier leaves an environment it cannot
// hold untouched from that substep on and says how many substeps are left; the next tier finishes it (results are what that
// tier alone would give: an environment's arithmetic is a function of its own state in every kernel).
//   tier 1  two lanes per environment (<= 8 rows per leg)        cassie_kernels_leg.hip   [h->leg]
//   tier 2  four environments per wavefront (<= 16 rows)          cassie_kernels_g16.hip
//   tier 3  one wavefront per environment (any number of rows)    cassie_kernels.hip
// On the height field (p.hf.fields) always in the one-stream order at the end, without the hints (robots on terrain have not been profiled
// lying down): the launch serial is not advanced, the hand-over ring is neither read nor cleared.
void launch_physics_tiers(CassieVec* h, int mode, const cassie::VecParams& pin) {
  cassie::VecParams p = pin;
  const bool flat = !p.hf.fields;
  if (flat) {
    p.deep_hint = h->deep_hint.dev(); p.serial = (int)++h->serial;   // the kernels only store the word; the comparison below is unsigned
    p.pend_hint = h->pend_hint.dev(); p.pend_count = h->pend_count.get();
  }
  if (flat && h->pend_hint.get()) {
    // estimated hand-overs of the recent launches, one pinned word per launch (ring of 64, read without synchronisation: a stale value
    // changes the schedule, never a result).  The host runs many launches ahead of the device, so the words of the newest launches
    // are still empty: the statistic is the SUM over the last 48 launches (the ones executed by now carry it), compared with what
    // 48 launches of SEG_MIN_HANDOVERS / 3 would give -- i.e. it tolerates two thirds of the window not having run yet.
    unsigned sum = 0;
    volatile unsigned* hint = h->pend_hint.get();
    for (unsigned k = 1; k <= 48; k++) sum += hint[(h->serial - k) & 63];
    h->pend_rate = sum / 16;
    hint[h->serial & 63] = 0;   // this launch's word (last used 64 launches ago)
  }
  // A handed-down environment costs its remaining substeps end to end whatever the batch size (~0.09 ms per substep in the middle
  // tier, 0.13-0.18 ms in the last).  While robots are down the lower tiers therefore take their environments AT THE SAME TIME on
  // two streams: a small kernel tags the environments the middle tier could not hold either (PENDING_DEEP), those go straight to
  // the wave-per-environment kernel on the side stream, and the middle tier plus the pass behind it (what it passed on after all)
  // run on the caller's stream -- disjoint sets of environments.  r03 trace of fallen robots: 0.9 + 1.7 ms one after the other
  // before, max(1.7, 0.9 + <= 1.2) ms now.  The tagging kernel and the fork / join cost ~70 us per launch (r03_i: headline 1.43 ->
  // 1.50 ms when they were unconditional), so this order is only used while the wave-per-environment kernel has had work in one
  // of the last 32 launches (a word in pinned host memory it writes, read here without synchronisation: a stale value changes the
  // schedule, never a result -- in the one-stream order the middle tier looks at the deep environments first, finds them too
  // large at the same substep, and passes them on untouched).
  // (unsigned difference: wrap-safe; a launch counter that wrapped past a stale hint turns the order on for at most 32 launches)
  const bool side_by_side = flat && h->leg && (h->side_mode >= 0 ? h->side_mode == 1 : (h->deep_hint.get() && h->serial - (unsigned)*(volatile int*)h->deep_hint.get() <= 32u));
  // fork: the side stream waits for the first tier.  If the event cannot be recorded / waited for, fall back to the one-stream order
  // below (same results) rather than let the side stream's kernel run concurrently with the first tier on the same records.
  // in segments only while MANY robots are down: the three extra launches of the first tier cost ~3 % of a step, and a handful of
  // hand-overs is a short tail (r04, alternating A/B at 65 536 envs: all-fallen floor 15.5 -> 17.0 M with ~270 hand-overs per step;
  // stand_torque_random 22.4 -> 21.6 M when forced; by this rule 22.7 M / 16.9 M)
  // r06: only where the first tier is the two-lanes kernel.  The segments are launches of that kernel (step_leg_segment); since the 64-environments
  // kernel sweeps its eight-row groups with a lane per environment it is ahead of four segments of the pair sweep on both falling-robot workloads
  // (tools/ab_segments.py, 65 536 envs: stand_torque_random 25.9 M never / 22.7 M always / 22.4 M by the estimate; all-fallen floor 17.5 / 17.2 / 17.2)
  const bool segments = h->seg_mode >= 0 ? h->seg_mode == 1 : (!h->duo && h->pend_rate >= SEG_MIN_HANDOVERS);
  if (side_by_side && segments && !h->seg_failed && p.n_sub >= 4 && !p.debug && seg_resources(h)) {
    // ---- the Env.step in segments (r04).  A robot that is down costs its substeps end to end (~0.13 ms each) in the lower tiers,
    // and in the order below these only start when the first tier has finished ALL its substeps: 1.4 ms of first tier + up to
    // 1.3 ms of tail.  Here the first tier runs the step as a first segment of ONE substep and up to three more of equal length;
    // after each, the environments that left it in that segment go to the lower tiers on the segment's own two streams (deep ones
    // straight to the wave-per-environment kernel, the others to the 4-environments-per-wavefront kernel and the pass behind it)
    // and are finished there to the END of the Env.step, while the first tier goes on with the next segment for everyone else
    // (`gone`).  A robot that was already down starts its ten substeps 0.2 ms into the step instead of 1.4; one that goes down in
    // the last segment has at most three substeps left.  Results: every environment is stepped by the same kernels on the same
    // data as in the one-launch order (an environment's arithmetic is a function of its own state in every kernel).
    int len[CassieVec::NSEG], later = p.n_sub;
    const int nseg = cassie::plan::segment_lengths_2d(p.n_sub, CassieVec::NSEG, len);
    bool forked[CassieVec::NSEG] = {};
    for (int j = 0; j < nseg; j++) {
      later -= len[j];
      cassie::VecParams ps = p;
      ps.n_sub = len[j];
      if (j != nseg - 1) { ps.obs = nullptr; ps.terminal_obs = nullptr; }
      L2::step_leg_segment(mode, h->n, h->stream, ps, h->seg_pend[j].get(), h->gone.get(), j == 0, later);
      L2::classify_pending(h->n, h->stream, p, h->seg_pend[j].get());
      // the segment's hand-overs on its own two streams; if the fork cannot be set up (or one failed before), on the caller's stream,
      // one after the other: the same kernels on the same data, only without the overlap
      const hipStream_t sd = h->seg_deep[j].get(), ss = h->seg_shal[j].get();
      forked[j] = !h->seg_failed && fork(h->stream, h->seg_fork[j].get(), {sd, ss});
      if (!forked[j]) h->seg_failed = true;
      launch_lower_tiers(h, mode, p, forked[j] ? sd : h->stream, forked[j] ? ss : h->stream, h->seg_pend[j].get(), h->seg_pend2[j].get());
    }
    for (int j = 0; j < nseg; j++) {   // join: the caller's stream continues behind every segment's lower tiers
      if (!forked[j]) continue;
      const bool deep = join(h->stream, h->seg_join_a[j].get(), h->seg_deep[j].get()), shallow = join(h->stream, h->seg_join_b[j].get(), h->seg_shal[j].get());
      if (!deep || !shallow) h->seg_failed = true;
    }
    return;
  }
  if (side_by_side) {
    launch_first_tier(h, mode, p);
    L2::classify_pending(h->n, h->stream, p, h->pending_leg.get());
    // the deep environments on the side stream; no fork: everything on the caller's stream (the deep ones first, then the others)
    const bool forked = fork(h->stream, h->ev_fork.get(), {h->side.get()});
    launch_lower_tiers(h, mode, p, forked ? h->side.get() : h->stream, h->stream, h->pending_leg.get(), h->pending.get());
    if (forked) (void)join(h->stream, h->ev_join.get(), h->side.get());
    return;
  }
  cassie::VecParams p2 = p, p3 = p;
  if (h->leg) {
    launch_first_tier(h, mode, p);
    p2.pending = h->pending_leg.get(); p2.pending_pick = cassie::PICK_ALL;
  }
  L2::step_g16(mode, h->n, h->stream, p2, h->pending.get());
  p3.pending = h->pending.get(); p3.pending_pick = cassie::PICK_ALL;
  L2::step_k1(mode, L2::K1_DEEP, h->n, h->stream, p3);
}

// controller-in-the-loop modes; zpos/zvel != null selects the scripted standing controllers
int launch_ctrl_step(CassieVec* h, int mode, const cassie::VecParams& p, const double* zpos, const double* zvel) {
  const bool scripted = zpos != nullptr;
  if (mode != CASSIE_CTRL_OSC && mode != CASSIE_CTRL_JACOBIAN)
    return fail(h, CASSIE_EINVAL, "controller-in-the-loop stepping exists for OSC and Jacobian modes only");
  // On terrain (rllab/envs/terrain_random.py rewrites the one MJCF every Step* variant loads) the controllers are what they are on
  // the floor -- OSC_RBDL / StepJacobian work from the RBDL model and the foot SITES, they never see MuJoCo's contacts
  // (OSC_RBDL.cpp:41-71, Cassie2d.cpp:119-209) -- and only the mj_step behind them collides with the height field.
  const int ctrl = mode == CASSIE_CTRL_OSC ? 2 : 3;
  const bool packed = h->g16 && !p.debug;
  for (int sub = 0; sub < p.n_sub; sub++) {
    cassie::VecParams ps = p;
    ps.n_sub = 1;
    if (sub != p.n_sub - 1) { ps.obs = nullptr; ps.terminal_obs = nullptr; }
    if (packed) {
      // Per StepOsc / StepJacobian: the packed controller kernel writes the motor commands into the state record, the packed
      // physics kernel (mode 2: commands from the record) does the mj_step, and the wave-per-environment physics kernel finishes the
      // (rare) environments with more than 16 constraint rows.  Observation / reward / reset ride on the last substep.
      L2::ctrl_g16(ctrl, scripted, h->n, h->stream, ps, zpos, zvel);
      launch_physics_tiers(h, 2, ps);
    } else {
      // wave-per-environment kernels only (CASSIE_WAVE_PER_ENV cross-check, debug record): same split, one wavefront per environment
      ps.pending = nullptr;
      L2::ctrl_k4(ctrl, scripted, h->n, h->stream, ps, zpos, zvel);
      ps.debug = nullptr;
      L2::step_k1(2, L2::K1_DEEP, h->n, h->stream, ps);
    }
  }
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int launch_step(CassieVec* h, int mode, const cassie::VecParams& p) {
  if (mode == CASSIE_CTRL_OSC || mode == CASSIE_CTRL_JACOBIAN) return launch_ctrl_step(h, mode, p, nullptr, nullptr);
  if (mode != CASSIE_CTRL_PD && mode != CASSIE_CTRL_TORQUE) return fail(h, CASSIE_EINVAL, "unknown control mode %d", mode);
  if (p.hf.fields && p.debug) return fail(h, CASSIE_EINVAL, "the debug substep has no height-field variant");
  // test hook: same code with only K1_MAXACT_DBG register-resident columns, so that the workspace path is exercised
  if (p.debug) L2::step_k1(mode, L2::K1_DEBUG, h->n, h->stream, p);
  // fast path: 4 environments per wavefront; environments with more than 16 active constraint rows are finished
  // by the wave-per-environment kernel, which returns immediately for every other environment
  else if (h->g16) launch_physics_tiers(h, mode, p);
  else L2::step_k1(mode, L2::K1_DEEP, h->n, h->stream, p);
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

// reset_mode: 0 = Cassie2dEnv.reset pose, 1 = states from arrays, 2 = keep state (mj_forward only)
int launch_reset(CassieVec* h, const uint8_t* mask, const double* q, const double* v, double* obs, bool keep) {
  HIPCHK(h, hipSetDevice(h->device));
  cassie::VecParams p = make_params(h);
  p.obs = obs;
  if (keep) {
    // forward only: feed the current state back in as the "new" state
    L2::get_state(h->n, h->stream, h->state.get(), h->d_q.get(), h->d_v.get());
    q = h->d_q.get(); v = h->d_v.get();
  }
  if (h->g16 && h->reset_packed && h->need_slow && !p.hf.fields) {
    // two lanes per environment, 32 environments per wavefront (flat floor only); a state with more than 8 rows on a leg is left to the
    // wave-per-environment kernel through the mask the packed kernel writes
    L2::reset_leg(h->n, h->stream, p, mask, q, v, h->need_slow.get());
    L2::reset(h->n, h->stream, p, h->need_slow.get(), q, v);
  } else L2::reset(h->n, h->stream, p, mask, q, v);
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

// what the plan needs, and the switches that are not part of it (false: a HIP call failed).  The device allocations keep the order they have
// always had: where a buffer lands next to the others is the one thing on this side that the kernels' timing can see.
bool allocate(CassieVec* h, int simds) {
  const size_t n = (size_t)h->n;
  auto ok = [](hipError_t e) { return e == hipSuccess; };
  if (!(ok(h->state.alloc(n * cassie::ENV_STRIDE)) && ok(h->d_act.alloc(n * 7)) && ok(h->d_obs.alloc(n * 26)) && ok(h->d_rew.alloc(n)) &&
        ok(h->d_done.alloc(n)) && ok(h->d_q.alloc(n * 18)) && ok(h->d_v.alloc(n * 13)) && ok(h->ovf.alloc(n * OVF_STRIDE)) &&
        ok(h->pending.alloc(n, 0)) && ok(h->pending_leg.alloc(n, 0))))
    return false;
#ifdef CASSIE_PHASE_TIMING
  if (!ok(h->phase.alloc(CASSIE_PHASE_WORDS, 0))) return false;
#endif
  if (!ok(h->stats.alloc(cassie::STAT_N, 0))) return false;
  if (h->duo) {
    h->duo_table = L2::duo_table_slots(h->duo_envs, simds);
    { const char* e = getenv("CASSIE2D_DUO_TABLE"); if (e && atoi(e) >= 2) { int t = 2; while (t < atoi(e)) t *= 2; h->duo_table = t; } }   // tests: a small batch through the claim path
    h->duo_flat_hint = env_switch("CASSIE2D_DUO_FLAT_HINT") == 1;
    h->duo_ws_bytes = L2::duo_workspace_bytes(h->duo_envs, h->duo_table);
    if (!ok(h->duo_ws.alloc(h->duo_ws_bytes, 0))) return false;
  }
  h->side_mode = env_switch("CASSIE2D_SIDE_BY_SIDE");
  h->seg_mode = env_switch("CASSIE2D_SEGMENTS");
  h->reset_packed = env_switch("CASSIE2D_RESET_PACKED") != 0;
  // pend_count: every word 0xFFFFFFFF but the launch's running sum and arrival ticket
  return ok(h->ev0.create()) && ok(h->ev1.create()) && ok(h->side.create(hipStreamNonBlocking)) && ok(h->pend_hint.alloc(64)) &&
         ok(h->pend_count.alloc(130, 0xFF)) && ok(hipMemset(h->pend_count.get(), 0, 2 * sizeof(unsigned))) && ok(h->need_slow.alloc(n)) && ok(h->deep_hint.alloc(1)) &&
         ok(h->ev_fork.create(hipEventDisableTiming)) && ok(h->ev_join.create(hipEventDisableTiming));
}

}  // namespace

extern "C" {

int CassieVecCreate(CassieVec** out, int n_envs, int device, const CassieVecConfig* cfg) {
  if (!out || n_envs <= 0) return CASSIE_EINVAL;
  *out = nullptr;
  if (int rc = open_device(device)) return rc;
  CassieVec* h = new CassieVec();
  h->n = n_envs; h->device = device;
  if (cfg) h->cfg = *cfg;
  else { h->cfg.env_kind = CASSIE_ENV_WALK; h->cfg.control_mode = CASSIE_CTRL_PD; h->cfg.n_substeps = 10; h->cfg.flags = 0; h->cfg.auto_reset = 1; }
  if (h->cfg.n_substeps <= 0) h->cfg.n_substeps = 10;
  // the first tier (cassie_tier_plan.h) by the batch size, the chip's SIMDs, the environment and the flags
  int simds = 1024;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) simds = 4 * prop.multiProcessorCount;
  cassie::plan::TierOverrides env;
  env.g16 = env_switch("CASSIE2D_G16"); env.leg = env_switch("CASSIE2D_LEG"); env.duo = env_switch("CASSIE2D_DUO");
  const cassie::plan::TierPlan plan = cassie::plan::plan_tiers(n_envs, simds, h->cfg.flags, env);
  h->g16 = plan.g16; h->leg = plan.leg; h->duo_envs = plan.duo_envs; h->duo = plan.duo_envs > 0;
  bool ok = allocate(h, simds);
  if (ok) {
    // Cassie2d::Cassie2d: ctor pose, mj_forward, setState (Cassie2d.cpp:56-64)
    L2::init_state(n_envs, h->stream, h->state.get());
    ok = launch_reset(h, nullptr, nullptr, nullptr, nullptr, true) == CASSIE_OK && hipStreamSynchronize(h->stream) == hipSuccess;
  }
  if (!ok) {
    CassieVecFree(h);
    return CASSIE_EHIP;
  }
  *out = h;
  return CASSIE_OK;
}

void CassieVecFree(CassieVec* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  sync(h->side);
  for (int j = 0; j < CassieVec::NSEG; j++) { sync(h->seg_deep[j]); sync(h->seg_shal[j]); }
  delete h;
}

const char* CassieVecLastError(const CassieVec* h) { return h ? h->err.c_str() : "null handle"; }
int CassieVecNumEnvs(const CassieVec* h) { return h ? h->n : 0; }
int CassieVecActionDim(const CassieVec* h) { return h ? adim_of(h->cfg.control_mode) : 0; }
int CassieVecSetStream(CassieVec* h, void* s) {
  if (!h) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // work queued on the old stream must not race with launches on the new one
  h->stream = (hipStream_t)s;                  // NULL: back to the default stream
  return CASSIE_OK;
}

int CassieVecGetCounters(CassieVec* h, uint64_t* out4) {
  if (!h || !out4) return CASSIE_EINVAL;
  unsigned long long host[cassie::STAT_N];
  if (int rc = read_counters(h, h->stats.get(), host)) return rc;
  out4[0] = h->substeps_requested;
  out4[1] = host[cassie::STAT_CLEANUP_SUBSTEPS];
  out4[2] = host[cassie::STAT_K1_SUBSTEPS];
  out4[3] = host[cassie::STAT_NONFINITE];
  return CASSIE_OK;
}

int CassieVecQpIterations(CassieVec* h, double* out4) {
  if (!h || !out4) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->n;
  out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
  if (!h->qp_stats) {   // first call: start counting
    HIPCHK(h, h->qp_stats.alloc(3 * n));
    HIPCHK(h, hipMemsetAsync(h->qp_stats.get(), 0, 3 * n * sizeof(unsigned), h->stream));
    return CASSIE_OK;
  }
  std::vector<unsigned> host(3 * n);
  if (int rc = to_host(h, host.data(), h->qp_stats.get(), 3 * n)) return rc;
  HIPCHK(h, hipMemsetAsync(h->qp_stats.get(), 0, 3 * n * sizeof(unsigned), h->stream));
  if (int rc = synchronize(h)) return rc;
  double sum = 0.0, calls = 0.0, mx = 0.0, env_mean_max = 0.0;
  for (size_t e = 0; e < n; e++) {
    sum += host[e]; calls += host[2 * n + e];
    if (host[n + e] > mx) mx = host[n + e];
    if (host[2 * n + e]) { const double m = (double)host[e] / host[2 * n + e]; if (m > env_mean_max) env_mean_max = m; }
  }
  out4[0] = calls > 0 ? sum / calls : 0.0; out4[1] = mx; out4[2] = calls; out4[3] = env_mean_max;
  return CASSIE_OK;
}

int CassieVecTierInfo(CassieVec* h, uint64_t* out8) {
  if (!h || !out8) return CASSIE_EINVAL;
  unsigned long long host[cassie::STAT_N];
  if (int rc = read_counters(h, h->stats.get(), host)) return rc;
  out8[0] = !h->g16 ? 0 : !h->leg ? 1 : !h->duo ? 2 : 3;
  out8[1] = (uint64_t)h->duo_table;
  out8[2] = (uint64_t)h->duo_ws_bytes;
  out8[3] = host[cassie::STAT_WS_PROBES];
  out8[4] = h->pend_rate;
  out8[5] = (uint64_t)L2::duo_workspace_slots_per_wave();
  out8[6] = (uint64_t)h->duo_envs;
  out8[7] = 0;
  return CASSIE_OK;
}

#ifdef CASSIE_PHASE_TIMING
extern "C" int CassieVecPhaseMode() {  // what CassieVecPhaseCycles counts: 1 the whole Env.step, 2 the reset pass alone (a product build has neither function)
#ifdef CASSIE_PHASE_RESET_ONLY
  return 2;
#else
  return 1;
#endif
}
extern "C" int CassieVecPhaseCycles(CassieVec* h, unsigned long long* out24) {  // profiling builds only; not part of the public ABI
  if (!h || !h->phase) return CASSIE_EINVAL;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return CASSIE_EHIP;
  if (hipMemcpy(out24, h->phase.get(), CASSIE_PHASE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return CASSIE_EHIP;
  hipMemset(h->phase.get(), 0, CASSIE_PHASE_WORDS * sizeof(unsigned long long));
  return CASSIE_OK;
}
#endif

int CassieVecAccumulate(CassieVec* h, const double* reward_dev, const uint8_t* done_dev, double* returns_dev, unsigned long long* episodes_dev) {
  if (!h || (returns_dev && !reward_dev) || (episodes_dev && !done_dev)) return fail(h, CASSIE_EINVAL, "CassieVecAccumulate: an accumulator without its input");
  if (!returns_dev && !episodes_dev) return CASSIE_OK;
  HIPCHK(h, hipSetDevice(h->device));
  L2::accumulate_returns(h->n, h->stream, reward_dev, done_dev, returns_dev, episodes_dev);
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int CassieVecResetCounters(CassieVec* h) { return h ? reset_counters(h, h->stats.get(), cassie::STAT_N) : CASSIE_EINVAL; }
int CassieVecSynchronize(CassieVec* h) { return h ? synchronize(h) : CASSIE_EINVAL; }
void* CassieVecStatePtr(CassieVec* h) { return h ? h->state.get() : nullptr; }

int CassieVecSetTrajectory(CassieVec* h, const double* time_host, const double* qpos_host, int n) {
  if (!h || !time_host || !qpos_host || n <= 0) return fail(h, CASSIE_EINVAL, "bad trajectory");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // no launch in flight reads the table this call replaces
  HIPCHK(h, h->traj_qpos.alloc((size_t)n * 13));
  HIPCHK(h, hipMemcpy(h->traj_qpos.get(), qpos_host, (size_t)n * 13 * sizeof(double), hipMemcpyHostToDevice));
  h->traj_tmax = time_host[n - 1];  // cassie2d_trajectory.py:17
  h->traj_n = n;
  return CASSIE_OK;
}

int CassieVecSetTerrainLibrary(CassieVec* h, int n_fields, const int* nrow, const int* ncol, const double (*size_xy)[2], const double* heights_host) {
  if (!h) return CASSIE_EINVAL;
  if (n_fields < 0 || (n_fields > 0 && (!nrow || !ncol || !size_xy || !heights_host))) return fail(h, CASSIE_EINVAL, "bad terrain library");
  size_t total = 0;
  for (int k = 0; k < n_fields; k++) {
    if (nrow[k] < 2 || ncol[k] < 2 || !(size_xy[k][0] > 0) || !(size_xy[k][1] > 0)) return fail(h, CASSIE_EINVAL, "bad height field %d of the terrain library", k);
    total += (size_t)nrow[k] * ncol[k];
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // no launch in flight reads the library this call replaces
  h->hf_heights.reset(); h->hf_fields.reset(); h->hf_n = 0;
  if (n_fields == 0) return CASSIE_OK;   // back to the flat floor
  std::vector<cassie::Terrain> desc(n_fields);
  HIPCHK(h, h->hf_heights.alloc(total));
  HIPCHK(h, hipMemcpy(h->hf_heights.get(), heights_host, total * sizeof(double), hipMemcpyHostToDevice));
  size_t off = 0;
  for (int k = 0; k < n_fields; k++) {
    const size_t cnt = (size_t)nrow[k] * ncol[k];
    double hmax = heights_host[off];
    for (size_t i = 1; i < cnt; i++) hmax = heights_host[off + i] > hmax ? heights_host[off + i] : hmax;
    desc[k].h = h->hf_heights.get() + off; desc[k].nrow = nrow[k]; desc[k].ncol = ncol[k];
    desc[k].sx = size_xy[k][0]; desc[k].sy = size_xy[k][1]; desc[k].hmax = hmax;
    off += cnt;
  }
  HIPCHK(h, h->hf_fields.alloc(n_fields));
  HIPCHK(h, hipMemcpy(h->hf_fields.get(), desc.data(), n_fields * sizeof(cassie::Terrain), hipMemcpyHostToDevice));
  HIPCHK(h, h->hf_ids.ensure((size_t)h->n));
  HIPCHK(h, hipMemsetAsync(h->hf_ids.get(), 0, (size_t)h->n * sizeof(int), h->stream));   // every environment on field 0
  h->hf_n = n_fields;
  return CASSIE_OK;
}

int CassieVecSetHeightField(CassieVec* h, const double* heights_host, int nrow, int ncol, double size_x, double size_y) {
  if (!h) return CASSIE_EINVAL;
  const int rc = CassieVecSetTerrainLibrary(h, 0, nullptr, nullptr, nullptr, nullptr);   // the field goes first, whatever follows
  if (rc != CASSIE_OK || !heights_host) return rc;                                       // NULL: back to the flat floor
  if (nrow < 2 || ncol < 2 || !(size_x > 0) || !(size_y > 0)) return fail(h, CASSIE_EINVAL, "bad height field");
  const double size_xy[1][2] = {{size_x, size_y}};
  return CassieVecSetTerrainLibrary(h, 1, &nrow, &ncol, size_xy, heights_host);   // a library of one
}

int CassieVecSetTerrainIds(CassieVec* h, const uint8_t* mask_dev, const int* ids_dev) {
  if (!h || !ids_dev) return fail(h, CASSIE_EINVAL, "ids_dev is required");
  if (!h->hf_n) return fail(h, CASSIE_EINVAL, "no terrain library is set");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->hf_bad.ensure(1));
  int bad = 0;
  HIPCHK(h, hipMemsetAsync(h->hf_bad.get(), 0, sizeof(int), h->stream));
  L2::terrain_ids_check(h->n, h->stream, ids_dev, mask_dev, h->hf_n, h->hf_bad.get());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(&bad, h->hf_bad.get(), sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the one synchronisation of this call: the range check decides whether anything is written
  if (bad) return fail(h, CASSIE_EINVAL, "terrain id outside [0, %d): the assignment is unchanged", h->hf_n);
  L2::terrain_ids_set(h->n, h->stream, h->hf_ids.get(), ids_dev, mask_dev);
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int CassieVecGetTerrainIds(CassieVec* h, int* ids_dev) {
  if (!h || !ids_dev) return fail(h, CASSIE_EINVAL, "ids_dev is required");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->hf_n) HIPCHK(h, hipMemcpyAsync(ids_dev, h->hf_ids.get(), (size_t)h->n * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  else HIPCHK(h, hipMemsetAsync(ids_dev, 0, (size_t)h->n * sizeof(int), h->stream));   // the flat floor: every id reads 0
  return CASSIE_OK;
}

int CassieVecReset(CassieVec* h, const uint8_t* mask_dev, double* obs_dev) {
  return h ? launch_reset(h, mask_dev, nullptr, nullptr, obs_dev, false) : CASSIE_EINVAL;
}

int CassieVecResetTo(CassieVec* h, const uint8_t* mask_dev, const double* qpos_dev, const double* qvel_dev, double* obs_dev) {
  if (!h || !qpos_dev) return fail(h, CASSIE_EINVAL, "qpos_dev is required");
  return launch_reset(h, mask_dev, qpos_dev, qvel_dev, obs_dev, false);
}

int CassieVecStep(CassieVec* h, const double* actions_dev, double* obs_dev, double* reward_dev, uint8_t* done_dev, double* terminal_obs_dev) {
  if (!h || !actions_dev || !obs_dev || !reward_dev || !done_dev) return fail(h, CASSIE_EINVAL, "null argument");
  if (h->cfg.env_kind == CASSIE_ENV_WALK && !h->traj_qpos) return fail(h, CASSIE_EINVAL, "walk env needs CassieVecSetTrajectory first");
  HIPCHK(h, hipSetDevice(h->device));
  cassie::VecParams p = make_params(h);
  p.actions = actions_dev; p.obs = obs_dev; p.reward = reward_dev; p.done = done_dev; p.terminal_obs = terminal_obs_dev;
  h->substeps_requested += (unsigned long long)h->n * p.n_sub;
  return launch_step(h, h->cfg.control_mode, p);
}

int CassieVecSubstep(CassieVec* h, int control_mode, const double* actions_dev, int n_sub) {
  if (!h || !actions_dev || n_sub <= 0) return fail(h, CASSIE_EINVAL, "bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  cassie::VecParams p = make_params(h);
  p.actions = actions_dev; p.adim = adim_of(control_mode); p.n_sub = n_sub; p.obs = nullptr;
  h->substeps_requested += (unsigned long long)h->n * n_sub;
  return launch_step(h, control_mode, p);
}

int CassieVecStandingStep(CassieVec* h, int control_mode, const double* zpos_dev, const double* zvel_dev, int n_sub) {
  if (!h || !zpos_dev || !zvel_dev || n_sub <= 0) return fail(h, CASSIE_EINVAL, "bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  cassie::VecParams p = make_params(h);
  p.actions = nullptr; p.n_sub = n_sub; p.obs = nullptr;
  h->substeps_requested += (unsigned long long)h->n * n_sub;
  return launch_ctrl_step(h, control_mode, p, zpos_dev, zvel_dev);
}

int CassieVecGetState(CassieVec* h, double* qpos_dev, double* qvel_dev) {
  if (!h) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  L2::get_state(h->n, h->stream, h->state.get(), qpos_dev, qvel_dev);
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int CassieVecGetOpState(CassieVec* h, double* x18_dev) {
  if (!h || !x18_dev) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  cassie::VecParams p = make_params(h);
  L2::opstate(h->n, h->stream, p, x18_dev);
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int CassieVecStepHost(CassieVec* h, const double* a, double* obs, double* rew, uint8_t* done) {
  if (!h || !a) return CASSIE_EINVAL;
  const size_t n = h->n;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = to_device(h, h->d_act.get(), a, n * adim_of(h->cfg.control_mode))) return rc;
  if (int rc = CassieVecStep(h, h->d_act.get(), h->d_obs.get(), h->d_rew.get(), h->d_done.get(), nullptr)) return rc;
  if (int rc = to_host(h, obs, h->d_obs.get(), n * 26)) return rc;
  if (int rc = to_host(h, rew, h->d_rew.get(), n)) return rc;
  if (int rc = to_host(h, done, h->d_done.get(), n)) return rc;
  return synchronize(h);
}

int CassieVecGetStateHost(CassieVec* h, double* q, double* v) {
  if (!h) return CASSIE_EINVAL;
  if (int rc = CassieVecGetState(h, h->d_q.get(), h->d_v.get())) return rc;
  const size_t n = h->n;
  if (int rc = to_host(h, q, h->d_q.get(), n * 13)) return rc;
  if (int rc = to_host(h, v, h->d_v.get(), n * 13)) return rc;
  return synchronize(h);
}

int CassieVecSetStateHost(CassieVec* h, const double* s) {
  if (!h || !s) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = to_device(h, h->state.get(), s, (size_t)h->n * cassie::ENV_STRIDE)) return rc;
  return synchronize(h);
}

int CassieVecGetFullStateHost(CassieVec* h, double* s) {
  if (!h || !s) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = to_host(h, s, h->state.get(), (size_t)h->n * cassie::ENV_STRIDE)) return rc;
  return synchronize(h);
}

int CassieVecDebugWorkspaceHost(CassieVec* h, double* out_host, uint64_t max_doubles, uint64_t* n_doubles) {
  if (!h || !n_doubles) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  *n_doubles = h->duo_ws_bytes / sizeof(double);
  if (!out_host || !h->duo_ws) return CASSIE_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const uint64_t m = *n_doubles < max_doubles ? *n_doubles : max_doubles;
  HIPCHK(h, hipMemcpy(out_host, h->duo_ws.get(), m * sizeof(double), hipMemcpyDeviceToHost));
  return CASSIE_OK;
}

int CassieVecDebugSubstepHost(CassieVec* h, int control_mode, const double* a, double* dbg_host) {
  if (!h || !a || !dbg_host) return CASSIE_EINVAL;
  const size_t n = h->n;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->d_dbg.ensure(n * cassie::DBG_STRIDE));
  HIPCHK(h, h->ovf_dbg.ensure(n * OVF_STRIDE_DBG));
  HIPCHK(h, hipMemsetAsync(h->d_dbg.get(), 0, n * cassie::DBG_STRIDE * sizeof(double), h->stream));
  if (int rc = to_device(h, h->d_act.get(), a, n * adim_of(control_mode))) return rc;
  cassie::VecParams p = make_params(h);
  p.actions = h->d_act.get(); p.adim = adim_of(control_mode); p.n_sub = 1; p.obs = nullptr; p.debug = h->d_dbg.get();
  if (control_mode == CASSIE_CTRL_PD || control_mode == CASSIE_CTRL_TORQUE) { p.ovf = h->ovf_dbg.get(); p.ovf_stride = OVF_STRIDE_DBG; }
  if (int rc = launch_step(h, control_mode, p)) return rc;
  if (int rc = to_host(h, dbg_host, h->d_dbg.get(), n * cassie::DBG_STRIDE)) return rc;
  return synchronize(h);
}

int CassieVecTimeSteps(CassieVec* h, const double* actions_dev, int steps, double* obs_dev, double* reward_dev, uint8_t* done_dev, float* avg_ms) {
  if (!h || steps <= 0 || !avg_ms) return CASSIE_EINVAL;
  return timed_steps(h, h->ev0.get(), h->ev1.get(), steps, avg_ms, [&] { return CassieVecStep(h, actions_dev, obs_dev, reward_dev, done_dev, nullptr); });
}

// ------------------------------------------------------------------------------------------------ legacy ABI
struct Cassie2d {
  CassieVec* vec;
  bool display;
};

static void legacy_die(const char* what, CassieVec* v) {
  fprintf(stderr, "libcassie2d: %s: %s\n", what, v ? CassieVecLastError(v) : "");
  abort();  // the reference exits the process on init failure too (Cassie2d.cpp:49-52)
}

Cassie2d* Cassie2dInit(void) {
  CassieVecConfig cfg{};
  cfg.env_kind = CASSIE_ENV_STAND; cfg.control_mode = CASSIE_CTRL_PD; cfg.n_substeps = 1; cfg.flags = 0; cfg.auto_reset = 0;
  CassieVec* v = nullptr;
  int rc = CassieVecCreate(&v, 1, 0, &cfg);
  if (rc != CASSIE_OK) { fprintf(stderr, "libcassie2d: Cassie2dInit failed (%d): no usable MI355X/HIP device\n", rc); abort(); }
  Cassie2d* c = new Cassie2d();
  c->vec = v; c->display = false;
  return c;
}

void Reset(Cassie2d* c, StateGeneral* s) {
  double q[13], v[13];
  for (int i = 0; i < 3; i++) { q[i] = s->base_pos[i]; v[i] = s->base_vel[i]; }
  for (int i = 0; i < 5; i++) { q[3 + i] = s->left_pos[i]; v[3 + i] = s->left_vel[i]; q[8 + i] = s->right_pos[i]; v[8 + i] = s->right_vel[i]; }
  CassieVec* h = c->vec;
  if (hipMemcpy(h->d_q.get(), q, sizeof q, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(h->d_v.get(), v, sizeof v, hipMemcpyHostToDevice) != hipSuccess)
    legacy_die("Reset copy", h);
  if (launch_reset(h, nullptr, h->d_q.get(), h->d_v.get(), nullptr, false)) legacy_die("Reset", h);
  if (CassieVecSynchronize(h)) legacy_die("Reset sync", h);
}

static void legacy_step(Cassie2d* c, int mode, const double* a, int adim) {
  CassieVec* h = c->vec;
  if (hipMemcpy(h->d_act.get(), a, adim * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) legacy_die("Step copy", h);
  if (CassieVecSubstep(h, mode, h->d_act.get(), 1)) legacy_die("Step", h);
  if (CassieVecSynchronize(h)) legacy_die("Step sync", h);
}

void StepTorque(Cassie2d* c, ControllerTorque* a) { legacy_step(c, CASSIE_CTRL_TORQUE, a->torques, 6); }
void StepPd(Cassie2d* c, ControllerPd* a) { legacy_step(c, CASSIE_CTRL_PD, a->angles, 6); }
void StepOsc(Cassie2d* c, ControllerOsc* a) { legacy_step(c, CASSIE_CTRL_OSC, a->body_xdd, 7); }
void StepJacobian(Cassie2d* c, ControllerForce* a) { legacy_step(c, CASSIE_CTRL_JACOBIAN, a->left_force, 6); }

void GetGeneralState(Cassie2d* c, StateGeneral* s) {
  double q[13], v[13];
  if (CassieVecGetStateHost(c->vec, q, v)) legacy_die("GetGeneralState", c->vec);
  for (int i = 0; i < 3; i++) { s->base_pos[i] = q[i]; s->base_vel[i] = v[i]; }
  for (int i = 0; i < 5; i++) { s->left_pos[i] = q[3 + i]; s->left_vel[i] = v[3 + i]; s->right_pos[i] = q[8 + i]; s->right_vel[i] = v[8 + i]; }
}

void GetOperationalSpaceState(Cassie2d* c, StateOperationalSpace* s) {
  double x[18];
  CassieVec* h = c->vec;
  if (CassieVecGetOpState(h, h->d_q.get())) legacy_die("GetOperationalSpaceState", h);
  if (hipMemcpy(x, h->d_q.get(), sizeof x, hipMemcpyDeviceToHost) != hipSuccess) legacy_die("GetOperationalSpaceState copy", h);
  // only elements [0],[1] of each vector and body_x[2]/body_xd[2] are written (Cassie2d.cpp:225-235, quirk Q4)
  for (int i = 0; i < 2; i++) {
    s->body_x[i] = x[i]; s->body_xd[i] = x[3 + i];
    s->left_x[i] = x[6 + i]; s->left_xd[i] = x[9 + i];
    s->right_x[i] = x[12 + i]; s->right_xd[i] = x[15 + i];
  }
  s->body_x[2] = x[2]; s->body_xd[2] = x[5];
}

void Display(Cassie2d* c, bool display) { c->display = display; }
void Render(Cassie2d*) {}

}  // extern "C"
