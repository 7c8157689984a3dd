// cassie3d_cabi.hip -- host side of the batched Cassie3d physics in libcassie2d.so: the C-ABI of include/cassie3d_vec.h on top of the
// launchers of tu_3d.hip (cassie_launch.h).  No kernel and no CPU code path here: every entry point launches HIP kernels or fails.
#include "../../include/cassie3d_vec.h"
#include "cassie3d_tables.h"
#include "cassie_host.h"
#include "cassie_launch.h"
#include "cassie_tier_plan.h"

using namespace cassie_host;
namespace L3 = cassie3d::launch;

static_assert(CASSIE3D_STATE_STRIDE == cassie3d::ENV3_STRIDE && CASSIE3D_NQ == cassie3d::NQ && CASSIE3D_NV == cassie3d::NV &&
                  CASSIE3D_NU == cassie3d::NU && CASSIE3D_DEBUG_STRIDE == cassie3d::D3_STRIDE && CASSIE3D_OFF_QVEL == cassie3d::E3_V &&
                  CASSIE3D_OFF_WARMSTART == cassie3d::E3_WS && CASSIE3D_OFF_CTRL == cassie3d::E3_CTRL && CASSIE3D_OFF_TIME == cassie3d::E3_TIME &&
                  CASSIE3D_OFF_OVERFLOW == cassie3d::E3_OVF,
              "public Cassie3d layout must match the kernel layout");
static_assert(CASSIE3D_NOBS == 45 && cassie3d::ENVC_N == 2, "public Cassie3d environment layout must match cassie3d_env.h");

CASSIE_HOST_PRIVATE_BEGIN
struct Cassie3dVec : Handle {   // kernels run on `stream`; `own_stream` is the one this handle created
  static constexpr int NSEG = cassie::plan::SEG3D;
  DeviceBuffer<double> state, d_act, d_dbg;
  DeviceBuffer<int> pending;
  DeviceBuffer<int> pending_leg;   // substeps left per env after the lane-per-leg kernel
  bool leg = true;    // first tier = the lane-per-leg kernel (cassie3d_leg.hip), 32 environments per wavefront; CASSIE3D_LEG=0: the r03 tiers only
  bool leg_full = false;   // CASSIE3D_LEG=64: 32 environments per wavefront instead of 16 (A/B)
  bool pair = false;  // CASSIE3D_PAIR=1: first pass with TWO environments per wavefront (cassie3d_pair.hip; parity-green, measured slower: kept as cross-check)
  DeviceBuffer<unsigned long long> stats;
  // the step in segments (launch3d): per segment the hand-over lists, a side stream and two events
  bool seg_on = true;                        // CASSIE3D_SEGMENTS=0: the whole step in one launch of the lane-per-leg kernel (A/B, tests)
  DeviceBuffer<int> seg_pend[NSEG], seg_pend2[NSEG], gone;
  Event ev0, ev1, seg_fork[NSEG], seg_join[NSEG];
  Stream seg_side[NSEG], own_stream;
  // the environment layer (Cassie3dVecEnv*): configuration, the PD gains kp[10] kd[10] on the device, the record a reset leaves, the
  // counters of the finish kernel and the buffers of the *Host conveniences
  Cassie3dEnvConfig env_cfg{};
  bool env_configured = false, env_stepped = false;
  DeviceBuffer<double> gains, reset_rec, d_obs, d_rew, d_tobs;
  DeviceBuffer<uint8_t> d_done;
  DeviceBuffer<unsigned long long> env_counters;
};
CASSIE_HOST_PRIVATE_END

namespace {
// fast kernel (<= 32 rows, 2 waves per SIMD) for everyone, then the general kernel for the environments it left pending
void launch3d(Cassie3dVec* h, cassie3d::Params3 p, const double* pd = nullptr) {   // pd: the PD gains table (PD mode: p.actions are targets)
  p.stats = h->stats.get();
  if (p.debug) {
    L3::step3d(1, h->n, h->stream, p, pd);
    return;
  }
  // tiers: one lane per leg (rows in per-lane LDS slots: 3 connect rows + 25 slots per limit + 81 per contact) -> one wavefront
  // per environment with at most 32 rows -> the general kernel (64 rows, capped); each leaves an environment it cannot hold
  // untouched from that substep on and says how many substeps are left
  p.gone = nullptr; p.seg_first = 1; p.seg_later = 0;
  if (h->leg && h->seg_on && h->gone && p.n_sub >= 2 * Cassie3dVec::NSEG) {
    // ---- the step in segments (r04): the lane-per-leg kernel runs the substeps in three launches; after each, the environments that
    // left its row capacity in that segment are finished -- to the END of the step -- by the wavefront-per-environment kernels on the
    // segment's own stream, while the lane-per-leg kernel goes on with the next segment for everyone else.  A hand-over costs ~0.25 ms
    // per substep in the lower tiers against ~0.5 ms per substep of the first tier's own chain, so all but the last segment's
    // hand-overs are off the step's critical path (16 384 envs: 0.26 ms of tail per step -> 0.0x).
    int len[Cassie3dVec::NSEG], later = p.n_sub;
    const int nseg = cassie::plan::segment_lengths_3d(p.n_sub, Cassie3dVec::NSEG, len);
    bool forked[Cassie3dVec::NSEG] = {};
    for (int j = 0; j < nseg; j++) {
      later -= len[j];
      cassie3d::Params3 ps = p;
      ps.n_sub = len[j]; ps.pending_in = nullptr; ps.pending_out = h->seg_pend[j].get();
      ps.gone = h->gone.get(); ps.seg_first = j == 0; ps.seg_later = later;
      L3::step3d(h->leg_full ? 4 : 3, h->n, h->stream, ps, pd);
      // the segment's hand-overs on its own stream; if the fork cannot be set up (or one failed before), on the caller's stream
      // behind the segment: the same kernels on the same data, only without the overlap
      forked[j] = h->seg_on && fork(h->stream, h->seg_fork[j].get(), {h->seg_side[j].get()});
      if (!forked[j]) h->seg_on = false;   // (this step is finished in segments, in order; the next ones in one launch)
      hipStream_t ss = forked[j] ? h->seg_side[j].get() : h->stream;
      cassie3d::Params3 pa = p, pb = p;
      pa.pending_in = h->seg_pend[j].get(); pa.pending_out = h->seg_pend2[j].get();
      L3::step3d(0, h->n, ss, pa, pd);
      pb.pending_in = h->seg_pend2[j].get(); pb.pending_out = nullptr;
      L3::step3d(1, h->n, ss, pb, pd);
    }
    for (int j = 0; j < nseg; j++)
      if (forked[j] && !join(h->stream, h->seg_join[j].get(), h->seg_side[j].get())) h->seg_on = false;
    return;
  }
  const int* in = nullptr;
  if (h->leg) {
    p.pending_in = nullptr; p.pending_out = h->pending_leg.get();
    L3::step3d(h->leg_full ? 4 : 3, h->n, h->stream, p, pd);
    in = h->pending_leg.get();
  }
  p.pending_in = in; p.pending_out = h->pending.get();
  L3::step3d(h->pair ? 2 : 0, h->n, h->stream, p, pd);
  p.pending_in = h->pending.get(); p.pending_out = nullptr;
  L3::step3d(1, h->n, h->stream, p, pd);
}

cassie3d::Params3 make_params3(Cassie3dVec* h, const double* actions, double* debug, int n_sub, int integrate) {
  cassie3d::Params3 p{};
  p.state = h->state.get(); p.actions = actions; p.debug = debug; p.n_envs = h->n; p.n_sub = n_sub; p.integrate = integrate;
  return p;
}

// kp[10] kd[10] of the handle's configuration to the device table the PD kernels read (synchronises: the source is host memory of the call)
int upload_gains(Cassie3dVec* h) {
  double g[2 * cassie3d::NU];
  for (int a = 0; a < cassie3d::NU; a++) { g[a] = h->env_cfg.kp[a]; g[cassie3d::NU + a] = h->env_cfg.kd[a]; }
  if (int rc = to_device(h, h->gains.get(), g, 2 * cassie3d::NU)) return rc;
  return synchronize(h);
}

// the PD kernels exist for the lane-per-leg tier and the two wavefront-per-environment tiers; the opt-in two-environments-per-wavefront
// cross-check kernel (CASSIE3D_PAIR=1) has none
int pd_available(Cassie3dVec* h) {
  return h->pair ? fail(h, CASSIE_EINVAL, "PD mode is not available on a handle created under CASSIE3D_PAIR=1") : CASSIE_OK;
}

bool allocate3d(Cassie3dVec* h) {
  const size_t n = (size_t)h->n;
  bool ok = h->own_stream.create() == hipSuccess && h->ev0.create() == hipSuccess && h->ev1.create() == hipSuccess &&
            h->state.alloc(n * cassie3d::ENV3_STRIDE) == hipSuccess && h->d_act.alloc(n * cassie3d::NU) == hipSuccess &&
            h->pending.alloc(n) == hipSuccess && h->pending_leg.alloc(n) == hipSuccess && h->stats.alloc(cassie3d::S3_N, 0) == hipSuccess;
  ok = ok && h->gains.alloc(2 * cassie3d::NU) == hipSuccess && h->reset_rec.alloc(cassie3d::ENV3_STRIDE) == hipSuccess &&
       h->env_counters.alloc(cassie3d::ENVC_N, 0) == hipSuccess;
  if (!ok) return false;
  h->stream = h->own_stream.get();
  if (h->leg && h->seg_on) {   // lists, streams and events of the segmented step (not available: one launch, same results)
    ok = h->gone.alloc(n) == hipSuccess;
    for (int j = 0; j < Cassie3dVec::NSEG && ok; j++)
      ok = h->seg_pend[j].alloc(n) == hipSuccess && h->seg_pend2[j].alloc(n) == hipSuccess && h->seg_side[j].create(hipStreamNonBlocking) == hipSuccess &&
           h->seg_fork[j].create(hipEventDisableTiming) == hipSuccess && h->seg_join[j].create(hipEventDisableTiming) == hipSuccess;
    if (!ok) { h->seg_on = false; (void)hipGetLastError(); }
  }
  return true;
}
}  // namespace

extern "C" {

int Cassie3dVecCreate(Cassie3dVec** out, int n_envs, int device) {
  if (!out || n_envs <= 0) return CASSIE_EINVAL;
  *out = nullptr;
  if (int rc = open_device(device)) return rc;
  Cassie3dVec* h = new Cassie3dVec();
  h->n = n_envs; h->device = device;
  h->leg = env_switch("CASSIE3D_LEG") != 0;
  { const char* e = getenv("CASSIE3D_LEG"); h->leg_full = e && e[0] == '6'; }
  if (env_switch("CASSIE3D_PAIR") == 1) { h->pair = true; h->leg = false; }   // the opt-in cross-check kernel is a FIRST tier (it takes no pending list)
  h->seg_on = env_switch("CASSIE3D_SEGMENTS") != 0;
  // the reset record of the environment layer: what the reset above leaves in environment 0; default gains kp = 10, kd = 5
  for (int a = 0; a < cassie3d::NU; a++) { h->env_cfg.kp[a] = 10.0; h->env_cfg.kd[a] = 5.0; }
  h->env_cfg.control_mode = CASSIE3D_CTRL_PD; h->env_cfg.n_substeps = 10; h->env_cfg.auto_reset = 1;
  if (!allocate3d(h) || Cassie3dVecReset(h, nullptr, nullptr) != CASSIE_OK ||
      hipMemcpyAsync(h->reset_rec.get(), h->state.get(), cassie3d::ENV3_STRIDE * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess ||
      upload_gains(h) != CASSIE_OK || hipStreamSynchronize(h->stream) != hipSuccess) {
    Cassie3dVecFree(h);
    return CASSIE_EHIP;
  }
  *out = h;
  return CASSIE_OK;
}

void Cassie3dVecFree(Cassie3dVec* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  sync(h->own_stream);
  for (const Stream& s : h->seg_side) sync(s);
  delete h;
}

const char* Cassie3dVecLastError(const Cassie3dVec* h) { return h ? h->err.c_str() : "null handle"; }

int Cassie3dVecSetStream(Cassie3dVec* h, void* s) {
  if (!h) return CASSIE_EINVAL;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->stream = s ? (hipStream_t)s : h->own_stream.get();  // NULL: back to the handle's own stream
  return CASSIE_OK;
}

int Cassie3dVecSynchronize(Cassie3dVec* h) { return h ? synchronize(h) : CASSIE_EINVAL; }

int Cassie3dVecReset(Cassie3dVec* h, const double* qpos_dev, const double* qvel_dev) {
  if (!h) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  L3::init3d(h->n, h->stream, h->state.get(), qpos_dev, qvel_dev);
  launch3d(h, make_params3(h, nullptr, nullptr, 1, 0));  // mj_forward
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int Cassie3dVecStep(Cassie3dVec* h, const double* torques_dev, int n_sub) {
  if (!h || !torques_dev || n_sub <= 0) return fail(h, CASSIE_EINVAL, "bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  h->substeps_requested += (unsigned long long)h->n * n_sub;
  launch3d(h, make_params3(h, torques_dev, nullptr, n_sub, 1));
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

double* Cassie3dVecStatePtr(Cassie3dVec* h) { return h ? h->state.get() : nullptr; }

int Cassie3dVecGetCounters(Cassie3dVec* h, uint64_t* out4) {
  if (!h || !out4) return CASSIE_EINVAL;
  unsigned long long host[cassie3d::S3_N];
  if (int rc = read_counters(h, h->stats.get(), host)) return rc;
  out4[0] = h->substeps_requested;
  out4[1] = host[cassie3d::S3_GENERAL_SUBSTEPS];
  out4[2] = host[cassie3d::S3_CAPPED_SUBSTEPS];
  out4[3] = host[cassie3d::S3_LEG_HANDOVER_SUBSTEPS];
  return CASSIE_OK;
}

int Cassie3dVecResetCounters(Cassie3dVec* h) { return h ? reset_counters(h, h->stats.get(), cassie3d::S3_N) : CASSIE_EINVAL; }

int Cassie3dVecStepHost(Cassie3dVec* h, const double* torques, int n_sub) {
  if (!h || !torques) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = to_device(h, h->d_act.get(), torques, (size_t)h->n * cassie3d::NU)) return rc;
  if (int rc = Cassie3dVecStep(h, h->d_act.get(), n_sub)) return rc;
  return synchronize(h);
}

int Cassie3dVecGetStateHost(Cassie3dVec* h, double* state) {
  if (!h || !state) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = to_host(h, state, h->state.get(), (size_t)h->n * cassie3d::ENV3_STRIDE)) return rc;
  return synchronize(h);
}

int Cassie3dVecSetStateHost(Cassie3dVec* h, const double* state) {
  if (!h || !state) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = to_device(h, h->state.get(), state, (size_t)h->n * cassie3d::ENV3_STRIDE)) return rc;
  return synchronize(h);
}

int Cassie3dVecDebugForwardHost(Cassie3dVec* h, const double* torques, double* dbg) {
  if (!h || !torques || !dbg) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nd = (size_t)h->n * cassie3d::D3_STRIDE;
  HIPCHK(h, h->d_dbg.ensure(nd));
  HIPCHK(h, hipMemsetAsync(h->d_dbg.get(), 0, nd * sizeof(double), h->stream));
  if (int rc = to_device(h, h->d_act.get(), torques, (size_t)h->n * cassie3d::NU)) return rc;
  launch3d(h, make_params3(h, h->d_act.get(), h->d_dbg.get(), 1, 0));
  HIPCHK(h, hipGetLastError());
  if (int rc = to_host(h, dbg, h->d_dbg.get(), nd)) return rc;
  return synchronize(h);
}

// ---------------------------------------------------------------- the environment layer
int Cassie3dVecEnvConfigure(Cassie3dVec* h, const Cassie3dEnvConfig* cfg) {
  if (!h || !cfg) return fail(h, CASSIE_EINVAL, "bad argument");
  if (h->env_stepped) return fail(h, CASSIE_EINVAL, "Cassie3dVecEnvConfigure comes before the first Cassie3dVecEnvStep");
  if (cfg->control_mode != CASSIE3D_CTRL_TORQUE && cfg->control_mode != CASSIE3D_CTRL_PD) return fail(h, CASSIE_EINVAL, "control_mode %d: CASSIE3D_CTRL_TORQUE or CASSIE3D_CTRL_PD", cfg->control_mode);
  if (cfg->n_substeps < 1 || cfg->n_substeps > 10000) return fail(h, CASSIE_EINVAL, "n_substeps %d: 1 .. 10000", cfg->n_substeps);
  if (cfg->auto_reset != 0 && cfg->auto_reset != 1) return fail(h, CASSIE_EINVAL, "auto_reset %d: 0 or 1", cfg->auto_reset);
  for (int a = 0; a < cassie3d::NU; a++)
    if (!(cfg->kp[a] >= 0.0 && cfg->kp[a] <= 1e10) || !(cfg->kd[a] >= 0.0 && cfg->kd[a] <= 1e10)) return fail(h, CASSIE_EINVAL, "gains of actuator %d: finite and not negative", a);
  if (cfg->control_mode == CASSIE3D_CTRL_PD)
    if (int rc = pd_available(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  h->env_cfg = *cfg;
  if (int rc = upload_gains(h)) return rc;
  h->env_configured = true;
  return CASSIE_OK;
}

int Cassie3dVecSubstepPd(Cassie3dVec* h, const double* targets_dev, int n_sub) {
  if (!h || !targets_dev || n_sub <= 0) return fail(h, CASSIE_EINVAL, "bad argument");
  if (int rc = pd_available(h)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  h->substeps_requested += (unsigned long long)h->n * n_sub;
  cassie3d::Params3 p = make_params3(h, targets_dev, nullptr, n_sub, 1);
  launch3d(h, p, h->gains.get());
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int Cassie3dVecEnvReset(Cassie3dVec* h, const uint8_t* mask_dev, double* obs_dev) {
  if (!h) return CASSIE_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  L3::env_reset3d(h->n, h->stream, h->state.get(), mask_dev, h->reset_rec.get(), obs_dev);
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int Cassie3dVecEnvStep(Cassie3dVec* h, const double* actions_dev, double* obs_dev, double* reward_dev, uint8_t* done_dev, double* terminal_obs_dev) {
  if (!h || !actions_dev || !obs_dev || !reward_dev || !done_dev) return fail(h, CASSIE_EINVAL, "bad argument");
  if (!h->env_configured) return fail(h, CASSIE_EINVAL, "Cassie3dVecEnvStep before Cassie3dVecEnvConfigure");
  const Cassie3dEnvConfig& c = h->env_cfg;
  if (int rc = c.control_mode == CASSIE3D_CTRL_PD ? Cassie3dVecSubstepPd(h, actions_dev, c.n_substeps) : Cassie3dVecStep(h, actions_dev, c.n_substeps)) return rc;
  h->env_stepped = true;
  cassie3d::EnvFinish3 f{};   // (launch3d has joined its side streams: the finish kernel sees every tier's records)
  f.state = h->state.get(); f.actions = actions_dev; f.reset_rec = h->reset_rec.get(); f.obs = obs_dev; f.reward = reward_dev;
  f.done = done_dev; f.terminal_obs = terminal_obs_dev; f.counters = h->env_counters.get(); f.n_envs = h->n; f.auto_reset = c.auto_reset;
  L3::env_finish3d(h->stream, f);
  HIPCHK(h, hipGetLastError());
  return CASSIE_OK;
}

int Cassie3dVecEnvStepHost(Cassie3dVec* h, const double* actions, double* obs, double* reward, uint8_t* done, double* terminal_obs) {
  if (!h || !actions) return fail(h, CASSIE_EINVAL, "bad argument");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->n;
  HIPCHK(h, h->d_obs.ensure(n * CASSIE3D_NOBS));
  HIPCHK(h, h->d_tobs.ensure(n * CASSIE3D_NOBS));
  HIPCHK(h, h->d_rew.ensure(n));
  HIPCHK(h, h->d_done.ensure(n));
  if (int rc = to_device(h, h->d_act.get(), actions, n * cassie3d::NU)) return rc;
  if (int rc = Cassie3dVecEnvStep(h, h->d_act.get(), h->d_obs.get(), h->d_rew.get(), h->d_done.get(), terminal_obs ? h->d_tobs.get() : nullptr)) return rc;
  if (int rc = to_host(h, obs, h->d_obs.get(), n * CASSIE3D_NOBS)) return rc;
  if (int rc = to_host(h, reward, h->d_rew.get(), n)) return rc;
  if (int rc = to_host(h, done, h->d_done.get(), n)) return rc;
  if (int rc = to_host(h, terminal_obs, h->d_tobs.get(), n * CASSIE3D_NOBS)) return rc;
  return synchronize(h);
}

int Cassie3dVecEnvGetCounters(Cassie3dVec* h, uint64_t* out2) {
  if (!h || !out2) return CASSIE_EINVAL;
  unsigned long long host[cassie3d::ENVC_N];
  if (int rc = read_counters(h, h->env_counters.get(), host)) return rc;
  out2[0] = host[cassie3d::ENVC_DONE];
  out2[1] = host[cassie3d::ENVC_GUARD];
  return CASSIE_OK;
}

int Cassie3dVecTimeSteps(Cassie3dVec* h, const double* torques_dev, int n_sub, int steps, float* avg_ms) {
  if (!h || steps <= 0 || !avg_ms) return CASSIE_EINVAL;
  return timed_steps(h, h->ev0.get(), h->ev1.get(), steps, avg_ms, [&] { return Cassie3dVecStep(h, torques_dev, n_sub); });
}

}  // extern "C"
