// tu_ddpg.hip -- fused kernels of DDPG (include/cassie_trpo.h, cassierl_amd/ddpg.py; rllab/envs/ddpg_cassie.py): the policy step that
// writes straight into the replay pool, the pool commit after Env.step, the critic's and the actor's gradient on a batch gathered from the
// pool by index, and the Adam step + soft target update.  One update is four launches (critic gradient, apply, actor gradient, apply)
// where the torch statement (ddpg.ddpg_update_torch_) is 60 or more.
//
// The networks are 32 x 32 with ReLU hidden units:
//   actor   mu(s) = tanh(W3 relu(W2 relu(W1 s + b1) + b2) + b3)          W1 [32][D], W2 [32][32], W3 [A][32]
//   critic  Q(s, a) = W3 relu(W2 [relu(W1 s + b1); a] + b2) + b3          W1 [32][D], W2 [32][32 + A], W3 [1][32]
// and the layout is tu_trpo.hip's (read its header first): exact float32 v_mfma_f32_32x32x2_f32, a tile of 32 samples per wavefront, every
// activation in the accumulator layout (sample on the lane c = lane & 31, hidden unit r(v, h) = (v & 3) + 8 (v >> 2) + 4 h in register v),
// the A operands of every product laid out once per workgroup in LDS, parameter gradients through per-wavefront LDS transposes.
// What is new against tu_trpo.hip:
//   * the ReLU mask (h > 0) replaces 1 - h^2;
//   * the critic's merge layer: the action joins as four more k-steps with the action a = v + 4 h in register v < 4 of lane (sample, h) --
//     the layout in which the actor's output layer leaves mu(s), so Q(s, mu(s)) needs no data movement, and the layout of the cotangent
//     dQ/da that the actor's reverse pass takes (tu_trpo.hip's `wt`);
//   * the critic's output layer has one row: q is a 16-term dot product per lane plus one cross-half shuffle, its gradient a per-lane
//     accumulation reduced over the lanes once per wavefront;
//   * every per-sample row is gathered from the pool through the batch's index (clamped to the pool's capacity);
//   * the four wavefronts of a workgroup add their accumulators in LDS in a fixed order: one partial row per WORKGROUP, at most 256 rows,
//     so that the single-workgroup apply kernel reads 2 MB and not 18.
// Every sum runs in a fixed order (k-ordered MFMA chains, tiles in a fixed order per wavefront, a fixed grid for a given n): a run repeats
// bit for bit.
// The building blocks are mlp32_tiles.h's, shared with tu_sac.hip and tu_td3.hip: the gather of a tile, the forward passes, the live critic's tile
// pass, the actor's reverse pass, the row stores, the policy step's body and the Adam step.  This unit keeps the target of its critic kernel, the
// cotangent of its actor kernel, the Ornstein-Uhlenbeck head of its policy step, the pool commit and the entry points.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "mlp32_tiles.h"

namespace cassie_ddpg {

using namespace cassie_mlp32;   // shapes, operand images, tile helpers (shared with tu_sac.hip, tu_td3.hip)

// ---------------------------------------------------------------------------------------------------------------- critic gradient
// Per sample b of the batch (pool row i = idx[b]):  y = r_i + (1 - terminal_i) gamma Q'(s'_i, mu'(s'_i)),  e = Q(s_i, a_i) - y, and the
// gradient of sum_b e^2 with respect to the live critic.  Row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum e^2 | sum Q].
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) critic_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net ta, Net tq, Net q, float gamma,
                                                                    float* __restrict__ partial) {
  typedef Shape<D, A> S;
  static_assert(S::NS == 4, "this unit's target action and cotangent are written for four slots, the action a = v + 4 h in register v < 4 (A <= 8)");
  enum { CQ_TA = 0, CQ_TQ = S::LA_N, CQ_Q = CQ_TQ + S::LQ_FWD, CQ_N = CQ_Q + S::LQ_N };
  constexpr int NROW = S::NPQ + 2, NQ1 = S::NQ1;
  static_assert(WAVES * NROW <= WAVES * 2 * 32 * TP, "the workgroup's reduction re-uses the transpose tiles");
  __shared__ alignas(16) float tilemem[WAVES * 2 * 32 * TP];
  __shared__ alignas(16) float sbias[8][32];   // target actor b1 b2 b3;  target critic b1 b2 (its W3 in registers);  live critic b1 b2 W3
  __shared__ float4 wimg[CQ_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = ta.b1[tid]; sbias[1][tid] = ta.b2[tid]; sbias[2][tid] = out_bias<A, K_OUT>(ta.b3, tid);
    sbias[3][tid] = tq.b1[tid]; sbias[4][tid] = tq.b2[tid];
    sbias[5][tid] = q.b1[tid]; sbias[6][tid] = q.b2[tid]; sbias[7][tid] = q.W3[tid];
  }
  {
    const Grp g[10] = {{K_FIRST, ta.W1, CQ_TA + S::LA_W1, NQ1}, {K_HID, ta.W2, CQ_TA + S::LA_W2, 4}, {K_OUT, ta.W3, CQ_TA + S::LA_W3, 4},
                       {K_FIRST, tq.W1, CQ_TQ + S::LQ_W1, NQ1}, {K_HIDQ, tq.W2, CQ_TQ + S::LQ_W2, 4}, {K_ACTIN, tq.W2, CQ_TQ + S::LQ_A, S::NQA},
                       {K_FIRST, q.W1, CQ_Q + S::LQ_W1, NQ1}, {K_HIDQ, q.W2, CQ_Q + S::LQ_W2, 4}, {K_ACTIN, q.W2, CQ_Q + S::LQ_A, S::NQA},
                       {K_HIDQT, q.W2, CQ_Q + S::LQ_W2T, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  float w3t[16];   // in registers: read from a row of sbias like the live critic's, the kernel takes 228 + 52 registers, not 186 + 48, and occupancy 1
#pragma unroll
  for (int v = 0; v < 16; v++) w3t[v] = tq.W3[row_of(v, h)];
  const float b3t = tq.b3[0], b3q = q.b3[0];
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  CriticAcc<S::NB1> acc;
  zero(acc);
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    Tile<D, A> t;
    gather<true>(pool, idx, n, tl, c, h, t);
    // ---- target: Q'(s', mu'(s'))
    float y;
    {
      v16f a1, a2, mu, u1, u2;
      float mt[4];
      actor_forward<D, A>(wimg, CQ_TA, sbias, t.xn, lane, h, a1, a2, mu);
#pragma unroll
      for (int v = 0; v < 4; v++) mt[v] = tanh_fast(mu[v]);   // rows a >= A: W3 and b3 padded with zeros -> tanh(0) = 0
      y = t.rew + t.live * gamma * critic_forward<D, A>(wimg, CQ_TQ, sbias + 3, w3t, b3t, t.xn, mt, lane, h, u1, u2);
    }
    critic_step(wimg, CQ_Q, sbias + 5, b3q, t, y, lane, c, h, t0, t1, acc);   // the live critic at (s, a)
  }
  // ---- this wavefront's row in LDS (the tiles are free once every wavefront has left the loop), then one row per workgroup
  __syncthreads();
  critic_row<D, A>(acc, tilemem + wave * NROW, lane, c, h);
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- actor gradient
// Gradient of -sum_b Q(s_b, mu(s_b)) with respect to the actor, through the live critic.  Row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum Q].
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) actor_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net th, Net q, float* __restrict__ partial) {
  typedef Shape<D, A> S;
  static_assert(S::NS == 4, "see critic_grad_kernel");
  enum { AG_PI = 0, AG_W2T = S::LA_N, AG_W3T = AG_W2T + 4, AG_Q = AG_W3T + S::NQA, AG_Q_DA = AG_Q + S::LQ_FWD, AG_N = AG_Q_DA + 4 };
  constexpr int NROW = S::NPA + 1, NQ1 = S::NQ1;
  static_assert(WAVES * NROW <= WAVES * 2 * 32 * TP, "the workgroup's reduction re-uses the transpose tiles");
  __shared__ alignas(16) float tilemem[WAVES * 2 * 32 * TP];
  __shared__ alignas(16) float sbias[5][32];   // actor b1 b2 b3, critic b1 b2 (its W3 stays in registers: the LDS of this kernel is full)
  __shared__ float4 wimg[AG_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = out_bias<A, K_OUT>(th.b3, tid);
    sbias[3][tid] = q.b1[tid]; sbias[4][tid] = q.b2[tid];
  }
  {
    const Grp g[9] = {{K_FIRST, th.W1, AG_PI + S::LA_W1, NQ1}, {K_HID, th.W2, AG_PI + S::LA_W2, 4}, {K_OUT, th.W3, AG_PI + S::LA_W3, 4},
                      {K_HIDT, th.W2, AG_W2T, 4}, {K_W3T, th.W3, AG_W3T, S::NQA}, {K_FIRST, q.W1, AG_Q + S::LQ_W1, NQ1}, {K_HIDQ, q.W2, AG_Q + S::LQ_W2, 4},
                      {K_ACTIN, q.W2, AG_Q + S::LQ_A, S::NQA}, {K_DA, q.W2, AG_Q_DA, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  float w3q[16];
#pragma unroll
  for (int v = 0; v < 16; v++) w3q[v] = q.W3[row_of(v, h)];
  const float b3q = q.b3[0];
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  ActorAcc<S::NB1> acc;
  zero(acc);
  float sq = 0.0f;
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    Tile<D, A> t;
    gather<false>(pool, idx, n, tl, c, h, t);
    // ---- actor forward: mu(s), action a = v + 4 h in register v < 4
    v16f a1, a2, z3;
    float aw[16], mu[4];
    actor_forward<D, A>(wimg, AG_PI, sbias, t.xb, lane, h, a1, a2, z3);
#pragma unroll
    for (int v = 0; v < 4; v++) mu[v] = tanh_fast(z3[v]);
    // ---- critic at (s, mu(s)) and dQ/da = W2a' (W3 o (h2 > 0))
    v16f c1, c2, da;
    const float qv = critic_forward<D, A>(wimg, AG_Q, sbias + 3, w3q, b3q, t.xb, mu, lane, h, c1, c2);
    if (h == 0 && t.valid) sq += qv;
#pragma unroll
    for (int v = 0; v < 16; v++) da[v] = 0.0f;
    aop(wimg, AG_Q_DA, lane, aw);
#pragma unroll
    for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], c2[v] > 0.0f ? w3q[v] : 0.0f, da);
    // cotangent of -Q on the output layer's pre-activation
    v16f wt;
#pragma unroll
    for (int v = 0; v < 16; v++) wt[v] = 0.0f;
#pragma unroll
    for (int v = 0; v < 4; v++) wt[v] = (t.valid && v + 4 * h < A) ? -da[v] * (1.0f - mu[v] * mu[v]) : 0.0f;
    actor_reverse<S::NQA>(wimg, AG_W2T, AG_W3T, a1, a2, wt, t.xt, t0, t1, lane, c, h, acc);
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) sq += __shfl_xor(sq, m, 64);
  __syncthreads();
  float* red = tilemem + wave * NROW;
  actor_row<S, D, A, K_OUT>(acc, red, c, h);
  if (lane == 0) red[S::NPA] = sq;
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- apply
// apply_rows (mlp32_tiles.h) on one network: Adam on the live network, the soft update of its target, the statistic columns.  One workgroup.
__global__ void __launch_bounds__(1024) apply_kernel(int rows, int ns, const float* __restrict__ partial, float scale, NetRW live, NetRW targ, Offsets off,
                                                     float* __restrict__ m, float* __restrict__ v, float a, float beta1, float beta2, float eps, float tau,
                                                     double* __restrict__ stats) {
  apply_rows(rows, ns, partial, scale, live, targ, off.o, m, v, a, beta1, beta2, eps, tau, stats);
}

// ---------------------------------------------------------------------------------------------------------------- policy step
// policy_step (mlp32_tiles.h) with a tanh output and Ornstein-Uhlenbeck noise (rllab's OUStrategy):
//   x = path_t == 0 ? mu : ou;  x += theta (mu - x) + sigma noise;  act = clip(mu(s) + x, -1, 1)
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ noise,
                                                                    const long long* __restrict__ path_t, float ou_theta, float ou_sigma, float ou_mu,
                                                                    float* __restrict__ ou, const double* __restrict__ low, const double* __restrict__ high,
                                                                    float* __restrict__ obs32, float* __restrict__ act, double* __restrict__ env_act) {
  policy_step<D, A, K_OUT>(obs, n, th, low, high, obs32, act, env_act, [&](const v16f& z3, int v, size_t o, int smp) {
    float x = path_t[smp] == 0 ? ou_mu : ou[o];
    x = x + ou_theta * (ou_mu - x) + ou_sigma * noise[o];
    ou[o] = x;
    const float val = tanh_fast(z3[v]) + x;
    return val < -1.0f ? -1.0f : (val > 1.0f ? 1.0f : val);
  });
}

// ---------------------------------------------------------------------------------------------------------------- pool commit
// After Env.step: reward (scaled in float64, stored in float32), terminal flag and the float32 next observation into the rows the policy
// step opened.  One lane per element of the next observation; the lane of element 0 also writes the two scalars of its row.
__global__ void __launch_bounds__(256) pool_commit_kernel(const double* __restrict__ rew, const uint8_t* __restrict__ done, const double* __restrict__ nobs, int n,
                                                          int D, double scale, float* __restrict__ prew, float* __restrict__ pterm, float* __restrict__ pnobs) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * D) return;
  pnobs[e] = (float)nobs[e];
  if (e % D == 0) {
    const size_t i = e / D;
    prew[i] = (float)(scale * rew[i]);
    pterm[i] = done[i] != 0 ? 1.0f : 0.0f;
  }
}

}  // namespace cassie_ddpg

extern "C" {

int CassieDdpgParamCount(int obs_dim, int act_dim, int which) {
  if (!cassie_ddpg::shape_ok(obs_dim, act_dim)) return 0;
  int off[7] = {0};
  if (which == CASSIE_DDPG_ACTOR) cassie_ddpg::actor_offsets(obs_dim, act_dim, off);
  else if (which == CASSIE_DDPG_CRITIC) cassie_ddpg::critic_offsets(obs_dim, act_dim, off);
  return off[6];
}
int CassieDdpgPartialRows(int batch) { return batch > 0 ? cassie_ddpg::blocks_for(batch) : 0; }

int CassieDdpgPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                         const float* b3, const float* noise_dev, const long long* path_t_dev, float ou_theta, float ou_sigma, float ou_mu, float* ou_state_dev,
                         const double* low_dev, const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream) {
  using namespace cassie_ddpg;
  if (!obs_dev || n <= 0 || !net_ok(W1, b1, W2, b2, W3, b3) || !noise_dev || !path_t_dev || !ou_state_dev || !low_dev || !high_dev || !pool_obs_row_dev ||
      !pool_act_row_dev || !env_actions_dev)
    return CASSIE_EINVAL;
  const Net th{W1, b1, W2, b2, W3, b3};
  MLP32_LAUNCH_STEP(policy_step_kernel, obs_dim, act_dim, policy_step_grid(n), stream, obs_dev, n, th, noise_dev, path_t_dev, ou_theta, ou_sigma, ou_mu, ou_state_dev,
                    low_dev, high_dev, pool_obs_row_dev, pool_act_row_dev, env_actions_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieDdpgPoolCommit(const double* rew_dev, const unsigned char* done_dev, const double* next_obs_dev, int n, int obs_dim, double scale_reward,
                         float* pool_rew_row_dev, float* pool_term_row_dev, float* pool_next_obs_row_dev, void* stream) {
  if (!rew_dev || !done_dev || !next_obs_dev || n <= 0 || obs_dim <= 0 || !pool_rew_row_dev || !pool_term_row_dev || !pool_next_obs_row_dev) return CASSIE_EINVAL;
  const size_t total = (size_t)n * obs_dim;
  hipLaunchKernelGGL(cassie_ddpg::pool_commit_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rew_dev, done_dev, next_obs_dev, n,
                     obs_dim, scale_reward, pool_rew_row_dev, pool_term_row_dev, pool_next_obs_row_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieDdpgCriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                         long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim,
                         const float* const* target_actor, const float* const* target_critic, const float* const* critic, float discount, float* partial_dev,
                         void* stream) {
  using namespace cassie_ddpg;
  const Pool pool{pool_obs, pool_act, pool_rew, pool_term, pool_next_obs, pool_capacity};
  if (!pool_ok(pool) || !idx_dev || batch <= 0 || !partial_dev || !aligned4(partial_dev)) return CASSIE_EINVAL;
  if (!net_ok(target_actor) || !net_ok(target_critic) || !net_ok(critic)) return CASSIE_EINVAL;
  MLP32_LAUNCH(critic_grad_kernel, obs_dim, act_dim, blocks_for(batch), stream, pool, idx_dev, batch, net_of(target_actor), net_of(target_critic), net_of(critic),
               discount, partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieDdpgActorGrad(const float* pool_obs, long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                        const float* const* critic, float* partial_dev, void* stream) {
  using namespace cassie_ddpg;
  if (!pool_obs || pool_capacity <= 0 || !idx_dev || batch <= 0 || !net_ok(actor) || !net_ok(critic) || !partial_dev || !aligned4(partial_dev)) return CASSIE_EINVAL;
  const Pool pool{pool_obs, nullptr, nullptr, nullptr, nullptr, pool_capacity};
  MLP32_LAUNCH(actor_grad_kernel, obs_dim, act_dim, blocks_for(batch), stream, pool, idx_dev, batch, net_of(actor), net_of(critic), partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieDdpgApply(int rows, int obs_dim, int act_dim, int which, const float* partial_dev, float scale, float* const* live, float* const* target, float* m_dev,
                    float* v_dev, int t, float lr, float beta1, float beta2, float eps, float tau, double* stats_dev, void* stream) {
  using namespace cassie_ddpg;
  const bool actor = which == CASSIE_DDPG_ACTOR;
  if (CassieDdpgParamCount(obs_dim, act_dim, which) == 0 || rows <= 0 || !partial_dev || !net_ok(live) || !net_ok(target) || !m_dev || !v_dev || t < 1)
    return CASSIE_EINVAL;
  Offsets off;
  if (actor) actor_offsets(obs_dim, act_dim, off.o);
  else critic_offsets(obs_dim, act_dim, off.o);
  hipLaunchKernelGGL(apply_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, actor ? 1 : 2, partial_dev, scale, net_rw(live), net_rw(target), off, m_dev, v_dev,
                     adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, tau, stats_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
