// tu_td3.hip -- fused kernels of TD3 (include/cassie_trpo.h, cassierl_amd/td3.py): the policy step with stateless Gaussian exploration that
// writes straight into the replay pool, the gradient of BOTH critics against a smoothed, clipped target action under the minimum of the two
// target critics in one launch, and both critics' Adam steps and soft updates in one launch of two workgroups.  An update that leaves the actor
// alone is these two launches; a delayed one adds tu_ddpg.hip's CassieDdpgActorGrad (through the first critic) and CassieDdpgApply (actor).
//
// The networks are tu_ddpg.hip's 32 x 32 ReLU networks and every convention is its (mlp32_tiles.h; read tu_ddpg.hip's header first).  Nothing
// here is a new building block: the target actor's forward pass is tu_ddpg.hip's, the two target critics under a minimum and the two live
// critics one after the other on the same registers are tu_sac.hip's (critic_step, critic_row and CriticAcc of mlp32_tiles.h), the Adam step
// is apply_rows of mlp32_tiles.h, which is CassieDdpgApply's body.  What is TD3's own is the target action
//   a' = clip(mu'(s') + clip(policy_noise eps, -noise_clip, noise_clip), -1, 1),
// formed in the registers in which the target actor's output layer leaves mu'(s') and the critics' merge layer takes it.  The noise eps
// arrives as a tensor indexed by the batch position (there is no generator in a kernel).
// Every sum runs in a fixed order: a launch repeats bit for bit.
#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "mlp32_tiles.h"

namespace cassie_td3 {

using namespace cassie_mlp32;

__device__ __forceinline__ float clip(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// ---------------------------------------------------------------------------------------------------------------- critic gradients
// Per sample b (pool row i = idx[b]):  a' as above from eps[b],  y = r_i + (1 - terminal_i) gamma min(Q1', Q2')(s'_i, a'),  e_k = Q_k(s_i, a_i) - y,
// and the gradient of sum_b e_k^2 with respect to live critic k.  Block k of partial: [rows][gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum e_k^2 |
// sum Q_k]: tu_sac.hip's layout.
enum { CQ_TA_W1 = 0, CQ_TA_W2 = 4, CQ_TA_W3 = 8, CQ_T1_W1 = 12, CQ_T1_W2 = 16, CQ_T1_A = 20, CQ_T2_W1 = 21, CQ_T2_W2 = 25, CQ_T2_A = 29, CQ_Q1 = 30, CQ_Q2 = CQ_Q1 + LQ_N,
       CQ_N = CQ_Q2 + LQ_N };
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) critic_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net ta, Net tq1, Net tq2, Net q1, Net q2,
                                                                    const float* __restrict__ eps_next, float policy_noise, float noise_clip, float gamma,
                                                                    float* __restrict__ partial) {
  typedef Shape<D, A> S;
  static_assert(D < 32 && A <= 8, "a column of ones next to the observations; the action rows in registers 0..3 of the two lane halves");
  constexpr int KS1 = (D + 1) / 2, NROW = S::NPQ + 2;
  static_assert(WAVES * NROW <= WAVES * 2 * 32 * TP, "the workgroup's reduction re-uses the transpose tiles");
  __shared__ alignas(16) float tilemem[WAVES * 2 * 32 * TP];
  __shared__ alignas(16) float sbias[15][32];   // target actor b1 b2 b3;  target critics b1 b2 W3 each;  live critics b1 b2 W3 each
  __shared__ float4 wimg[CQ_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = ta.b1[tid]; sbias[1][tid] = ta.b2[tid]; sbias[2][tid] = tid < A ? ta.b3[tid] : 0.0f;
    sbias[3][tid] = tq1.b1[tid]; sbias[4][tid] = tq1.b2[tid]; sbias[5][tid] = tq1.W3[tid];
    sbias[6][tid] = tq2.b1[tid]; sbias[7][tid] = tq2.b2[tid]; sbias[8][tid] = tq2.W3[tid];
    sbias[9][tid] = q1.b1[tid]; sbias[10][tid] = q1.b2[tid]; sbias[11][tid] = q1.W3[tid];
    sbias[12][tid] = q2.b1[tid]; sbias[13][tid] = q2.b2[tid]; sbias[14][tid] = q2.W3[tid];
  }
  {
    const Grp g[17] = {{K_FIRST, ta.W1, CQ_TA_W1, 4}, {K_HID, ta.W2, CQ_TA_W2, 4}, {K_OUT, ta.W3, CQ_TA_W3, 4},
                       {K_FIRST, tq1.W1, CQ_T1_W1, 4}, {K_HIDQ, tq1.W2, CQ_T1_W2, 4}, {K_ACTIN, tq1.W2, CQ_T1_A, 1},
                       {K_FIRST, tq2.W1, CQ_T2_W1, 4}, {K_HIDQ, tq2.W2, CQ_T2_W2, 4}, {K_ACTIN, tq2.W2, CQ_T2_A, 1},
                       {K_FIRST, q1.W1, CQ_Q1 + LQ_W1, 4}, {K_HIDQ, q1.W2, CQ_Q1 + LQ_W2, 4}, {K_ACTIN, q1.W2, CQ_Q1 + LQ_A, 1}, {K_HIDQT, q1.W2, CQ_Q1 + LQ_W2T, 4},
                       {K_FIRST, q2.W1, CQ_Q2 + LQ_W1, 4}, {K_HIDQ, q2.W2, CQ_Q2 + LQ_W2, 4}, {K_ACTIN, q2.W2, CQ_Q2 + LQ_A, 1}, {K_HIDQT, q2.W2, CQ_Q2 + LQ_W2T, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  const float b3t1 = tq1.b3[0], b3t2 = tq2.b3[0], b3q1 = q1.b3[0], b3q2 = q2.b3[0];
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  CriticAcc acc1, acc2;
  zero(acc1); zero(acc2);
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    const int s0 = tl * 32, smp = s0 + c;
    const bool valid = smp < n;
    const long long gi = valid ? clamp_row(idx[smp], pool.cap) : 0;
    float xb[KS1], xn[KS1], ab[4], en[4], xt[16], at[16];
#pragma unroll
    for (int s = 0; s < KS1; s++) {
      const int k = 2 * s + h;
      const bool on = valid && k < D;
      xb[s] = on ? pool.obs[gi * D + k] : 0.0f; xn[s] = on ? pool.nobs[gi * D + k] : 0.0f;
    }
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const bool on = valid && v + 4 * h < A;
      ab[v] = on ? pool.act[gi * A + v + 4 * h] : 0.0f;
      en[v] = on ? eps_next[(size_t)smp * A + v + 4 * h] : 0.0f;
    }
    // transposed operands of the parameter gradients: feature (action component) on the lane, column D (A) = ones
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int sm = s0 + 16 * h + s;
      const bool on = sm < n;
      const long long gs = on ? clamp_row(idx[sm], pool.cap) : 0;
      xt[s] = c < D ? (on ? pool.obs[gs * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f);
      at[s] = (c < A && on) ? pool.act[gs * A + c] : 0.0f;
    }
    const float rew = valid ? pool.rew[gi] : 0.0f, live = valid ? 1.0f - pool.term[gi] : 0.0f;
    // ---- target: min(Q1', Q2')(s', a')
    float y;
    {
      v16f a1, a2, u1, u2;
      float an[4], aw[16], w3a[16];
      two_layers<KS1>(wimg, CQ_TA_W1, CQ_TA_W2, sbias[0], sbias[1], xn, lane, h, a1, a2);
      relu16(a2);
      v16f mu = bias_tile(sbias[2], h);
      aop(wimg, CQ_TA_W3, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) mu = TILE_MFMA(aw[v], a2[v], mu);
#pragma unroll
      for (int v = 0; v < 4; v++)   // rows a >= A: W3, b3 and the noise are zeros -> a' = 0, on zero columns of the merge layer's image
        an[v] = clip(tanh_fast(mu[v]) + clip(policy_noise * en[v], -noise_clip, noise_clip), -1.0f, 1.0f);
      two_layers<KS1>(wimg, CQ_T1_W1, CQ_T1_W2, sbias[3], sbias[4], xn, lane, h, u1, u2);
      add_action(wimg, CQ_T1_A, lane, an, u2);
      relu16(u2);
      v16f w3 = bias_tile(sbias[5], h);
#pragma unroll
      for (int v = 0; v < 16; v++) w3a[v] = w3[v];
      const float qt1 = q_head(w3a, b3t1, u2);
      two_layers<KS1>(wimg, CQ_T2_W1, CQ_T2_W2, sbias[6], sbias[7], xn, lane, h, u1, u2);
      add_action(wimg, CQ_T2_A, lane, an, u2);
      relu16(u2);
      w3 = bias_tile(sbias[8], h);
#pragma unroll
      for (int v = 0; v < 16; v++) w3a[v] = w3[v];
      const float qt2 = q_head(w3a, b3t2, u2);
      y = rew + live * gamma * fminf(qt1, qt2);
    }
    critic_step<KS1>(wimg, CQ_Q1, sbias[9], sbias[10], sbias[11], b3q1, xb, ab, xt, at, y, valid, lane, c, h, t0, t1, acc1);
    critic_step<KS1>(wimg, CQ_Q2, sbias[12], sbias[13], sbias[14], b3q2, xb, ab, xt, at, y, valid, lane, c, h, t0, t1, acc2);
  }
  // ---- the wavefronts' rows in LDS (the tiles are free once every wavefront has left the loop), one row per workgroup and critic
  float* red = tilemem + wave * NROW;
  __syncthreads();
  critic_row<D, A>(acc1, red, lane, c, h);
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
  __syncthreads();
  critic_row<D, A>(acc2, red, lane, c, h);
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + ((size_t)gridDim.x + blockIdx.x) * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- apply (both critics)
// Workgroup k is CassieDdpgApply's workgroup on critic k: apply_rows (mlp32_tiles.h) on block k of the partial tensor, with the critic's two
// statistic columns added to stats[2 k], stats[2 k + 1].
struct CriticSide { const float* partial; NetRW live, targ; float *m, *v; double* stats; };
struct CriticPair { CriticSide side[2]; int off[7]; };
__global__ void __launch_bounds__(1024) critic_apply_kernel(int rows, float scale, CriticPair pair, float a, float beta1, float beta2, float eps, float tau) {
  const CriticSide& s = pair.side[blockIdx.x];
  apply_rows(rows, 2, s.partial, scale, s.live, s.targ, pair.off, s.m, s.v, a, beta1, beta2, eps, tau, s.stats);
}

// ---------------------------------------------------------------------------------------------------------------- policy step
// tu_ddpg.hip's policy_step_kernel with stateless exploration: act = clip(mu(s) + sigma noise, -1, 1).  obs32 and act are the pool's rows
// [top, top + n) (the caller passes the offset pointers).
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ noise, float sigma,
                                                                    const double* __restrict__ low, const double* __restrict__ high, float* __restrict__ obs32,
                                                                    float* __restrict__ act, double* __restrict__ env_act) {
  constexpr int KS1 = (D + 1) / 2;
  __shared__ alignas(16) float sbias[3][32];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) { sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = tid < A ? th.b3[tid] : 0.0f; }
  float aW1[KS1], aW2[16], aW3[16];
  double lo[4], hi[4];
#pragma unroll
  for (int s = 0; s < KS1; s++) aW1[s] = wel<D, A>(K_FIRST, th.W1, s, c, h);
#pragma unroll
  for (int v = 0; v < 16; v++) { aW2[v] = wel<D, A>(K_HID, th.W2, v, c, h); aW3[v] = wel<D, A>(K_OUT, th.W3, v, c, h); }
#pragma unroll
  for (int v = 0; v < 4; v++) { const int a = v + 4 * h; lo[v] = a < A ? low[a] : 0.0; hi[v] = a < A ? high[a] : 0.0; }
  __syncthreads();
  const int tl = blockIdx.x * WAVES + wave;   // one tile per wavefront
  const int smp = tl * 32 + c;
  const bool valid = smp < n;
  float xb[KS1];
#pragma unroll
  for (int s = 0; s < KS1; s++) {
    const int k = 2 * s + h;
    const bool on = valid && k < D;
    xb[s] = on ? (float)obs[(size_t)smp * D + k] : 0.0f;
    if (on) obs32[(size_t)smp * D + k] = xb[s];
  }
  v16f h1 = bias_tile(sbias[0], h);
#pragma unroll
  for (int s = 0; s < KS1; s++) h1 = TILE_MFMA(aW1[s], xb[s], h1);
  relu16(h1);
  v16f h2 = bias_tile(sbias[1], h);
#pragma unroll
  for (int v = 0; v < 16; v++) h2 = TILE_MFMA(aW2[v], h1[v], h2);
  relu16(h2);
  v16f z3 = bias_tile(sbias[2], h);
#pragma unroll
  for (int v = 0; v < 16; v++) z3 = TILE_MFMA(aW3[v], h2[v], z3);
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int a = v + 4 * h;
    if (valid && a < A) {
      const size_t o = (size_t)smp * A + a;
      const float val = clip(tanh_fast(z3[v]) + sigma * noise[o], -1.0f, 1.0f);
      act[o] = val;
      double e = lo[v] + ((double)val + 1.0) * 0.5 * (hi[v] - lo[v]);
      e = e < lo[v] ? lo[v] : (e > hi[v] ? hi[v] : e);
      env_act[o] = e;
    }
  }
}

}  // namespace cassie_td3

extern "C" {

int CassieTd3PolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, float sigma, const double* low_dev,
                        const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream) {
  using namespace cassie_td3;
  if (!obs_dev || n <= 0 || !net_ok(actor) || !noise_dev || !low_dev || !high_dev || !pool_obs_row_dev || !pool_act_row_dev || !env_actions_dev) return CASSIE_EINVAL;
  MLP32_LAUNCH_STEP(policy_step_kernel, obs_dim, act_dim, policy_step_grid(n), stream, obs_dev, n, net_of(actor), noise_dev, sigma, low_dev, high_dev, pool_obs_row_dev,
                    pool_act_row_dev, env_actions_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieTd3CriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                        long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* target_actor,
                        const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                        const float* eps_next_dev, float policy_noise, float noise_clip, float discount, float* partial_dev, void* stream) {
  using namespace cassie_td3;
  const Pool pool{pool_obs, pool_act, pool_rew, pool_term, pool_next_obs, pool_capacity};
  if (!pool_ok(pool) || !idx_dev || batch <= 0 || !eps_next_dev || !(noise_clip >= 0.0f) || !partial_dev || !aligned4(partial_dev)) return CASSIE_EINVAL;
  if (!net_ok(target_actor) || !net_ok(target_qf1) || !net_ok(target_qf2) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  MLP32_LAUNCH(critic_grad_kernel, obs_dim, act_dim, blocks_for(batch), stream, pool, idx_dev, batch, net_of(target_actor), net_of(target_qf1), net_of(target_qf2),
               net_of(qf1), net_of(qf2), eps_next_dev, policy_noise, noise_clip, discount, partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieTd3CriticApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* qf1, float* const* qf2, float* const* target_qf1,
                         float* const* target_qf2, float* m1_dev, float* v1_dev, float* m2_dev, float* v2_dev, int t, float lr, float beta1, float beta2, float eps,
                         float tau, double* stats_dev, void* stream) {
  using namespace cassie_td3;
  const int np = CassieDdpgParamCount(obs_dim, act_dim, CASSIE_DDPG_CRITIC);
  if (np == 0 || rows <= 0 || !partial_dev || !m1_dev || !v1_dev || !m2_dev || !v2_dev || t < 1) return CASSIE_EINVAL;
  if (!net_ok(qf1) || !net_ok(qf2) || !net_ok(target_qf1) || !net_ok(target_qf2)) return CASSIE_EINVAL;
  CriticPair pair;
  pair.side[0] = CriticSide{partial_dev, net_rw(qf1), net_rw(target_qf1), m1_dev, v1_dev, stats_dev};
  pair.side[1] = CriticSide{partial_dev + (size_t)rows * (np + 2), net_rw(qf2), net_rw(target_qf2), m2_dev, v2_dev, stats_dev ? stats_dev + 2 : nullptr};
  critic_offsets(obs_dim, act_dim, pair.off);   // the critic's row, as CassieDdpgApply lays it out
  hipLaunchKernelGGL(critic_apply_kernel, dim3(2), dim3(1024), 0, (hipStream_t)stream, rows, scale, pair, adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, tau);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
