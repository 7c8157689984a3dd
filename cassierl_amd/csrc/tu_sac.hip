// tu_sac.hip -- fused kernels of Soft Actor-Critic (include/cassie_trpo.h, cassierl_amd/sac.py): the policy step that samples the squashed
// Gaussian and writes straight into the replay pool, the gradient of BOTH critics in one launch, the actor's gradient through the minimum of
// the two critics and through log pi, and the actor's Adam step with the temperature's.  One update is five launches (critic gradient,
// CassieDdpgApply for each critic, actor gradient, CassieSacApply) where the torch statement (sac.sac_update_torch_) is well over a hundred.
//
// The networks are tu_ddpg.hip's 32 x 32 ReLU networks and every convention is its (mlp32_tiles.h; read tu_ddpg.hip's header first).  The
// critics ARE DDPG's critics, so their Adam step and soft update are CassieDdpgApply.  What is new:
//   * the actor's output layer has 2 A rows, mean [0, A) and log_std [A, 2 A).  Its A-operand image permutes them: image row a holds mean a,
//     image row 8 + a holds log_std a (a < A <= 8).  In the accumulator layout the lane (sample, h) then holds, for the action a = v + 4 h,
//     the mean in register v < 4 and log_std in register v + 4: the sample u = mean + exp(log_std) eps, a = tanh(u) and log pi need no data
//     movement, the action sits where the critic's merge layer takes it (tu_ddpg.hip), and the cotangents of both heads sit where the
//     reverse pass takes them (two quads of k-steps instead of DDPG's one);
//   * log pi(a|s) = sum_k (-eps_k^2 / 2 - log_std_k - log(2 pi) / 2) - sum_k 2 (log 2 - u_k - softplus(-2 u_k)); its derivative with respect
//     to u_k is 2 tanh(u_k), with respect to log_std_k directly -1; the clamp of log_std to [-20, 2] passes no gradient outside;
//   * the noise eps arrives as a tensor indexed by the batch position (there is no generator in a kernel); the temperature as a device
//     pointer to log_alpha, so that no launch waits for a read-back;
//   * the critic kernel computes y once per sample and runs the two live critics one after the other on the same registers; each critic
//     has its own block [rows][NPq + 2] of the partial tensor, which is CassieDdpgApply's row format.  Its body is twin_critic_grad of
//     mlp32_tiles.h, shared with tu_td3.hip: this unit gives it the target action and the entropy term.
// What this unit keeps: the squashed-Gaussian head (squash, actor_sample), the cotangents of its actor kernel, the temperature's Adam step and
// its statistics, and the entry points; everything else is mlp32_tiles.h's.
// Every sum runs in a fixed order: a launch repeats bit for bit.
#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "mlp32_tiles.h"

namespace cassie_sac {

using namespace cassie_mlp32;

constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;

// one component of the squashed Gaussian: action, its log-density term, exp(log_std) eps, and whether the clamp lets a gradient through
__device__ __forceinline__ void squash(float mean, float ls_raw, float eps, float& act, float& logp, float& sde, bool& inside) {
  const float ls = fminf(fmaxf(ls_raw, LOG_STD_MIN), LOG_STD_MAX);
  inside = ls_raw >= LOG_STD_MIN && ls_raw <= LOG_STD_MAX;
  sde = expf(ls) * eps;
  const float u = mean + sde, m2u = -2.0f * u;
  act = tanh_fast(u);
  const float softplus = fmaxf(m2u, 0.0f) + log1pf(expf(-fabsf(m2u)));
  logp = (-0.5f * eps * eps - ls - 0.9189385332046727f) - 2.0f * (0.6931471805599453f - u - softplus);
}

// the actor (images at q0, rows sb[0 .. 2]: mlp32_tiles.h, actor_forward) on the first-layer operand xb with the noise eps [4] of the lane's
// actions a = v + 4 h: hidden activations a1, a2, the squashed action act [4] (0 for a >= A), log pi of the sample (both lane halves hold it)
template <int A, int KS1>
__device__ __forceinline__ void actor_sample(const float4 (*wimg)[64], int q0, const float (*sb)[32], const float (&xb)[KS1], const float (&eps)[4], int lane, int h,
                                             v16f& a1, v16f& a2, float (&act)[4], float (&sde)[4], bool (&inside)[4], float& logpi) {
  v16f z3;
  actor_forward<KS1>(wimg, q0, sb, xb, lane, h, a1, a2, z3);
  float lp = 0.0f;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    float l;
    squash(z3[v], z3[v + 4], eps[v], act[v], l, sde[v], inside[v]);
    if (v + 4 * h < A) lp += l; else act[v] = 0.0f;
  }
  logpi = lp + __shfl_xor(lp, 32, 64);
}

// ---------------------------------------------------------------------------------------------------------------- critic gradients
// twin_critic_grad (mlp32_tiles.h) with  a' = pi(s'_i; eps[b])  and  sub = alpha log pi(a'|s'_i).
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) critic_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net pi, Net tq1, Net tq2, Net q1, Net q2,
                                                                    const float* __restrict__ eps_next, const float* __restrict__ log_alpha, float gamma,
                                                                    float* __restrict__ partial) {
  const float alpha = expf(log_alpha[0]);
  const auto target = [=](const float4 (*wimg)[64], const float (*sb)[32], const float (&xn)[(D + 1) / 2], const float (&en)[4], int lane, int h, float (&an)[4]) {
    v16f a1, a2;
    float sde[4], logpi;
    bool inside[4];
    actor_sample<A>(wimg, TC_PI, sb, xn, en, lane, h, a1, a2, an, sde, inside, logpi);
    return alpha * logpi;
  };
  twin_critic_grad<D, A, K_HEAD>(pool, idx, n, pi, tq1, tq2, q1, q2, eps_next, gamma, partial, target);
}

// ---------------------------------------------------------------------------------------------------------------- actor gradient
// Gradient of sum_b (alpha log pi(a~_b|s_b) - min(Q1, Q2)(s_b, a~_b)), a~ = pi(s; eps), with respect to the actor, through the live critics.
// Row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum log pi | sum min Q].
enum { AG_PI = 0, AG_W2T = LA_N, AG_W3T = 16, AG_Q1 = 18, AQ_DA = LQ_FWD, AQ_N = AQ_DA + 4, AG_Q2 = AG_Q1 + AQ_N, AG_N = AG_Q2 + AQ_N };
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) actor_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net th, Net q1, Net q2,
                                                                   const float* __restrict__ eps_dev, const float* __restrict__ log_alpha, float* __restrict__ partial) {
  typedef Shape<D, A, 2 * A> S;   // the actor's row with the 2 A output rows
  static_assert(D < 32 && A <= 8, "a column of ones next to the observations; mean and log_std of an action in registers v and v + 4 of one lane");
  constexpr int KS1 = (D + 1) / 2, NROW = S::NPA + 2, TILES = WAVES * 2 * 32 * TP;
  // the workgroup's reduction re-uses the transpose tiles; with D = 26 the four rows of 2 A output rows are a little longer than the tiles
  __shared__ alignas(16) float tilemem[TILES > WAVES * NROW ? TILES : WAVES * NROW];
  __shared__ alignas(16) float sbias[9][32];   // actor b1 b2 b3;  critics b1 b2 W3 each
  __shared__ float4 wimg[AG_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = out_bias<A, K_HEAD>(th.b3, tid);
    sbias[3][tid] = q1.b1[tid]; sbias[4][tid] = q1.b2[tid]; sbias[5][tid] = q1.W3[tid];
    sbias[6][tid] = q2.b1[tid]; sbias[7][tid] = q2.b2[tid]; sbias[8][tid] = q2.W3[tid];
  }
  {
    const Grp g[13] = {{K_FIRST, th.W1, AG_PI + LA_W1, 4}, {K_HID, th.W2, AG_PI + LA_W2, 4}, {K_HEAD, th.W3, AG_PI + LA_W3, 4}, {K_HIDT, th.W2, AG_W2T, 4},
                       {K_HEADT, th.W3, AG_W3T, 2},
                       {K_FIRST, q1.W1, AG_Q1 + LQ_W1, 4}, {K_HIDQ, q1.W2, AG_Q1 + LQ_W2, 4}, {K_ACTIN, q1.W2, AG_Q1 + LQ_A, 1}, {K_DA, q1.W2, AG_Q1 + AQ_DA, 4},
                       {K_FIRST, q2.W1, AG_Q2 + LQ_W1, 4}, {K_HIDQ, q2.W2, AG_Q2 + LQ_W2, 4}, {K_ACTIN, q2.W2, AG_Q2 + LQ_A, 1}, {K_DA, q2.W2, AG_Q2 + AQ_DA, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  const float b3q1 = q1.b3[0], b3q2 = q2.b3[0], alpha = expf(log_alpha[0]);
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  ActorAcc acc;
  zero(acc);
  float slp = 0.0f, sq = 0.0f;
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    Tile<D, A> t;
    gather<false>(pool, idx, n, tl, c, h, t);
    float ep[4];
    action_quad<A>(eps_dev, t.smp, t.valid, h, ep);
    // ---- actor forward: a~ = tanh(mean + exp(log_std) eps), action a = v + 4 h in register v < 4
    v16f a1, a2;
    float act[4], sde[4], logpi, aw[16];
    bool inside[4];
    actor_sample<A>(wimg, AG_PI, sbias, t.xb, ep, lane, h, a1, a2, act, sde, inside, logpi);
    // ---- both critics at (s, a~);  d min(Q1, Q2) / da = W2a' (W3 o (h2 > 0)) of the smaller one
    v16f da;
#pragma unroll
    for (int v = 0; v < 16; v++) da[v] = 0.0f;
    float qmin;
    {
      v16f c1, h2a, h2b;
      float wa[16], wb[16];
      w3_row(sbias[5], h, wa); w3_row(sbias[8], h, wb);
      const float qa = critic_forward<KS1>(wimg, AG_Q1, sbias + 3, wa, b3q1, t.xb, act, lane, h, c1, h2a);
      const float qb = critic_forward<KS1>(wimg, AG_Q2, sbias + 6, wb, b3q2, t.xb, act, lane, h, c1, h2b);
      const bool first = qa <= qb;
      qmin = first ? qa : qb;
      aop(wimg, AG_Q1 + AQ_DA, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], (first && h2a[v] > 0.0f) ? wa[v] : 0.0f, da);
      aop(wimg, AG_Q2 + AQ_DA, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], (!first && h2b[v] > 0.0f) ? wb[v] : 0.0f, da);
    }
    if (h == 0 && t.valid) { slp += logpi; sq += qmin; }
    // cotangents of alpha log pi - min Q on the output layer: d/du = 2 alpha a~ - dQ/da (1 - a~^2) on the mean row, that times
    // exp(log_std) eps, minus alpha, on the log_std row (nothing where the clamp is active)
    v16f wt;
#pragma unroll
    for (int v = 0; v < 16; v++) wt[v] = 0.0f;
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const bool on = t.valid && v + 4 * h < A;
      const float du = 2.0f * alpha * act[v] - da[v] * (1.0f - act[v] * act[v]);
      wt[v] = on ? du : 0.0f;
      wt[v + 4] = (on && inside[v]) ? du * sde[v] - alpha : 0.0f;
    }
    actor_reverse<2>(wimg, AG_W2T, AG_W3T, a1, a2, wt, t.xt, t0, t1, lane, c, h, acc);   // two quads of output rows
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) { slp += __shfl_xor(slp, m, 64); sq += __shfl_xor(sq, m, 64); }
  __syncthreads();
  float* red = tilemem + wave * NROW;
  actor_row<S, D, A, K_HEAD>(acc, red, c, h);
  if (lane == 0) { red[S::NPA] = slp; red[S::NPA + 1] = sq; }
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- apply (actor, temperature)
// The actor's Adam step from the pieces of apply_rows (mlp32_tiles.h), without a target network; the last thread takes log_alpha's Adam step on
// the gradient -(scale * sum log pi + target_entropy), the log pi column added in row order (alpha_m == NULL: the temperature is fixed).
__global__ void __launch_bounds__(1024) apply_kernel(int rows, const float* __restrict__ partial, float scale, NetRW live, Offsets off, float* __restrict__ m,
                                                     float* __restrict__ v, float a, float beta1, float beta2, float eps, float* __restrict__ log_alpha,
                                                     float* __restrict__ alpha_m, float* __restrict__ alpha_v, float a_alpha, float target_entropy,
                                                     double* __restrict__ stats) {
  constexpr int NS = 2;
  const int np = off.o[6], stride = np + NS;
  if ((int)threadIdx.x <= NS && stats) {   // (sum log pi, sum min Q, the summed actor loss at the temperature BEFORE its step)
    double s[NS] = {0.0, 0.0};
    for (int r = 0; r < rows; r++) {
      s[0] += (double)partial[(size_t)r * stride + np]; s[1] += (double)partial[(size_t)r * stride + np + 1];
    }
    stats[threadIdx.x] += threadIdx.x == 0 ? s[0] : (threadIdx.x == 1 ? s[1] : exp((double)log_alpha[0]) * s[0] - s[1]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < np; i += 1024)
    adam_entry(column_sum(partial + i, rows, stride, scale), m + i, v + i, entry_of(live, off.o, i), a, beta1, beta2, eps);
  if (threadIdx.x == 1023 && alpha_m)
    adam_entry(-(column_sum(partial + np, rows, stride, scale) + target_entropy), alpha_m, alpha_v, log_alpha, a_alpha, beta1, beta2, eps);
}

// ---------------------------------------------------------------------------------------------------------------- policy step
// policy_step (mlp32_tiles.h) with the squashed-Gaussian head: act = tanh(mean + exp(clamp(log_std)) noise), in [-1, 1] by construction.
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ noise,
                                                                    const double* __restrict__ low, const double* __restrict__ high, float* __restrict__ obs32,
                                                                    float* __restrict__ act, double* __restrict__ env_act) {
  policy_step<D, A, K_HEAD>(obs, n, th, low, high, obs32, act, env_act, [&](const v16f& z3, int v, size_t o, int) {
    const float ls = fminf(fmaxf(z3[v + 4], LOG_STD_MIN), LOG_STD_MAX);
    return tanh_fast(z3[v] + expf(ls) * noise[o]);
  });
}

}  // namespace cassie_sac

extern "C" {

int CassieSacParamCount(int obs_dim, int act_dim) {
  if (!cassie_sac::shape_ok(obs_dim, act_dim)) return 0;
  int off[7];
  cassie_sac::actor_offsets(obs_dim, 2 * act_dim, off);
  return off[6];
}

int CassieSacPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, const double* low_dev,
                        const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream) {
  using namespace cassie_sac;
  if (!obs_dev || n <= 0 || !net_ok(actor) || !noise_dev || !low_dev || !high_dev || !pool_obs_row_dev || !pool_act_row_dev || !env_actions_dev) return CASSIE_EINVAL;
  MLP32_LAUNCH_STEP(policy_step_kernel, obs_dim, act_dim, policy_step_grid(n), stream, obs_dev, n, net_of(actor), noise_dev, low_dev, high_dev, pool_obs_row_dev,
                    pool_act_row_dev, env_actions_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieSacCriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                        long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                        const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                        const float* eps_next_dev, const float* log_alpha_dev, float discount, float* partial_dev, void* stream) {
  using namespace cassie_sac;
  const Pool pool{pool_obs, pool_act, pool_rew, pool_term, pool_next_obs, pool_capacity};
  if (!pool_ok(pool) || !idx_dev || batch <= 0 || !eps_next_dev || !log_alpha_dev || !partial_dev || !aligned4(partial_dev)) return CASSIE_EINVAL;
  if (!net_ok(actor) || !net_ok(target_qf1) || !net_ok(target_qf2) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  MLP32_LAUNCH(critic_grad_kernel, obs_dim, act_dim, blocks_for(batch), stream, pool, idx_dev, batch, net_of(actor), net_of(target_qf1), net_of(target_qf2), net_of(qf1),
               net_of(qf2), eps_next_dev, log_alpha_dev, discount, partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieSacActorGrad(const float* pool_obs, long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                       const float* const* qf1, const float* const* qf2, const float* eps_dev, const float* log_alpha_dev, float* partial_dev, void* stream) {
  using namespace cassie_sac;
  if (!pool_obs || pool_capacity <= 0 || !idx_dev || batch <= 0 || !eps_dev || !log_alpha_dev || !partial_dev || !aligned4(partial_dev)) return CASSIE_EINVAL;
  if (!net_ok(actor) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  const Pool pool{pool_obs, nullptr, nullptr, nullptr, nullptr, pool_capacity};
  MLP32_LAUNCH(actor_grad_kernel, obs_dim, act_dim, blocks_for(batch), stream, pool, idx_dev, batch, net_of(actor), net_of(qf1), net_of(qf2), eps_dev, log_alpha_dev,
               partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieSacApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* actor, float* m_dev, float* v_dev, int t, float lr,
                   float beta1, float beta2, float eps, float* log_alpha_dev, float* alpha_m_dev, float* alpha_v_dev, int alpha_t, float alpha_lr,
                   float target_entropy, double* stats_dev, void* stream) {
  using namespace cassie_sac;
  if (CassieSacParamCount(obs_dim, act_dim) == 0 || rows <= 0 || !partial_dev || !net_ok(actor) || !m_dev || !v_dev || t < 1 || !log_alpha_dev) return CASSIE_EINVAL;
  if (alpha_m_dev && (!alpha_v_dev || alpha_t < 1)) return CASSIE_EINVAL;
  Offsets off;
  actor_offsets(obs_dim, 2 * act_dim, off.o);
  hipLaunchKernelGGL(apply_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, partial_dev, scale, net_rw(actor), off, m_dev, v_dev,
                     adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, log_alpha_dev, alpha_m_dev, alpha_v_dev,
                     alpha_m_dev ? adam_step_size(alpha_lr, beta1, beta2, alpha_t) : 0.0f, target_entropy, stats_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
