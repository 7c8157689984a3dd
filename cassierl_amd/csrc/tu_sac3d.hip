// tu_sac3d.hip -- Soft Actor-Critic's fused kernels at the Cassie3d shape, 45 observations and 10 actions (include/cassie_trpo.h, "SAC at 45 x 10";
// cassierl_amd/sac.py with env="cassie3d").  The contracts, the algorithm and the order of one update -- five launches -- are tu_sac.hip's (read its
// header first); the networks are still the family's 32 x 32 ReLU networks.  What differs is the shape of the input and output layers, and
// mlp32_tiles3d.h holds what that needs: the twelve action slots, the two-headed output layer on image rows a and 16 + a, the merge layer's six
// k-steps, the 24 k-steps of the first layer and [gW1 | gb1] as two accumulator tiles.  This unit keeps what is SAC's: the squashed-Gaussian head,
// the cotangents of the actor kernel, the temperature's Adam step, the statistics and the entry points.  No kernel of tu_ddpg.hip, tu_sac.hip or
// tu_td3.hip is touched; CassieDdpgPoolCommit and CassieDdpgPartialRows are shape-free and are used as they are.
// Every sum runs in a fixed order: a launch repeats bit for bit.
#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "mlp32_tiles3d.h"

namespace cassie_sac3d {

using namespace cassie_mlp32_3d;

constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;

// one component of the squashed Gaussian (tu_sac.hip: squash)
__device__ __forceinline__ void squash(float mean, float ls_raw, float eps, float& act, float& logp, float& sde, bool& inside) {
  const float ls = fminf(fmaxf(ls_raw, LOG_STD_MIN), LOG_STD_MAX);
  inside = ls_raw >= LOG_STD_MIN && ls_raw <= LOG_STD_MAX;
  sde = expf(ls) * eps;
  const float u = mean + sde, m2u = -2.0f * u;
  act = tanh_fast(u);
  const float softplus = fmaxf(m2u, 0.0f) + log1pf(expf(-fabsf(m2u)));
  logp = (-0.5f * eps * eps - ls - 0.9189385332046727f) - 2.0f * (0.6931471805599453f - u - softplus);
}

// the actor (images at q0, rows sb[0 .. 2]) on the first-layer operand xb with the noise eps of the lane's slots: hidden activations a1, a2, the
// squashed action in the slots (0 in the dead ones), log pi of the sample (both lane halves hold it)
__device__ __forceinline__ void actor_sample3(const float4 (*wimg)[64], int q0, const float (*sb)[32], const float (&xb)[XS], const float (&eps)[NS], int lane, int h,
                                              v16f& a1, v16f& a2, float (&act)[NS], float (&sde)[NS], bool (&inside)[NS], float& logpi) {
  v16f z3;
  actor_forward3(wimg, q0, sb, xb, lane, h, a1, a2, z3);
  float lp = 0.0f;
#pragma unroll
  for (int v = 0; v < NS; v++) {
    float l;
    squash(z3[v], z3[v + 8], eps[v], act[v], l, sde[v], inside[v]);
    if (row_of(v, h) < A3) lp += l; else act[v] = 0.0f;
  }
  logpi = lp + __shfl_xor(lp, 32, 64);
}

// ---------------------------------------------------------------------------------------------------------------- critic gradients
// twin_critic_grad3 (mlp32_tiles3d.h) with  a' = pi(s'_i; eps[b])  and  sub = alpha log pi(a'|s'_i).
__global__ void __launch_bounds__(64 * WAVES, 1) critic_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net pi, Net tq1, Net tq2, Net q1, Net q2,
                                                                    const float* __restrict__ eps_next, const float* __restrict__ log_alpha, float gamma,
                                                                    float* __restrict__ partial) {
  const float alpha = expf(log_alpha[0]);
  const auto target = [=](const float4 (*wimg)[64], const float (*sb)[32], const float (&xn)[XS], const float (&en)[NS], int lane, int h, float (&an)[NS]) {
    v16f a1, a2;
    float sde[NS], logpi;
    bool inside[NS];
    actor_sample3(wimg, TC3_PI, sb, xn, en, lane, h, a1, a2, an, sde, inside, logpi);
    return alpha * logpi;
  };
  twin_critic_grad3(pool, idx, n, pi, K3_HEAD, tq1, tq2, q1, q2, eps_next, gamma, partial, target);
}

// ---------------------------------------------------------------------------------------------------------------- actor gradient
// tu_sac.hip's actor_grad_kernel at this shape.  Row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum log pi | sum min Q].
enum { AG3_PI = 0, AG3_W2T = LA3_N, AG3_W3T = AG3_W2T + 4, AG3_Q1 = AG3_W3T + 4, AQ3_DA = LQ3_FWD, AQ3_N = AQ3_DA + 4, AG3_Q2 = AG3_Q1 + AQ3_N, AG3_N = AG3_Q2 + AQ3_N };
__global__ void __launch_bounds__(64 * WAVES, 1) actor_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net th, Net q1, Net q2,
                                                                   const float* __restrict__ eps_dev, const float* __restrict__ log_alpha, float* __restrict__ partial) {
  typedef Shape<D3, A3, 2 * A3> S;
  constexpr int NROW = S::NPA + 2, TILES = WAVES * 2 * 32 * TP;
  __shared__ alignas(16) float tilemem[TILES > WAVES * NROW ? TILES : WAVES * NROW];
  __shared__ alignas(16) float sbias[9][32];   // actor b1 b2 b3;  critics b1 b2 W3 each
  __shared__ float4 wimg[AG3_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = head_bias3(th.b3, tid);
    sbias[3][tid] = q1.b1[tid]; sbias[4][tid] = q1.b2[tid]; sbias[5][tid] = q1.W3[tid];
    sbias[6][tid] = q2.b1[tid]; sbias[7][tid] = q2.b2[tid]; sbias[8][tid] = q2.W3[tid];
  }
  {
    const Grp g[13] = {{K_FIRST, th.W1, AG3_PI + LA3_W1, 6}, {K_HID, th.W2, AG3_PI + LA3_W2, 4}, {K3_HEAD, th.W3, AG3_PI + LA3_W3, 4}, {K_HIDT, th.W2, AG3_W2T, 4},
                       {K3_HEADT, th.W3, AG3_W3T, 4},
                       {K_FIRST, q1.W1, AG3_Q1 + LQ3_W1, 6}, {K_HIDQ, q1.W2, AG3_Q1 + LQ3_W2, 4}, {K3_ACTIN, q1.W2, AG3_Q1 + LQ3_A, 2}, {K_DA, q1.W2, AG3_Q1 + AQ3_DA, 4},
                       {K_FIRST, q2.W1, AG3_Q2 + LQ3_W1, 6}, {K_HIDQ, q2.W2, AG3_Q2 + LQ3_W2, 4}, {K3_ACTIN, q2.W2, AG3_Q2 + LQ3_A, 2}, {K_DA, q2.W2, AG3_Q2 + AQ3_DA, 4}};
    fill_images3(wimg, g, wave, lane);
  }
  const float b3q1 = q1.b3[0], b3q2 = q2.b3[0], alpha = expf(log_alpha[0]);
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  ActorAcc3 acc;
  zero(acc);
  float slp = 0.0f, sq = 0.0f;
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    Tile3 t;
    gather3<false>(pool, idx, n, tl, c, h, t);
    float ep[NS];
    action_slots(eps_dev, t.smp, t.valid, h, ep);
    // ---- actor forward: a~ = tanh(mean + exp(log_std) eps) in the slots
    v16f a1, a2;
    float act[NS], sde[NS], logpi, aw[16];
    bool inside[NS];
    actor_sample3(wimg, AG3_PI, sbias, t.xb, ep, lane, h, a1, a2, act, sde, inside, logpi);
    // ---- both critics at (s, a~);  d min(Q1, Q2) / da = W2a' (W3 o (h2 > 0)) of the smaller one, action a in register v of its slot
    v16f da = zero16();
    float qmin;
    {
      v16f c1, h2a, h2b;
      float wa[16], wb[16];
      w3_row(sbias[5], h, wa); w3_row(sbias[8], h, wb);
      const float qa = critic_forward3(wimg, AG3_Q1, sbias + 3, wa, b3q1, t.xb, act, lane, h, c1, h2a);
      const float qb = critic_forward3(wimg, AG3_Q2, sbias + 6, wb, b3q2, t.xb, act, lane, h, c1, h2b);
      const bool first = qa <= qb;
      qmin = first ? qa : qb;
      aop(wimg, AG3_Q1 + AQ3_DA, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], (first && h2a[v] > 0.0f) ? wa[v] : 0.0f, da);
      aop(wimg, AG3_Q2 + AQ3_DA, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], (!first && h2b[v] > 0.0f) ? wb[v] : 0.0f, da);
    }
    if (h == 0 && t.valid) { slp += logpi; sq += qmin; }
    // cotangents of alpha log pi - min Q on the output layer: d/du = 2 alpha a~ - dQ/da (1 - a~^2) on the mean row, that times
    // exp(log_std) eps, minus alpha, on the log_std row (nothing where the clamp is active)
    v16f wt = zero16();
#pragma unroll
    for (int v = 0; v < NS; v++) {
      const bool on = t.valid && row_of(v, h) < A3;
      const float du = 2.0f * alpha * act[v] - da[v] * (1.0f - act[v] * act[v]);
      wt[v] = on ? du : 0.0f;
      wt[v + 8] = (on && inside[v]) ? du * sde[v] - alpha : 0.0f;
    }
    actor_reverse3(wimg, AG3_W2T, AG3_W3T, a1, a2, wt, t, t0, t1, lane, c, h, acc);
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) { slp += __shfl_xor(slp, m, 64); sq += __shfl_xor(sq, m, 64); }
  __syncthreads();
  float* red = tilemem + wave * NROW;
  actor_row3(acc, red, c, h);
  if (lane == 0) { red[S::NPA] = slp; red[S::NPA + 1] = sq; }
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- apply
// a critic: apply_rows (mlp32_tiles.h), as tu_ddpg.hip's apply_kernel
__global__ void __launch_bounds__(1024) critic_apply_kernel(int rows, const float* __restrict__ partial, float scale, NetRW live, NetRW targ, Offsets off,
                                                            float* __restrict__ m, float* __restrict__ v, float a, float beta1, float beta2, float eps, float tau,
                                                            double* __restrict__ stats) {
  apply_rows(rows, 2, partial, scale, live, targ, off.o, m, v, a, beta1, beta2, eps, tau, stats);
}
// the actor and the temperature: tu_sac.hip's apply_kernel from the same pieces (which keep contraction off)
__global__ void __launch_bounds__(1024) actor_apply_kernel(int rows, const float* __restrict__ partial, float scale, NetRW live, Offsets off, float* __restrict__ m,
                                                           float* __restrict__ v, float a, float beta1, float beta2, float eps, float* __restrict__ log_alpha,
                                                           float* __restrict__ alpha_m, float* __restrict__ alpha_v, float a_alpha, float target_entropy,
                                                           double* __restrict__ stats) {
  constexpr int NS2 = 2;
  const int np = off.o[6], stride = np + NS2;
  if ((int)threadIdx.x <= NS2 && stats) {   // (sum log pi, sum min Q, the summed actor loss at the temperature BEFORE its step)
    double s[NS2] = {0.0, 0.0};
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
// mlp32_tiles.h's policy_step at this shape with the squashed-Gaussian head.  One tile per wavefront; rows past n are not touched.
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ noise,
                                                                    const double* __restrict__ low, const double* __restrict__ high, float* __restrict__ obs32,
                                                                    float* __restrict__ act, double* __restrict__ env_act) {
  constexpr int D = D3, A = A3;
  __shared__ alignas(16) float sbias[3][32];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) { sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = head_bias3(th.b3, tid); }
  float aW1[XS], aW2[16], aW3[16];
#pragma unroll
  for (int s = 0; s < XS; s++) aW1[s] = wel3(K_FIRST, th.W1, s, c, h);
#pragma unroll
  for (int v = 0; v < 16; v++) { aW2[v] = wel3(K_HID, th.W2, v, c, h); aW3[v] = wel3(K3_HEAD, th.W3, v, c, h); }
  __syncthreads();
  const int smp = (blockIdx.x * WAVES + wave) * 32 + c;
  const bool valid = smp < n;
  float xb[XS];
#pragma unroll
  for (int s = 0; s < XS; s++) {
    const int k = 2 * s + h;
    const bool on = valid && k < D;
    xb[s] = on ? (float)obs[(size_t)smp * D + k] : 0.0f;
    if (on) obs32[(size_t)smp * D + k] = xb[s];
  }
  v16f h1 = bias_tile(sbias[0], h);
#pragma unroll
  for (int s = 0; s < XS; s++) h1 = TILE_MFMA(aW1[s], xb[s], h1);
  relu16(h1);
  v16f h2 = bias_tile(sbias[1], h);
#pragma unroll
  for (int v = 0; v < 16; v++) h2 = TILE_MFMA(aW2[v], h1[v], h2);
  relu16(h2);
  v16f z3 = bias_tile(sbias[2], h);
#pragma unroll
  for (int v = 0; v < 16; v++) z3 = TILE_MFMA(aW3[v], h2[v], z3);
#pragma unroll
  for (int v = 0; v < NS; v++) {
    const int a = row_of(v, h);
    if (valid && a < A) {
      const size_t o = (size_t)smp * A + a;
      const float ls = fminf(fmaxf(z3[v + 8], LOG_STD_MIN), LOG_STD_MAX);
      const float val = tanh_fast(z3[v] + expf(ls) * noise[o]);
      act[o] = val;
      const double lo = low[a], hi = high[a];
      double e = lo + ((double)val + 1.0) * 0.5 * (hi - lo);
      e = e < lo ? lo : (e > hi ? hi : e);
      env_act[o] = e;
    }
  }
}

}  // namespace cassie_sac3d

extern "C" {

int CassieSac3dParamCount(int obs_dim, int act_dim, int which) {
  typedef cassie_mlp32::Shape<cassie_mlp32_3d::D3, cassie_mlp32_3d::A3, 2 * cassie_mlp32_3d::A3> S;
  if (!cassie_mlp32_3d::shape_ok3(obs_dim, act_dim)) return 0;
  return which == CASSIE_DDPG_ACTOR ? S::NPA : (which == CASSIE_DDPG_CRITIC ? S::NPQ : 0);
}

int CassieSac3dPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, const double* low_dev,
                          const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream) {
  using namespace cassie_sac3d;
  if (!shape_ok3(obs_dim, act_dim) || !obs_dev || n <= 0 || !net_ok(actor) || !noise_dev || !low_dev || !high_dev || !pool_obs_row_dev || !pool_act_row_dev ||
      !env_actions_dev)
    return CASSIE_EINVAL;
  if (!aligned4(noise_dev) || !aligned4(pool_obs_row_dev) || !aligned4(pool_act_row_dev) || ((uintptr_t)obs_dev & 7) || ((uintptr_t)env_actions_dev & 7) ||
      ((uintptr_t)low_dev & 7) || ((uintptr_t)high_dev & 7))
    return CASSIE_EINVAL;
  hipLaunchKernelGGL(policy_step_kernel, dim3(policy_step_grid(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, net_of(actor), noise_dev, low_dev, high_dev,
                     pool_obs_row_dev, pool_act_row_dev, env_actions_dev);
  return launched();
}

int CassieSac3dCriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                          long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                          const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                          const float* eps_next_dev, const float* log_alpha_dev, float discount, float* partial_dev, void* stream) {
  using namespace cassie_sac3d;
  const Pool pool{pool_obs, pool_act, pool_rew, pool_term, pool_next_obs, pool_capacity};
  if (!shape_ok3(obs_dim, act_dim) || !pool_ok(pool) || !idx_dev || batch <= 0 || !eps_next_dev || !log_alpha_dev || !partial_dev) return CASSIE_EINVAL;
  if (!aligned4(partial_dev) || !aligned4(eps_next_dev) || !aligned4(log_alpha_dev) || ((uintptr_t)idx_dev & 7)) return CASSIE_EINVAL;
  if (!net_ok(actor) || !net_ok(target_qf1) || !net_ok(target_qf2) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  hipLaunchKernelGGL(critic_grad_kernel, dim3(blocks_for(batch)), dim3(64 * WAVES), 0, (hipStream_t)stream, pool, idx_dev, batch, net_of(actor), net_of(target_qf1),
                     net_of(target_qf2), net_of(qf1), net_of(qf2), eps_next_dev, log_alpha_dev, discount, partial_dev);
  return launched();
}

int CassieSac3dActorGrad(const float* pool_obs, long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                         const float* const* qf1, const float* const* qf2, const float* eps_dev, const float* log_alpha_dev, float* partial_dev, void* stream) {
  using namespace cassie_sac3d;
  if (!shape_ok3(obs_dim, act_dim) || !pool_obs || pool_capacity <= 0 || !idx_dev || batch <= 0 || !eps_dev || !log_alpha_dev || !partial_dev) return CASSIE_EINVAL;
  if (!aligned4(partial_dev) || !aligned4(eps_dev) || !aligned4(log_alpha_dev) || ((uintptr_t)idx_dev & 7)) return CASSIE_EINVAL;
  if (!net_ok(actor) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  const Pool pool{pool_obs, nullptr, nullptr, nullptr, nullptr, pool_capacity};
  hipLaunchKernelGGL(actor_grad_kernel, dim3(blocks_for(batch)), dim3(64 * WAVES), 0, (hipStream_t)stream, pool, idx_dev, batch, net_of(actor), net_of(qf1), net_of(qf2),
                     eps_dev, log_alpha_dev, partial_dev);
  return launched();
}

int CassieSac3dCriticApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* live, float* const* target, float* m_dev,
                           float* v_dev, int t, float lr, float beta1, float beta2, float eps, float tau, double* stats_dev, void* stream) {
  using namespace cassie_sac3d;
  if (!shape_ok3(obs_dim, act_dim) || rows <= 0 || !partial_dev || !aligned4(partial_dev) || !net_ok(live) || !net_ok(target) || !m_dev || !v_dev || t < 1)
    return CASSIE_EINVAL;
  Offsets off;
  critic_offsets(obs_dim, act_dim, off.o);
  hipLaunchKernelGGL(critic_apply_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, partial_dev, scale, net_rw(live), net_rw(target), off, m_dev, v_dev,
                     adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, tau, stats_dev);
  return launched();
}

int CassieSac3dActorApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* actor, float* m_dev, float* v_dev, int t, float lr,
                          float beta1, float beta2, float eps, float* log_alpha_dev, float* alpha_m_dev, float* alpha_v_dev, int alpha_t, float alpha_lr,
                          float target_entropy, double* stats_dev, void* stream) {
  using namespace cassie_sac3d;
  if (!shape_ok3(obs_dim, act_dim) || rows <= 0 || !partial_dev || !aligned4(partial_dev) || !net_ok(actor) || !m_dev || !v_dev || t < 1 || !log_alpha_dev)
    return CASSIE_EINVAL;
  if (alpha_m_dev && (!alpha_v_dev || alpha_t < 1)) return CASSIE_EINVAL;
  Offsets off;
  actor_offsets(obs_dim, 2 * act_dim, off.o);
  hipLaunchKernelGGL(actor_apply_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, partial_dev, scale, net_rw(actor), off, m_dev, v_dev,
                     adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, log_alpha_dev, alpha_m_dev, alpha_v_dev,
                     alpha_m_dev ? adam_step_size(alpha_lr, beta1, beta2, alpha_t) : 0.0f, target_entropy, stats_dev);
  return launched();
}

}  // extern "C"
