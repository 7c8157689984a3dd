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
//     has its own block [rows][NPq + 2] of the partial tensor, which is CassieDdpgApply's row format.
// Every sum runs in a fixed order: a launch repeats bit for bit.
#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "mlp32_tiles.h"

namespace cassie_sac {

using namespace cassie_mlp32;

constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;

template <int D, int A> struct ActorShape {   // actor row [W1 | b1 | W2 | b2 | W3 | b3] with the 2 A output rows
  static constexpr int A2 = 2 * A;
  static constexpr int NPA = H * D + H + H * H + H + A2 * H + A2;
  static constexpr int A_W1 = 0, A_B1 = H * D, A_W2 = A_B1 + H, A_B2 = A_W2 + H * H, A_W3 = A_B2 + H, A_B3 = A_W3 + A2 * H;
};

// b3 on the image rows of the output tile (mlp32_tiles.h: head_row, K_HEAD, K_HEADT)
template <int A> __device__ __forceinline__ float head_bias(const float* b3, int i) { const int r = head_row<A>(i); return r >= 0 ? b3[r] : 0.0f; }

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

// the actor on the first-layer operand xb with the noise eps [4] of the lane's actions a = v + 4 h: hidden activations a1, a2, the
// squashed action act [4] (0 for a >= A), log pi of the sample (both lane halves hold it)
template <int A, int KS1>
__device__ __forceinline__ void actor_sample(const float4 (*wimg)[64], int qW1, int qW2, int qW3, const float* sb1, const float* sb2, const float* sb3,
                                             const float (&xb)[KS1], const float (&eps)[4], int lane, int h, v16f& a1, v16f& a2, float (&act)[4],
                                             float (&sde)[4], bool (&inside)[4], float& logpi) {
  two_layers<KS1>(wimg, qW1, qW2, sb1, sb2, xb, lane, h, a1, a2);
  relu16(a2);
  float aw[16];
  v16f z3 = bias_tile(sb3, h);
  aop(wimg, qW3, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) z3 = TILE_MFMA(aw[v], a2[v], z3);
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
// Per sample b (pool row i = idx[b]):  a' = pi(s'_i; eps[b]),  y = r_i + (1 - terminal_i) gamma (min(Q1', Q2')(s'_i, a') - alpha log pi(a'|s'_i)),
// e_k = Q_k(s_i, a_i) - y, and the gradient of sum_b e_k^2 with respect to live critic k.  Block k of partial: [rows][gW1 | gb1 | gW2 | gb2 |
// gW3 | gb3 | sum e_k^2 | sum Q_k].
// CriticAcc, critic_step and critic_row (the live critic's forward and reverse pass on a tile, its row of partial sums) are mlp32_tiles.h's.
enum { CQ_PI_W1 = 0, CQ_PI_W2 = 4, CQ_PI_W3 = 8, CQ_T1_W1 = 12, CQ_T1_W2 = 16, CQ_T1_A = 20, CQ_T2_W1 = 21, CQ_T2_W2 = 25, CQ_T2_A = 29, CQ_Q1 = 30, CQ_Q2 = CQ_Q1 + LQ_N,
       CQ_N = CQ_Q2 + LQ_N };
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) critic_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net pi, Net tq1, Net tq2, Net q1, Net q2,
                                                                    const float* __restrict__ eps_next, const float* __restrict__ log_alpha, float gamma,
                                                                    float* __restrict__ partial) {
  typedef Shape<D, A> S;
  static_assert(D < 32 && A <= 8, "a column of ones next to the observations; mean and log_std of an action in registers v and v + 4 of one lane");
  constexpr int KS1 = (D + 1) / 2, NROW = S::NPQ + 2;
  static_assert(WAVES * NROW <= WAVES * 2 * 32 * TP, "the workgroup's reduction re-uses the transpose tiles");
  __shared__ alignas(16) float tilemem[WAVES * 2 * 32 * TP];
  __shared__ alignas(16) float sbias[15][32];   // actor b1 b2 b3;  target critics b1 b2 W3 each;  live critics b1 b2 W3 each
  __shared__ float4 wimg[CQ_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = pi.b1[tid]; sbias[1][tid] = pi.b2[tid]; sbias[2][tid] = head_bias<A>(pi.b3, tid);
    sbias[3][tid] = tq1.b1[tid]; sbias[4][tid] = tq1.b2[tid]; sbias[5][tid] = tq1.W3[tid];
    sbias[6][tid] = tq2.b1[tid]; sbias[7][tid] = tq2.b2[tid]; sbias[8][tid] = tq2.W3[tid];
    sbias[9][tid] = q1.b1[tid]; sbias[10][tid] = q1.b2[tid]; sbias[11][tid] = q1.W3[tid];
    sbias[12][tid] = q2.b1[tid]; sbias[13][tid] = q2.b2[tid]; sbias[14][tid] = q2.W3[tid];
  }
  {
    const Grp g[17] = {{K_FIRST, pi.W1, CQ_PI_W1, 4}, {K_HID, pi.W2, CQ_PI_W2, 4}, {K_HEAD, pi.W3, CQ_PI_W3, 4},
                       {K_FIRST, tq1.W1, CQ_T1_W1, 4}, {K_HIDQ, tq1.W2, CQ_T1_W2, 4}, {K_ACTIN, tq1.W2, CQ_T1_A, 1},
                       {K_FIRST, tq2.W1, CQ_T2_W1, 4}, {K_HIDQ, tq2.W2, CQ_T2_W2, 4}, {K_ACTIN, tq2.W2, CQ_T2_A, 1},
                       {K_FIRST, q1.W1, CQ_Q1 + LQ_W1, 4}, {K_HIDQ, q1.W2, CQ_Q1 + LQ_W2, 4}, {K_ACTIN, q1.W2, CQ_Q1 + LQ_A, 1}, {K_HIDQT, q1.W2, CQ_Q1 + LQ_W2T, 4},
                       {K_FIRST, q2.W1, CQ_Q2 + LQ_W1, 4}, {K_HIDQ, q2.W2, CQ_Q2 + LQ_W2, 4}, {K_ACTIN, q2.W2, CQ_Q2 + LQ_A, 1}, {K_HIDQT, q2.W2, CQ_Q2 + LQ_W2T, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  const float b3t1 = tq1.b3[0], b3t2 = tq2.b3[0], b3q1 = q1.b3[0], b3q2 = q2.b3[0], alpha = expf(log_alpha[0]);
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
    // ---- target: min(Q1', Q2')(s', a') - alpha log pi(a'|s')
    float y;
    {
      v16f a1, a2, u1, u2;
      float an[4], sde[4], logpi, w3a[16];
      bool inside[4];
      actor_sample<A, KS1>(wimg, CQ_PI_W1, CQ_PI_W2, CQ_PI_W3, sbias[0], sbias[1], sbias[2], xn, en, lane, h, a1, a2, an, sde, inside, logpi);
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
      y = rew + live * gamma * (fminf(qt1, qt2) - alpha * logpi);
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

// ---------------------------------------------------------------------------------------------------------------- actor gradient
// Gradient of sum_b (alpha log pi(a~_b|s_b) - min(Q1, Q2)(s_b, a~_b)), a~ = pi(s; eps), with respect to the actor, through the live critics.
// Row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum log pi | sum min Q].
enum { AQ_W1 = 0, AQ_W2 = 4, AQ_A = 8, AQ_DA = 9, AQ_N = 13 };   // a critic's images in the actor kernel
enum { AG_W1 = 0, AG_W2 = 4, AG_W3 = 8, AG_W2T = 12, AG_W3T = 16, AG_Q1 = 18, AG_Q2 = AG_Q1 + AQ_N, AG_N = AG_Q2 + AQ_N };
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) actor_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net th, Net q1, Net q2,
                                                                   const float* __restrict__ eps_dev, const float* __restrict__ log_alpha, float* __restrict__ partial) {
  typedef ActorShape<D, A> S;
  static_assert(D < 32 && A <= 8, "see critic_grad_kernel");
  constexpr int KS1 = (D + 1) / 2, NROW = S::NPA + 2, TILES = WAVES * 2 * 32 * TP;
  // the workgroup's reduction re-uses the transpose tiles; with D = 26 the four rows of 2 A output rows are a little longer than the tiles
  __shared__ alignas(16) float tilemem[TILES > WAVES * NROW ? TILES : WAVES * NROW];
  __shared__ alignas(16) float sbias[9][32];   // actor b1 b2 b3;  critics b1 b2 W3 each
  __shared__ float4 wimg[AG_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = head_bias<A>(th.b3, tid);
    sbias[3][tid] = q1.b1[tid]; sbias[4][tid] = q1.b2[tid]; sbias[5][tid] = q1.W3[tid];
    sbias[6][tid] = q2.b1[tid]; sbias[7][tid] = q2.b2[tid]; sbias[8][tid] = q2.W3[tid];
  }
  {
    const Grp g[13] = {{K_FIRST, th.W1, AG_W1, 4}, {K_HID, th.W2, AG_W2, 4}, {K_HEAD, th.W3, AG_W3, 4}, {K_HIDT, th.W2, AG_W2T, 4}, {K_HEADT, th.W3, AG_W3T, 2},
                       {K_FIRST, q1.W1, AG_Q1 + AQ_W1, 4}, {K_HIDQ, q1.W2, AG_Q1 + AQ_W2, 4}, {K_ACTIN, q1.W2, AG_Q1 + AQ_A, 1}, {K_DA, q1.W2, AG_Q1 + AQ_DA, 4},
                       {K_FIRST, q2.W1, AG_Q2 + AQ_W1, 4}, {K_HIDQ, q2.W2, AG_Q2 + AQ_W2, 4}, {K_ACTIN, q2.W2, AG_Q2 + AQ_A, 1}, {K_DA, q2.W2, AG_Q2 + AQ_DA, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  const float b3q1 = q1.b3[0], b3q2 = q2.b3[0], alpha = expf(log_alpha[0]);
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  v16f gW1, gW2, gW3;
#pragma unroll
  for (int v = 0; v < 16; v++) { gW1[v] = 0.0f; gW2[v] = 0.0f; gW3[v] = 0.0f; }
  float gb2 = 0.0f, gb3 = 0.0f, slp = 0.0f, sq = 0.0f;
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    const int s0 = tl * 32, smp = s0 + c;
    const bool valid = smp < n;
    const long long gi = valid ? clamp_row(idx[smp], pool.cap) : 0;
    float xb[KS1], xt[16], ep[4];
#pragma unroll
    for (int s = 0; s < KS1; s++) { const int k = 2 * s + h; xb[s] = (valid && k < D) ? pool.obs[gi * D + k] : 0.0f; }
#pragma unroll
    for (int v = 0; v < 4; v++) ep[v] = (valid && v + 4 * h < A) ? eps_dev[(size_t)smp * A + v + 4 * h] : 0.0f;
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int sm = s0 + 16 * h + s;
      const bool on = sm < n;
      const long long gs = on ? clamp_row(idx[sm], pool.cap) : 0;
      xt[s] = c < D ? (on ? pool.obs[gs * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f);
    }
    // ---- actor forward: a~ = tanh(mean + exp(log_std) eps), action a = v + 4 h in register v < 4
    v16f a1, a2;
    float act[4], sde[4], logpi, aw[16];
    bool inside[4];
    actor_sample<A, KS1>(wimg, AG_W1, AG_W2, AG_W3, sbias[0], sbias[1], sbias[2], xb, ep, lane, h, a1, a2, act, sde, inside, logpi);
    // ---- both critics at (s, a~);  d min(Q1, Q2) / da = W2a' (W3 o (h2 > 0)) of the smaller one
    v16f da;
#pragma unroll
    for (int v = 0; v < 16; v++) da[v] = 0.0f;
    float qmin;
    {
      v16f c1, h2a, h2b;
      two_layers<KS1>(wimg, AG_Q1 + AQ_W1, AG_Q1 + AQ_W2, sbias[3], sbias[4], xb, lane, h, c1, h2a);
      add_action(wimg, AG_Q1 + AQ_A, lane, act, h2a);
      relu16(h2a);
      two_layers<KS1>(wimg, AG_Q2 + AQ_W1, AG_Q2 + AQ_W2, sbias[6], sbias[7], xb, lane, h, c1, h2b);
      add_action(wimg, AG_Q2 + AQ_A, lane, act, h2b);
      relu16(h2b);
      const v16f w3a = bias_tile(sbias[5], h), w3b = bias_tile(sbias[8], h);
      float wa[16], wb[16];
#pragma unroll
      for (int v = 0; v < 16; v++) { wa[v] = w3a[v]; wb[v] = w3b[v]; }
      const float qa = q_head(wa, b3q1, h2a), qb = q_head(wb, b3q2, h2b);
      const bool first = qa <= qb;
      qmin = first ? qa : qb;
      aop(wimg, AG_Q1 + AQ_DA, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], (first && h2a[v] > 0.0f) ? wa[v] : 0.0f, da);
      aop(wimg, AG_Q2 + AQ_DA, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], (!first && h2b[v] > 0.0f) ? wb[v] : 0.0f, da);
    }
    if (h == 0 && valid) { slp += logpi; sq += qmin; }
    // cotangents of alpha log pi - min Q on the output layer: d/du = 2 alpha a~ - dQ/da (1 - a~^2) on the mean row, that times
    // exp(log_std) eps, minus alpha, on the log_std row (nothing where the clamp is active)
    v16f wt;
#pragma unroll
    for (int v = 0; v < 16; v++) wt[v] = 0.0f;
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const bool on = valid && v + 4 * h < A;
      const float du = 2.0f * alpha * act[v] - da[v] * (1.0f - act[v] * act[v]);
      wt[v] = on ? du : 0.0f;
      wt[v + 4] = (on && inside[v]) ? du * sde[v] - alpha : 0.0f;
    }
    // ---- the actor's reverse pass (tu_ddpg.hip's, with two quads of output rows)
    v16f g2, g1;
#pragma unroll
    for (int v = 0; v < 16; v++) { g2[v] = 0.0f; g1[v] = 0.0f; }
    {
      const float4 w = wimg[AG_W3T][lane], x = wimg[AG_W3T + 1][lane];
      g2 = TILE_MFMA(w.x, wt[0], g2); g2 = TILE_MFMA(w.y, wt[1], g2); g2 = TILE_MFMA(w.z, wt[2], g2); g2 = TILE_MFMA(w.w, wt[3], g2);
      g2 = TILE_MFMA(x.x, wt[4], g2); g2 = TILE_MFMA(x.y, wt[5], g2); g2 = TILE_MFMA(x.z, wt[6], g2); g2 = TILE_MFMA(x.w, wt[7], g2);
    }
#pragma unroll
    for (int v = 0; v < 16; v++) g2[v] = a2[v] > 0.0f ? g2[v] : 0.0f;
    aop(wimg, AG_W2T, lane, aw);
#pragma unroll
    for (int v = 0; v < 16; v++) g1 = TILE_MFMA(aw[v], g2[v], g1);
#pragma unroll
    for (int v = 0; v < 16; v++) g1[v] = a1[v] > 0.0f ? g1[v] : 0.0f;
    float ta_[16], tb_[16];
    put(t0, g2, c, h); put(t1, a1, c, h);
    wave_lds_sync();
    get(t0, ta_, c, h); get(t1, tb_, c, h);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; s++) { gW2 = TILE_MFMA(ta_[s], tb_[s], gW2); gb2 += ta_[s]; }
    put(t0, g1, c, h);
    wave_lds_sync();
    get(t0, ta_, c, h);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; s++) gW1 = TILE_MFMA(ta_[s], xt[s], gW1);
    put(t0, wt, c, h); put(t1, a2, c, h);
    wave_lds_sync();
    get(t0, ta_, c, h); get(t1, tb_, c, h);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; s++) { gW3 = TILE_MFMA(ta_[s], tb_[s], gW3); gb3 += ta_[s]; }
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) { slp += __shfl_xor(slp, m, 64); sq += __shfl_xor(sq, m, 64); }
  gb2 += __shfl_xor(gb2, 32, 64); gb3 += __shfl_xor(gb3, 32, 64);
  __syncthreads();
  float* red = tilemem + wave * NROW;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h), hr = head_row<A>(r);
    red[S::A_W2 + r * H + c] = gW2[v];
    if (c < D) red[S::A_W1 + r * D + c] = gW1[v];
    if (c == D) red[S::A_B1 + r] = gW1[v];
    if (hr >= 0) red[S::A_W3 + hr * H + c] = gW3[v];
  }
  if (h == 0) red[S::A_B2 + c] = gb2;
  if (h == 0 && head_row<A>(c) >= 0) red[S::A_B3 + head_row<A>(c)] = gb3;
  if (lane == 0) { red[S::NPA] = slp; red[S::NPA + 1] = sq; }
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- apply (actor, temperature)
// tu_ddpg.hip's apply_kernel without a target network; the thread behind the last parameter takes log_alpha's Adam step on the gradient
// -(scale * sum log pi + target_entropy), the log pi column added in row order (alpha_m == NULL: the temperature is fixed).
struct Offsets { int o[7]; };
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
  for (int i = threadIdx.x; i <= np; i += 1024) {
    if (i == np && !alpha_m) break;
    float g = 0.0f;
    const float* p = partial + i;
    int r = 0;
    for (; r + 8 <= rows; r += 8) {   // eight loads in flight, added in row order
      float x[8];
#pragma unroll
      for (int k = 0; k < 8; k++) x[k] = p[(size_t)(r + k) * stride];
#pragma unroll
      for (int k = 0; k < 8; k++) g += x[k];
    }
    for (; r < rows; r++) g += p[(size_t)r * stride];
    g *= scale;
    float *th, *mi_, *vi_;
    float step = a;
    if (i == np) { th = log_alpha; mi_ = alpha_m; vi_ = alpha_v; step = a_alpha; g = -(g + target_entropy); }
    else {
      mi_ = m + i; vi_ = v + i;
      if (i < off.o[1]) th = live.W1 + (i - off.o[0]);
      else if (i < off.o[2]) th = live.b1 + (i - off.o[1]);
      else if (i < off.o[3]) th = live.W2 + (i - off.o[2]);
      else if (i < off.o[4]) th = live.b2 + (i - off.o[3]);
      else if (i < off.o[5]) th = live.W3 + (i - off.o[4]);
      else th = live.b3 + (i - off.o[5]);
    }
    const float mi = beta1 * *mi_ + (1.0f - beta1) * g;
    const float vi = beta2 * *vi_ + (1.0f - beta2) * (g * g);
    *mi_ = mi; *vi_ = vi;
    *th = *th - step * mi / (sqrtf(vi) + eps);
  }
}

// ---------------------------------------------------------------------------------------------------------------- policy step
// tu_ddpg.hip's policy_step_kernel with the squashed-Gaussian head: act = tanh(mean + exp(clamp(log_std)) noise).  obs32 and act are the pool's
// rows [top, top + n) (the caller passes the offset pointers).
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ noise,
                                                                    const double* __restrict__ low, const double* __restrict__ high, float* __restrict__ obs32,
                                                                    float* __restrict__ act, double* __restrict__ env_act) {
  constexpr int KS1 = (D + 1) / 2;
  __shared__ alignas(16) float sbias[3][32];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) { sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = head_bias<A>(th.b3, tid); }
  float aW1[KS1], aW2[16], aW3[16];
  double lo[4], hi[4];
#pragma unroll
  for (int s = 0; s < KS1; s++) aW1[s] = wel<D, A>(K_FIRST, th.W1, s, c, h);
#pragma unroll
  for (int v = 0; v < 16; v++) { aW2[v] = wel<D, A>(K_HID, th.W2, v, c, h); aW3[v] = wel<D, A>(K_HEAD, th.W3, v, c, h); }
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
      const float ls = fminf(fmaxf(z3[v + 4], LOG_STD_MIN), LOG_STD_MAX);
      const float val = tanh_fast(z3[v] + expf(ls) * noise[o]);   // in [-1, 1] by construction
      act[o] = val;
      double e = lo[v] + ((double)val + 1.0) * 0.5 * (hi[v] - lo[v]);
      e = e < lo[v] ? lo[v] : (e > hi[v] ? hi[v] : e);
      env_act[o] = e;
    }
  }
}

}  // namespace cassie_sac

extern "C" {

int CassieSacParamCount(int obs_dim, int act_dim) {
  if (!cassie_sac::shape_ok(obs_dim, act_dim)) return 0;
  return 32 * obs_dim + 32 + 32 * 32 + 32 + 2 * act_dim * 32 + 2 * act_dim;
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
