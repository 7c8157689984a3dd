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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "mlp32_tiles.h"

namespace cassie_ddpg {

using namespace cassie_mlp32;   // shapes, operand images, tile helpers (shared with tu_sac.hip)

// ---------------------------------------------------------------------------------------------------------------- critic gradient
// Per sample b of the batch (pool row i = idx[b]):  y = r_i + (1 - terminal_i) gamma Q'(s'_i, mu'(s'_i)),  e = Q(s_i, a_i) - y, and the
// gradient of sum_b e^2 with respect to the live critic.  Row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum e^2 | sum Q].
enum { CQ_TA_W1 = 0, CQ_TA_W2 = 4, CQ_TA_W3 = 8, CQ_TQ_W1 = 12, CQ_TQ_W2 = 16, CQ_TQ_A = 20, CQ_Q_W1 = 21, CQ_Q_W2 = 25, CQ_Q_A = 29, CQ_Q_W2T = 30, CQ_N = 34 };
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) critic_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net ta, Net tq, Net q, float gamma,
                                                                    float* __restrict__ partial) {
  typedef Shape<D, A> S;
  static_assert(D < 32 && A <= 8, "a column of ones next to the observations; the action rows in registers 0..3 of the two lane halves");
  constexpr int KS1 = (D + 1) / 2, NROW = S::NPQ + 2;
  static_assert(WAVES * NROW <= WAVES * 2 * 32 * TP, "the workgroup's reduction re-uses the transpose tiles");
  __shared__ alignas(16) float tilemem[WAVES * 2 * 32 * TP];
  __shared__ alignas(16) float sbias[7][32];   // target actor b1 b2 b3, target critic b1 b2, live critic b1 b2
  __shared__ float4 wimg[CQ_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = ta.b1[tid]; sbias[1][tid] = ta.b2[tid]; sbias[2][tid] = tid < A ? ta.b3[tid] : 0.0f;
    sbias[3][tid] = tq.b1[tid]; sbias[4][tid] = tq.b2[tid]; sbias[5][tid] = q.b1[tid]; sbias[6][tid] = q.b2[tid];
  }
  {
    const Grp g[10] = {{K_FIRST, ta.W1, CQ_TA_W1, 4}, {K_HID, ta.W2, CQ_TA_W2, 4}, {K_OUT, ta.W3, CQ_TA_W3, 4}, {K_FIRST, tq.W1, CQ_TQ_W1, 4},
                       {K_HIDQ, tq.W2, CQ_TQ_W2, 4}, {K_ACTIN, tq.W2, CQ_TQ_A, 1}, {K_FIRST, q.W1, CQ_Q_W1, 4}, {K_HIDQ, q.W2, CQ_Q_W2, 4},
                       {K_ACTIN, q.W2, CQ_Q_A, 1}, {K_HIDQT, q.W2, CQ_Q_W2T, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  float w3t[16], w3q[16];
#pragma unroll
  for (int v = 0; v < 16; v++) { w3t[v] = tq.W3[row_of(v, h)]; w3q[v] = q.W3[row_of(v, h)]; }
  const float b3t = tq.b3[0], b3q = q.b3[0];
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  v16f gW1, gW2, gW2a;
  float gW3[16];
#pragma unroll
  for (int v = 0; v < 16; v++) { gW1[v] = 0.0f; gW2[v] = 0.0f; gW2a[v] = 0.0f; gW3[v] = 0.0f; }
  float gb2 = 0.0f, gb3 = 0.0f, sse = 0.0f, sq = 0.0f;
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    const int s0 = tl * 32, smp = s0 + c;
    const bool valid = smp < n;
    const long long gi = valid ? clamp_row(idx[smp], pool.cap) : 0;
    float xb[KS1], xn[KS1], ab[4], xt[16], at[16];
#pragma unroll
    for (int s = 0; s < KS1; s++) {
      const int k = 2 * s + h;
      const bool on = valid && k < D;
      xb[s] = on ? pool.obs[gi * D + k] : 0.0f; xn[s] = on ? pool.nobs[gi * D + k] : 0.0f;
    }
#pragma unroll
    for (int v = 0; v < 4; v++) ab[v] = (valid && v + 4 * h < A) ? pool.act[gi * A + v + 4 * h] : 0.0f;
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
    // ---- target: Q'(s', mu'(s'))
    v16f u1, u2;
    float mt[4];
    {
      v16f a1, a2;
      two_layers<KS1>(wimg, CQ_TA_W1, CQ_TA_W2, sbias[0], sbias[1], xn, lane, h, a1, a2);
      relu16(a2);
      float aw[16];
      v16f mu = bias_tile(sbias[2], h);
      aop(wimg, CQ_TA_W3, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) mu = TILE_MFMA(aw[v], a2[v], mu);
#pragma unroll
      for (int v = 0; v < 4; v++) mt[v] = tanh_fast(mu[v]);   // rows a >= A: W3 and b3 padded with zeros -> tanh(0) = 0
    }
    two_layers<KS1>(wimg, CQ_TQ_W1, CQ_TQ_W2, sbias[3], sbias[4], xn, lane, h, u1, u2);
    add_action(wimg, CQ_TQ_A, lane, mt, u2);
    relu16(u2);
    const float y = rew + live * gamma * q_head(w3t, b3t, u2);
    // ---- live critic at (s, a)
    v16f c1, c2;
    two_layers<KS1>(wimg, CQ_Q_W1, CQ_Q_W2, sbias[5], sbias[6], xb, lane, h, c1, c2);
    add_action(wimg, CQ_Q_A, lane, ab, c2);
    relu16(c2);
    const float qv = q_head(w3q, b3q, c2);
    const float e = valid ? qv - y : 0.0f, dq = 2.0f * e;
    if (h == 0 && valid) { sse += e * e; sq += qv; gb3 += dq; }
    // ---- reverse mode: G2 = (W3' dq) o (h2 > 0), G1 = (W2h' G2) o (h1 > 0)
    v16f g2, g1;
#pragma unroll
    for (int v = 0; v < 16; v++) {
      gW3[v] = __builtin_fmaf(dq, c2[v], gW3[v]);
      g2[v] = c2[v] > 0.0f ? w3q[v] * dq : 0.0f;
      g1[v] = 0.0f;
    }
    float aw[16], ta_[16], tb_[16];
    aop(wimg, CQ_Q_W2T, lane, aw);
#pragma unroll
    for (int v = 0; v < 16; v++) g1 = TILE_MFMA(aw[v], g2[v], g1);
#pragma unroll
    for (int v = 0; v < 16; v++) g1[v] = c1[v] > 0.0f ? g1[v] : 0.0f;
    put(t0, g2, c, h); put(t1, c1, c, h);
    wave_lds_sync();
    get(t0, ta_, c, h); get(t1, tb_, c, h);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; s++) { gW2 = TILE_MFMA(ta_[s], tb_[s], gW2); gW2a = TILE_MFMA(ta_[s], at[s], gW2a); gb2 += ta_[s]; }
    put(t0, g1, c, h);
    wave_lds_sync();
    get(t0, ta_, c, h);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; s++) gW1 = TILE_MFMA(ta_[s], xt[s], gW1);
  }
  // ---- this wavefront's row in LDS (the tiles are free once every wavefront has left the loop), then one row per workgroup
#pragma unroll
  for (int v = 0; v < 16; v++) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) gW3[v] += __shfl_xor(gW3[v], m, 64);   // over the 32 samples of the lane half
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) { sse += __shfl_xor(sse, m, 64); sq += __shfl_xor(sq, m, 64); gb3 += __shfl_xor(gb3, m, 64); }
  gb2 += __shfl_xor(gb2, 32, 64);
  __syncthreads();
  float* red = tilemem + wave * NROW;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
    red[S::Q_W2 + r * S::HA + c] = gW2[v];
    if (c < A) red[S::Q_W2 + r * S::HA + H + c] = gW2a[v];
    if (c < D) red[S::Q_W1 + r * D + c] = gW1[v];
    if (c == D) red[S::Q_B1 + r] = gW1[v];
    if (c == 0) red[S::Q_W3 + r] = gW3[v];
  }
  if (h == 0) red[S::Q_B2 + c] = gb2;
  if (lane == 0) { red[S::Q_B3] = gb3; red[S::NPQ] = sse; red[S::NPQ + 1] = sq; }
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- actor gradient
// Gradient of -sum_b Q(s_b, mu(s_b)) with respect to the actor, through the live critic.  Row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum Q].
enum { AG_W1 = 0, AG_W2 = 4, AG_W3 = 8, AG_W2T = 12, AG_W3T = 16, AG_Q_W1 = 17, AG_Q_W2 = 21, AG_Q_A = 25, AG_Q_DA = 26, AG_N = 30 };
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) actor_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net th, Net q, float* __restrict__ partial) {
  typedef Shape<D, A> S;
  static_assert(D < 32 && A <= 8, "see critic_grad_kernel");
  constexpr int KS1 = (D + 1) / 2, NROW = S::NPA + 1;
  static_assert(WAVES * NROW <= WAVES * 2 * 32 * TP, "the workgroup's reduction re-uses the transpose tiles");
  __shared__ alignas(16) float tilemem[WAVES * 2 * 32 * TP];
  __shared__ alignas(16) float sbias[5][32];   // actor b1 b2 b3, critic b1 b2
  __shared__ float4 wimg[AG_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = tid < A ? th.b3[tid] : 0.0f;
    sbias[3][tid] = q.b1[tid]; sbias[4][tid] = q.b2[tid];
  }
  {
    const Grp g[9] = {{K_FIRST, th.W1, AG_W1, 4}, {K_HID, th.W2, AG_W2, 4}, {K_OUT, th.W3, AG_W3, 4}, {K_HIDT, th.W2, AG_W2T, 4}, {K_W3T, th.W3, AG_W3T, 1},
                      {K_FIRST, q.W1, AG_Q_W1, 4}, {K_HIDQ, q.W2, AG_Q_W2, 4}, {K_ACTIN, q.W2, AG_Q_A, 1}, {K_DA, q.W2, AG_Q_DA, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  float w3q[16];
#pragma unroll
  for (int v = 0; v < 16; v++) w3q[v] = q.W3[row_of(v, h)];
  const float b3q = q.b3[0];
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  v16f gW1, gW2, gW3;
#pragma unroll
  for (int v = 0; v < 16; v++) { gW1[v] = 0.0f; gW2[v] = 0.0f; gW3[v] = 0.0f; }
  float gb2 = 0.0f, gb3 = 0.0f, sq = 0.0f;
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    const int s0 = tl * 32, smp = s0 + c;
    const bool valid = smp < n;
    const long long gi = valid ? clamp_row(idx[smp], pool.cap) : 0;
    float xb[KS1], xt[16];
#pragma unroll
    for (int s = 0; s < KS1; s++) { const int k = 2 * s + h; xb[s] = (valid && k < D) ? pool.obs[gi * D + k] : 0.0f; }
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int sm = s0 + 16 * h + s;
      const bool on = sm < n;
      const long long gs = on ? clamp_row(idx[sm], pool.cap) : 0;
      xt[s] = c < D ? (on ? pool.obs[gs * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f);
    }
    // ---- actor forward: mu(s), action a = v + 4 h in register v < 4
    v16f a1, a2;
    float aw[16], mu[4];
    two_layers<KS1>(wimg, AG_W1, AG_W2, sbias[0], sbias[1], xb, lane, h, a1, a2);
    relu16(a2);
    {
      v16f z3 = bias_tile(sbias[2], h);
      aop(wimg, AG_W3, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) z3 = TILE_MFMA(aw[v], a2[v], z3);
#pragma unroll
      for (int v = 0; v < 4; v++) mu[v] = tanh_fast(z3[v]);
    }
    // ---- critic at (s, mu(s)) and dQ/da = W2a' (W3 o (h2 > 0))
    v16f c1, c2, da;
    two_layers<KS1>(wimg, AG_Q_W1, AG_Q_W2, sbias[3], sbias[4], xb, lane, h, c1, c2);
    add_action(wimg, AG_Q_A, lane, mu, c2);
    relu16(c2);
    const float qv = q_head(w3q, b3q, c2);
    if (h == 0 && valid) sq += qv;
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
    for (int v = 0; v < 4; v++) wt[v] = (valid && v + 4 * h < A) ? -da[v] * (1.0f - mu[v] * mu[v]) : 0.0f;
    // ---- the actor's reverse pass (tu_trpo.hip with the ReLU mask)
    v16f g2, g1;
#pragma unroll
    for (int v = 0; v < 16; v++) { g2[v] = 0.0f; g1[v] = 0.0f; }
    {
      const float4 w = wimg[AG_W3T][lane];
      g2 = TILE_MFMA(w.x, wt[0], g2); g2 = TILE_MFMA(w.y, wt[1], g2); g2 = TILE_MFMA(w.z, wt[2], g2); g2 = TILE_MFMA(w.w, wt[3], g2);
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
  for (int m = 16; m >= 1; m >>= 1) sq += __shfl_xor(sq, m, 64);
  gb2 += __shfl_xor(gb2, 32, 64); gb3 += __shfl_xor(gb3, 32, 64);
  __syncthreads();
  float* red = tilemem + wave * NROW;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
    red[S::A_W2 + r * H + c] = gW2[v];
    if (c < D) red[S::A_W1 + r * D + c] = gW1[v];
    if (c == D) red[S::A_B1 + r] = gW1[v];
    if (r < A) red[S::A_W3 + r * H + c] = gW3[v];
  }
  if (h == 0) red[S::A_B2 + c] = gb2;
  if (h == 0 && c < A) red[S::A_B3 + c] = gb3;
  if (lane == 0) red[S::NPA] = sq;
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- apply
// g = scale * (rows of partial added in order);  Lasagne's Adam on the live network (tu_pg.hip: pg_adam_kernel);  target <- (1 - tau) target
// + tau live;  stats[k] += the row sums of the `ns` columns behind the gradient (float64).  One workgroup.
struct Offsets { int o[7]; };   // starts of W1, b1, W2, b2, W3, b3 in the row, and the parameter count
__global__ void __launch_bounds__(1024) apply_kernel(int rows, int ns, const float* __restrict__ partial, float scale, NetRW live, NetRW targ, Offsets off,
                                                     float* __restrict__ m, float* __restrict__ v, float a, float beta1, float beta2, float eps, float tau,
                                                     double* __restrict__ stats) {
  apply_rows(rows, ns, partial, scale, live, targ, off.o, m, v, a, beta1, beta2, eps, tau, stats);   // mlp32_tiles.h
}

// ---------------------------------------------------------------------------------------------------------------- policy step
// tu_trpo.hip's policy_step_mfma_kernel with ReLU hidden units, a tanh output and Ornstein-Uhlenbeck noise (rllab's OUStrategy):
//   x = path_t == 0 ? mu : ou;  x += theta (mu - x) + sigma noise;  act = clip(mu(s) + x, -1, 1)
// obs32 and act are the pool's rows [top, top + n) (the caller passes the offset pointers).
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ noise,
                                                                    const long long* __restrict__ path_t, float ou_theta, float ou_sigma, float ou_mu,
                                                                    float* __restrict__ ou, const double* __restrict__ low, const double* __restrict__ high,
                                                                    float* __restrict__ obs32, float* __restrict__ act, double* __restrict__ env_act) {
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
  const bool fresh = valid && path_t[smp] == 0;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int a = v + 4 * h;
    if (valid && a < A) {
      const size_t o = (size_t)smp * A + a;
      float x = fresh ? ou_mu : ou[o];
      x = x + ou_theta * (ou_mu - x) + ou_sigma * noise[o];
      ou[o] = x;
      float val = tanh_fast(z3[v]) + x;
      val = val < -1.0f ? -1.0f : (val > 1.0f ? 1.0f : val);
      act[o] = val;
      double e = lo[v] + ((double)val + 1.0) * 0.5 * (hi[v] - lo[v]);
      e = e < lo[v] ? lo[v] : (e > hi[v] ? hi[v] : e);
      env_act[o] = e;
    }
  }
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
  if (which == CASSIE_DDPG_ACTOR) return 32 * obs_dim + 32 + 32 * 32 + 32 + act_dim * 32 + act_dim;
  if (which == CASSIE_DDPG_CRITIC) return 32 * obs_dim + 32 + 32 * (32 + act_dim) + 32 + 32 + 1;
  return 0;
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
