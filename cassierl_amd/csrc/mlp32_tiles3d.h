// mlp32_tiles3d.h -- the shape-bound device code of the 32 x 32 ReLU networks at the Cassie3d shape, 45 observations and 10 actions (tu_sac3d.hip; the
// twin-critic body takes the target action as a callable, as mlp32_tiles.h's does, so that TD3 and DDPG at this shape are a unit each on top of
// it).  Read mlp32_tiles.h first: the layout, the conventions and everything that does not depend on the shape are its (q_head, w3_row, relu16,
// reduce_rows, the Adam pieces, Offsets, blocks_for, put / get, Shape).  Two of its assumptions do not hold at 45 x 10, and this file is what
// replaces them (the rule is tu_pg3d.hip's, row_of(v, h) = (v & 3) + 8 (v >> 2) + 4 h):
//
//   * ten actions.  An action tile has twelve SLOTS, registers v < NS = 6 of the two lane halves, and slot (v, h) is action a = row_of(v, h) where
//     that is < 10: six live slots on half 0 (actions 0..3, 8, 9), four on half 1 (4..7; its slots 4 and 5 are rows 12, 13, dead).  The noise and
//     the pool's action are loaded into the slots (action_slots), the merge layer takes the action as six k-steps, k-step v carrying slot v of
//     both halves (K3_ACTIN, two quads of which the second is half padding), dQ/da comes out of wel's K_DA in the same slots.  The two-headed
//     output layer has mean a on image row a and log_std a on image row 16 + a (head_row3): the lane that holds mean a in register v holds its
//     log_std in register v + 8, so the sample, log pi and both cotangents need no data movement; the reverse pass of the output layer runs over
//     all 16 k-steps of the cotangent tile (K3_HEADT, four quads).
//   * [obs | 1] is 46 columns.  The first layer has 23 k-steps, padded to XS = 24 (six image quads; the operand's element 23 is zero on both
//     sides).  [gW1 | gb1] of a network is two accumulator tiles, columns 0..31 and 32..63 (column 45 is gb1, 46..63 are fed zeros), and the
//     transposed observations exist once per column block (Tile3::xt0, xt1).  Both blocks are fed from ONE read of the G1 image: the registers
//     are there (profiles/sac_cassie3d_kernel_resources.txt), unlike in the width-128 kernel of tu_pg3d.hip.
#pragma once
#include "mlp32_tiles.h"

namespace cassie_mlp32_3d {

using namespace cassie_mlp32;

constexpr int D3 = 45, A3 = 10;
constexpr int XS = 24;   // k-steps of the first layer, padded to whole quads
constexpr int NS = 6;    // action slots per lane half
constexpr int HA3 = H + A3;

// image kinds of this shape, behind cassie_tiles' (wel3 passes every other kind on to wel<45, 10>, which is generic in them)
enum Kind3 { K3_ACTIN = 100, K3_HEAD, K3_HEADT };
// row of the two-headed output layer (mean [0, 10), log_std [10, 20)) on image row i: mean a on row a, log_std a on row 16 + a; -1: padding
__device__ __forceinline__ int head_row3(int i) { return i < A3 ? i : (i >= 16 && i < 16 + A3 ? A3 + i - 16 : -1); }
__device__ __forceinline__ float wel3(int kind, const float* __restrict__ W, int st, int c, int h) {
  const int r = row_of(st, h);
  switch (kind) {
    case K3_ACTIN: return (st < NS && r < A3) ? W[c * HA3 + H + r] : 0.0f;                        // k-step st sums over the actions of slot st
    case K3_HEAD: { const int o = head_row3(c); return o >= 0 ? W[o * H + r] : 0.0f; }
    case K3_HEADT: { const int o = head_row3(r); return o >= 0 ? W[o * H + c] : 0.0f; }
    default: return wel<D3, A3>(kind, W, st, c, h);
  }
}
template <int NG> __device__ __forceinline__ void fill_images3(float4 (*wimg)[64], const Grp (&g)[NG], int wave, int lane) {
  const int c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int k = 0; k < NG; k++) {
    for (int q = wave; q < g[k].nq; q += WAVES) {
      float v4[4];
#pragma unroll
      for (int e = 0; e < 4; e++) v4[e] = wel3(g[k].kind, g[k].W, 4 * q + e, c, h);
      wimg[g[k].q0 + q][lane] = make_float4(v4[0], v4[1], v4[2], v4[3]);
    }
  }
}
__device__ __forceinline__ float head_bias3(const float* b3, int i) { const int o = head_row3(i); return o >= 0 ? b3[o] : 0.0f; }

// A network's images in LDS, counted from its first one: an actor's W1 6, W2 4, W3 4; a critic's W1 6, W2 4, action 2 and then what the kernel adds
enum { LA3_W1 = 0, LA3_W2 = 6, LA3_W3 = 10, LA3_N = 14 };
enum { LQ3_W1 = 0, LQ3_W2 = 6, LQ3_A = 10, LQ3_FWD = 12, LQ3_W2T = 12, LQ3_N = 16 };

// ---- the operands of a tile (mlp32_tiles.h: Tile, gather)
struct Tile3 {
  int smp;
  bool valid;
  float xb[XS], xt0[16], xt1[16];             // the observation as the first layer's operand; transposed, columns c and 32 + c (column 45 = ones)
  float xn[XS], ab[NS], at[16], rew, live;    // ALL: next observation, action in the slots and transposed, reward, 1 - terminal
};
// the lane's action slots from row `row` of an [.][10] array: the pool's actions, or noise indexed by the batch position; zeros in the dead slots
__device__ __forceinline__ void action_slots(const float* __restrict__ p, size_t row, bool valid, int h, float (&q)[NS]) {
#pragma unroll
  for (int v = 0; v < NS; v++) { const int a = row_of(v, h); q[v] = (valid && a < A3) ? p[row * A3 + a] : 0.0f; }
}
template <bool ALL> __device__ __forceinline__ void gather3(const Pool& pool, const long long* __restrict__ idx, int n, int tl, int c, int h, Tile3& t) {
  constexpr int D = D3, A = A3;
  const int s0 = tl * 32;
  t.smp = s0 + c;
  t.valid = t.smp < n;
  const long long gi = t.valid ? clamp_row(idx[t.smp], pool.cap) : 0;
#pragma unroll
  for (int s = 0; s < XS; s++) {
    const int k = 2 * s + h;
    const bool on = t.valid && k < D;
    t.xb[s] = on ? pool.obs[gi * D + k] : 0.0f;
    if constexpr (ALL) t.xn[s] = on ? pool.nobs[gi * D + k] : 0.0f;
  }
  if constexpr (ALL) action_slots(pool.act, gi, t.valid, h, t.ab);
#pragma unroll
  for (int s = 0; s < 16; s++) {
    const int sm = s0 + 16 * h + s, cc = 32 + c;
    const bool on = sm < n;
    const long long gs = on ? clamp_row(idx[sm], pool.cap) : 0;
    t.xt0[s] = on ? pool.obs[gs * D + c] : 0.0f;
    t.xt1[s] = cc < D ? (on ? pool.obs[gs * D + cc] : 0.0f) : (cc == D ? 1.0f : 0.0f);
    if constexpr (ALL) t.at[s] = (c < A && on) ? pool.act[gs * A + c] : 0.0f;
  }
  if constexpr (ALL) { t.rew = t.valid ? pool.rew[gi] : 0.0f; t.live = t.valid ? 1.0f - pool.term[gi] : 0.0f; }
}

// ---- forward passes (mlp32_tiles.h: two_layers, add_action, actor_forward, critic_forward)
__device__ __forceinline__ void two_layers3(const float4 (*wimg)[64], int qW1, int qW2, const float* sb1, const float* sb2, const float (&xb)[XS], int lane, int h,
                                            v16f& h1, v16f& z2) {
  h1 = bias_tile(sb1, h);
#pragma unroll
  for (int q = 0; q < XS / 4; q++) {
    const float4 w = wimg[qW1 + q][lane];
    h1 = TILE_MFMA(w.x, xb[4 * q], h1); h1 = TILE_MFMA(w.y, xb[4 * q + 1], h1); h1 = TILE_MFMA(w.z, xb[4 * q + 2], h1); h1 = TILE_MFMA(w.w, xb[4 * q + 3], h1);
  }
  relu16(h1);
  float aw[16];
  z2 = bias_tile(sb2, h);
  aop(wimg, qW2, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) z2 = TILE_MFMA(aw[v], h1[v], z2);
}
// + W2[:, 32:] a for the action in the slots: six k-steps
__device__ __forceinline__ void add_action3(const float4 (*wimg)[64], int qA, int lane, const float (&ab)[NS], v16f& z2) {
  const float4 w = wimg[qA][lane], u = wimg[qA + 1][lane];
  z2 = TILE_MFMA(w.x, ab[0], z2); z2 = TILE_MFMA(w.y, ab[1], z2); z2 = TILE_MFMA(w.z, ab[2], z2); z2 = TILE_MFMA(w.w, ab[3], z2);
  z2 = TILE_MFMA(u.x, ab[4], z2); z2 = TILE_MFMA(u.y, ab[5], z2);
}
__device__ __forceinline__ void actor_forward3(const float4 (*wimg)[64], int q0, const float (*sb)[32], const float (&xb)[XS], int lane, int h, v16f& a1, v16f& a2,
                                               v16f& z3) {
  two_layers3(wimg, q0 + LA3_W1, q0 + LA3_W2, sb[0], sb[1], xb, lane, h, a1, a2);
  relu16(a2);
  float aw[16];
  z3 = bias_tile(sb[2], h);
  aop(wimg, q0 + LA3_W3, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) z3 = TILE_MFMA(aw[v], a2[v], z3);
}
__device__ __forceinline__ float critic_forward3(const float4 (*wimg)[64], int q0, const float (*sb)[32], const float (&w3)[16], float b3, const float (&xb)[XS],
                                                 const float (&ab)[NS], int lane, int h, v16f& h1, v16f& h2) {
  two_layers3(wimg, q0 + LQ3_W1, q0 + LQ3_W2, sb[0], sb[1], xb, lane, h, h1, h2);
  add_action3(wimg, q0 + LQ3_A, lane, ab, h2);
  relu16(h2);
  return q_head(w3, b3, h2);
}

// ---- the live critic on a tile and its row of partial sums (mlp32_tiles.h: CriticAcc, critic_step, critic_row), [gW1 | gb1] in two column blocks
struct CriticAcc3 { v16f gW1a, gW1b, gW2, gW2a; float gW3[16]; float gb2, gb3, sse, sq; };
__device__ __forceinline__ void zero(CriticAcc3& a) {
#pragma unroll
  for (int v = 0; v < 16; v++) { a.gW1a[v] = 0.0f; a.gW1b[v] = 0.0f; a.gW2[v] = 0.0f; a.gW2a[v] = 0.0f; a.gW3[v] = 0.0f; }
  a.gb2 = a.gb3 = a.sse = a.sq = 0.0f;
}
__device__ __forceinline__ void critic_step3(const float4 (*wimg)[64], int q0, const float (*sb)[32], float b3, const Tile3& t, float y, int lane, int c, int h,
                                             float* t0, float* t1, CriticAcc3& acc) {
  v16f c1, c2;
  float w3a[16];
  w3_row(sb[2], h, w3a);
  const float qv = critic_forward3(wimg, q0, sb, w3a, b3, t.xb, t.ab, lane, h, c1, c2);
  const float e = t.valid ? qv - y : 0.0f, dq = 2.0f * e;
  if (h == 0 && t.valid) { acc.sse += e * e; acc.sq += qv; acc.gb3 += dq; }
  v16f g2, g1;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    acc.gW3[v] = __builtin_fmaf(dq, c2[v], acc.gW3[v]);
    g2[v] = c2[v] > 0.0f ? w3a[v] * dq : 0.0f;
    g1[v] = 0.0f;
  }
  float aw[16], ta_[16], tb_[16];
  aop(wimg, q0 + LQ3_W2T, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) g1 = TILE_MFMA(aw[v], g2[v], g1);
#pragma unroll
  for (int v = 0; v < 16; v++) g1[v] = c1[v] > 0.0f ? g1[v] : 0.0f;
  put(t0, g2, c, h); put(t1, c1, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h); get(t1, tb_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { acc.gW2 = TILE_MFMA(ta_[s], tb_[s], acc.gW2); acc.gW2a = TILE_MFMA(ta_[s], t.at[s], acc.gW2a); acc.gb2 += ta_[s]; }
  put(t0, g1, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { acc.gW1a = TILE_MFMA(ta_[s], t.xt0[s], acc.gW1a); acc.gW1b = TILE_MFMA(ta_[s], t.xt1[s], acc.gW1b); }
}
// [gW1 | gb1] of a wavefront into its row: columns c and 32 + c of the two tiles
__device__ __forceinline__ void first_layer_rows(const v16f& ga, const v16f& gb, float* gW1, float* gb1, int c, int h) {
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
    gW1[r * D3 + c] = ga[v];
    if (32 + c < D3) gW1[r * D3 + 32 + c] = gb[v];
    if (32 + c == D3) gb1[r] = gb[v];
  }
}
__device__ __forceinline__ void critic_row3(CriticAcc3& a, float* red, int lane, int c, int h) {
  typedef Shape<D3, A3> S;
#pragma unroll
  for (int v = 0; v < 16; v++) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) a.gW3[v] += __shfl_xor(a.gW3[v], m, 64);
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) { a.sse += __shfl_xor(a.sse, m, 64); a.sq += __shfl_xor(a.sq, m, 64); a.gb3 += __shfl_xor(a.gb3, m, 64); }
  a.gb2 += __shfl_xor(a.gb2, 32, 64);
  first_layer_rows(a.gW1a, a.gW1b, red + S::Q_W1, red + S::Q_B1, c, h);
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
    red[S::Q_W2 + r * S::HA + c] = a.gW2[v];
    if (c < A3) red[S::Q_W2 + r * S::HA + H + c] = a.gW2a[v];
    if (c == 0) red[S::Q_W3 + r] = a.gW3[v];
  }
  if (h == 0) red[S::Q_B2 + c] = a.gb2;
  if (lane == 0) { red[S::Q_B3] = a.gb3; red[S::NPQ] = a.sse; red[S::NPQ + 1] = a.sq; }
}

// ---- the twin-critic kernel's body (mlp32_tiles.h: twin_critic_grad, whose contract this keeps).  `pi` gives the target action through
// target(wimg, sb, xn, en, lane, h, an): images at TC3_PI (its output image of Kind kout), rows sb[0 .. 2], the next observation xn, the noise en in
// the slots; it leaves the action a' in the slots of an (0 in the dead ones) and returns `sub`.
enum { TC3_PI = 0, TC3_T1 = LA3_N, TC3_T2 = TC3_T1 + LQ3_FWD, TC3_Q1 = TC3_T2 + LQ3_FWD, TC3_Q2 = TC3_Q1 + LQ3_N, TC3_N = TC3_Q2 + LQ3_N };
template <class Target>
__device__ __forceinline__ void twin_critic_grad3(const Pool& pool, const long long* __restrict__ idx, int n, const Net& pi, int kout, const Net& tq1, const Net& tq2,
                                                  const Net& q1, const Net& q2, const float* __restrict__ eps_next, float gamma, float* __restrict__ partial, Target target) {
  typedef Shape<D3, A3> S;
  constexpr int NROW = S::NPQ + 2, TILES = WAVES * 2 * 32 * TP;
  // the workgroup's reduction re-uses the transpose tiles; at this shape the four rows are longer than the tiles
  __shared__ alignas(16) float tilemem[TILES > WAVES * NROW ? TILES : WAVES * NROW];
  __shared__ alignas(16) float sbias[15][32];   // pi b1 b2 b3;  target critics b1 b2 W3 each;  live critics b1 b2 W3 each
  __shared__ float4 wimg[TC3_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = pi.b1[tid]; sbias[1][tid] = pi.b2[tid]; sbias[2][tid] = kout == K3_HEAD ? head_bias3(pi.b3, tid) : (tid < A3 ? pi.b3[tid] : 0.0f);
    sbias[3][tid] = tq1.b1[tid]; sbias[4][tid] = tq1.b2[tid]; sbias[5][tid] = tq1.W3[tid];
    sbias[6][tid] = tq2.b1[tid]; sbias[7][tid] = tq2.b2[tid]; sbias[8][tid] = tq2.W3[tid];
    sbias[9][tid] = q1.b1[tid]; sbias[10][tid] = q1.b2[tid]; sbias[11][tid] = q1.W3[tid];
    sbias[12][tid] = q2.b1[tid]; sbias[13][tid] = q2.b2[tid]; sbias[14][tid] = q2.W3[tid];
  }
  {
    const Grp g[17] = {{K_FIRST, pi.W1, TC3_PI + LA3_W1, 6}, {K_HID, pi.W2, TC3_PI + LA3_W2, 4}, {kout, pi.W3, TC3_PI + LA3_W3, 4},
                       {K_FIRST, tq1.W1, TC3_T1 + LQ3_W1, 6}, {K_HIDQ, tq1.W2, TC3_T1 + LQ3_W2, 4}, {K3_ACTIN, tq1.W2, TC3_T1 + LQ3_A, 2},
                       {K_FIRST, tq2.W1, TC3_T2 + LQ3_W1, 6}, {K_HIDQ, tq2.W2, TC3_T2 + LQ3_W2, 4}, {K3_ACTIN, tq2.W2, TC3_T2 + LQ3_A, 2},
                       {K_FIRST, q1.W1, TC3_Q1 + LQ3_W1, 6}, {K_HIDQ, q1.W2, TC3_Q1 + LQ3_W2, 4}, {K3_ACTIN, q1.W2, TC3_Q1 + LQ3_A, 2}, {K_HIDQT, q1.W2, TC3_Q1 + LQ3_W2T, 4},
                       {K_FIRST, q2.W1, TC3_Q2 + LQ3_W1, 6}, {K_HIDQ, q2.W2, TC3_Q2 + LQ3_W2, 4}, {K3_ACTIN, q2.W2, TC3_Q2 + LQ3_A, 2}, {K_HIDQT, q2.W2, TC3_Q2 + LQ3_W2T, 4}};
    fill_images3(wimg, g, wave, lane);
  }
  const float b3t1 = tq1.b3[0], b3t2 = tq2.b3[0], b3q1 = q1.b3[0], b3q2 = q2.b3[0];
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  CriticAcc3 acc1, acc2;
  zero(acc1); zero(acc2);
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    Tile3 t;
    gather3<true>(pool, idx, n, tl, c, h, t);
    float en[NS];
    action_slots(eps_next, t.smp, t.valid, h, en);
    float y;
    {
      v16f u1, u2;
      float an[NS], w3[16];
      const float sub = target(wimg, sbias, t.xn, en, lane, h, an);
      w3_row(sbias[5], h, w3);
      const float qt1 = critic_forward3(wimg, TC3_T1, sbias + 3, w3, b3t1, t.xn, an, lane, h, u1, u2);
      w3_row(sbias[8], h, w3);
      const float qt2 = critic_forward3(wimg, TC3_T2, sbias + 6, w3, b3t2, t.xn, an, lane, h, u1, u2);
      y = t.rew + t.live * gamma * (fminf(qt1, qt2) - sub);
    }
    critic_step3(wimg, TC3_Q1, sbias + 9, b3q1, t, y, lane, c, h, t0, t1, acc1);
    critic_step3(wimg, TC3_Q2, sbias + 12, b3q2, t, y, lane, c, h, t0, t1, acc2);
  }
  // ---- the wavefronts' rows in LDS (the tiles are free once every wavefront has left the loop), one row per workgroup and critic
  float* red = tilemem + wave * NROW;
  __syncthreads();
  critic_row3(acc1, red, lane, c, h);
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
  __syncthreads();
  critic_row3(acc2, red, lane, c, h);
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + ((size_t)gridDim.x + blockIdx.x) * NROW);
}

// ---- the two-headed actor's reverse pass on a tile and its row of partial sums (mlp32_tiles.h: ActorAcc, actor_reverse, actor_row)
struct ActorAcc3 { v16f gW1a, gW1b, gW2, gW3; float gb2, gb3; };
__device__ __forceinline__ void zero(ActorAcc3& g) {
#pragma unroll
  for (int v = 0; v < 16; v++) { g.gW1a[v] = 0.0f; g.gW1b[v] = 0.0f; g.gW2[v] = 0.0f; g.gW3[v] = 0.0f; }
  g.gb2 = g.gb3 = 0.0f;
}
// wt: the cotangent on the output layer's pre-activation, mean rows in registers v < NS, log_std rows in v + 8, zeros elsewhere
__device__ __forceinline__ void actor_reverse3(const float4 (*wimg)[64], int qW2T, int qW3T, const v16f& a1, const v16f& a2, const v16f& wt, const Tile3& t, float* t0,
                                               float* t1, int lane, int c, int h, ActorAcc3& g) {
  v16f g2 = zero16(), g1 = zero16();
  float aw[16], ta_[16], tb_[16];
  aop(wimg, qW3T, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) g2 = TILE_MFMA(aw[v], wt[v], g2);
#pragma unroll
  for (int v = 0; v < 16; v++) g2[v] = a2[v] > 0.0f ? g2[v] : 0.0f;
  aop(wimg, qW2T, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) g1 = TILE_MFMA(aw[v], g2[v], g1);
#pragma unroll
  for (int v = 0; v < 16; v++) g1[v] = a1[v] > 0.0f ? g1[v] : 0.0f;
  put(t0, g2, c, h); put(t1, a1, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h); get(t1, tb_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { g.gW2 = TILE_MFMA(ta_[s], tb_[s], g.gW2); g.gb2 += ta_[s]; }
  put(t0, g1, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { g.gW1a = TILE_MFMA(ta_[s], t.xt0[s], g.gW1a); g.gW1b = TILE_MFMA(ta_[s], t.xt1[s], g.gW1b); }
  put(t0, wt, c, h); put(t1, a2, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h); get(t1, tb_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { g.gW3 = TILE_MFMA(ta_[s], tb_[s], g.gW3); g.gb3 += ta_[s]; }
}
__device__ __forceinline__ void actor_row3(ActorAcc3& g, float* red, int c, int h) {
  typedef Shape<D3, A3, 2 * A3> S;
  g.gb2 += __shfl_xor(g.gb2, 32, 64); g.gb3 += __shfl_xor(g.gb3, 32, 64);
  first_layer_rows(g.gW1a, g.gW1b, red + S::A_W1, red + S::A_B1, c, h);
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h), o = head_row3(r);
    red[S::A_W2 + r * H + c] = g.gW2[v];
    if (o >= 0) red[S::A_W3 + o * H + c] = g.gW3[v];
  }
  if (h == 0) red[S::A_B2 + c] = g.gb2;
  if (h == 0 && head_row3(c) >= 0) red[S::A_B3 + head_row3(c)] = g.gb3;
}

inline bool shape_ok3(int obs_dim, int act_dim) { return obs_dim == D3 && act_dim == A3; }

}  // namespace cassie_mlp32_3d
