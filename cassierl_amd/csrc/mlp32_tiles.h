// mlp32_tiles.h -- the device code of the kernels of the 32 x 32 ReLU networks, one copy for every shape (D observations, A actions) the family is
// built for: 26 x 6, 26 x 7, 17 x 6, 17 x 7 and Cassie3d's 45 x 10 (tu_ddpg.hip, tu_sac.hip + tu_sac3d.hip through sac_kernels.h, tu_td3.hip keep
// what is their own: the heads of their policies, their target action, their statistics and their entry points).  In the order of this file:
//   * the shapes of a parameter row, the operand counts that follow from D and A and the images of a network in LDS (Shape: KS1, NQ1, NB1, NS,
//     HREG, LA_*, LQ_*), the rule of the actor's output rows (out_row, out_bias);
//   * the gather of a tile's operands from the pool through the batch's index (Tile, gather, action_slots);
//   * forward passes: two_layers, add_action, q_head, actor_forward, w3_row, critic_forward;
//   * the live critic's tile pass and its row of partial sums (CriticAcc, critic_step, critic_row) and the twin-critic kernel (twin_critic_grad);
//   * the actor's reverse pass and its row of partial sums (ActorAcc, actor_reverse, actor_row);
//   * the sampler's policy step (policy_step);
//   * the Adam step and soft target update (column_sum, entry_of, adam_entry, apply_rows, Offsets).
// The layout is tu_trpo.hip's (read its header first).  The accumulator-layout primitives, the A-operand images of every matrix product (laid
// out once per workgroup in LDS) and the per-wavefront LDS transposes are cassie_tiles.h's, shared with the tanh policies.
//
// No function here knows a robot: what differs between the shapes follows from D and A (Shape; cassie_tiles.h: act_slots, head_reg).
//   * The actions.  An action tile has NS slots per lane half, registers v < NS, slot (v, h) = action row_of(v, h) where that is < A: four slots
//     (a = v + 4 h) up to eight actions, A - 4 above (45 x 10: six, of which 4 and 5 of half 1 are rows 12, 13, dead).  The noise and the pool's
//     action are loaded into the slots (action_slots), the merge layer takes the action as NS k-steps, k-step v carrying slot v of both halves
//     (K_ACTIN; six k-steps are two image quads of which the second is half padding), dQ/da comes out of K_DA in the same slots.  A two-headed
//     output layer keeps log_std a in register v + HREG of the lane that holds mean a in register v: the sample, log pi and both cotangents need
//     no data movement.  Its reverse pass runs over the 2 HREG k-steps that can hold a cotangent (K_HEADT, HREG / 2 quads; at HREG = 8 that is the
//     whole tile: four zero k-steps are cheaper than a special case).
//   * [obs | 1] is D + 1 columns.  The first layer has KS1 = (D + 1) / 2 k-steps in NQ1 image quads.  [gW1 | gb1] of a network is NB1 accumulator
//     tiles, columns 32 b .. 32 b + 31 (column D is gb1, the columns behind it are fed zeros), and the transposed observations exist once per
//     column block (Tile::xt).  At 45 observations both blocks are fed from ONE read of the G1 image: the registers are there
//     (profiles/offpolicy_shape_dedup_kernel_resources.txt), unlike in the width-128 kernel of tu_pg3d.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cassie_tiles.h"

namespace cassie_mlp32 {

using namespace cassie_tiles;
using namespace cassie_tiles::w32;   // H, TP, WAVES, Kind, wel, Grp, fill_images, aop, put, get, act_slots, head_reg

constexpr int MAX_BLOCKS = 256;   // one workgroup per CU; one partial row per workgroup

// NOUT: rows of the actor's output layer (A, or 2 A with the two heads of sac_kernels.h)
template <int D, int A, int NOUT = A> struct Shape {
  static_assert(D >= 1 && A >= 1 && A <= 12, "the action slots: registers v < NS <= 8 of the two lane halves are rows 0 .. 15 (cassie_tiles.h: act_slots)");
  static constexpr int HA = H + A;   // row length of the critic's merge layer
  // actor row  [W1 | b1 | W2 | b2 | W3 | b3]
  static constexpr int NPA = H * D + H + H * H + H + NOUT * H + NOUT;
  static constexpr int A_W1 = 0, A_B1 = H * D, A_W2 = A_B1 + H, A_B2 = A_W2 + H * H, A_W3 = A_B2 + H, A_B3 = A_W3 + NOUT * H;
  // critic row [W1 | b1 | W2 | b2 | W3 | b3]
  static constexpr int NPQ = H * D + H + H * HA + H + H + 1;
  static constexpr int Q_W1 = 0, Q_B1 = H * D, Q_W2 = Q_B1 + H, Q_B2 = Q_W2 + H * HA, Q_W3 = Q_B2 + H, Q_B3 = Q_W3 + H;
  // operands
  static constexpr int KS1 = (D + 1) / 2;                  // k-steps of the first layer, two observations each
  static constexpr int NQ1 = D < 32 ? 4 : (KS1 + 3) / 4;   // image quads of W1: one product's four below 32 observations, whole quads of k-steps above
  static constexpr int NB1 = (D + 32) / 32;                // column blocks of [obs | 1]
  static constexpr int NS = act_slots(A), HREG = head_reg(A);
  static constexpr int NQA = (NS + 3) / 4, NQH = HREG / 2;   // image quads of K_ACTIN / K_W3T, and of K_HEADT
  // A network's images in LDS, counted from its first one: an actor's W1 NQ1, W2 4, W3 4; a critic's W1 NQ1, W2 4, action NQA and then what the
  // kernel adds (critic_step: W2' 4).  Its rows of sbias: an actor's b1 b2 b3, a critic's b1 b2 W3.
  enum { LA_W1 = 0, LA_W2 = NQ1, LA_W3 = LA_W2 + 4, LA_N = LA_W3 + 4 };
  enum { LQ_W1 = 0, LQ_W2 = NQ1, LQ_A = LQ_W2 + 4, LQ_FWD = LQ_A + NQA, LQ_W2T = LQ_FWD, LQ_N = LQ_W2T + 4 };
};

struct NetRW { float *W1, *b1, *W2, *b2, *W3, *b3; };
struct Pool { const float *obs, *act, *rew, *term, *nobs; long long cap; };

// row of the actor's output layer that image row i of the output tile holds, -1 for a padding row.  KOUT is the Kind of the output layer's image:
// K_OUT (row a on image row a) or K_HEAD (cassie_tiles.h: head_row).  out_bias: b3 on the image rows.
template <int A, int KOUT> __device__ __forceinline__ int out_row(int i) {
  static_assert(KOUT == K_OUT || KOUT == K_HEAD, "the Kind of an actor's output image");
  if constexpr (KOUT == K_HEAD) return head_row<A>(i);
  else return i < A ? i : -1;
}
template <int A, int KOUT> __device__ __forceinline__ float out_bias(const float* b3, int i) { const int r = out_row<A, KOUT>(i); return r >= 0 ? b3[r] : 0.0f; }

__device__ __forceinline__ void relu16(v16f& x) {
#pragma unroll
  for (int v = 0; v < 16; v++) x[v] = x[v] > 0.0f ? x[v] : 0.0f;
}
__device__ __forceinline__ long long clamp_row(long long i, long long cap) { return i < 0 ? 0 : (i >= cap ? cap - 1 : i); }

// ---- the operands of a tile (samples 32 tl .. 32 tl + 31 of the batch), every per-sample row gathered from the pool through the batch's
// index, clamped to the pool's capacity; zeros past the batch's end
template <int D, int A> struct Tile {
  typedef Shape<D, A> S;
  int smp;                  // the lane's sample, and whether the batch has it
  bool valid;
  float xb[S::KS1], xt[S::NB1][16];   // the observation as the first layer's operand; transposed per column block (feature 32 b + c on the lane, column D = ones)
  float xn[S::KS1], ab[S::NS], at[16], rew, live;   // ALL: next observation, action in the slots and transposed, reward, 1 - terminal
};
// the lane's action slots from row `row` of an [.][A] array: the pool's actions, or noise indexed by the batch position; zeros in the dead slots
template <int A> __device__ __forceinline__ void action_slots(const float* __restrict__ p, size_t row, bool valid, int h, float (&q)[act_slots(A)]) {
#pragma unroll
  for (int v = 0; v < act_slots(A); v++) { const int a = row_of(v, h); q[v] = (valid && a < A) ? p[row * A + a] : 0.0f; }
}
// ALL = false: smp, valid, xb, xt (the actor kernels); true: everything (the critic kernels)
template <bool ALL, int D, int A> __device__ __forceinline__ void gather(const Pool& pool, const long long* __restrict__ idx, int n, int tl, int c, int h, Tile<D, A>& t) {
  typedef Shape<D, A> S;
  const int s0 = tl * 32;
  t.smp = s0 + c;
  t.valid = t.smp < n;
  const long long gi = t.valid ? clamp_row(idx[t.smp], pool.cap) : 0;
#pragma unroll
  for (int s = 0; s < S::KS1; s++) {
    const int k = 2 * s + h;
    const bool on = t.valid && k < D;
    t.xb[s] = on ? pool.obs[gi * D + k] : 0.0f;
    if constexpr (ALL) t.xn[s] = on ? pool.nobs[gi * D + k] : 0.0f;
  }
  if constexpr (ALL) action_slots<A>(pool.act, gi, t.valid, h, t.ab);
#pragma unroll
  for (int s = 0; s < 16; s++) {
    const int sm = s0 + 16 * h + s;
    const bool on = sm < n;
    const long long gs = on ? clamp_row(idx[sm], pool.cap) : 0;
#pragma unroll
    for (int b = 0; b < S::NB1; b++) {
      const int cc = 32 * b + c;
      t.xt[b][s] = cc < D ? (on ? pool.obs[gs * D + cc] : 0.0f) : (cc == D ? 1.0f : 0.0f);
    }
    if constexpr (ALL) t.at[s] = (c < A && on) ? pool.act[gs * A + c] : 0.0f;
  }
  if constexpr (ALL) { t.rew = t.valid ? pool.rew[gi] : 0.0f; t.live = t.valid ? 1.0f - pool.term[gi] : 0.0f; }
}

// ---- forward passes
// hidden layers of a network on the first-layer operand xb: h1 = relu(W1 x + b1) and z2 = W2 h1 + b2 (not yet rectified: the critic adds
// its action columns first)
template <int D, int A> __device__ __forceinline__ void two_layers(const float4 (*wimg)[64], int qW1, int qW2, const float* sb1, const float* sb2,
                                                                   const float (&xb)[Shape<D, A>::KS1], int lane, int h, v16f& h1, v16f& z2) {
  typedef Shape<D, A> S;
  float aw1[4 * S::NQ1], aw[16];
  h1 = bias_tile(sb1, h);
  aop<S::NQ1>(wimg, qW1, lane, aw1);
#pragma unroll
  for (int s = 0; s < S::KS1; s++) h1 = TILE_MFMA(aw1[s], xb[s], h1);
  relu16(h1);
  z2 = bias_tile(sb2, h);
  aop(wimg, qW2, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) z2 = TILE_MFMA(aw[v], h1[v], z2);
}
// + W2[:, 32:] a for the action in the slots: NS k-steps
template <int A> __device__ __forceinline__ void add_action(const float4 (*wimg)[64], int qA, int lane, const float (&ab)[act_slots(A)], v16f& z2) {
  constexpr int NS = act_slots(A), NQA = (NS + 3) / 4;
  float aw[4 * NQA];
  aop<NQA>(wimg, qA, lane, aw);
#pragma unroll
  for (int v = 0; v < NS; v++) z2 = TILE_MFMA(aw[v], ab[v], z2);
}
// q = b3 + W3 . h2 for the sample of this lane (both halves of the wavefront hold the result)
__device__ __forceinline__ float q_head(const float (&w3)[16], float b3, const v16f& h2) {
  float q = 0.0f;
#pragma unroll
  for (int v = 0; v < 16; v++) q = __builtin_fmaf(w3[v], h2[v], q);
  q += __shfl_xor(q, 32, 64);
  return q + b3;
}
// the actor whose images start at q0 (LA_*) and whose rows are sb[0 .. 2]: hidden activations a1, a2 and the output layer's pre-activation z3
// on the image rows of its Kind
template <int D, int A> __device__ __forceinline__ void actor_forward(const float4 (*wimg)[64], int q0, const float (*sb)[32], const float (&xb)[Shape<D, A>::KS1], int lane,
                                                                      int h, v16f& a1, v16f& a2, v16f& z3) {
  typedef Shape<D, A> S;
  two_layers<D, A>(wimg, q0 + S::LA_W1, q0 + S::LA_W2, sb[0], sb[1], xb, lane, h, a1, a2);
  relu16(a2);
  float aw[16];
  z3 = bias_tile(sb[2], h);
  aop(wimg, q0 + S::LA_W3, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) z3 = TILE_MFMA(aw[v], a2[v], z3);
}
// a critic's W3 from its row of sbias: W3[row_of(v, h)] in w3[v]
__device__ __forceinline__ void w3_row(const float* sw3, int h, float (&w3)[16]) {
  const v16f w = bias_tile(sw3, h);
#pragma unroll
  for (int v = 0; v < 16; v++) w3[v] = w[v];
}
// Q(x, a) of the critic whose images start at q0 (LQ_W1, LQ_W2, LQ_A) and whose rows b1, b2 are sb[0], sb[1], with W3 in w3 (w3_row); h1 and
// h2 are its hidden activations
template <int D, int A> __device__ __forceinline__ float critic_forward(const float4 (*wimg)[64], int q0, const float (*sb)[32], const float (&w3)[16], float b3,
                                                                        const float (&xb)[Shape<D, A>::KS1], const float (&ab)[Shape<D, A>::NS], int lane, int h, v16f& h1,
                                                                        v16f& h2) {
  typedef Shape<D, A> S;
  two_layers<D, A>(wimg, q0 + S::LQ_W1, q0 + S::LQ_W2, sb[0], sb[1], xb, lane, h, h1, h2);
  add_action<A>(wimg, q0 + S::LQ_A, lane, ab, h2);
  relu16(h2);
  return q_head(w3, b3, h2);
}

// the wavefronts' rows of partial sums -> one row per workgroup, added in the order wave 0, 1, 2, 3
template <int NROW> __device__ __forceinline__ void reduce_rows(const float* red, float* __restrict__ out) {
  for (int i = threadIdx.x; i < NROW; i += 64 * WAVES) out[i] = ((red[i] + red[NROW + i]) + red[2 * NROW + i]) + red[3 * NROW + i];
}
// the transpose tiles of a workgroup, which its reduction re-uses for the wavefronts' rows of NROW floats: the larger of the two (with 2 A output
// rows at 26 observations, and at 45 observations, the four rows are longer than the tiles)
template <int NROW> constexpr int tilemem_floats() { return WAVES * 2 * 32 * TP > WAVES * NROW ? WAVES * 2 * 32 * TP : WAVES * NROW; }
// [gW1 | gb1] of register v (row r) into a wavefront's row: column 32 b + c of block b
template <int D, int NB1> __device__ __forceinline__ void first_layer_row(const v16f (&g)[NB1], int v, int r, float* gW1, float* gb1, int c) {
#pragma unroll
  for (int b = 0; b < NB1; b++) {
    const int cc = 32 * b + c;
    if (cc < D) gW1[r * D + cc] = g[b][v];
    if (cc == D) gb1[r] = g[b][v];
  }
}

// ---- the live critic on a tile and its row of partial sums [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum e^2 | sum Q]
template <int NB1> struct CriticAcc { v16f gW1[NB1], gW2, gW2a; float gW3[16]; float gb2, gb3, sse, sq; };
template <int NB1> __device__ __forceinline__ void zero(CriticAcc<NB1>& a) {
#pragma unroll
  for (int b = 0; b < NB1; b++) a.gW1[b] = zero16();
  a.gW2 = zero16(); a.gW2a = zero16();
#pragma unroll
  for (int v = 0; v < 16; v++) a.gW3[v] = 0.0f;
  a.gb2 = a.gb3 = a.sse = a.sq = 0.0f;
}
// e = Q(s, a) - y of the critic at images q0 (LQ_*, with W2' at LQ_W2T) and rows sb[0 .. 2], and the gradient of sum e^2 in reverse mode:
// G2 = (W3' dq) o (h2 > 0), G1 = (W2h' G2) o (h1 > 0), then the parameter gradients -- products over the SAMPLE index, operands transposed
// through the wavefront's LDS tiles t0, t1; one read of the G1 image feeds every column block of [gW1 | gb1]
template <int D, int A>
__device__ __forceinline__ void critic_step(const float4 (*wimg)[64], int q0, const float (*sb)[32], float b3, const Tile<D, A>& t, float y, int lane, int c, int h,
                                            float* t0, float* t1, CriticAcc<Shape<D, A>::NB1>& acc) {
  typedef Shape<D, A> S;
  v16f c1, c2;
  float w3a[16];
  w3_row(sb[2], h, w3a);
  const float qv = critic_forward<D, A>(wimg, q0, sb, w3a, b3, t.xb, t.ab, lane, h, c1, c2);
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
  aop(wimg, q0 + S::LQ_W2T, lane, aw);
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
  for (int s = 0; s < 16; s++) {
#pragma unroll
    for (int b = 0; b < S::NB1; b++) acc.gW1[b] = TILE_MFMA(ta_[s], t.xt[b][s], acc.gW1[b]);
  }
}
// this wavefront's row of a critic into LDS
template <int D, int A> __device__ __forceinline__ void critic_row(CriticAcc<Shape<D, A>::NB1>& a, float* red, int lane, int c, int h) {
  typedef Shape<D, A> S;
#pragma unroll
  for (int v = 0; v < 16; v++) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) a.gW3[v] += __shfl_xor(a.gW3[v], m, 64);   // over the 32 samples of the lane half
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) { a.sse += __shfl_xor(a.sse, m, 64); a.sq += __shfl_xor(a.sq, m, 64); a.gb3 += __shfl_xor(a.gb3, m, 64); }
  a.gb2 += __shfl_xor(a.gb2, 32, 64);
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
    red[S::Q_W2 + r * S::HA + c] = a.gW2[v];
    if (c < A) red[S::Q_W2 + r * S::HA + H + c] = a.gW2a[v];
    first_layer_row<D>(a.gW1, v, r, red + S::Q_W1, red + S::Q_B1, c);
    if (c == 0) red[S::Q_W3 + r] = a.gW3[v];
  }
  if (h == 0) red[S::Q_B2 + c] = a.gb2;
  if (lane == 0) { red[S::Q_B3] = a.gb3; red[S::NPQ] = a.sse; red[S::NPQ + 1] = a.sq; }
}

// ---- the twin-critic kernel (sac_kernels.h's and tu_td3.hip's critic_grad_kernel).  Per sample b (pool row i = idx[b]):
//   y = r_i + (1 - terminal_i) gamma (min(Q1', Q2')(s'_i, a') - sub),  e_k = Q_k(s_i, a_i) - y,
// and the gradient of sum_b e_k^2 with respect to live critic k; the two live critics run one after the other on the same registers.  Block k
// of partial: [rows][gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum e_k^2 | sum Q_k], CassieDdpgApply's row format.
// `pi` is the network that gives the target action, its output image of Kind KOUT.  target(wimg, sb, xn, en, lane, h, an) runs it (images at
// TC_PI, rows sb[0 .. 2]) on the next observation xn with the noise en of the batch position in the slots, leaves the action a' in the slots of an
// (0 in the dead ones) and returns `sub`.
constexpr int TC_PI = 0;
template <int D, int A, int KOUT, class Target>
__device__ __forceinline__ void twin_critic_grad(const Pool& pool, const long long* __restrict__ idx, int n, const Net& pi, const Net& tq1, const Net& tq2, const Net& q1,
                                                 const Net& q2, const float* __restrict__ eps_next, float gamma, float* __restrict__ partial, Target target) {
  typedef Shape<D, A> S;
  enum { TC_T1 = S::LA_N, TC_T2 = TC_T1 + S::LQ_FWD, TC_Q1 = TC_T2 + S::LQ_FWD, TC_Q2 = TC_Q1 + S::LQ_N, TC_N = TC_Q2 + S::LQ_N };
  constexpr int NROW = S::NPQ + 2, NQ1 = S::NQ1, NQA = S::NQA;
  __shared__ alignas(16) float tilemem[tilemem_floats<NROW>()];
  __shared__ alignas(16) float sbias[15][32];   // pi b1 b2 b3;  target critics b1 b2 W3 each;  live critics b1 b2 W3 each
  __shared__ float4 wimg[TC_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = pi.b1[tid]; sbias[1][tid] = pi.b2[tid]; sbias[2][tid] = out_bias<A, KOUT>(pi.b3, tid);
    sbias[3][tid] = tq1.b1[tid]; sbias[4][tid] = tq1.b2[tid]; sbias[5][tid] = tq1.W3[tid];
    sbias[6][tid] = tq2.b1[tid]; sbias[7][tid] = tq2.b2[tid]; sbias[8][tid] = tq2.W3[tid];
    sbias[9][tid] = q1.b1[tid]; sbias[10][tid] = q1.b2[tid]; sbias[11][tid] = q1.W3[tid];
    sbias[12][tid] = q2.b1[tid]; sbias[13][tid] = q2.b2[tid]; sbias[14][tid] = q2.W3[tid];
  }
  {
    const Grp g[17] = {{K_FIRST, pi.W1, TC_PI + S::LA_W1, NQ1}, {K_HID, pi.W2, TC_PI + S::LA_W2, 4}, {KOUT, pi.W3, TC_PI + S::LA_W3, 4},
                       {K_FIRST, tq1.W1, TC_T1 + S::LQ_W1, NQ1}, {K_HIDQ, tq1.W2, TC_T1 + S::LQ_W2, 4}, {K_ACTIN, tq1.W2, TC_T1 + S::LQ_A, NQA},
                       {K_FIRST, tq2.W1, TC_T2 + S::LQ_W1, NQ1}, {K_HIDQ, tq2.W2, TC_T2 + S::LQ_W2, 4}, {K_ACTIN, tq2.W2, TC_T2 + S::LQ_A, NQA},
                       {K_FIRST, q1.W1, TC_Q1 + S::LQ_W1, NQ1}, {K_HIDQ, q1.W2, TC_Q1 + S::LQ_W2, 4}, {K_ACTIN, q1.W2, TC_Q1 + S::LQ_A, NQA},
                       {K_HIDQT, q1.W2, TC_Q1 + S::LQ_W2T, 4},
                       {K_FIRST, q2.W1, TC_Q2 + S::LQ_W1, NQ1}, {K_HIDQ, q2.W2, TC_Q2 + S::LQ_W2, 4}, {K_ACTIN, q2.W2, TC_Q2 + S::LQ_A, NQA},
                       {K_HIDQT, q2.W2, TC_Q2 + S::LQ_W2T, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  const float b3t1 = tq1.b3[0], b3t2 = tq2.b3[0], b3q1 = q1.b3[0], b3q2 = q2.b3[0];
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  CriticAcc<S::NB1> acc1, acc2;
  zero(acc1); zero(acc2);
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    Tile<D, A> t;
    gather<true>(pool, idx, n, tl, c, h, t);
    float en[S::NS];
    action_slots<A>(eps_next, t.smp, t.valid, h, en);
    float y;
    {
      v16f u1, u2;
      float an[S::NS], w3[16];
      const float sub = target(wimg, sbias, t.xn, en, lane, h, an);
      w3_row(sbias[5], h, w3);
      const float qt1 = critic_forward<D, A>(wimg, TC_T1, sbias + 3, w3, b3t1, t.xn, an, lane, h, u1, u2);
      w3_row(sbias[8], h, w3);
      const float qt2 = critic_forward<D, A>(wimg, TC_T2, sbias + 6, w3, b3t2, t.xn, an, lane, h, u1, u2);
      y = t.rew + t.live * gamma * (fminf(qt1, qt2) - sub);
    }
    critic_step(wimg, TC_Q1, sbias + 9, b3q1, t, y, lane, c, h, t0, t1, acc1);
    critic_step(wimg, TC_Q2, sbias + 12, b3q2, t, y, lane, c, h, t0, t1, acc2);
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

// ---- the actor's reverse pass on a tile and its row of partial sums [gW1 | gb1 | gW2 | gb2 | gW3 | gb3]
template <int NB1> struct ActorAcc { v16f gW1[NB1], gW2, gW3; float gb2, gb3; };
template <int NB1> __device__ __forceinline__ void zero(ActorAcc<NB1>& g) {
#pragma unroll
  for (int b = 0; b < NB1; b++) g.gW1[b] = zero16();
  g.gW2 = zero16(); g.gW3 = zero16();
  g.gb2 = g.gb3 = 0.0f;
}
// Reverse mode from the cotangent wt on the output layer's pre-activation (image rows in registers v < 4 QUADS, the others zero; QUADS is NQA for one
// head, NQH for two): G2 = (W3' wt) o (a2 > 0), G1 = (W2' G2) o (a1 > 0) with the images at qW3T (QUADS of them) and qW2T (four), then the
// parameter gradients through the wavefront's LDS tiles (tu_trpo.hip's pass with the ReLU mask)
template <int QUADS, int NB1>
__device__ __forceinline__ void actor_reverse(const float4 (*wimg)[64], int qW2T, int qW3T, const v16f& a1, const v16f& a2, const v16f& wt, const float (&xt)[NB1][16],
                                              float* t0, float* t1, int lane, int c, int h, ActorAcc<NB1>& g) {
  v16f g2 = zero16(), g1 = zero16();
#pragma unroll
  for (int q = 0; q < QUADS; q++) {
    const float4 w = wimg[qW3T + q][lane];
    g2 = TILE_MFMA(w.x, wt[4 * q], g2); g2 = TILE_MFMA(w.y, wt[4 * q + 1], g2); g2 = TILE_MFMA(w.z, wt[4 * q + 2], g2); g2 = TILE_MFMA(w.w, wt[4 * q + 3], g2);
  }
#pragma unroll
  for (int v = 0; v < 16; v++) g2[v] = a2[v] > 0.0f ? g2[v] : 0.0f;
  float aw[16], ta_[16], tb_[16];
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
  for (int s = 0; s < 16; s++) {
#pragma unroll
    for (int b = 0; b < NB1; b++) g.gW1[b] = TILE_MFMA(ta_[s], xt[b][s], g.gW1[b]);
  }
  put(t0, wt, c, h); put(t1, a2, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h); get(t1, tb_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { g.gW3 = TILE_MFMA(ta_[s], tb_[s], g.gW3); g.gb3 += ta_[s]; }
}
// this wavefront's row of an actor into LDS; S is the row's shape (D observations, an output layer of Kind KOUT)
template <class S, int D, int A, int KOUT> __device__ __forceinline__ void actor_row(ActorAcc<S::NB1>& g, float* red, int c, int h) {
  g.gb2 += __shfl_xor(g.gb2, 32, 64); g.gb3 += __shfl_xor(g.gb3, 32, 64);
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h), o = out_row<A, KOUT>(r);
    red[S::A_W2 + r * H + c] = g.gW2[v];
    first_layer_row<D>(g.gW1, v, r, red + S::A_W1, red + S::A_B1, c);
    if (o >= 0) red[S::A_W3 + o * H + c] = g.gW3[v];
  }
  if (h == 0) red[S::A_B2 + c] = g.gb2;
  if (h == 0 && out_row<A, KOUT>(c) >= 0) red[S::A_B3 + out_row<A, KOUT>(c)] = g.gb3;
}

// ---- the sampler's policy step: tu_trpo.hip's policy_step_mfma_kernel with ReLU hidden units.  One tile per wavefront; the float32 copy of the
// observation goes into the pool's row obs32, the action into act and, mapped to the environment's range [low, high], into env_act (obs32 and
// act are the pool's rows [top, top + n): the caller passes the offset pointers; rows past n are not touched).  The output layer's image is of
// Kind KOUT; head(z3, v, o, smp) gives the action component of slot v, a = row_of(v, h), of sample smp in [-1, 1] from the pre-activation z3
// (o = smp A + a).
template <int D, int A, int KOUT, class Head>
__device__ __forceinline__ void policy_step(const double* __restrict__ obs, int n, const Net& th, const double* __restrict__ low, const double* __restrict__ high,
                                            float* __restrict__ obs32, float* __restrict__ act, double* __restrict__ env_act, Head head) {
  constexpr int KS1 = Shape<D, A>::KS1, NS = Shape<D, A>::NS;
  __shared__ alignas(16) float sbias[3][32];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) { sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = out_bias<A, KOUT>(th.b3, tid); }
  float aW1[KS1], aW2[16], aW3[16];
  double lo[NS], hi[NS];
#pragma unroll
  for (int s = 0; s < KS1; s++) aW1[s] = wel<D, A>(K_FIRST, th.W1, s, c, h);
#pragma unroll
  for (int v = 0; v < 16; v++) { aW2[v] = wel<D, A>(K_HID, th.W2, v, c, h); aW3[v] = wel<D, A>(KOUT, th.W3, v, c, h); }
#pragma unroll
  for (int v = 0; v < NS; v++) { const int a = row_of(v, h); lo[v] = a < A ? low[a] : 0.0; hi[v] = a < A ? high[a] : 0.0; }
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
  for (int v = 0; v < NS; v++) {
    const int a = row_of(v, h);
    if (valid && a < A) {
      const size_t o = (size_t)smp * A + a;
      const float val = head(z3, v, o, smp);
      act[o] = val;
      double e = lo[v] + ((double)val + 1.0) * 0.5 * (hi[v] - lo[v]);
      e = e < lo[v] ? lo[v] : (e > hi[v] ? hi[v] : e);
      env_act[o] = e;
    }
  }
}

// ---- Adam step and soft target update on rows of partial sums (tu_ddpg.hip's apply_kernel, tu_td3.hip's critic_apply_kernel; sac_kernels.h's
// actor_apply_rows takes the pieces)
struct Offsets { int o[7]; };   // starts of W1, b1, W2, b2, W3, b3 in the row [W1 | b1 | W2 | b2 | W3 | b3], and the parameter count
// Every product of the three functions below is rounded (contraction off): left to the compiler, which multiply-adds are fused follows the code
// around them, and the kernels have to give the same bits as each other (CassieTd3CriticApply is CassieDdpgApply bit for bit).
// scale * (one column of `rows` rows added in row order, eight loads in flight)
__device__ __forceinline__ float column_sum(const float* p, int rows, int stride, float scale) {
#pragma clang fp contract(off)
  float g = 0.0f;
  int r = 0;
  for (; r + 8 <= rows; r += 8) {
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = p[(size_t)(r + k) * stride];
#pragma unroll
    for (int k = 0; k < 8; k++) g += x[k];
  }
  for (; r < rows; r++) g += p[(size_t)r * stride];
  return g * scale;
}
// entry i of the row -> the parameter of the network it belongs to
__device__ __forceinline__ float* entry_of(const NetRW& n, const int (&off)[7], int i) {
  if (i < off[1]) return n.W1 + (i - off[0]);
  if (i < off[2]) return n.b1 + (i - off[1]);
  if (i < off[3]) return n.W2 + (i - off[2]);
  if (i < off[4]) return n.b2 + (i - off[3]);
  if (i < off[5]) return n.W3 + (i - off[4]);
  return n.b3 + (i - off[5]);
}
// Lasagne's Adam on one entry (tu_pg.hip: pg_adam_kernel), a: adam_step_size; returns the new parameter
__device__ __forceinline__ float adam_entry(float g, float* m, float* v, float* th, float a, float beta1, float beta2, float eps) {
#pragma clang fp contract(off)
  const float mi = beta1 * *m + (1.0f - beta1) * g;
  const float vi = beta2 * *v + (1.0f - beta2) * (g * g);
  *m = mi; *v = vi;
  const float t = *th - a * mi / (sqrtf(vi) + eps);
  *th = t;
  return t;
}
// One workgroup of 1024 threads.  g = scale * (rows of partial added in order);  Adam on the live network;  target <- (1 - tau) target + tau
// live;  stats[k] += the row sums of the `ns` columns behind the gradient (float64).
__device__ __forceinline__ void apply_rows(int rows, int ns, const float* partial, float scale, NetRW live, NetRW targ, const int (&off)[7], float* m, float* v, float a,
                                           float beta1, float beta2, float eps, float tau, double* stats) {
#pragma clang fp contract(off)
  const int np = off[6], stride = np + ns;
  for (int i = threadIdx.x; i < np; i += 1024) {
    const float g = column_sum(partial + i, rows, stride, scale);
    const float t = adam_entry(g, m + i, v + i, entry_of(live, off, i), a, beta1, beta2, eps);
    float* tg = entry_of(targ, off, i);
    *tg = (1.0f - tau) * *tg + tau * t;
  }
  if ((int)threadIdx.x < ns && stats) {
    double s = 0.0;
    for (int r = 0; r < rows; r++) s += (double)partial[(size_t)r * stride + np + threadIdx.x];
    stats[threadIdx.x] += s;
  }
}

inline int blocks_for(int n) {
  const int tiles = (n + 31) / 32;
  const int b = (tiles + WAVES - 1) / WAVES;
  return b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b);
}
inline int policy_step_grid(int n) { return ((n + 31) / 32 + WAVES - 1) / WAVES; }   // the policy-step kernels: one tile per wavefront
inline bool shape_ok(int D, int A) { return (D == 26 || D == 17) && (A == 6 || A == 7); }
inline bool net_ok(const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3) { return net_ok(Net{W1, b1, W2, b2, W3, b3}); }
// a network as the C ABI passes it: a host array of the six device pointers {W1, b1, W2, b2, W3, b3}
template <class P> inline bool net_ok(P p) { return p && net_ok(p[0], p[1], p[2], p[3], p[4], p[5]); }
inline Net net_of(const float* const* p) { return Net{p[0], p[1], p[2], p[3], p[4], p[5]}; }
inline NetRW net_rw(float* const* p) { return NetRW{p[0], p[1], p[2], p[3], p[4], p[5]}; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
inline bool pool_ok(const Pool& p) { return p.obs && p.act && p.rew && p.term && p.nobs && p.cap > 0; }

// `off` for a row [W1 | b1 | W2 | b2 | W3 | b3] (off[6]: the parameter count): an actor with rows_out output units (A, or 2 A with two heads),
// and the critic
inline void row_offsets(int obs_dim, int w2_cols, int rows_out, int (&off)[7]) {
  const int len[6] = {H * obs_dim, H, H * w2_cols, H, rows_out * H, rows_out};
  off[0] = 0;
  for (int k = 0; k < 6; k++) off[k + 1] = off[k] + len[k];
}
inline void actor_offsets(int obs_dim, int rows_out, int (&off)[7]) { row_offsets(obs_dim, H, rows_out, off); }
inline void critic_offsets(int obs_dim, int act_dim, int (&off)[7]) { row_offsets(obs_dim, H + act_dim, 1, off); }
// Lasagne's Adam: the step size of step t with both bias corrections folded in (float64 on the host, as tu_pg.hip)
inline float adam_step_size(float lr, float beta1, float beta2, int t) { return (float)((double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t))); }

}  // namespace cassie_mlp32

// Launch KERNEL<D, A>(...) on `grid` workgroups of WAVES wavefronts for the (obs_dim, act_dim) the library is built for, in a function that
// returns a CASSIE_* code: any other shape returns CASSIE_EINVAL from it.  MLP32_LAUNCH: the update kernels (D 26 or 17, A 6 or 7);
// MLP32_LAUNCH_STEP: the policy-step kernels (the environment's 26-wide rows only).
#define MLP32_CASE(KERNEL, D_, A_, obs_dim, act_dim, grid, stream, ...) \
  if ((obs_dim) == D_ && (act_dim) == A_) hipLaunchKernelGGL((KERNEL<D_, A_>), dim3(grid), dim3(64 * cassie_mlp32::WAVES), 0, (hipStream_t)(stream), __VA_ARGS__); else
#define MLP32_LAUNCH_STEP(KERNEL, ...) MLP32_CASE(KERNEL, 26, 6, __VA_ARGS__) MLP32_CASE(KERNEL, 26, 7, __VA_ARGS__) return CASSIE_EINVAL
#define MLP32_LAUNCH(KERNEL, ...) \
  MLP32_CASE(KERNEL, 26, 6, __VA_ARGS__) MLP32_CASE(KERNEL, 26, 7, __VA_ARGS__) MLP32_CASE(KERNEL, 17, 6, __VA_ARGS__) MLP32_CASE(KERNEL, 17, 7, __VA_ARGS__) \
  return CASSIE_EINVAL
