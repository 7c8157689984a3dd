// mlp32_tiles.h -- what the kernels of the 32 x 32 ReLU networks share (tu_ddpg.hip, tu_sac.hip, tu_td3.hip): the shapes of a parameter row, the
// fixed-order reduction of the wavefronts' rows, the live critic's tile pass of the twin-critic kernels and the Adam / soft-update body of the
// apply kernels.  The layout is tu_trpo.hip's (read its header first).  The accumulator-layout primitives, the A-operand images of every matrix
// product (laid out once per workgroup in LDS) and the per-wavefront LDS transposes are cassie_tiles.h's, shared with the tanh policies.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cassie_tiles.h"

namespace cassie_mlp32 {

using namespace cassie_tiles;
using namespace cassie_tiles::w32;   // H, TP, WAVES, Kind, wel, Grp, fill_images, aop, put, get

constexpr int MAX_BLOCKS = 256;   // one workgroup per CU; one partial row per workgroup

template <int D, int A> struct Shape {
  static constexpr int HA = H + A;   // row length of the critic's merge layer
  // actor row  [W1 | b1 | W2 | b2 | W3 | b3]
  static constexpr int NPA = H * D + H + H * H + H + A * H + A;
  static constexpr int A_W1 = 0, A_B1 = H * D, A_W2 = A_B1 + H, A_B2 = A_W2 + H * H, A_W3 = A_B2 + H, A_B3 = A_W3 + A * H;
  // critic row [W1 | b1 | W2 | b2 | W3 | b3]
  static constexpr int NPQ = H * D + H + H * HA + H + H + 1;
  static constexpr int Q_W1 = 0, Q_B1 = H * D, Q_W2 = Q_B1 + H, Q_B2 = Q_W2 + H * HA, Q_W3 = Q_B2 + H, Q_B3 = Q_W3 + H;
};

struct NetRW { float *W1, *b1, *W2, *b2, *W3, *b3; };
struct Pool { const float *obs, *act, *rew, *term, *nobs; long long cap; };

__device__ __forceinline__ void relu16(v16f& x) {
#pragma unroll
  for (int v = 0; v < 16; v++) x[v] = x[v] > 0.0f ? x[v] : 0.0f;
}
__device__ __forceinline__ long long clamp_row(long long i, long long cap) { return i < 0 ? 0 : (i >= cap ? cap - 1 : i); }

// hidden layers of a network on the first-layer operand xb: h1 = relu(W1 x + b1) and z2 = W2 h1 + b2 (not yet rectified: the critic adds
// its action columns first)
template <int KS1> __device__ __forceinline__ void two_layers(const float4 (*wimg)[64], int qW1, int qW2, const float* sb1, const float* sb2, const float (&xb)[KS1],
                                                              int lane, int h, v16f& h1, v16f& z2) {
  float aw[16];
  h1 = bias_tile(sb1, h);
  aop(wimg, qW1, lane, aw);
#pragma unroll
  for (int s = 0; s < KS1; s++) h1 = TILE_MFMA(aw[s], xb[s], h1);
  relu16(h1);
  z2 = bias_tile(sb2, h);
  aop(wimg, qW2, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) z2 = TILE_MFMA(aw[v], h1[v], z2);
}
// + W2[:, 32:] a for the action a = v + 4 h in register v < 4 (one quad of k-steps)
__device__ __forceinline__ void add_action(const float4 (*wimg)[64], int qA, int lane, const float (&ab)[4], v16f& z2) {
  const float4 w = wimg[qA][lane];
  z2 = TILE_MFMA(w.x, ab[0], z2); z2 = TILE_MFMA(w.y, ab[1], z2); z2 = TILE_MFMA(w.z, ab[2], z2); z2 = TILE_MFMA(w.w, ab[3], z2);
}
// q = b3 + W3 . h2 for the sample of this lane (both halves of the wavefront hold the result)
__device__ __forceinline__ float q_head(const float (&w3)[16], float b3, const v16f& h2) {
  float q = 0.0f;
#pragma unroll
  for (int v = 0; v < 16; v++) q = __builtin_fmaf(w3[v], h2[v], q);
  q += __shfl_xor(q, 32, 64);
  return q + b3;
}

// the wavefronts' rows of partial sums -> one row per workgroup, added in the order wave 0, 1, 2, 3
template <int NROW> __device__ __forceinline__ void reduce_rows(const float* red, float* __restrict__ out) {
  for (int i = threadIdx.x; i < NROW; i += 64 * WAVES) out[i] = ((red[i] + red[NROW + i]) + red[2 * NROW + i]) + red[3 * NROW + i];
}

// ---- the live critic on a tile and its row of partial sums (tu_sac.hip, tu_td3.hip: both critics of a twin pair run through these)
struct CriticAcc { v16f gW1, gW2, gW2a; float gW3[16]; float gb2, gb3, sse, sq; };
__device__ __forceinline__ void zero(CriticAcc& a) {
#pragma unroll
  for (int v = 0; v < 16; v++) { a.gW1[v] = 0.0f; a.gW2[v] = 0.0f; a.gW2a[v] = 0.0f; a.gW3[v] = 0.0f; }
  a.gb2 = a.gb3 = a.sse = a.sq = 0.0f;
}
// tu_ddpg.hip's critic_grad_kernel from "live critic at (s, a)" on, for the critic whose images start at q0 (W1 4, W2 4, action 1, W2' 4)
enum { LQ_W1 = 0, LQ_W2 = 4, LQ_A = 8, LQ_W2T = 9, LQ_N = 13 };
template <int KS1>
__device__ __forceinline__ void critic_step(const float4 (*wimg)[64], int q0, const float* sb1, const float* sb2, const float* sw3, float b3, const float (&xb)[KS1],
                                            const float (&ab)[4], const float (&xt)[16], const float (&at)[16], float y, bool valid, int lane, int c, int h,
                                            float* t0, float* t1, CriticAcc& acc) {
  v16f c1, c2;
  two_layers<KS1>(wimg, q0 + LQ_W1, q0 + LQ_W2, sb1, sb2, xb, lane, h, c1, c2);
  add_action(wimg, q0 + LQ_A, lane, ab, c2);
  relu16(c2);
  const v16f w3 = bias_tile(sw3, h);   // W3[r(v, h)] in register v
  float w3a[16];
#pragma unroll
  for (int v = 0; v < 16; v++) w3a[v] = w3[v];
  const float qv = q_head(w3a, b3, c2);
  const float e = valid ? qv - y : 0.0f, dq = 2.0f * e;
  if (h == 0 && valid) { acc.sse += e * e; acc.sq += qv; acc.gb3 += dq; }
  v16f g2, g1;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    acc.gW3[v] = __builtin_fmaf(dq, c2[v], acc.gW3[v]);
    g2[v] = c2[v] > 0.0f ? w3a[v] * dq : 0.0f;
    g1[v] = 0.0f;
  }
  float aw[16], ta_[16], tb_[16];
  aop(wimg, q0 + LQ_W2T, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) g1 = TILE_MFMA(aw[v], g2[v], g1);
#pragma unroll
  for (int v = 0; v < 16; v++) g1[v] = c1[v] > 0.0f ? g1[v] : 0.0f;
  put(t0, g2, c, h); put(t1, c1, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h); get(t1, tb_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { acc.gW2 = TILE_MFMA(ta_[s], tb_[s], acc.gW2); acc.gW2a = TILE_MFMA(ta_[s], at[s], acc.gW2a); acc.gb2 += ta_[s]; }
  put(t0, g1, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) acc.gW1 = TILE_MFMA(ta_[s], xt[s], acc.gW1);
}
// this wavefront's row of a critic into LDS (tu_ddpg.hip's order)
template <int D, int A> __device__ __forceinline__ void critic_row(CriticAcc& a, float* red, int lane, int c, int h) {
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
    if (c < D) red[S::Q_W1 + r * D + c] = a.gW1[v];
    if (c == D) red[S::Q_B1 + r] = a.gW1[v];
    if (c == 0) red[S::Q_W3 + r] = a.gW3[v];
  }
  if (h == 0) red[S::Q_B2 + c] = a.gb2;
  if (lane == 0) { red[S::Q_B3] = a.gb3; red[S::NPQ] = a.sse; red[S::NPQ + 1] = a.sq; }
}

// ---- Adam step and soft target update on a row of partial sums (tu_ddpg.hip's apply_kernel, tu_td3.hip's critic_apply_kernel): one workgroup of
// 1024 threads.  g = scale * (rows of partial added in order);  Lasagne's Adam on the live network (tu_pg.hip: pg_adam_kernel);  target <- (1 - tau)
// target + tau live;  stats[k] += the row sums of the `ns` columns behind the gradient (float64).  off: the starts of W1, b1, W2, b2, W3, b3 in the
// row, and the parameter count.
__device__ __forceinline__ void apply_rows(int rows, int ns, const float* partial, float scale, NetRW live, NetRW targ, const int (&off)[7], float* m, float* v, float a,
                                           float beta1, float beta2, float eps, float tau, double* stats) {
  const int np = off[6], stride = np + ns;
  for (int i = threadIdx.x; i < np; i += 1024) {
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
    float *th, *tg;
    int j;
    if (i < off[1]) { th = live.W1; tg = targ.W1; j = i - off[0]; }
    else if (i < off[2]) { th = live.b1; tg = targ.b1; j = i - off[1]; }
    else if (i < off[3]) { th = live.W2; tg = targ.W2; j = i - off[2]; }
    else if (i < off[4]) { th = live.b2; tg = targ.b2; j = i - off[3]; }
    else if (i < off[5]) { th = live.W3; tg = targ.W3; j = i - off[4]; }
    else { th = live.b3; tg = targ.b3; j = i - off[5]; }
    const float mi = beta1 * m[i] + (1.0f - beta1) * g;
    const float vi = beta2 * v[i] + (1.0f - beta2) * (g * g);
    m[i] = mi; v[i] = vi;
    const float t = th[j] - a * mi / (sqrtf(vi) + eps);
    th[j] = t;
    tg[j] = (1.0f - tau) * tg[j] + tau * t;
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

// apply_rows' `off` for a row [W1 | b1 | W2 | b2 | W3 | b3]: an actor with rows_out output units (A, or 2 A with two heads), and the critic
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
