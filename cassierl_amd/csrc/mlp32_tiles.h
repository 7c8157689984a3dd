// mlp32_tiles.h -- what the kernels of the 32 x 32 ReLU networks share (tu_ddpg.hip, tu_sac.hip, tu_td3.hip): the shapes of a parameter row, the
// A-operand images of every matrix product (laid out once per workgroup in LDS), the accumulator-layout helpers, the per-wavefront LDS
// transposes, the fixed-order reduction of the wavefronts' rows, the live critic's tile pass of the twin-critic kernels and the Adam / soft-update
// body of the apply kernels.  The layout is tu_trpo.hip's (read its header first): exact float32
// v_mfma_f32_32x32x2_f32, a tile of 32 samples per wavefront, sample on the lane c = lane & 31, hidden unit r(v, h) = (v & 3) + 8 (v >> 2) + 4 h
// in register v of the lane half h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace cassie_mlp32 {

constexpr int H = 32;
constexpr int TP = 36;            // floats per row of a transpose tile (tu_trpo.hip)
constexpr int WAVES = 4;
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

struct Net { const float *W1, *b1, *W2, *b2, *W3, *b3; };
struct NetRW { float *W1, *b1, *W2, *b2, *W3, *b3; };
struct Pool { const float *obs, *act, *rew, *term, *nobs; long long cap; };

typedef float v16f __attribute__((ext_vector_type(16)));
#define DDPG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float tanh_fast(float x) {   // tu_trpo.hip: 1 - 2 / (e^2x + 1), absolute error ~1e-7
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int row_of(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// Element `st` (k-step) of the A operand of a product for lane (c, h): see tu_trpo.hip's header for why W[c][r(st, h)] is what k-step st
// of Y = W X needs when X sits in the accumulator layout.
enum Kind {
  K_FIRST,   // first layer, W [32][D]: k = 2 st + h
  K_HID,     // W [32][32] on an activation
  K_HIDQ,    // the critic's W2 [32][32 + A], hidden columns
  K_OUT,     // the actor's W3 [A][32] padded to 32 rows
  K_HIDT,    // W [32][32] transposed (reverse mode)
  K_HIDQT,   // the critic's W2 hidden columns transposed
  K_ACTIN,   // the critic's W2 action columns: k-step st < 4 sums over action a = st + 4 h
  K_W3T,     // the actor's W3 transposed: cotangent row a = st + 4 h, st < 4
  K_DA,      // the critic's W2 action columns transposed, padded to 32 rows: dQ/da = W2a' G2
  K_HEAD,    // a two-headed actor's W3 [2 A][32], rows permuted by head_row and padded to 32 (tu_sac.hip)
  K_HEADT    // that W3 transposed: cotangent row head_row(r(st, h)), st < 8
};
// row of a two-headed output layer (mean [0, A), log_std [A, 2 A)) that image row i of the output tile holds: mean a on image row a, log_std a on
// image row 8 + a (a < A <= 8), -1 for a padding row
template <int A> __device__ __forceinline__ int head_row(int i) { return i < 8 ? (i < A ? i : -1) : (i < 16 && i - 8 < A ? A + i - 8 : -1); }
template <int D, int A> __device__ __forceinline__ float wel(int kind, const float* __restrict__ W, int st, int c, int h) {
  constexpr int HA = H + A, KS1 = (D + 1) / 2;
  const int r = row_of(st, h);
  switch (kind) {
    case K_FIRST: { const int k = 2 * st + h; return (st < KS1 && k < D) ? W[c * D + k] : 0.0f; }
    case K_HID: return W[c * H + r];
    case K_HIDQ: return W[c * HA + r];
    case K_OUT: return c < A ? W[c * H + r] : 0.0f;
    case K_HIDT: return W[r * H + c];
    case K_HIDQT: return W[r * HA + c];
    case K_ACTIN: { const int a = st + 4 * h; return (st < 4 && a < A) ? W[c * HA + H + a] : 0.0f; }
    case K_W3T: { const int a = st + 4 * h; return (st < 4 && a < A) ? W[a * H + c] : 0.0f; }
    case K_HEAD: { const int o = head_row<A>(c); return o >= 0 ? W[o * H + r] : 0.0f; }
    case K_HEADT: { const int o = st < 8 ? head_row<A>(r) : -1; return o >= 0 ? W[o * H + c] : 0.0f; }
    default: return c < A ? W[r * HA + H + c] : 0.0f;   // K_DA
  }
}
struct Grp { int kind; const float* W; int q0, nq; };

template <int D, int A, int NG> __device__ __forceinline__ void fill_images(float4 (*wimg)[64], const Grp (&g)[NG], int wave, int lane) {
  const int c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int k = 0; k < NG; k++) {
    for (int q = wave; q < g[k].nq; q += WAVES) {
      float v4[4];
#pragma unroll
      for (int e = 0; e < 4; e++) v4[e] = wel<D, A>(g[k].kind, g[k].W, 4 * q + e, c, h);
      wimg[g[k].q0 + q][lane] = make_float4(v4[0], v4[1], v4[2], v4[3]);
    }
  }
}
__device__ __forceinline__ void aop(const float4 (*wimg)[64], int q0, int lane, float (&a)[16]) {   // the 16 k-steps of a product
#pragma unroll
  for (int q = 0; q < 4; q++) { const float4 w = wimg[q0 + q][lane]; a[4 * q] = w.x; a[4 * q + 1] = w.y; a[4 * q + 2] = w.z; a[4 * q + 3] = w.w; }
}
__device__ __forceinline__ v16f bias_tile(const float* sb, int h) {   // C operand: bias[r(v, h)] in register v
  v16f z;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const float4 b = *reinterpret_cast<const float4*>(&sb[8 * g + 4 * h]);
    z[4 * g] = b.x; z[4 * g + 1] = b.y; z[4 * g + 2] = b.z; z[4 * g + 3] = b.w;
  }
  return z;
}
__device__ __forceinline__ void put(float* t, const v16f& x, int c, int h) {   // accumulator layout -> [row][sample] image
#pragma unroll
  for (int v = 0; v < 16; v++) t[row_of(v, h) * TP + c] = x[v];
}
__device__ __forceinline__ void get(const float* t, float (&y)[16], int c, int h) {   // lane (i = c, h): row i, samples 16 h .. 16 h + 15
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float4 b = *reinterpret_cast<const float4*>(&t[c * TP + 16 * h + 4 * q]);
    y[4 * q] = b.x; y[4 * q + 1] = b.y; y[4 * q + 2] = b.z; y[4 * q + 3] = b.w;
  }
}
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
  for (int s = 0; s < KS1; s++) h1 = DDPG_MFMA(aw[s], xb[s], h1);
  relu16(h1);
  z2 = bias_tile(sb2, h);
  aop(wimg, qW2, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) z2 = DDPG_MFMA(aw[v], h1[v], z2);
}
// + W2[:, 32:] a for the action a = v + 4 h in register v < 4 (one quad of k-steps)
__device__ __forceinline__ void add_action(const float4 (*wimg)[64], int qA, int lane, const float (&ab)[4], v16f& z2) {
  const float4 w = wimg[qA][lane];
  z2 = DDPG_MFMA(w.x, ab[0], z2); z2 = DDPG_MFMA(w.y, ab[1], z2); z2 = DDPG_MFMA(w.z, ab[2], z2); z2 = DDPG_MFMA(w.w, ab[3], z2);
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
  for (int v = 0; v < 16; v++) g1 = DDPG_MFMA(aw[v], g2[v], g1);
#pragma unroll
  for (int v = 0; v < 16; v++) g1[v] = c1[v] > 0.0f ? g1[v] : 0.0f;
  put(t0, g2, c, h); put(t1, c1, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h); get(t1, tb_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { acc.gW2 = DDPG_MFMA(ta_[s], tb_[s], acc.gW2); acc.gW2a = DDPG_MFMA(ta_[s], at[s], acc.gW2a); acc.gb2 += ta_[s]; }
  put(t0, g1, c, h);
  wave_lds_sync();
  get(t0, ta_, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) acc.gW1 = DDPG_MFMA(ta_[s], xt[s], acc.gW1);
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
inline bool net_ok(const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3) { return W1 && b1 && W2 && b2 && W3 && b3; }
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
