// tu_vf.hip -- kernels of PPO's learned value network (include/cassie_trpo.h, "value network"; cassierl_amd/value.py): V(s) of the 128 x 128 tanh
// network with ONE output row, for both robots (26 and 45 observations): the prediction, GAE(lambda) on predicted values with the value
// target, and the gradient of the squared-error loss on one minibatch.
//
// Read tu_pg.hip's and tu_pg3d.hip's headers first: the layout (exact float32 v_mfma_f32_32x32x2_f32, a tile of 32 samples per wavefront,
// activations in the accumulator layout, four wavefronts exchanging transposed tiles through two LDS slots) is theirs, and the forward pass of the
// hidden layers is cassie_pg_net.h's forward_hidden<D, true>: tanh_near0, the series below 1/16, because gW3 = sum_s w_s H2[:, s] carries the
// RELATIVE error of H2 and tanh_fast's is 1e-3 on an activation of 1e-4 (tests/test_gpu_value_edges.py, `tiny`).  The output layer is the padded
// 32-row tile with W3 on row 0: V of sample c leaves it in register 0 of lane (c, 0).  What one output row changes in the reverse pass:
//
//   * the cotangent w = scale (V - target) is one number per sample.  It is formed on lane (c, 0), handed to lane (c, 1) by one shuffle and to the
//     other wavefronts through 32 floats of LDS per tile (scot);
//   * G2 = w (x) W3 o (1 - H2^2) is register-wise: W3[32 ob + row_of(v, h)] is bias_tile's image of W3.  No MFMA;
//   * gW3[r] = sum_s w_s H2[r][s] is a REDUCTION, not a tile product (the choice the contract leaves open): wavefront q's lane (c, h) holds row
//     32 q + c of H2 at the samples 16 h .. 16 h + 15 of a tile anyway (the transposed read of the first exchange), so the row's sum is a chain of 16
//     fmaf per tile and one shuffle across the halves at the end.  A tile product would spend 16 MFMAs per tile on a 32 x 32 accumulator of which one
//     row is wanted.  gb3 = sum_s w_s runs beside it;
//   * [gW1 | gb1] is one accumulator tile at D = 26 (27 columns of [obs | 1]) and two at D = 45 (46 columns; the third exchange runs twice over the
//     G1 image, as in tu_pg3d.hip).  One kernel text, `if constexpr (D >= 32)`.
//
// The reverse pass is written out here, as tu_pg3d.hip writes its own out: cassie_pg_vjp.inc fixes four cotangent registers, a gW3 tile and one gW1
// tile, and it is shared as text by two kernels at the register limit whose instructions must not change.  For the same reason this is a unit of
// its own, and batch_row and the float64 butterfly of tu_pg3d.hip are repeated below.  Fixed summation order throughout (k-ordered MFMA and fmaf
// chains, tiles in a fixed order per workgroup, a fixed grid for a given m): a call repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_pg_net.h"

namespace cassie_vf {

using namespace cassie_pg;

// ---------------------------------------------------------------------------------------------------------------- prediction
// One tile per wavefront (tu_pg.hip: a tile loop makes the compiler hoist a tile's weight loads out of it, and spill).
template <int D>
__global__ void __launch_bounds__(64 * WAVES, 2) predict_kernel(const float* __restrict__ obs, int n, Net th, float* __restrict__ value) {
  constexpr int KS1 = (D + 1) / 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int smp = (blockIdx.x * WAVES + wave) * 32 + c;
  const bool valid = smp < n;
  float xb[KS1];
#pragma unroll
  for (int s = 0; s < KS1; s++) { const int k = 2 * s + h; xb[s] = (valid && k < D) ? obs[(size_t)smp * D + k] : 0.0f; }
  v16f h1[NB], h2[NB];
  forward_hidden<D, true>(th, xb, h1, h2, c, h);
  v16f mu = zero16();
  mu[0] = h == 0 ? th.b3[0] : 0.0f;
#pragma unroll
  for (int kb = 0; kb < NB; kb++) gemm_block(th.W3, H, 0, 32 * kb, c < 1, h2[kb], mu, c, h);
  if (valid && h == 0) value[smp] = mu[0];
}

// ---------------------------------------------------------------------------------------------------------------- GAE on predicted values
// tu_ppo.hip's gae_kernel with the value read, not computed: one lane per environment, backwards over the T steps of its column.
__global__ void __launch_bounds__(256) gae_kernel(const float* __restrict__ values, const float* __restrict__ last_value, const double* __restrict__ rew,
                                                  const uint8_t* __restrict__ cut, int T, int n, double gamma, double lambda, double* __restrict__ returns,
                                                  double* __restrict__ adv, double* __restrict__ vtarget, double* __restrict__ partial) {
  __shared__ double red[2][256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  if (i < n) {
    double run = last_value ? (double)last_value[i] : 0.0;
    double v_next = run, a_next = 0.0, y_next = run;
    for (int tt = T - 1; tt >= 0; tt--) {
      const size_t s = (size_t)tt * n + i;
      const double value = (double)values[s];
      const double r = rew[s], live = cut[s] ? 0.0 : 1.0;
      run = r + gamma * run * live;
      const double delta = r + gamma * live * v_next - value;
      const double a = delta + gamma * lambda * live * a_next;
      // the value target a + value by the lambda-return's own recurrence, in which `value` does not appear: a + value cancels where |value| is
      // far above the return (values of 1e4 beside returns of 5 cost it four digits)
      const double y = r + gamma * live * ((1.0 - lambda) * v_next + lambda * y_next);
      returns[s] = run; adv[s] = a; vtarget[s] = y;
      s1 += a; s2 += a * a;
      v_next = value; a_next = a; y_next = y;
    }
  }
  red[0][threadIdx.x] = s1; red[1][threadIdx.x] = s2;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) { red[0][threadIdx.x] += red[0][threadIdx.x + m]; red[1][threadIdx.x] += red[1][threadIdx.x + m]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = red[0][0]; partial[2 * blockIdx.x + 1] = red[1][0]; }
}

// ---------------------------------------------------------------------------------------------------------------- gradient
struct Fit {   // what a launch adds to the network's arguments
  const long long* idx;
  int m;
  const float* target;
  float scale;
};

// batch row of minibatch position p (-1 behind the end of the minibatch); a wild index is clamped into the batch (tu_pg3d.hip's)
__device__ __forceinline__ int batch_row(const Fit& k, int p, int n) {
  if (p >= k.m) return -1;
  if (!k.idx) return p;
  const long long r = k.idx[p];
  return (int)(r < 0 ? 0 : (r >= n ? (long long)n - 1 : r));
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// partial [gridDim.x][NP]: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3] of this workgroup's tiles, stats [gridDim.x]: sum of (V - target)^2 / 2.  Wavefront q
// accumulates rows 32 q .. 32 q + 31 of gW1 / gb1 / gW2 / gb2 and entries 32 q .. 32 q + 31 of gW3 from the group's four tiles; wavefront 0 gb3.
template <int D>
__global__ void __launch_bounds__(64 * WAVES, 1) grad_kernel(const float* __restrict__ obs, int n, Net th0, Fit k0, float* __restrict__ partial,
                                                         double* __restrict__ stats) {
  typedef Shape<D, 1> S;
  static_assert(D < 64, "[obs | 1] in one or two 32-column blocks");
  constexpr int KS1 = (D + 1) / 2;
  constexpr bool TWO = D >= 32;   // two column blocks of [obs | 1]
  __shared__ alignas(16) float stage[2][WAVES][H * TP];
  __shared__ alignas(16) float scot[WAVES][32];   // the cotangent of the group's four tiles, by sample
  __shared__ int srow[WAVES][32];
  __shared__ Net snet;
  __shared__ Fit sfit;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid == 0) { snet = th0; sfit = k0; }
  v16f gW2[NB], gW1a = zero16(), gW1b = zero16();
#pragma unroll
  for (int b = 0; b < NB; b++) gW2[b] = zero16();
  float gb2 = 0.0f, gb3 = 0.0f, gw3 = 0.0f;
  double accL = 0.0;
  const int ntiles = (k0.m + 31) / 32, ngroups = (ntiles + WAVES - 1) / WAVES;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {   // the same trip count for every wavefront of the workgroup
    // (pointers re-read from LDS behind the barrier, as in pg_vjp_kernel: no load through them can be hoisted out of the loop; the barrier
    // also orders this group's first LDS writes after the previous group's last reads)
    __syncthreads();
    const Net th = snet;
    const Fit k = sfit;
    const int gs0 = grp * WAVES * 32;
    const int row = batch_row(k, gs0 + 32 * wave + c, n);
    const bool valid = row >= 0;                                    // a tile past the end runs with w = 0: its G2, G1 are zero
    if (h == 0) srow[wave][c] = row;
    float xb[KS1];
#pragma unroll
    for (int s = 0; s < KS1; s++) { const int kk = 2 * s + h; xb[s] = (valid && kk < D) ? obs[(size_t)row * D + kk] : 0.0f; }
    v16f h1[NB], h2[NB], g2[NB], g1[NB];
    forward_hidden<D, true>(th, xb, h1, h2, c, h);
    float w = 0.0f;
    {
      v16f mu = zero16();
      mu[0] = h == 0 ? th.b3[0] : 0.0f;
#pragma unroll
      for (int kb = 0; kb < NB; kb++) gemm_block(th.W3, H, 0, 32 * kb, c < 1, h2[kb], mu, c, h);
      if (valid && h == 0) {
        const float r = mu[0] - k.target[row];
        w = k.scale * r;
        accL += 0.5 * (double)r * (double)r;
      }
    }
    w = __shfl(w, c, 64);   // lane (c, 0)'s cotangent on both halves
    if (h == 0) scot[wave][c] = w;
    // G2 = w (x) W3 o (1 - H2^2), register-wise
#pragma unroll
    for (int ob = 0; ob < NB; ob++) {
      const v16f w3 = bias_tile(th.W3 + 32 * ob, h);
      v16f y;
#pragma unroll
      for (int v = 0; v < 16; v++) y[v] = (w * w3[v]) * (1.0f - h2[ob][v] * h2[ob][v]);
      g2[ob] = y;
    }
    // Three exchanges through the two LDS slots, so that no more than two 128 x 32 activations of the tile are live in registers:
    // ---- 1. H1 (slot 0, kept to the third exchange) and H2 (slot 1): gW3[32 q + c] += sum_s w[s] H2[32 q + c][s], a chain per lane half
    wave_put(stage[0][wave], h1, c, h);
    wave_put(stage[1][wave], h2, c, h);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], wa[16];
#pragma unroll
      for (int q4 = 0; q4 < 4; q4++) {
        const float4 b = *reinterpret_cast<const float4*>(&scot[u][16 * h + 4 * q4]);
        wa[4 * q4] = b.x; wa[4 * q4 + 1] = b.y; wa[4 * q4 + 2] = b.z; wa[4 * q4 + 3] = b.w;
      }
      wave_get(stage[1][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) { gw3 = __builtin_fmaf(wa[s], ta[s], gw3); gb3 += wa[s]; }   // (gb3: the same sum on every lane of a half; lane 0 of wavefront 0 stores it)
    }
    // ---- 2. G2 (slot 1): gW2[32 q + i][32 kb + j] += sum_s G2[32 q + i][s] H1[32 kb + j][s]
    __syncthreads();
    wave_put(stage[1][wave], g2, c, h);
    __syncthreads();
    // G1 = (W2' G2) o (1 - H1^2) of this wavefront's tile (H1 from its slot-0 image): k-step v of block (ob, kb) reads W2[32 kb + r(v, h)][32 ob + c]
    const float* myh1 = stage[0][wave];
#pragma unroll
    for (int ob = 0; ob < NB; ob++) {
      v16f y = zero16();
#pragma unroll
      for (int kb = 0; kb < NB; kb++)
#pragma unroll
        for (int v = 0; v < 16; v++) y = TILE_MFMA(th.W2[(size_t)ROW_AT(32 * kb, v, h) * H + 32 * ob + c], g2[kb][v], y);
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const float x = myh1[ROW_AT(32 * ob, v, h) * TP + c];
        y[v] *= 1.0f - x * x;
      }
      g1[ob] = y;
    }
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], tb[16];
      wave_get(stage[1][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) gb2 += ta[s];
#pragma unroll
      for (int kb = 0; kb < NB; kb++) {
        wave_get(stage[0][u] + 32 * kb * TP, tb, c, h);
#pragma unroll
        for (int s = 0; s < 16; s++) gW2[kb] = TILE_MFMA(ta[s], tb[s], gW2[kb]);
      }
    }
    // ---- 3. G1 (slot 0): [gW1 | gb1][32 q + i][k] += sum_s G1[32 q + i][s] [obs | 1][s][k], columns k = c and, for D >= 32, then k = 32 + c (column D: gb1)
    __syncthreads();
    wave_put(stage[0][wave], g1, c, h);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], xt[16];
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int rs = srow[u][16 * h + e];
        if constexpr (TWO) xt[e] = rs >= 0 ? obs[(size_t)rs * D + c] : 0.0f;
        else xt[e] = c < D ? (rs >= 0 ? obs[(size_t)rs * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f);
      }
      wave_get(stage[0][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) gW1a = TILE_MFMA(ta[s], xt[s], gW1a);
    }
    if constexpr (TWO) {
#pragma unroll 1
      for (int u = 0; u < WAVES; u++) {
        float ta[16], xt[16];
        const int cc = 32 + c;
#pragma unroll
        for (int e = 0; e < 16; e++) { const int rs = srow[u][16 * h + e]; xt[e] = cc < D ? (rs >= 0 ? obs[(size_t)rs * D + cc] : 0.0f) : (cc == D ? 1.0f : 0.0f); }
        wave_get(stage[0][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
        for (int s = 0; s < 16; s++) gW1b = TILE_MFMA(ta[s], xt[s], gW1b);
      }
    }
  }
  // the workgroup's row: gW[row_of(v, h)][c] in register v
  float* out = partial + (size_t)blockIdx.x * S::NP;
  const int q = wave;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
#pragma unroll
    for (int kb = 0; kb < NB; kb++) out[S::O_W2 + (32 * q + r) * H + 32 * kb + c] = gW2[kb][v];
    if constexpr (TWO) {
      out[S::O_W1 + (32 * q + r) * D + c] = gW1a[v];
      if (32 + c < D) out[S::O_W1 + (32 * q + r) * D + 32 + c] = gW1b[v];
      if (32 + c == D) out[S::O_B1 + 32 * q + r] = gW1b[v];
    } else {
      if (c < D) out[S::O_W1 + (32 * q + r) * D + c] = gW1a[v];
      if (c == D) out[S::O_B1 + 32 * q + r] = gW1a[v];
    }
  }
  gb2 += __shfl_xor(gb2, 32, 64); gb3 += __shfl_xor(gb3, 32, 64); gw3 += __shfl_xor(gw3, 32, 64);
  if (h == 0) { out[S::O_B2 + 32 * q + c] = gb2; out[S::O_W3 + 32 * q + c] = gw3; }
  if (tid == 0) out[S::O_B3] = gb3;
  // the statistic: per wavefront by a butterfly, the four wavefronts added in order by wavefront 0 (through LDS)
  __syncthreads();
  double* red = reinterpret_cast<double*>(&stage[0][0][0]);   // [WAVES]
  accL = wave_sum64(accL);
  if (lane == 0) red[wave] = accL;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < WAVES; w++) s += red[w];
    stats[blockIdx.x] = s;
  }
}

inline int step_blocks(int n) { return ((n + 31) / 32 + WAVES - 1) / WAVES; }
inline bool shape_ok(int obs_dim) { return obs_dim == 26 || obs_dim == 45; }

}  // namespace cassie_vf

extern "C" {

int CassieVfParamCount(int obs_dim) { return cassie_vf::shape_ok(obs_dim) ? 128 * obs_dim + 128 + 128 * 128 + 128 + 128 + 1 : 0; }
int CassieVfGradRows(int m) { return cassie_pg::vjp_blocks(m); }

int CassieVfPredict(const float* obs_dev, int n, int obs_dim, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                    const float* b3, float* value_dev, void* stream) {
  using namespace cassie_vf;
  const Net th{W1, b1, W2, b2, W3, b3};   // b1, W2, b2, W3 are read as float4
  if (!obs_dev || n <= 0 || !net_ok16(th) || !value_dev || !shape_ok(obs_dim)) return CASSIE_EINVAL;
  if (obs_dim == 26) hipLaunchKernelGGL(predict_kernel<26>, dim3(step_blocks(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, value_dev);
  else hipLaunchKernelGGL(predict_kernel<45>, dim3(step_blocks(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, value_dev);
  return launched();
}

int CassieVfGae(const float* values_dev, const float* last_value_dev, const double* rew_dev, const unsigned char* cut_dev, int T, int n, double gamma,
                double lambda, double* returns_dev, double* adv_dev, double* vtarget_dev, double* partial_dev, void* stream) {
  if (!values_dev || !rew_dev || !cut_dev || T <= 0 || n <= 0 || !returns_dev || !adv_dev || !vtarget_dev || !partial_dev) return CASSIE_EINVAL;
  hipLaunchKernelGGL(cassie_vf::gae_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, values_dev, last_value_dev, rew_dev, cut_dev, T, n, gamma, lambda,
                     returns_dev, adv_dev, vtarget_dev, partial_dev);
  return cassie_tiles::launched();
}

int CassieVfGrad(const float* obs_dev, int n, int obs_dim, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                 const float* b3, const long long* idx_dev, int m, const float* target_dev, float scale, float* partial_dev, double* stats_dev, void* stream) {
  using namespace cassie_vf;
  const Net th{W1, b1, W2, b2, W3, b3};   // b1, W2, b2, W3 are read as float4
  if (!net_ok16(th) || !obs_dev || n <= 0 || m <= 0 || !target_dev || !partial_dev || !stats_dev || !(idx_dev || m <= n) || !shape_ok(obs_dim))
    return CASSIE_EINVAL;   // without an index the minibatch is rows 0 .. m - 1
  const Fit k{idx_dev, m, target_dev, scale};
  if (obs_dim == 26) hipLaunchKernelGGL(grad_kernel<26>, dim3(vjp_blocks(m)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, k, partial_dev, stats_dev);
  else hipLaunchKernelGGL(grad_kernel<45>, dim3(vjp_blocks(m)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, k, partial_dev, stats_dev);
  return launched();
}

}  // extern "C"
