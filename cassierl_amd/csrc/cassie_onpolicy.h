// cassie_onpolicy.h -- device code the on-policy units share beyond cassie_tiles.h's primitives, one copy of each:
//   * tanh32: the 32 x 32 tanh policy's row of parameters, and the reverse pass of one tile with its parameter-gradient accumulation and the
//     wavefront's row store -- what trpo_kernel (tu_trpo.hip) and w32::clip_grad_kernel (tu_ppo.hip) do behind their cotangent;
//   * clip10, path_clock: the baseline's feature arithmetic (tu_trpo_baseline.hip, tu_ppo.hip's GAE);
//   * block_sum_1024, cg_update_kernel<PER>: the vector work of one conjugate-gradient iteration on up to 1024 PER entries (tu_trpo.hip: 3,
//     tu_pg_trpo.hip: 21).
// The width-128 policy's shared device code is cassie_pg_net.h / cassie_pg_vjp.inc.
#pragma once
#include "cassie_tiles.h"

namespace cassie_onpolicy {

using namespace cassie_tiles;

// ---------------------------------------------------------------------------------------------------------------- 32 x 32 tanh policy
namespace tanh32 {

using namespace cassie_tiles::w32;   // H, TP, WAVES, the A-operand images, aop, put, get

constexpr int MAX_BLOCKS = 512;   // two workgroups of four wavefronts per CU

template <int D, int A> struct Shape {
  static constexpr int NP = H * D + H + H * H + H + A * H + A;
  static constexpr int O_W1 = 0, O_B1 = H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H;
};

inline int blocks_for(int n) {
  const int tiles = (n + 31) / 32;
  int b = (tiles + WAVES - 1) / WAVES;
  return b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

// J' w of a wavefront's tiles: three accumulator tiles, gW[row_of(v, h)][c] in register v; the bias gradients are row sums (b1 rides on a
// column of ones next to the observations)
struct Grad { v16f gW1, gW2, gW3; float gb2, gb3; };
__device__ __forceinline__ void zero(Grad& g) {
#pragma unroll
  for (int v = 0; v < 16; v++) { g.gW1[v] = 0.0f; g.gW2[v] = 0.0f; g.gW3[v] = 0.0f; }
  g.gb2 = g.gb3 = 0.0f;
}

// Reverse mode of one tile from the cotangent wt on the mean (rows a = v + 4 h in registers v = 0 .. 3, the others zero):
// G2 = (W3' w) o (1 - H2^2), G1 = (W2' G2) o (1 - H1^2) with the images at quads qW3T (one) and qW2T (four), then the parameter gradients --
// products over the SAMPLE index, operands transposed through the wavefront's LDS tiles t0, t1.  xt: [obs | 1] transposed (feature on the lane).
__device__ __forceinline__ void reverse_tile(const float4 (*wimg)[64], int qW2T, int qW3T, const v16f& h1, const v16f& h2, const v16f& wt, const float (&xt)[16],
                                             float* t0, float* t1, int lane, int c, int h, Grad& g) {
  v16f g2, g1;
#pragma unroll
  for (int v = 0; v < 16; v++) { g2[v] = 0.0f; g1[v] = 0.0f; }
  {
    const float4 w = wimg[qW3T][lane];
    g2 = TILE_MFMA(w.x, wt[0], g2); g2 = TILE_MFMA(w.y, wt[1], g2); g2 = TILE_MFMA(w.z, wt[2], g2); g2 = TILE_MFMA(w.w, wt[3], g2);
  }
#pragma unroll
  for (int v = 0; v < 16; v++) g2[v] *= 1.0f - h2[v] * h2[v];
  float aw[16];
  aop(wimg, qW2T, lane, aw);
#pragma unroll
  for (int v = 0; v < 16; v++) g1 = TILE_MFMA(aw[v], g2[v], g1);
#pragma unroll
  for (int v = 0; v < 16; v++) g1[v] *= 1.0f - h1[v] * h1[v];
  float ta[16], tb[16];
  put(t0, g2, c, h); put(t1, h1, c, h);
  wave_lds_sync();
  get(t0, ta, c, h); get(t1, tb, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { g.gW2 = TILE_MFMA(ta[s], tb[s], g.gW2); g.gb2 += ta[s]; }
  put(t0, g1, c, h);
  wave_lds_sync();
  get(t0, ta, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) g.gW1 = TILE_MFMA(ta[s], xt[s], g.gW1);
  put(t0, wt, c, h); put(t1, h2, c, h);
  wave_lds_sync();
  get(t0, ta, c, h); get(t1, tb, c, h);
  wave_lds_sync();
#pragma unroll
  for (int s = 0; s < 16; s++) { g.gW3 = TILE_MFMA(ta[s], tb[s], g.gW3); g.gb3 += ta[s]; }
}

// the wavefront's row of partial sums [gW1 | gb1 | gW2 | gb2 | gW3 | gb3] (NP floats; the caller's row may be longer)
template <int D, int A> __device__ __forceinline__ void store_row(Grad& g, float* __restrict__ out, int c, int h) {
  typedef Shape<D, A> S;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
    out[S::O_W2 + r * H + c] = g.gW2[v];
    if (c < D) out[S::O_W1 + r * D + c] = g.gW1[v];
    if (c == D) out[S::O_B1 + r] = g.gW1[v];
    if (r < A) out[S::O_W3 + r * H + c] = g.gW3[v];
  }
  g.gb2 += __shfl_xor(g.gb2, 32, 64); g.gb3 += __shfl_xor(g.gb3, 32, 64);
  if (h == 0) out[S::O_B2 + c] = g.gb2;
  if (h == 0 && c < A) out[S::O_B3 + c] = g.gb3;
}

}  // namespace tanh32

// ---------------------------------------------------------------------------------------------------------------- baseline features
// float32 as the torch expressions evaluate them, promoted to float64 by the callers
__device__ __forceinline__ float clip10(float x) { return fminf(fmaxf(x, -10.0f), 10.0f); }
// t / 100 as torch evaluates `t.to(float32) / 100.0` on the device: a multiplication by the float32 reciprocal of the scalar
__device__ __forceinline__ float path_clock(long long t) { return (float)t * (1.0f / 100.0f); }

// ---------------------------------------------------------------------------------------------------------------- CG vector step
// What rllab's conjugate gradient (rllab/misc/krylov.py: cg) does between two Fisher-vector products, in one workgroup of 1024 threads: F p from
// the mean network's part (summed over wavefronts and ranks by the caller) + the log-std block + the damping, step length, x and r updates, new
// residual, early exit as a frozen step length (no host read-back), new direction.  Entry i = threadIdx.x + 1024 k in register k < PER.
// Dot products: per thread in k order, then the fixed-order block sum.
__device__ __forceinline__ float block_sum_1024(float v, float* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float t = 0.0f;
#pragma unroll
  for (int i = 0; i < 16; i++) t += red[i];   // every thread adds the 16 wavefront sums in the same order
  return t;
}
template <int PER>
__global__ void __launch_bounds__(1024) cg_update_kernel(int n, int ls_off, int n_ls, const float* __restrict__ Apm, const float* __restrict__ hls, float reg,
                                                        float tol, float* __restrict__ x, float* __restrict__ r, float* __restrict__ p, float* __restrict__ scal) {
  __shared__ float red[16];
  float pv[PER], ap[PER], rv[PER];
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int i = threadIdx.x + 1024 * k;
    pv[k] = 0.0f; ap[k] = 0.0f; rv[k] = 0.0f;
    if (i < n) {
      pv[k] = p[i]; rv[k] = r[i];
      const bool ls = i >= ls_off && i < ls_off + n_ls;
      const float f = ls ? hls[i - ls_off] * pv[k] : Apm[i < ls_off ? i : i - n_ls];
      ap[k] = f + reg * pv[k];
      s += pv[k] * ap[k];
    }
  }
  const float pAp = block_sum_1024(s, red);
  const float rr = scal[0];
  const bool running = scal[1] != 0.0f;
  const float alpha = running ? rr / pAp : 0.0f;
  s = 0.0f;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int i = threadIdx.x + 1024 * k;
    if (i < n) { x[i] += alpha * pv[k]; rv[k] -= alpha * ap[k]; r[i] = rv[k]; s += rv[k] * rv[k]; }
  }
  const float rr_new = block_sum_1024(s, red);
  const bool go_on = running && rr_new >= tol;
  const float beta = go_on ? rr_new / rr : 0.0f;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int i = threadIdx.x + 1024 * k;
    if (i < n) p[i] = rv[k] + beta * pv[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) { scal[0] = rr_new; scal[1] = go_on ? 1.0f : 0.0f; }
}

}  // namespace cassie_onpolicy
