// cassie_pg_net.h -- device code shared by the width-128 policy units (tu_pg.hip: policy step, J' w, Adam; tu_pg_trpo.hip: Fisher-vector
// product, line search, CG step; tu_ppo.hip: clipped-surrogate gradient): the shapes, the forward pass of one tile of 32 samples in the
// accumulator layout, the per-wavefront LDS transposes of the VJP (wave_put, wave_get).  The VJP's reverse pass of a group of four tiles and
// the workgroup's row store are cassie_pg_vjp.inc and cassie_pg_vjp_row.inc (shared as text: see there).  The layout primitives (v16f, TILE_MFMA, Net, tanh_fast, zero16,
// row_of, bias_tile) are cassie_tiles.h's.  Read tu_pg.hip's header for the layout.
#ifndef CASSIE_PG_NET_H_
#define CASSIE_PG_NET_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cassie_tiles.h"

namespace cassie_pg {

using namespace cassie_tiles;

constexpr int H = 128;            // hidden units (both layers)
constexpr int NB = H / 32;        // 32-row blocks of a hidden layer
constexpr int TP = 36;            // floats per row of a transposed tile (16-byte aligned rows, ds_read_b128 conflict-free)
constexpr int WAVES = 4;          // wavefronts per workgroup: one per SIMD
constexpr int MAX_VJP_BLOCKS = 256;   // one VJP workgroup per CU (144 KB of LDS)

template <int D, int A> struct Shape {
  static constexpr int NP = H * D + H + H * H + H + A * H + A;
  static constexpr int O_W1 = 0, O_B1 = H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H;
};

// y += W[row0 + c][col0 + r(v, h)] x[v] over the 16 k-steps (W row-major with ld floats per row; col0 and ld multiples of 4)
__device__ __forceinline__ void gemm_block(const float* __restrict__ W, int ld, int row0, int col0, bool on, const v16f& x, v16f& y, int c, int h) {
#pragma unroll
  for (int g = 0; g < 4; g++) {
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (on) a = *reinterpret_cast<const float4*>(W + (size_t)(row0 + c) * ld + col0 + 8 * g + 4 * h);
    y = TILE_MFMA(a.x, x[4 * g], y); y = TILE_MFMA(a.y, x[4 * g + 1], y); y = TILE_MFMA(a.z, x[4 * g + 2], y); y = TILE_MFMA(a.w, x[4 * g + 3], y);
  }
}

// tanh_fast without its cancellation near 0: 1 - 2 / (e + 1) has an ABSOLUTE error of about 1e-7, a relative one of 1e-3 on an activation of 1e-4.
// Below 1/16 the odd series x - x^3 / 3 + 2 x^5 / 15 (next term 17 x^7 / 315: 3e-9 of tanh at 1/16); from there on tanh_fast, whose relative
// error is then 3e-6 or less.
__device__ __forceinline__ float tanh_near0(float x) {
  const float x2 = x * x;
  const float p = x2 * __builtin_fmaf(x2, 0.133333333f, -0.333333333f);
  return __builtin_fabsf(x) < 0.0625f ? __builtin_fmaf(x, p, x) : tanh_fast(x);
}

// Forward pass of one tile: h1 = tanh(W1 x + b1), h2 = tanh(W2 h1 + b2) (four blocks each); first layer k = 2 s + h.  NEAR0: tanh_near0 for
// tanh_fast (tu_vf.hip: a value gradient is judged block by block, and gW3 = sum_s w_s H2[:, s] carries H2's RELATIVE error; the policy units
// keep tanh_fast and their instructions)
template <int D, bool NEAR0 = false>
__device__ __forceinline__ void forward_hidden(const Net& th, const float (&xb)[(D + 1) / 2], v16f (&h1)[NB], v16f (&h2)[NB], int c, int h) {
  constexpr int KS1 = (D + 1) / 2;
#pragma unroll
  for (int ob = 0; ob < NB; ob++) {
    v16f y = bias_tile(th.b1 + 32 * ob, h);
#pragma unroll
    for (int s = 0; s < KS1; s++) {
      const int k = 2 * s + h;
      const float a = k < D ? th.W1[(32 * ob + c) * D + k] : 0.0f;
      y = TILE_MFMA(a, xb[s], y);
    }
#pragma unroll
    for (int v = 0; v < 16; v++) y[v] = NEAR0 ? tanh_near0(y[v]) : tanh_fast(y[v]);
    h1[ob] = y;
  }
#pragma unroll
  for (int ob = 0; ob < NB; ob++) {
    v16f y = bias_tile(th.b2 + 32 * ob, h);
#pragma unroll
    for (int kb = 0; kb < NB; kb++) gemm_block(th.W2, H, 32 * ob, 32 * kb, true, h1[kb], y, c, h);
#pragma unroll
    for (int v = 0; v < 16; v++) y[v] = NEAR0 ? tanh_near0(y[v]) : tanh_fast(y[v]);
    h2[ob] = y;
  }
}

// ---------------------------------------------------------------------------------------------------------------- VJP (tu_pg.hip, tu_ppo.hip)
__device__ __forceinline__ void wave_put(float* __restrict__ t, const v16f (&x)[NB], int c, int h) {   // accumulator layout -> [row][sample]
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int v = 0; v < 16; v++) t[ROW_AT(32 * b, v, h) * TP + c] = x[b][v];
}
__device__ __forceinline__ void wave_get(const float* __restrict__ t, float (&y)[16], int c, int h) {   // lane (c, h): row c, samples 16 h .. 16 h + 15
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float4 b = *reinterpret_cast<const float4*>(&t[c * TP + 16 * h + 4 * q]);
    y[4 * q] = b.x; y[4 * q + 1] = b.y; y[4 * q + 2] = b.z; y[4 * q + 3] = b.w;
  }
}

inline int vjp_blocks(int n) {   // groups of four tiles, one workgroup per CU at the most
  const int groups = ((n + 31) / 32 + WAVES - 1) / WAVES;
  return groups < 1 ? 1 : (groups > MAX_VJP_BLOCKS ? MAX_VJP_BLOCKS : groups);
}

}  // namespace cassie_pg

#endif
