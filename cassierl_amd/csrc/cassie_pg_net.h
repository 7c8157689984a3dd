// cassie_pg_net.h -- device code shared by the width-128 policy units (tu_pg.hip: policy step, J' w, Adam; tu_pg_trpo.hip: Fisher-vector
// product, line search, CG step): the shapes, the weight pointers, and the forward pass of one tile of 32 samples in the accumulator layout.
// Read tu_pg.hip's header for the layout.
#ifndef CASSIE_PG_NET_H_
#define CASSIE_PG_NET_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cassie_pg {

constexpr int H = 128;            // hidden units (both layers)
constexpr int NB = H / 32;        // 32-row blocks of a hidden layer
constexpr int TP = 36;            // floats per row of a transposed tile (16-byte aligned rows, ds_read_b128 conflict-free)
constexpr int WAVES = 4;          // wavefronts per workgroup: one per SIMD
constexpr int MAX_VJP_BLOCKS = 256;   // one VJP workgroup per CU (144 KB of LDS)

template <int D, int A> struct Shape {
  static constexpr int NP = H * D + H + H * H + H + A * H + A;
  static constexpr int O_W1 = 0, O_B1 = H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H;
};

struct Net { const float *W1, *b1, *W2, *b2, *W3, *b3; };

typedef float v16f __attribute__((ext_vector_type(16)));
#define PG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// tanh through the hardware exp2 / rcp, as in tu_trpo.hip: 1 - 2 / (e^2x + 1)
__device__ __forceinline__ float tanh_fast(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

__device__ __forceinline__ v16f zero16() {
  v16f z;
#pragma unroll
  for (int v = 0; v < 16; v++) z[v] = 0.0f;
  return z;
}

// C operand: b[r(v, h)] in register v (rows 8 g + 4 h .. + 3 are one float4)
__device__ __forceinline__ v16f bias_tile(const float* __restrict__ b, int h) {
  v16f z;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const float4 x = *reinterpret_cast<const float4*>(b + 8 * g + 4 * h);
    z[4 * g] = x.x; z[4 * g + 1] = x.y; z[4 * g + 2] = x.z; z[4 * g + 3] = x.w;
  }
  return z;
}

// y += W[row0 + c][col0 + r(v, h)] x[v] over the 16 k-steps (W row-major with ld floats per row; col0 and ld multiples of 4)
__device__ __forceinline__ void gemm_block(const float* __restrict__ W, int ld, int row0, int col0, bool on, const v16f& x, v16f& y, int c, int h) {
#pragma unroll
  for (int g = 0; g < 4; g++) {
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (on) a = *reinterpret_cast<const float4*>(W + (size_t)(row0 + c) * ld + col0 + 8 * g + 4 * h);
    y = PG_MFMA(a.x, x[4 * g], y); y = PG_MFMA(a.y, x[4 * g + 1], y); y = PG_MFMA(a.z, x[4 * g + 2], y); y = PG_MFMA(a.w, x[4 * g + 3], y);
  }
}

// Forward pass of one tile: h1 = tanh(W1 x + b1), h2 = tanh(W2 h1 + b2) (four blocks each); first layer k = 2 s + h
template <int D>
__device__ __forceinline__ void forward_hidden(const Net& th, const float (&xb)[(D + 1) / 2], v16f (&h1)[NB], v16f (&h2)[NB], int c, int h) {
  constexpr int KS1 = (D + 1) / 2;
#pragma unroll
  for (int ob = 0; ob < NB; ob++) {
    v16f y = bias_tile(th.b1 + 32 * ob, h);
#pragma unroll
    for (int s = 0; s < KS1; s++) {
      const int k = 2 * s + h;
      const float a = k < D ? th.W1[(32 * ob + c) * D + k] : 0.0f;
      y = PG_MFMA(a, xb[s], y);
    }
#pragma unroll
    for (int v = 0; v < 16; v++) y[v] = tanh_fast(y[v]);
    h1[ob] = y;
  }
#pragma unroll
  for (int ob = 0; ob < NB; ob++) {
    v16f y = bias_tile(th.b2 + 32 * ob, h);
#pragma unroll
    for (int kb = 0; kb < NB; kb++) gemm_block(th.W2, H, 32 * ob, 32 * kb, true, h1[kb], y, c, h);
#pragma unroll
    for (int v = 0; v < 16; v++) y[v] = tanh_fast(y[v]);
    h2[ob] = y;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace cassie_pg

#endif
