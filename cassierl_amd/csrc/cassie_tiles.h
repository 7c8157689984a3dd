// cassie_tiles.h -- the accumulator-layout primitives every matrix-core network kernel of the library is written in, one copy: the tanh policies
// of both widths (tu_trpo.hip, tu_ppo.hip, cassie_onpolicy.h; cassie_pg_net.h, tu_pg.hip, tu_pg_trpo.hip) and the 32 x 32 ReLU networks
// (mlp32_tiles.h, sac_kernels.h, tu_ddpg.hip, tu_sac.hip, tu_sac3d.hip, tu_td3.hip).  tu_es.hip and tu_es_wide.hip take tanh_fast and wave_lds_sync from here.
//
// The layout (tu_trpo.hip's header tells why): exact float32 v_mfma_f32_32x32x2_f32, a tile of 32 samples per wavefront, the sample on the lane
// c = lane & 31, row row_of(v, h) of a 32-row block in register v of the lane half h = lane >> 5.
//   * cassie_tiles:       v16f, TILE_MFMA, Net, tanh_fast, wave_lds_sync, zero16, row_of, bias_tile; the host side's net_ok / net_ok16 / aligned16 and
//                         the dispatch on (obs_dim, act_dim): launch_shape, launch_obs.
//   * cassie_tiles::w32:  what the 32-wide networks of both activation families share: the A-operand images of a workgroup (Kind, wel, Grp,
//                         fill_images, aop) and the per-wavefront LDS transposes (put, get).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/cassie_vec.h"

namespace cassie_tiles {

struct Net { const float *W1, *b1, *W2, *b2, *W3, *b3; };

typedef float v16f __attribute__((ext_vector_type(16)));
#define TILE_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// tanh through the hardware exp2 / rcp: 1 - 2 / (e^2x + 1); absolute error ~1e-7 (the saturated ends are exact: e = inf or 0)
__device__ __forceinline__ float tanh_fast(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}
__device__ __forceinline__ void wave_lds_sync() {   // a wavefront's LDS accesses complete in order; this keeps the compiler from moving them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ v16f zero16() {
  v16f z;
#pragma unroll
  for (int v = 0; v < 16; v++) z[v] = 0.0f;
  return z;
}
__device__ __forceinline__ int row_of(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }   // row of a 32-row block in register v of lane half h
// r0 + row_of(v, h), summed from the left, for the index expressions inside the unrolled MFMA loops of the width-128 VJP (cassie_pg_net.h: wave_put;
// cassie_pg_vjp.inc).  Those kernels sit at the register limit: with the rule behind the function call there, pg_vjp_kernel spills 464 .. 476 B per lane
// (table in profiles/onpolicy_dedup_kernel_resources.txt); written out like this it compiles to the instructions it had.  Everywhere else: row_of.
#define ROW_AT(r0, v, h) ((r0) + ((v) & 3) + 8 * ((v) >> 2) + 4 * (h))

// C operand: b[row_of(v, h)] in register v (rows 8 g + 4 h .. + 3 are one float4)
__device__ __forceinline__ v16f bias_tile(const float* __restrict__ b, int h) {
  v16f z;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const float4 x = *reinterpret_cast<const float4*>(b + 8 * g + 4 * h);
    z[4 * g] = x.x; z[4 * g + 1] = x.y; z[4 * g + 2] = x.z; z[4 * g + 3] = x.w;
  }
  return z;
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool net_ok(const Net& t) { return t.W1 && t.b1 && t.W2 && t.b2 && t.W3 && t.b3; }
// ... and what the width-128 kernels read as float4 is 16-byte aligned
inline bool net_ok16(const Net& t) { return net_ok(t) && aligned16(t.b1) && aligned16(t.W2) && aligned16(t.b2) && aligned16(t.W3); }

// Call launch(D, A) -- a generic lambda holding the one hipLaunchKernelGGL of KERNEL<D(), A(), ...> -- for the (obs_dim, act_dim) the library is
// built for; any other shape is CASSIE_EINVAL.  ROWS26: only the environment's own 26-wide rows (the policy-step kernels).  Only the pairs
// named here are instantiated.  launch_obs: the kernels that depend on obs_dim alone.
template <int V> using Int = std::integral_constant<int, V>;
inline int launched() { return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP; }
template <bool ROWS26 = false, class F> inline int launch_shape(int obs_dim, int act_dim, F&& launch) {
  if (obs_dim == 26 && act_dim == 6) launch(Int<26>(), Int<6>());
  else if (obs_dim == 26 && act_dim == 7) launch(Int<26>(), Int<7>());
  else if constexpr (ROWS26) return CASSIE_EINVAL;
  else if (obs_dim == 17 && act_dim == 6) launch(Int<17>(), Int<6>());
  else if (obs_dim == 17 && act_dim == 7) launch(Int<17>(), Int<7>());
  else return CASSIE_EINVAL;
  return launched();
}
template <class F> inline int launch_obs(int obs_dim, F&& launch) {
  if (obs_dim == 26) launch(Int<26>());
  else if (obs_dim == 17) launch(Int<17>());
  else return CASSIE_EINVAL;
  return launched();
}
// launch_obs plus Cassie3d's 45-wide observation: the baseline kernels (tu_trpo_baseline.hip, tu_ppo.hip's GAE), which are generic in obs_dim
template <class F> inline int launch_obs3d(int obs_dim, F&& launch) {
  if (obs_dim != 45) return launch_obs(obs_dim, launch);
  launch(Int<45>());
  return launched();
}

// ---------------------------------------------------------------------------------------------------------------- 32-wide networks
namespace w32 {

constexpr int H = 32;
constexpr int TP = 36;            // floats per row of a transpose tile (16-byte aligned rows; ds_read_b128 of 16 lanes conflict-free)
constexpr int WAVES = 4;          // wavefronts per workgroup: one per SIMD

// The actions in the accumulator layout, from A alone.  An action tile has NS = act_slots(A) SLOTS per lane half, registers v < NS, and slot (v, h) is
// action a = row_of(v, h) where that is < A.  A <= 8: NS = 4 and a = v + 4 h (row_of's first quad).  8 < A <= 12: NS = A - 4, registers 4 .. NS - 1 are
// rows 8 .. on half 0 and dead rows 12 .. on half 1 (A = 10: six live slots on half 0, actions 0..3, 8, 9, four on half 1, 4..7).  A two-headed
// output layer (mean [0, A), log_std [A, 2 A)) keeps log_std a in register v + HREG = head_reg(A) of the lane that holds mean a in register v:
// row_of(v + HREG, h) = row_of(v, h) + 2 HREG for v < HREG, so log_std a sits on image row 2 HREG + a (head_row).
constexpr int act_slots(int A) { return A <= 8 ? 4 : A - 4; }
constexpr int head_reg(int A) { return A <= 8 ? 4 : 8; }

// Element `st` (k-step) of the A operand of a product for lane (c, h): see tu_trpo.hip's header for why W[c][row_of(st, h)] is what k-step st
// of Y = W X needs when X sits in the accumulator layout.
enum Kind {
  K_FIRST,   // first layer, W [32][D]: k = 2 st + h
  K_HID,     // W [32][32] on an activation
  K_HIDQ,    // the critic's W2 [32][32 + A], hidden columns
  K_OUT,     // the actor's W3 [A][32] padded to 32 rows
  K_HIDT,    // W [32][32] transposed (reverse mode)
  K_HIDQT,   // the critic's W2 hidden columns transposed
  K_ACTIN,   // the critic's W2 action columns: k-step st < NS sums over the actions of slot st, a = row_of(st, h)
  K_W3T,     // the actor's W3 transposed: cotangent row a = row_of(st, h), st < NS
  K_DA,      // the critic's W2 action columns transposed, padded to 32 rows: dQ/da = W2a' G2
  K_HEAD,    // a two-headed actor's W3 [2 A][32], rows permuted by head_row and padded to 32 (sac_kernels.h)
  K_HEADT    // that W3 transposed: cotangent row head_row(row_of(st, h)), st < 2 HREG
};
// row of a two-headed output layer (mean [0, A), log_std [A, 2 A)) that image row i of the output tile holds: mean a on image row a, log_std a on
// image row 2 HREG + a (8 + a for A <= 8, 16 + a above), -1 for a padding row
template <int A> __device__ __forceinline__ int head_row(int i) {
  constexpr int R = 2 * head_reg(A);
  static_assert(A <= 12, "mean a in a register v < NS <= HREG, log_std a in v + HREG < 16");
  return i < A ? i : (i >= R && i - R < A ? A + i - R : -1);
}
template <int D, int A> __device__ __forceinline__ float wel(int kind, const float* __restrict__ W, int st, int c, int h) {
  constexpr int HA = H + A, KS1 = (D + 1) / 2, NS = act_slots(A);
  const int r = row_of(st, h);
  switch (kind) {
    case K_FIRST: { const int k = 2 * st + h; return (st < KS1 && k < D) ? W[c * D + k] : 0.0f; }
    case K_HID: return W[c * H + r];
    case K_HIDQ: return W[c * HA + r];
    case K_OUT: return c < A ? W[c * H + r] : 0.0f;
    case K_HIDT: return W[r * H + c];
    case K_HIDQT: return W[r * HA + c];
    case K_ACTIN: return (st < NS && r < A) ? W[c * HA + H + r] : 0.0f;
    case K_W3T: return (st < NS && r < A) ? W[r * H + c] : 0.0f;
    case K_HEAD: { const int o = head_row<A>(c); return o >= 0 ? W[o * H + r] : 0.0f; }
    case K_HEADT: { const int o = st < 2 * head_reg(A) ? head_row<A>(r) : -1; return o >= 0 ? W[o * H + c] : 0.0f; }
    default: return c < A ? W[r * HA + H + c] : 0.0f;   // K_DA
  }
}
struct Grp { int kind; const float* W; int q0, nq; };

// The A operands are the same for every tile and every wavefront: the workgroup lays them out ONCE in LDS as [quad of k-steps][lane] float4
// images, and a wavefront reads the four quads of a product right before its 16 MFMAs (conflict-free ds_read_b128).
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
template <int NQ = 4> __device__ __forceinline__ void aop(const float4 (*wimg)[64], int q0, int lane, float (&a)[4 * NQ]) {   // the k-steps of a product: 16, or NQ quads
#pragma unroll
  for (int q = 0; q < NQ; q++) { const float4 w = wimg[q0 + q][lane]; a[4 * q] = w.x; a[4 * q + 1] = w.y; a[4 * q + 2] = w.z; a[4 * q + 3] = w.w; }
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

}  // namespace w32
}  // namespace cassie_tiles
