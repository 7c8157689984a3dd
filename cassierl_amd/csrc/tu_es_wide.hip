// tu_es_wide.hip -- ES's policy step for the 128 x 128 tanh mean network (cassierl_amd/es.py, include/cassie_trpo.h: CassieEsWide*).
//
// The contract is tu_es.hip's: environment i runs the mean network with w_i = theta + s_i sigma eps_(i >> 1), eps_d = table[off_d : off_d + P], and
// the weights never exist in memory.  What differs is the size: P is about 20 700 floats (83 KB), so neither theta nor a direction fits into LDS once
// per wavefront.  theta sits ONCE per workgroup in a padded LDS image (86 KB); a wavefront handles one pair at a time and STREAMS the pair's slice of
// the table in six chunks, in the order of the row:
//
//   chunk 0     [W1 | b1]             128 D + 128 floats   layer 1: lane (h, c) = (lane >> 5, lane & 31) evaluates units c, c + 32, c + 64, c + 96 of
//                                                          environment 2 d + h
//   chunk 1..4  rows 32 j .. 32 j + 31 of W2, 4096 floats  lane (h, c) accumulates unit 32 j + c (b2 comes behind W2: it is added with the tail)
//   tail        [b2 | W3 | b3]        128 + 129 A floats   tanh of layer 2 stays in registers (the lane owns units c + 32 u), every output is a
//                                                          32-lane butterfly sum of 4 products per lane: a fixed order, the same bits in every lane
//
// A chunk is read with coalesced dword loads into 64 registers per lane (an offset has any alignment; the tail of a chunk is predicated, so nothing
// outside [off, off + P) is touched), ONE CHUNK AHEAD of the one being evaluated, and written to the wavefront's own LDS buffer with the padding
// of theta's image: rows of W1 have an odd length (32 lanes of a half read 32 banks with ds_read_b32), rows of W2 have 132 floats (the 16 lanes
// of a group of ds_read_b128 read 16 bytes each from 64 different banks).  Every entry of the slice is read once and serves both environments of the pair;
// a pair with both environments dead reads nothing.  LDS: 86 KB + 4 x 16.9 KB + 4 KB = 158 KB, one workgroup (one wavefront per SIMD) per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_tiles.h"   // tanh_fast, wave_lds_sync

namespace cassie_es_wide {

constexpr int H = 128;
constexpr int WAVES = 4;            // wavefronts per workgroup
constexpr int PAIRS_PER_WAVE = 8;   // directions a wavefront evaluates one after the other (theta is staged once for all of them)
constexpr int PPW = WAVES * PAIRS_PER_WAVE;
constexpr int CH = 32;              // rows of W2 per chunk
constexpr int NCH = H / CH;
constexpr int UPL = H / 32;         // hidden units per lane
constexpr int HP = H + 4;           // row length of W2 in the images: 4 (mod 64), so that the 16-byte reads of a 16-lane group cover the 64 banks

using cassie_tiles::tanh_fast;       // 1 - 2 / (e^2x + 1) through the hardware exp2 / rcp, absolute error ~1e-7, exact at the saturated ends
using cassie_tiles::wave_lds_sync;
constexpr int cmax(int a, int b) { return a > b ? a : b; }

// The parameter row [W1 | b1 | W2 | b2 | W3 | b3], its chunks and the padded images in LDS.
template <int D, int A> struct Shape {
  static constexpr int NP = H * D + H + H * H + H + A * H + A;
  static constexpr int O_B1 = H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H;
  static constexpr int DP = D | 1;
  // theta's image; its first L_W2 floats are also the image of chunk 0, [L_B2, L_B3 + A) is the tail as it stands in the row
  static constexpr int L_W1 = 0, L_B1 = H * DP, L_W2 = L_B1 + H, L_B2 = L_W2 + H * HP, L_W3 = L_B2 + H, L_B3 = L_W3 + A * H, LN = (L_B3 + A + 3) & ~3;
  static constexpr int N_C0 = O_W2, N_C2 = CH * H, N_CT = NP - O_B2;   // entries of chunk 0, of a chunk of W2 and of the tail
  static constexpr int T_W3 = H, T_B3 = H + A * H;                     // the tail's buffer: [b2 | W3 | b3]
  static constexpr int BUF = (cmax(cmax(L_W2, CH * HP), N_CT) + 3) & ~3;
  static_assert(L_W2 % 4 == 0 && HP % 4 == 0 && N_C0 <= 64 * 64 && N_C2 == 64 * 64 && N_CT <= 64 * 64, "16-byte reads, 64 dwords per lane");
  __device__ static __forceinline__ int pos0(int j) { return j < O_B1 ? j + (j / D) * (DP - D) : j - O_B1 + L_B1; }   // entry j of chunk 0
  __device__ static __forceinline__ int pos2(int j) { return j + (j >> 7) * (HP - H); }                                  // entry j of W2 or of a chunk of it
  __device__ static __forceinline__ int pos(int j) {                                                                       // entry j of the row
    if (j < O_W2) return pos0(j);
    if (j < O_B2) return L_W2 + pos2(j - O_W2);
    return L_B2 + (j - O_B2);
  }
};

template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES) es_wide_policy_step_kernel(const double* __restrict__ obs, int n, const float* __restrict__ theta,
                                                                      const float* __restrict__ table, const long long* __restrict__ offsets, float sigma,
                                                                      const uint8_t* __restrict__ alive, const double* __restrict__ low,
                                                                      const double* __restrict__ high, double* __restrict__ env_act) {
  typedef Shape<D, A> S;
  static_assert(D <= 32 && A <= 32, "one lane per input / output of a half");
  __shared__ __attribute__((aligned(16))) float s_theta[S::LN];
  __shared__ __attribute__((aligned(16))) float s_buf[WAVES][S::BUF];
  __shared__ __attribute__((aligned(16))) float s_x[WAVES][2][H];   // the observation, then the activations of layer 1: [environment of the pair][unit]
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: the pair's offset and alive bytes are scalar loads
  for (int j = tid; j < S::NP; j += 64 * WAVES) s_theta[S::pos(j)] = theta[j];
  __syncthreads();
  const int pairs = n >> 1;
  float* buf = s_buf[wave];
  float* x = s_x[wave][h];
  const float ss = h ? -sigma : sigma;
  const double lo = c < A ? low[c] : 0.0, hi = c < A ? high[c] : 0.0;
  // The chunk ahead (and, with chunk 0 of a pair, the pair's observations) in registers.  `on`: bit 0 / 1 = environment 2 d / 2 d + 1 is alive
  // (uniform over the wavefront).
  float r[64];
  double xo = 0.0;
  auto state_of = [&](int d) -> int {
    if (d >= pairs) return 0;
    return alive ? (alive[2 * d] != 0 ? 1 : 0) | (alive[2 * d + 1] != 0 ? 2 : 0) : 3;
  };
#define ES_WIDE_FETCH(LEN, SRC) \
  { \
    const float* src_ = (SRC); \
    _Pragma("unroll") for (int it = 0; it < ((LEN) + 63) / 64; it++) { \
      const int j = lane + 64 * it; \
      r[it] = (64 * it + 64 <= (LEN) || j < (LEN)) ? src_[j] : 0.0f; \
    } \
  }
#define ES_WIDE_STASH(LEN, POS) \
  { \
    _Pragma("unroll") for (int it = 0; it < ((LEN) + 63) / 64; it++) { \
      const int j = lane + 64 * it; \
      if (64 * it + 64 <= (LEN) || j < (LEN)) buf[POS(j)] = r[it]; \
    } \
  }
#define ES_WIDE_ID(j) (j)
  auto fetch_first = [&](int d) {   // chunk 0 of pair d and its observations
    ES_WIDE_FETCH(S::N_C0, table + offsets[d])
    xo = c < D ? obs[(size_t)(2 * d + h) * D + c] : 0.0;
  };
  const int d_first = (blockIdx.x * WAVES + wave) * PAIRS_PER_WAVE;
  int on = state_of(d_first);
  if (on) fetch_first(d_first);   // a pair with both environments dead reads nothing from the table
#pragma unroll 1
  for (int q = 0; q < PAIRS_PER_WAVE; q++) {
    const int d = d_first + q;
    if (d >= pairs) break;
    const int env = 2 * d + h;
    const bool up = (on >> h) & 1;
    const bool run = on != 0;
    const int on_next = q + 1 < PAIRS_PER_WAVE ? state_of(d + 1) : 0;
    float mu = 0.0f;
    if (run) {
      const float* src = table + offsets[d];
      // ---- chunk 0: layer 1
      ES_WIDE_STASH(S::N_C0, S::pos0)
      if (c < D) x[c] = (float)xo;
      ES_WIDE_FETCH(S::N_C2, src + S::O_W2)
      wave_lds_sync();
      float a1[UPL];
#pragma unroll
      for (int u = 0; u < UPL; u++) a1[u] = __builtin_fmaf(ss, buf[S::L_B1 + 32 * u + c], s_theta[S::L_B1 + 32 * u + c]);
#pragma unroll
      for (int k = 0; k < D; k++) {
        const float xk = x[k];
#pragma unroll
        for (int u = 0; u < UPL; u++) {
          const int w = S::L_W1 + (32 * u + c) * S::DP + k;
          a1[u] = __builtin_fmaf(__builtin_fmaf(ss, buf[w], s_theta[w]), xk, a1[u]);
        }
      }
      wave_lds_sync();   // every lane has read the observation
#pragma unroll
      for (int u = 0; u < UPL; u++) x[32 * u + c] = tanh_fast(a1[u]);
      // ---- chunks 1 .. 4: rows 32 j + c of W2 against the activations of layer 1, two partial sums (even / odd columns) per unit
      float a2[NCH];
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        wave_lds_sync();   // the buffer is free (and, for j = 0, the activations are written)
        ES_WIDE_STASH(S::N_C2, S::pos2)
        if (j + 1 < NCH) ES_WIDE_FETCH(S::N_C2, src + S::O_W2 + (j + 1) * S::N_C2)
        else ES_WIDE_FETCH(S::N_CT, src + S::O_B2)
        wave_lds_sync();
        const float* wt = s_theta + S::L_W2 + (CH * j + c) * HP;
        const float* we = buf + c * HP;
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll 8
        for (int k = 0; k < H; k += 4) {
          const float4 xv = *reinterpret_cast<const float4*>(x + k);
          const float4 e = *reinterpret_cast<const float4*>(we + k), t = *reinterpret_cast<const float4*>(wt + k);
          s0 = __builtin_fmaf(__builtin_fmaf(ss, e.x, t.x), xv.x, s0);
          s1 = __builtin_fmaf(__builtin_fmaf(ss, e.y, t.y), xv.y, s1);
          s0 = __builtin_fmaf(__builtin_fmaf(ss, e.z, t.z), xv.z, s0);
          s1 = __builtin_fmaf(__builtin_fmaf(ss, e.w, t.w), xv.w, s1);
        }
        a2[j] = s0 + s1;
      }
      // ---- the tail: b2, W3, b3
      wave_lds_sync();
      ES_WIDE_STASH(S::N_CT, ES_WIDE_ID)
      on = on_next;
      if (on) fetch_first(d + 1);
      wave_lds_sync();
      float h2[UPL];
#pragma unroll
      for (int u = 0; u < UPL; u++) h2[u] = tanh_fast(a2[u] + __builtin_fmaf(ss, buf[32 * u + c], s_theta[S::L_B2 + 32 * u + c]));
#pragma unroll
      for (int o = 0; o < A; o++) {
        float p = 0.0f;
#pragma unroll
        for (int u = 0; u < UPL; u++) {
          const int w = S::T_W3 + o * H + 32 * u + c;
          p = __builtin_fmaf(__builtin_fmaf(ss, buf[w], s_theta[S::L_B2 + w]), h2[u], p);
        }
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) p += __shfl_xor(p, m, 32);   // a + b = b + a: every lane of the half ends with the same bits
        p += __builtin_fmaf(ss, buf[S::T_B3 + o], s_theta[S::L_B2 + S::T_B3 + o]);
        if (c == o) mu = p;
      }
      wave_lds_sync();   // the buffer and the activations are free for the next pair
    } else {
      on = on_next;
      if (on) fetch_first(d + 1);
    }
    if (c < A) {
      const float v = up ? mu : 0.0f;   // a dead environment gets the middle of the box
      double e = lo + ((double)v + 1.0) * 0.5 * (hi - lo);
      e = e < lo ? lo : (e > hi ? hi : e);
      env_act[(size_t)env * A + c] = e;
    }
  }
#undef ES_WIDE_FETCH
#undef ES_WIDE_STASH
#undef ES_WIDE_ID
}

}  // namespace cassie_es_wide

extern "C" {

int CassieEsWideParamCount(int obs_dim, int act_dim) {
  using cassie_es_wide::H;
  if ((obs_dim != 26 && obs_dim != 17) || (act_dim != 6 && act_dim != 7)) return 0;
  return H * obs_dim + H + H * H + H + act_dim * H + act_dim;
}

int CassieEsWidePairsPerWorkgroup(void) { return cassie_es_wide::PPW; }

int CassieEsWidePolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* theta_dev, const float* table_dev, long long table_len,
                           const long long* offsets_dev, float sigma, const unsigned char* alive_dev, const double* low_dev, const double* high_dev,
                           double* env_actions_dev, void* stream) {
  using namespace cassie_es_wide;
  const int np = CassieEsWideParamCount(obs_dim, act_dim);
  if (!obs_dev || n <= 0 || (n & 1) || np == 0 || !theta_dev || !table_dev || table_len < np || !offsets_dev || !low_dev || !high_dev || !env_actions_dev)
    return CASSIE_EINVAL;
  const dim3 grid(((n >> 1) + PPW - 1) / PPW), block(64 * WAVES);
  hipStream_t s = (hipStream_t)stream;
#define ES_WIDE_STEP_CASE(D, A) \
  if (obs_dim == D && act_dim == A) \
    hipLaunchKernelGGL((es_wide_policy_step_kernel<D, A>), grid, block, 0, s, obs_dev, n, theta_dev, table_dev, offsets_dev, sigma, alive_dev, low_dev, high_dev, env_actions_dev);
  ES_WIDE_STEP_CASE(26, 6) ES_WIDE_STEP_CASE(26, 7) ES_WIDE_STEP_CASE(17, 6) ES_WIDE_STEP_CASE(17, 7)
#undef ES_WIDE_STEP_CASE
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
