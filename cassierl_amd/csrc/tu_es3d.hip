// tu_es3d.hip -- ES's policy steps at Cassie3d's shape, 45 observations and 10 actions (cassierl_amd/es.py, include/cassie_trpo.h: CassieEs3d*).
//
// The contract is tu_es.hip's and tu_es_wide.hip's word for word: environment i runs the tanh mean network with w_i = theta + s_i sigma eps_(i >> 1),
// s_i = +1 for even i and -1 for odd i, eps_d = table[off_d : off_d + P], weight = fmaf(s sigma, eps, theta) formed on the fly, the action map in
// double, a dead environment gets the middle of the box, a pair with both environments dead reads nothing from the table, nothing outside
// [off, off + P) is touched and a launch repeats bit for bit.  What differs from those units is what 45 inputs do to their organisation:
//
//   width 32   (cassie_es3d)  an observation has 45 entries and a half has 32 lanes: lane (h, c) fetches and stages entries c and c + 32 (the second
//              where it is below 45), and the activations' buffer has max(D, H) = 45 floats per environment.  Rows of W1 have 45 floats, odd as they
//              stand.  A direction is 45 dwords per lane in flight (2858 = 44 * 64 + 42: the last 22 lanes of the last pass are predicated off).
//              LDS: five images of 2900 floats + 1440 B = 59 440 B, two workgroups per CU.
//   width 128  (cassie_es3d_wide)  theta's image is 24 204 floats (96 816 B); with it, four wavefront buffers of 32 rows of W2 do not fit into 160 KB,
//              so a workgroup has THREE wavefronts (96 816 + 3 * 16 896 + 3072 = 150 576 B) and chunks of W2 stay 32 rows = 64 dwords per lane.
//              [W1 | b1] is 5888 floats, more than a buffer and more than 64 dwords per lane: it is streamed as two row blocks, rows 0..63
//              (2880 floats, 45 dwords per lane) and rows 64..127 with b1 (3008 floats, 47 dwords per lane) -- the lane's units c, c + 32 and
//              c + 64, c + 96.  b1 arrives with the second block, so the bias is added behind the sum over the inputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_tiles.h"   // tanh_fast, wave_lds_sync

namespace cassie_es3d {

constexpr int D = 45, A = 10;
constexpr int H = 32;
constexpr int WAVES = 4;            // wavefronts per workgroup
constexpr int PAIRS_PER_WAVE = 4;   // directions a wavefront evaluates one after the other (theta is staged once for all of them)
constexpr int PPW = WAVES * PAIRS_PER_WAVE;
constexpr int XW = D > H ? D : H;   // floats of the observation / activation buffer of one environment

using cassie_tiles::tanh_fast;
using cassie_tiles::wave_lds_sync;

// The parameter row [W1 | b1 | W2 | b2 | W3 | b3] and its padded image in LDS (tu_es.hip's Shape at D = 45: a row of W1 is odd without padding).
struct S {
  static constexpr int NP = H * D + H + H * H + H + A * H + A;
  static constexpr int O_B1 = H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H;
  static constexpr int DP = D | 1, HP = H + 1;
  static constexpr int L_W1 = 0, L_B1 = H * DP, L_W2 = L_B1 + H, L_B2 = L_W2 + H * HP, L_W3 = L_B2 + H, L_B3 = L_W3 + A * HP, LN = L_B3 + A;
  __device__ static __forceinline__ int pos(int j) {   // entry j of the row -> its place in the image
    if (j < O_B1) return j + (j / D) * (DP - D);
    if (j < O_W2) return j - O_B1 + L_B1;
    if (j < O_B2) return L_W2 + (j - O_W2) + ((j - O_W2) >> 5);
    if (j < O_W3) return j - O_B2 + L_B2;
    if (j < O_B3) return L_W3 + (j - O_W3) + ((j - O_W3) >> 5);
    return j - O_B3 + L_B3;
  }
};
static_assert(S::NP == 2858 && S::LN == 2900 && D > 32 && D <= 64 && A <= 32, "two inputs per lane of a half, one output");
static_assert((1 + WAVES) * S::LN * 4 + WAVES * 2 * XW * 4 <= 80 * 1024, "two workgroups per CU");

__global__ void __launch_bounds__(64 * WAVES, 2) es3d_policy_step_kernel(const double* __restrict__ obs, int n, const float* __restrict__ theta,
                                                                       const float* __restrict__ table, const long long* __restrict__ offsets, float sigma,
                                                                       const uint8_t* __restrict__ alive, const double* __restrict__ low,
                                                                       const double* __restrict__ high, double* __restrict__ env_act) {
  __shared__ float s_theta[S::LN];
  __shared__ float s_eps[WAVES][S::LN];
  __shared__ float s_x[WAVES][2][XW];   // the observation, then the activations of a layer: [environment of the pair][entry]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  for (int j = tid; j < S::NP; j += 64 * WAVES) s_theta[S::pos(j)] = theta[j];
  __syncthreads();
  const int pairs = n >> 1;
  constexpr int NIT = (S::NP + 63) / 64;   // dwords of a direction per lane
  float* eps = s_eps[wave];
  float* x = s_x[wave][h];
  const float ss = h ? -sigma : sigma;
  const double lo = c < A ? low[c] : 0.0, hi = c < A ? high[c] : 0.0;
  // A pair's slice of the table and its observations are fetched into registers one pair ahead.  `on`: bit 0 / 1 = environment 2 d / 2 d + 1 is
  // alive (uniform over the wavefront).
  float r[NIT];
  double xo0 = 0.0, xo1 = 0.0;   // entries c and c + 32 of the observation
  auto state_of = [&](int d) -> int {
    if (d >= pairs) return 0;
    return alive ? (alive[2 * d] != 0 ? 1 : 0) | (alive[2 * d + 1] != 0 ? 2 : 0) : 3;
  };
  auto fetch = [&](int d) {
    const float* src = table + offsets[d];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int j = lane + 64 * it;
      r[it] = (64 * it + 64 <= S::NP || j < S::NP) ? src[j] : 0.0f;
    }
    const double* o = obs + (size_t)(2 * d + h) * D;
    xo0 = o[c];
    xo1 = c + 32 < D ? o[c + 32] : 0.0;
  };
  const int d_first = (blockIdx.x * WAVES + wave) * PAIRS_PER_WAVE;
  int on = state_of(d_first);
  if (on) fetch(d_first);   // a pair with both environments dead reads nothing from the table
#pragma unroll 1
  for (int q = 0; q < PAIRS_PER_WAVE; q++) {
    const int d = d_first + q;
    if (d >= pairs) break;
    const int env = 2 * d + h;
    const bool up = (on >> h) & 1;
    const bool run = on != 0;
    if (run) {
#pragma unroll
      for (int it = 0; it < NIT; it++) {
        const int j = lane + 64 * it;
        if (64 * it + 64 <= S::NP || j < S::NP) eps[S::pos(j)] = r[it];
      }
      x[c] = (float)xo0;
      if (c + 32 < D) x[c + 32] = (float)xo1;
    }
    on = q + 1 < PAIRS_PER_WAVE ? state_of(d + 1) : 0;
    if (on) fetch(d + 1);
    float mu = 0.0f;
    if (run) {
      wave_lds_sync();
      // layer 1: unit c of environment h
      float a = __builtin_fmaf(ss, eps[S::L_B1 + c], s_theta[S::L_B1 + c]);
#pragma unroll
      for (int k = 0; k < D; k++) {
        const int w = S::L_W1 + c * S::DP + k;
        a = __builtin_fmaf(__builtin_fmaf(ss, eps[w], s_theta[w]), x[k], a);
      }
      const float h1 = tanh_fast(a);
      wave_lds_sync();   // every lane has read the observation
      x[c] = h1;
      wave_lds_sync();
      a = __builtin_fmaf(ss, eps[S::L_B2 + c], s_theta[S::L_B2 + c]);
#pragma unroll
      for (int k = 0; k < H; k++) {
        const int w = S::L_W2 + c * S::HP + k;
        a = __builtin_fmaf(__builtin_fmaf(ss, eps[w], s_theta[w]), x[k], a);
      }
      const float h2 = tanh_fast(a);
      wave_lds_sync();
      x[c] = h2;
      wave_lds_sync();
      if (c < A) {
        a = __builtin_fmaf(ss, eps[S::L_B3 + c], s_theta[S::L_B3 + c]);
#pragma unroll
        for (int k = 0; k < H; k++) {
          const int w = S::L_W3 + c * S::HP + k;
          a = __builtin_fmaf(__builtin_fmaf(ss, eps[w], s_theta[w]), x[k], a);
        }
        mu = a;
      }
      wave_lds_sync();   // the image and the activations are free for the next pair
    }
    if (c < A) {
      const float v = up ? mu : 0.0f;   // a dead environment gets the middle of the box
      double e = lo + ((double)v + 1.0) * 0.5 * (hi - lo);
      e = e < lo ? lo : (e > hi ? hi : e);
      env_act[(size_t)env * A + c] = e;
    }
  }
}

}  // namespace cassie_es3d

namespace cassie_es3d_wide {

constexpr int D = 45, A = 10;
constexpr int H = 128;
constexpr int WAVES = 3;            // wavefronts per workgroup: what 160 KB of LDS hold next to theta's image
constexpr int PAIRS_PER_WAVE = 8;   // directions a wavefront evaluates one after the other (theta is staged once for all of them)
constexpr int PPW = WAVES * PAIRS_PER_WAVE;
constexpr int CH = 32;              // rows of W2 per chunk
constexpr int NCH = H / CH;
constexpr int UPL = H / 32;         // hidden units per lane
constexpr int HP = H + 4;           // row length of W2 in the images: 4 (mod 64), so that the 16-byte reads of a 16-lane group cover the 64 banks
constexpr int RB = 64;              // rows of W1 per block of [W1 | b1]

using cassie_tiles::tanh_fast;
using cassie_tiles::wave_lds_sync;
constexpr int cmax(int a, int b) { return a > b ? a : b; }

// The parameter row [W1 | b1 | W2 | b2 | W3 | b3], its chunks and the padded images in LDS.
struct S {
  static constexpr int NP = H * D + H + H * H + H + A * H + A;
  static constexpr int O_B1 = H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H;
  static constexpr int DP = D;   // odd as it stands: rows of W1 are not padded, in theta's image and in a block's
  static constexpr int L_W1 = 0, L_B1 = H * DP, L_W2 = L_B1 + H, L_B2 = L_W2 + H * HP, L_W3 = L_B2 + H, L_B3 = L_W3 + A * H, LN = (L_B3 + A + 3) & ~3;
  static constexpr int N_CA = RB * D, N_CB = (H - RB) * D + H;   // the two blocks of [W1 | b1]: rows 0..63; rows 64..127 and b1
  static constexpr int B_B1 = (H - RB) * D;                     // b1 in the second block's buffer
  static constexpr int N_C2 = CH * H, N_CT = NP - O_B2;         // entries of a chunk of W2 and of the tail
  static constexpr int T_W3 = H, T_B3 = H + A * H;              // the tail's buffer: [b2 | W3 | b3]
  static constexpr int BUF = (cmax(cmax(cmax(N_CA, N_CB), CH * HP), N_CT) + 3) & ~3;
  __device__ static __forceinline__ int pos2(int j) { return j + (j >> 7) * (HP - H); }   // entry j of W2 or of a chunk of it
  __device__ static __forceinline__ int pos(int j) {                                        // entry j of the row
    if (j < O_W2) return j;
    if (j < O_B2) return L_W2 + pos2(j - O_W2);
    return L_B2 + (j - O_B2);
  }
};
static_assert(S::NP == 23690 && S::LN == 24204 && (D & 1) && D > 32 && D <= 64 && A <= 32 && RB == 2 * 32 && H == 2 * RB, "two inputs per lane of a half, two units per lane and block");
static_assert(S::L_W2 % 4 == 0 && HP % 4 == 0 && S::N_CA <= 64 * 64 && S::N_CB <= 64 * 64 && S::N_C2 == 64 * 64 && S::N_CT <= 64 * 64, "16-byte reads, 64 dwords per lane");
static_assert(S::N_CA + S::N_CB == S::O_W2 && S::BUF == CH * HP, "the blocks are the row's first 5888 entries; a buffer is a chunk of W2");
static_assert((S::LN + WAVES * S::BUF + WAVES * 2 * H) * 4 <= 160 * 1024, "LDS of a CU");

__global__ void __launch_bounds__(64 * WAVES) es3d_wide_policy_step_kernel(const double* __restrict__ obs, int n, const float* __restrict__ theta,
                                                                        const float* __restrict__ table, const long long* __restrict__ offsets, float sigma,
                                                                        const uint8_t* __restrict__ alive, const double* __restrict__ low,
                                                                        const double* __restrict__ high, double* __restrict__ env_act) {
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
  // The chunk ahead (and, with the first block of a pair, the pair's observations) in registers.  `on`: bit 0 / 1 = environment 2 d / 2 d + 1 is
  // alive (uniform over the wavefront).
  float r[64];
  double xo0 = 0.0, xo1 = 0.0;   // entries c and c + 32 of the observation
  auto state_of = [&](int d) -> int {
    if (d >= pairs) return 0;
    return alive ? (alive[2 * d] != 0 ? 1 : 0) | (alive[2 * d + 1] != 0 ? 2 : 0) : 3;
  };
#define ES3D_FETCH(LEN, SRC) \
  { \
    const float* src_ = (SRC); \
    _Pragma("unroll") for (int it = 0; it < ((LEN) + 63) / 64; it++) { \
      const int j = lane + 64 * it; \
      r[it] = (64 * it + 64 <= (LEN) || j < (LEN)) ? src_[j] : 0.0f; \
    } \
  }
#define ES3D_STASH(LEN, POS) \
  { \
    _Pragma("unroll") for (int it = 0; it < ((LEN) + 63) / 64; it++) { \
      const int j = lane + 64 * it; \
      if (64 * it + 64 <= (LEN) || j < (LEN)) buf[POS(j)] = r[it]; \
    } \
  }
#define ES3D_ID(j) (j)
  auto fetch_first = [&](int d) {   // rows 0..63 of W1 of pair d and its observations
    ES3D_FETCH(S::N_CA, table + offsets[d])
    const double* o = obs + (size_t)(2 * d + h) * D;
    xo0 = o[c];
    xo1 = c + 32 < D ? o[c + 32] : 0.0;
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
      // ---- layer 1, first block: rows c and c + 32 of W1
      ES3D_STASH(S::N_CA, ES3D_ID)
      x[c] = (float)xo0;
      if (c + 32 < D) x[c + 32] = (float)xo1;
      ES3D_FETCH(S::N_CB, src + S::N_CA)
      wave_lds_sync();
      float a1[UPL];
#pragma unroll
      for (int u = 0; u < UPL; u++) a1[u] = 0.0f;
#pragma unroll
      for (int k = 0; k < D; k++) {
        const float xk = x[k];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const int w = (32 * u + c) * D + k;
          a1[u] = __builtin_fmaf(__builtin_fmaf(ss, buf[w], s_theta[S::L_W1 + w]), xk, a1[u]);
        }
      }
      // ---- second block: rows 64 + c and 96 + c, then b1 of all four units
      wave_lds_sync();   // the buffer is free
      ES3D_STASH(S::N_CB, ES3D_ID)
      ES3D_FETCH(S::N_C2, src + S::O_W2)
      wave_lds_sync();
#pragma unroll
      for (int k = 0; k < D; k++) {
        const float xk = x[k];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const int w = (32 * u + c) * D + k;
          a1[2 + u] = __builtin_fmaf(__builtin_fmaf(ss, buf[w], s_theta[S::L_W1 + RB * D + w]), xk, a1[2 + u]);
        }
      }
#pragma unroll
      for (int u = 0; u < UPL; u++) a1[u] += __builtin_fmaf(ss, buf[S::B_B1 + 32 * u + c], s_theta[S::L_B1 + 32 * u + c]);
      wave_lds_sync();   // every lane has read the observation
#pragma unroll
      for (int u = 0; u < UPL; u++) x[32 * u + c] = tanh_fast(a1[u]);
      // ---- chunks of W2: rows 32 j + c against the activations of layer 1, two partial sums (even / odd columns) per unit
      float a2[NCH];
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        wave_lds_sync();   // the buffer is free (and, for j = 0, the activations are written)
        ES3D_STASH(S::N_C2, S::pos2)
        if (j + 1 < NCH) ES3D_FETCH(S::N_C2, src + S::O_W2 + (j + 1) * S::N_C2)
        else ES3D_FETCH(S::N_CT, src + S::O_B2)
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
      ES3D_STASH(S::N_CT, ES3D_ID)
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
#undef ES3D_FETCH
#undef ES3D_STASH
#undef ES3D_ID
}

}  // namespace cassie_es3d_wide

extern "C" {

int CassieEs3dParamCount(int obs_dim, int act_dim) { return obs_dim == cassie_es3d::D && act_dim == cassie_es3d::A ? cassie_es3d::S::NP : 0; }

int CassieEs3dPairsPerWorkgroup(void) { return cassie_es3d::PPW; }

int CassieEs3dPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* theta_dev, const float* table_dev, long long table_len,
                         const long long* offsets_dev, float sigma, const unsigned char* alive_dev, const double* low_dev, const double* high_dev,
                         double* env_actions_dev, void* stream) {
  using namespace cassie_es3d;
  const int np = CassieEs3dParamCount(obs_dim, act_dim);
  if (!obs_dev || n <= 0 || (n & 1) || np == 0 || !theta_dev || !table_dev || table_len < np || !offsets_dev || !low_dev || !high_dev || !env_actions_dev)
    return CASSIE_EINVAL;
  const dim3 grid(((n >> 1) + PPW - 1) / PPW), block(64 * WAVES);
  hipLaunchKernelGGL(es3d_policy_step_kernel, grid, block, 0, (hipStream_t)stream, obs_dev, n, theta_dev, table_dev, offsets_dev, sigma, alive_dev, low_dev, high_dev,
                     env_actions_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieEs3dWideParamCount(int obs_dim, int act_dim) { return obs_dim == cassie_es3d_wide::D && act_dim == cassie_es3d_wide::A ? cassie_es3d_wide::S::NP : 0; }

int CassieEs3dWidePairsPerWorkgroup(void) { return cassie_es3d_wide::PPW; }

int CassieEs3dWidePolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* theta_dev, const float* table_dev, long long table_len,
                             const long long* offsets_dev, float sigma, const unsigned char* alive_dev, const double* low_dev, const double* high_dev,
                             double* env_actions_dev, void* stream) {
  using namespace cassie_es3d_wide;
  const int np = CassieEs3dWideParamCount(obs_dim, act_dim);
  if (!obs_dev || n <= 0 || (n & 1) || np == 0 || !theta_dev || !table_dev || table_len < np || !offsets_dev || !low_dev || !high_dev || !env_actions_dev)
    return CASSIE_EINVAL;
  const dim3 grid(((n >> 1) + PPW - 1) / PPW), block(64 * WAVES);
  hipLaunchKernelGGL(es3d_wide_policy_step_kernel, grid, block, 0, (hipStream_t)stream, obs_dev, n, theta_dev, table_dev, offsets_dev, sigma, alive_dev, low_dev, high_dev,
                     env_actions_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
