// tu_es.hip -- kernels of the evolution strategy (cassierl_amd/es.py, include/cassie_trpo.h: CassieEs*).
//
// ES evaluates a POPULATION: environment i runs the 32 x 32 tanh mean network with its own weights w_i = theta + s_i sigma eps_(i >> 1), s_i = +1 for
// even i and -1 for odd i, eps_d = table[off_d : off_d + P] a slice of one shared noise table.  The matrix-core policy steps (tu_trpo.hip) share one
// weight image among the 32 samples of a tile and cannot express that; the torch route materialises the [n, P] weight matrix (555 MB at 65 536
// environments) and runs a dozen bmm / element-wise launches on it.  Here the weights never exist in memory:
//
//   * policy step: a wavefront per direction (pair of environments).  theta is staged in LDS once per workgroup, the wavefront copies its eps slice
//     from the table into its own LDS image with coalesced dword loads (an offset has any alignment), and lane (h, c) = (lane >> 5, lane & 31)
//     evaluates hidden unit c of environment 2 d + h: weight = fmaf(s sigma, eps, theta) formed on the fly, the activations of a layer passed
//     through 64 floats of LDS and read back as broadcasts.  Rows of W1 are padded to an odd length and rows of W2, W3 to 33 floats in both images,
//     so that the 32 lanes of a half read 32 different banks.  The action map runs in double exactly as tu_trpo.hip's policy_step_kernel writes it.
//     What the kernel costs is the table read (P floats per pair: 277 MB per step at 65 536 environments); no matrix cores.
//   * bookkeeping of a step (fitness, length, alive) in one launch, one lane per environment.
//   * gradient: partial[r][k] = sum over the directions of row r of w_d table[off_d + k], lane = parameter k (coalesced table reads, w_d and off_d
//     uniform over the wavefront), the directions of a row in ascending order: a call repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_tiles.h"   // tanh_fast, wave_lds_sync

namespace cassie_es {

constexpr int H = 32;
constexpr int WAVES = 4;            // wavefronts per workgroup
constexpr int PAIRS_PER_WAVE = 4;   // directions a wavefront evaluates one after the other (theta is staged once for all of them)
constexpr int PPW = WAVES * PAIRS_PER_WAVE;
constexpr int GRAD_BLOCK = 256;     // parameters per workgroup of the gradient kernel
constexpr int GRAD_MAX_ROWS = 128;
constexpr int GRAD_MIN_CHUNK = 64;  // directions per row before a second row is opened

using cassie_tiles::tanh_fast;       // 1 - 2 / (e^2x + 1) through the hardware exp2 / rcp, absolute error ~1e-7, exact at the saturated ends
using cassie_tiles::wave_lds_sync;

// The parameter row [W1 | b1 | W2 | b2 | W3 | b3] (mlp32_tiles.h's actor row) and its padded image in LDS.
template <int D, int A> struct Shape {
  static constexpr int NP = H * D + H + H * H + H + A * H + A;
  static constexpr int O_B1 = H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H;
  static constexpr int DP = D | 1, HP = H + 1;   // row lengths of the image: odd, so the lanes of a half hit different banks
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

template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 3) es_policy_step_kernel(const double* __restrict__ obs, int n, const float* __restrict__ theta,
                                                                    const float* __restrict__ table, const long long* __restrict__ offsets, float sigma,
                                                                    const uint8_t* __restrict__ alive, const double* __restrict__ low,
                                                                    const double* __restrict__ high, double* __restrict__ env_act) {
  typedef Shape<D, A> S;
  static_assert(D <= 32 && A <= 32, "one lane per input / output of a half");
  __shared__ float s_theta[S::LN];
  __shared__ float s_eps[WAVES][S::LN];
  __shared__ float s_x[WAVES][2][H];   // the observation, then the activations of a layer: [environment of the pair][unit]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  for (int j = tid; j < S::NP; j += 64 * WAVES) s_theta[S::pos(j)] = theta[j];
  __syncthreads();
  const int pairs = n >> 1;
  constexpr int NIT = (S::NP + 63) / 64;   // dwords of a direction per lane
  float* eps = s_eps[wave];
  float* x = s_x[wave][h];
  const float ss = h ? -sigma : sigma;
  const double lo = c < A ? low[c] : 0.0, hi = c < A ? high[c] : 0.0;
  // A pair's slice of the table and its observations are fetched into registers one pair ahead, so that the reads of pair q + 1 are in flight
  // while pair q is evaluated out of LDS.  `on`: bit 0 / 1 = environment 2 d / 2 d + 1 is alive (uniform over the wavefront).
  float r[NIT];
  double xo = 0.0;
  auto state_of = [&](int d) -> int {
    if (d >= pairs) return 0;
    return alive ? (alive[2 * d] != 0 ? 1 : 0) | (alive[2 * d + 1] != 0 ? 2 : 0) : 3;
  };
  auto fetch = [&](int d) {
    const float* src = table + offsets[d];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int j = lane + 64 * it;
      r[it] = j < S::NP ? src[j] : 0.0f;
    }
    xo = c < D ? obs[(size_t)(2 * d + h) * D + c] : 0.0;
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
        if (j < S::NP) eps[S::pos(j)] = r[it];
      }
      if (c < D) x[c] = (float)xo;
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

__global__ void __launch_bounds__(256) es_book_kernel(const double* __restrict__ rew, const uint8_t* __restrict__ done, int n, uint8_t* __restrict__ alive,
                                                      double* __restrict__ fitness, long long* __restrict__ length) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool up = alive[i] != 0;
  if (up) { fitness[i] += rew[i]; length[i] += 1; }
  alive[i] = up && done[i] == 0 ? 1 : 0;
}

inline int grad_rows(int m) {
  if (m <= 0) return 0;
  const int r = (m + GRAD_MIN_CHUNK - 1) / GRAD_MIN_CHUNK;
  return r > GRAD_MAX_ROWS ? GRAD_MAX_ROWS : r;
}

// Row r = blockIdx.y sums the directions [r chunk, min(m, (r + 1) chunk)) in ascending order; four table reads are in flight per lane.
__global__ void __launch_bounds__(GRAD_BLOCK) es_grad_kernel(const float* __restrict__ table, const long long* __restrict__ offsets, const float* __restrict__ w,
                                                             int m, int n_params, int chunk, float* __restrict__ partial) {
  const int k = blockIdx.x * GRAD_BLOCK + threadIdx.x;
  if (k >= n_params) return;
  const int d0 = blockIdx.y * chunk;
  int d1 = d0 + chunk;
  if (d1 > m) d1 = m;
  float acc = 0.0f;
  int d = d0;
  for (; d + 4 <= d1; d += 4) {
    const float e0 = table[offsets[d] + k], e1 = table[offsets[d + 1] + k], e2 = table[offsets[d + 2] + k], e3 = table[offsets[d + 3] + k];
    acc = __builtin_fmaf(w[d], e0, acc);
    acc = __builtin_fmaf(w[d + 1], e1, acc);
    acc = __builtin_fmaf(w[d + 2], e2, acc);
    acc = __builtin_fmaf(w[d + 3], e3, acc);
  }
  for (; d < d1; d++) acc = __builtin_fmaf(w[d], table[offsets[d] + k], acc);
  partial[(size_t)blockIdx.y * n_params + k] = acc;
}

}  // namespace cassie_es

extern "C" {

int CassieEsParamCount(int obs_dim, int act_dim) {
  if ((obs_dim != 26 && obs_dim != 17) || (act_dim != 6 && act_dim != 7)) return 0;
  return cassie_es::H * obs_dim + cassie_es::H + cassie_es::H * cassie_es::H + cassie_es::H + act_dim * cassie_es::H + act_dim;
}

int CassieEsPairsPerWorkgroup(void) { return cassie_es::PPW; }

int CassieEsPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* theta_dev, const float* table_dev, long long table_len,
                       const long long* offsets_dev, float sigma, const unsigned char* alive_dev, const double* low_dev, const double* high_dev,
                       double* env_actions_dev, void* stream) {
  using namespace cassie_es;
  const int np = CassieEsParamCount(obs_dim, act_dim);
  if (!obs_dev || n <= 0 || (n & 1) || np == 0 || !theta_dev || !table_dev || table_len < np || !offsets_dev || !low_dev || !high_dev || !env_actions_dev)
    return CASSIE_EINVAL;
  const dim3 grid(((n >> 1) + PPW - 1) / PPW), block(64 * WAVES);
  hipStream_t s = (hipStream_t)stream;
#define ES_STEP_CASE(D, A) \
  if (obs_dim == D && act_dim == A) \
    hipLaunchKernelGGL((es_policy_step_kernel<D, A>), grid, block, 0, s, obs_dev, n, theta_dev, table_dev, offsets_dev, sigma, alive_dev, low_dev, high_dev, env_actions_dev);
  ES_STEP_CASE(26, 6) ES_STEP_CASE(26, 7) ES_STEP_CASE(17, 6) ES_STEP_CASE(17, 7)
#undef ES_STEP_CASE
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieEsBook(const double* rew_dev, const unsigned char* done_dev, int n, unsigned char* alive_dev, double* fitness_dev, long long* length_dev, void* stream) {
  if (!rew_dev || !done_dev || n <= 0 || !alive_dev || !fitness_dev || !length_dev) return CASSIE_EINVAL;
  hipLaunchKernelGGL(cassie_es::es_book_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, rew_dev, done_dev, n, alive_dev, fitness_dev, length_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieEsGradRows(int m) { return cassie_es::grad_rows(m); }

int CassieEsGrad(const float* table_dev, long long table_len, const long long* offsets_dev, const float* w_dev, int m, int n_params, float* partial_dev,
                 void* stream) {
  using namespace cassie_es;
  if (!table_dev || !offsets_dev || !w_dev || m <= 0 || n_params < 1 || table_len < n_params || !partial_dev) return CASSIE_EINVAL;
  const int rows = grad_rows(m), chunk = (m + rows - 1) / rows;
  hipLaunchKernelGGL(es_grad_kernel, dim3((n_params + GRAD_BLOCK - 1) / GRAD_BLOCK, rows), dim3(GRAD_BLOCK), 0, (hipStream_t)stream, table_dev, offsets_dev, w_dev, m,
                     n_params, chunk, partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
