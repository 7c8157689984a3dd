// tu_pg.hip -- fused kernels of the width-128 policy (include/cassie_trpo.h, "width-128 policy"; rllab/envs/vpg_cassie.py:15-48):
// the sampler's policy step, the policy gradient J' w of the 128-128 tanh mean network, and Lasagne's Adam step.
//
// The layout is tu_trpo.hip's (read its header first): exact float32 v_mfma_f32_32x32x2_f32, a tile of 32 samples per wavefront, every
// activation in the accumulator layout (sample on the lane c = lane & 31, hidden unit r(v, h) = (v & 3) + 8 (v >> 2) + 4 h in register v),
// so that tanh and 1 - h^2 are register-wise and a layer takes the previous activation's registers as its B operand.  A 128-wide layer
// is four 32-row blocks (v16f[4], 64 registers); the 128 x 128 layer is 4 x 4 blocks of 16 k-steps (256 MFMAs per tile).
//
// Differences from the width-32 kernels, and why:
//   * the A operands are read straight from global memory (L1 / L2), not from a per-workgroup LDS image.  In the accumulator order the
//     four k-steps 4 g .. 4 g + 3 of lane (c, h) are W[row][32 kb + 8 g + 4 h + 0..3]: one aligned float4 of a row-major weight.  At
//     65 536 environments there are two tiles per SIMD, so an image (93 KB per workgroup) would be read from L2 about as often as the
//     weights themselves, and it would allow one workgroup per CU.  The policy step runs one tile per wavefront: with a tile loop the
//     compiler hoists a tile's 372 weight loads out of it and spills;
//   * the VJP's gradient accumulators do not fit one wavefront (gW2 alone is 256 registers per lane).  The four wavefronts of a
//     workgroup each run the forward and backward pass of their own tile and put its transposed tiles in LDS (two slots of
//     4 x 128 x 36 floats = 144 KB, three exchanges per group of four tiles: H1 and H2, then G2, then G1), and wavefront q accumulates
//     the 32-row quarter q of gW1, gW2 and the 32-column quarter q of gW3 from all four tiles (96 accumulator registers).  One row of
//     partial sums per WORKGROUP; the caller adds the rows;
//   * the 6- or 7-row output layer is padded to 32 rows, as in tu_trpo.hip (64 of the 372 MFMAs of a forward tile).
// Where the pieces live: the layout primitives in cassie_tiles.h; shapes, forward pass, wave_put / wave_get and vjp_blocks in cassie_pg_net.h; the VJP's
// reverse pass of a group and the workgroup's row store in cassie_pg_vjp.inc / cassie_pg_vjp_row.inc (text shared with tu_ppo.hip's clip-gradient
// kernel); the (obs_dim, act_dim) dispatch and the argument check (launch_shape, net_ok16) in cassie_tiles.h.
// Every sum runs in a fixed order (k-ordered MFMA chains, tiles in a fixed order per workgroup, a fixed grid for a given n): a run
// repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_pg_net.h"   // H, WAVES, Shape, gemm_block, forward_hidden, wave_put, wave_get (shared with tu_pg_trpo.hip, tu_ppo.hip)

namespace cassie_pg {

// ---------------------------------------------------------------------------------------------------------------- policy step
// CassieTrpoPolicyStep's contract for the 128-128 network: a wavefront per tile of 32 environments; the mean comes out with action
// a = v + 4 h in register v < 4 of lane (environment, h).
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) pg_policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ log_std,
                                                                   const float* __restrict__ noise, const double* __restrict__ low, const double* __restrict__ high,
                                                                   float* __restrict__ obs32, float* __restrict__ mean, float* __restrict__ act, double* __restrict__ env_act) {
  constexpr int KS1 = (D + 1) / 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  float sd[4];
  double lo[4], hi[4];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int a = v + 4 * h;
    sd[v] = a < A ? expf(log_std[a]) : 0.0f;
    lo[v] = a < A ? low[a] : 0.0; hi[v] = a < A ? high[a] : 0.0;
  }
  {   // one tile per wavefront: no loop for the compiler to hoist the 372 weight loads of a tile out of (they would not fit in registers)
    const int smp = (blockIdx.x * WAVES + wave) * 32 + c;
    const bool valid = smp < n;
    float xb[KS1];
#pragma unroll
    for (int s = 0; s < KS1; s++) {
      const int k = 2 * s + h;
      const bool on = valid && k < D;
      xb[s] = on ? (float)obs[(size_t)smp * D + k] : 0.0f;
      if (on) obs32[(size_t)smp * D + k] = xb[s];
    }
    v16f h1[NB], h2[NB];
    forward_hidden<D>(th, xb, h1, h2, c, h);
    v16f mu;
#pragma unroll
    for (int v = 0; v < 16; v++) mu[v] = (v < 4 && v + 4 * h < A) ? th.b3[v + 4 * h] : 0.0f;
#pragma unroll
    for (int kb = 0; kb < NB; kb++) gemm_block(th.W3, H, 0, 32 * kb, c < A, h2[kb], mu, c, h);
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int a = v + 4 * h;
      if (valid && a < A) {
        const size_t o = (size_t)smp * A + a;
        const float val = mu[v] + noise[o] * sd[v];
        mean[o] = mu[v]; act[o] = val;
        double e = lo[v] + ((double)val + 1.0) * 0.5 * (hi[v] - lo[v]);
        e = e < lo[v] ? lo[v] : (e > hi[v] ? hi[v] : e);
        env_act[o] = e;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- VJP
// partial [gridDim.x][NP]: J' w of this workgroup's tiles, [gW1 | gb1 | gW2 | gb2 | gW3 | gb3].  Wavefront q writes rows 32 q .. 32 q + 31
// of gW1 / gb1 / gW2 / gb2 and columns 32 q .. 32 q + 31 of gW3; wavefront 0 writes gb3.
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) pg_vjp_kernel(const float* __restrict__ obs, int n, Net th0, const float* __restrict__ wext, float* __restrict__ partial) {
  typedef Shape<D, A> S;
  static_assert(D < 32 && A <= 8, "a column of ones next to the observations; the cotangent rows in registers 0..3 of the two lane halves");
  constexpr int KS1 = (D + 1) / 2;
  __shared__ alignas(16) float stage[2][WAVES][H * TP];
  __shared__ Net snet;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid == 0) snet = th0;
  v16f gW2[NB], gW1 = zero16(), gW3 = zero16();
#pragma unroll
  for (int b = 0; b < NB; b++) gW2[b] = zero16();
  float gb2 = 0.0f, gb3 = 0.0f;
  const int ntiles = (n + 31) / 32, ngroups = (ntiles + WAVES - 1) / WAVES;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {   // the same trip count for every wavefront of the workgroup
    // The weight pointers are re-read from LDS behind the barrier: loads through them cannot be hoisted out of the loop (the compiler
    // otherwise keeps ~800 weight values of a tile in registers across the iterations, and spills).  The barrier also orders this
    // group's first LDS writes after the previous group's last reads.
    __syncthreads();
    const Net th = snet;
    const int gs0 = grp * WAVES * 32;                               // first sample of the group; tile u starts at gs0 + 32 u
    const int s0 = gs0 + 32 * wave, smp = s0 + c;
    const bool valid = smp < n;                                    // a tile past the end runs with w = 0: its G2, G1 are zero
    float xb[KS1];
#pragma unroll
    for (int s = 0; s < KS1; s++) { const int k = 2 * s + h; xb[s] = (valid && k < D) ? obs[(size_t)smp * D + k] : 0.0f; }
    v16f h1[NB], h2[NB], g2[NB], g1[NB];
    forward_hidden<D>(th, xb, h1, h2, c, h);
    float wt[4];
#pragma unroll
    for (int v = 0; v < 4; v++) wt[v] = (valid && v + 4 * h < A) ? wext[(size_t)smp * A + v + 4 * h] : 0.0f;
    // the reverse pass of the group reads the cotangent and the observations of the OTHER wavefronts' tiles, transposed, from memory
#define PG_VJP_COT_ROW(u, wa) \
  _Pragma("unroll") for (int e = 0; e < 16; e++) { const int sm = gs0 + 32 * (u) + 16 * h + e; (wa)[e] = (c < A && sm < n) ? wext[(size_t)sm * A + c] : 0.0f; }   // sm: the sample of k-step e
#define PG_VJP_OBS_T(u, e, x) { const int sm = gs0 + 32 * (u) + 16 * h + (e); (x) = c < D ? (sm < n ? obs[(size_t)sm * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f); }
#include "cassie_pg_vjp.inc"
#undef PG_VJP_COT_ROW
#undef PG_VJP_OBS_T
  }
  float* out = partial + (size_t)blockIdx.x * S::NP;
#include "cassie_pg_vjp_row.inc"
}

// ---------------------------------------------------------------------------------------------------------------- Adam
// Lasagne's adam (lasagne.updates.adam), one lane per parameter: t is the step count AFTER the increment;
//   a = lr sqrt(1 - beta2^t) / (1 - beta1^t),  m = beta1 m + (1 - beta1) g,  v = beta2 v + (1 - beta2) g^2,  theta -= a m / (sqrt(v) + eps).
__global__ void __launch_bounds__(256) pg_adam_kernel(int n, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float* __restrict__ theta,
                                                      float a, float beta1, float beta2, float eps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  const float mi = beta1 * m[i] + (1.0f - beta1) * gi;   // 1 - beta is exact in float32
  const float vi = beta2 * v[i] + (1.0f - beta2) * (gi * gi);
  m[i] = mi; v[i] = vi;
  theta[i] = theta[i] - a * mi / (sqrtf(vi) + eps);
}

inline int step_blocks(int n) { return ((n + 31) / 32 + WAVES - 1) / WAVES; }
}  // namespace cassie_pg

extern "C" {

int CassiePgParamCount(int obs_dim, int act_dim) {
  if ((obs_dim != 26 && obs_dim != 17) || (act_dim != 6 && act_dim != 7)) return 0;
  return 128 * obs_dim + 128 + 128 * 128 + 128 + act_dim * 128 + act_dim;
}
int CassiePgPartialRows(int n_samples) { return cassie_pg::vjp_blocks(n_samples); }

int CassiePgPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2,
                       const float* b2, const float* W3, const float* b3, const float* log_std, const float* noise_dev,
                       const double* low_dev, const double* high_dev, float* obs32_dev, float* mean_dev, float* act_dev,
                       double* env_actions_dev, void* stream) {
  using namespace cassie_pg;
  const Net th{W1, b1, W2, b2, W3, b3};
  if (!obs_dev || n <= 0 || !net_ok16(th) || !log_std || !noise_dev || !low_dev || !high_dev || !obs32_dev || !mean_dev || !act_dev || !env_actions_dev)
    return CASSIE_EINVAL;
  return launch_shape<true>(obs_dim, act_dim, [&](auto d, auto a) {
    hipLaunchKernelGGL((pg_policy_step_kernel<d(), a()>), dim3(step_blocks(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, log_std, noise_dev, low_dev, high_dev,
                       obs32_dev, mean_dev, act_dev, env_actions_dev);
  });
}

int CassiePgVjp(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* W3, const float* b3, const float* w_dev, float* partial_dev, void* stream) {
  using namespace cassie_pg;
  const Net th{W1, b1, W2, b2, W3, b3};
  if (!obs_dev || n <= 0 || !net_ok16(th) || !w_dev || !partial_dev) return CASSIE_EINVAL;
  return launch_shape(obs_dim, act_dim, [&](auto d, auto a) {
    hipLaunchKernelGGL((pg_vjp_kernel<d(), a()>), dim3(vjp_blocks(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, w_dev, partial_dev);
  });
}

int CassiePgAdam(int n, const float* g, float* m, float* v, float* theta, int t, float lr, float beta1, float beta2, float eps, void* stream) {
  if (n <= 0 || !g || !m || !v || !theta || t < 1) return CASSIE_EINVAL;
  const double a = (double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t));
  hipLaunchKernelGGL(cassie_pg::pg_adam_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, g, m, v, theta, (float)a, beta1, beta2, eps);
  return cassie_tiles::launched();
}

}  // extern "C"
