// tu_ppo.hip -- kernels of PPO (include/cassie_trpo.h, "PPO"; cassierl_amd/ppo.py): GAE(lambda) advantages of the [T][n] batch, and the
// gradient of the clipped surrogate on one minibatch for the two policy widths.
//
// The clip-gradient kernels are the VJP kernels of their width (tu_trpo.hip: trpo_kernel<FVP = false>; tu_pg.hip: pg_vjp_kernel; read those
// headers first, the layouts are theirs) with two differences:
//   * the samples of a tile are rows of the batch gathered through a minibatch index (position p of the minibatch -> row idx[p], clamped);
//   * the cotangent on the mean does not come from memory.  PPO's cotangent depends on the forward pass at the CURRENT weights (likelihood
//     ratio, clip mask), so the forward pass runs on through the output layer -- the mean leaves it with action a = v + 4 h in register
//     v < 4 of lane (sample, h), which is the layout the reverse pass takes its cotangent in -- and ratio, mask, weight and cotangent are
//     formed in those registers (clip_cotangent below).  The log-likelihood difference is the difference of the two quadratic forms and of
//     the log-stds, never two large log-likelihoods: the ratio stays accurate near 1, where the clip decision is taken.
// Besides the parameter gradient a row carries g_log_std (without an entropy bonus: a constant of the caller) and three float64 statistics
// (clipped-surrogate loss, KL(old || new), clipped samples).  Fixed summation order throughout: a call repeats bit for bit.
// What a clip-gradient kernel has in common with the VJP kernel of its width is one copy: cassie_onpolicy.h's tanh32 (the policy's row, the reverse
// pass of a tile with its accumulation, the row store) for width 32; cassie_pg_net.h with cassie_pg_vjp.inc / cassie_pg_vjp_row.inc (the reverse
// pass of a group of four tiles and the workgroup's row store, shared as text) for width 128.  The kernels here supply the minibatch gather, the
// output layer and the cotangent.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_onpolicy.h"
#include "cassie_pg_net.h"

namespace cassie_ppo {

// ---------------------------------------------------------------------------------------------------------------- GAE
using cassie_onpolicy::clip10;   // tu_trpo_baseline.hip's feature arithmetic (float32 as the torch expressions evaluate it, promoted to float64)
using cassie_onpolicy::path_clock;

// One lane per environment, backwards over the T steps of its column.  The value of a sample is evaluated once: it is V(s_t) of its own
// step and, carried in a register, V(s_{t+1}) of the step before it.
template <int D>
__global__ void __launch_bounds__(256) gae_kernel(const float* __restrict__ obs, const long long* __restrict__ t, const double* __restrict__ rew,
                                                  const uint8_t* __restrict__ cut, int T, int n, const double* __restrict__ coeffs,
                                                  const double* __restrict__ last_value, double gamma, double lambda, double* __restrict__ returns,
                                                  double* __restrict__ adv, double* __restrict__ partial) {
  constexpr int NF = 2 * D + 4;
  __shared__ double red[2][256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  if (i < n) {
    double run = last_value ? last_value[i] : 0.0;
    double v_next = run, a_next = 0.0;
    for (int tt = T - 1; tt >= 0; tt--) {
      const size_t s = (size_t)tt * n + i;
      double value = 0.0;
      if (coeffs) {
        const float* o = obs + s * D;
        const float al = path_clock(t[s]);
#pragma unroll
        for (int j = 0; j < D; j++) {
          const float v = clip10(o[j]);
          value = fma((double)v, coeffs[j], value);
          value = fma((double)(v * v), coeffs[D + j], value);
        }
        value = fma((double)al, coeffs[2 * D], value);
        value = fma((double)(al * al), coeffs[2 * D + 1], value);
        value = fma((double)(al * al * al), coeffs[2 * D + 2], value);
        value += coeffs[NF - 1];
      }
      const double r = rew[s], live = cut[s] ? 0.0 : 1.0;
      run = r + gamma * run * live;
      const double delta = r + gamma * live * v_next - value;
      const double a = delta + gamma * lambda * live * a_next;
      returns[s] = run; adv[s] = a;
      s1 += a; s2 += a * a;
      v_next = value; a_next = a;
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

// ---------------------------------------------------------------------------------------------------------------- the cotangent
struct Clip {   // what a launch adds to the VJP's arguments
  const long long* idx;
  int m;
  const float *act, *adv, *old_mean, *ls_old, *ls_new;
  float clip, scale;
};

// per-action constants of the two Gaussians for the actions a = v + 4 h of this lane half (GaussianMLPPolicy.log_likelihood / .kl of trpo.py)
struct Gauss { float isn[4], iso[4], dls[4], kden[4], kvar[4]; };
template <int A> __device__ __forceinline__ void gauss_init(Gauss& g, const float* __restrict__ ls_new, const float* __restrict__ ls_old, int h) {
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int a = v + 4 * h;
    const float ln = a < A ? ls_new[a] : 0.0f, lo = a < A ? ls_old[a] : 0.0f;
    const float sn = expf(ln), so = expf(lo);
    g.isn[v] = 1.0f / sn; g.iso[v] = 1.0f / so; g.dls[v] = ln - lo;
    g.kden[v] = 1.0f / (2.0f * sn * sn + 1e-8f); g.kvar[v] = so * so - sn * sn;
  }
}

// batch row of minibatch position p (-1 behind the end of the minibatch)
__device__ __forceinline__ int batch_row(const Clip& k, int p, int n) {
  if (p >= k.m) return -1;
  if (!k.idx) return p;
  const long long r = k.idx[p];
  return (int)(r < 0 ? 0 : (r >= n ? (long long)n - 1 : r));
}

__device__ __forceinline__ float mul_rn(float a, float b) {   // a product that is rounded: never contracted into a multiply-add
#pragma clang fp contract(off)
  return a * b;
}

// One sample on lanes (c, 0) and (c, 1): mean mu[v] of action a = v + 4 h -> cotangent wt[v] = d L / d mean = -scale w z / std, and this
// lane's sums: g_log_std (actions of its half), and on the h = 0 lane the sample's loss term, KL and clip flag.
template <int A>
__device__ __forceinline__ void clip_cotangent(const Clip& k, const Gauss& g, int row, int h, const float (&mu)[4], float (&wt)[4], float (&gls)[4], double& accL,
                                               double& accK, double& accC) {
  const bool valid = row >= 0;
  float ll = 0.0f, kl = 0.0f, zn[4];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    zn[v] = 0.0f;
    if (valid && v + 4 * h < A) {
      const size_t o = (size_t)row * A + v + 4 * h;
      const float ac = k.act[o], om = k.old_mean[o];
      const float zo = (ac - om) * g.iso[v], dm = om - mu[v];
      zn[v] = (ac - mu[v]) * g.isn[v];
      ll += 0.5f * (zo * zo - zn[v] * zn[v]) - g.dls[v];
      kl += (dm * dm + g.kvar[v]) * g.kden[v] + g.dls[v];
    }
  }
  ll += __shfl_xor(ll, 32, 64); kl += __shfl_xor(kl, 32, 64);
  const float ad = valid ? k.adv[row] : 0.0f;
  const float ratio = expf(ll), lo = 1.0f - k.clip, hi = 1.0f + k.clip;
  const bool clipped = (ad > 0.0f && ratio > hi) || (ad < 0.0f && ratio < lo);
  const float w = (valid && !clipped) ? ratio * ad : 0.0f;
  const float ws = -k.scale * w;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const bool on = v + 4 * h < A;
    wt[v] = on ? ws * zn[v] * g.isn[v] : 0.0f;
    // g_log_std's term ws (z^2 - 1), with its roundings written out.  Left to the compiler's contraction, which multiply-adds are fused depends on the
    // code AROUND this function (the order it is inlined in), and two builds of the same arithmetic differ in the row's last bit.  The form is the one
    // these kernels have had since they exist: z^2 - 1 fused (not for the last action of act_dim 7, whose z^2 is the rounded one of the likelihood), the
    // sums of the lane's first two actions fused, the other two a rounded product behind the mask.
    const float t = (A == 7 && v == 3) ? mul_rn(zn[v], zn[v]) - 1.0f : __builtin_fmaf(zn[v], zn[v], -1.0f);
    if (v < 2) gls[v] = __builtin_fmaf(t, ws, gls[v]);
    else gls[v] += on ? mul_rn(ws, t) : 0.0f;
  }
  if (h == 0 && valid) {
    accL -= (double)fminf(ratio * ad, fminf(fmaxf(ratio, lo), hi) * ad);
    accK += (double)kl;
    accC += clipped ? 1.0 : 0.0;
  }
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float half_sum32(float v) {   // over the 32 lanes of one half h
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- width 32
namespace w32 {

using namespace cassie_onpolicy;
using namespace cassie_onpolicy::tanh32;   // H, TP, WAVES, Shape, blocks_for, the A-operand images, Grad, reverse_tile, store_row

// trpo_kernel<D, A, false> with the output layer and the cotangent between its forward and reverse pass; one row of partial sums and of
// statistics per wavefront.
enum { Q_W1 = 0, Q_W2 = 4, Q_W3 = 8, Q_W2T = 12, Q_W3T = 16, Q_N = 17 };
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) clip_grad_kernel(const float* __restrict__ obs, int n, Net th, Clip k, float* __restrict__ partial,
                                                              double* __restrict__ stats) {
  typedef Shape<D, A> S;
  static_assert(D < 32 && A <= 8, "a column of ones next to the observations; the cotangent rows in registers 0..3 of the two lane halves");
  constexpr int KS1 = (D + 1) / 2;
  __shared__ alignas(16) float tile[WAVES][2][32 * TP];
  __shared__ alignas(16) float sbias[3][32];   // b1, b2, b3 (zero padded)
  __shared__ float4 wimg[Q_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) { sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = tid < A ? th.b3[tid] : 0.0f; }
  const Grp img[] = {{K_FIRST, th.W1, Q_W1, 4}, {K_HID, th.W2, Q_W2, 4}, {K_OUT, th.W3, Q_W3, 4}, {K_HIDT, th.W2, Q_W2T, 4}, {K_W3T, th.W3, Q_W3T, 1}};
  fill_images<D, A>(wimg, img, wave, lane);
  Gauss gs;
  gauss_init<A>(gs, k.ls_new, k.ls_old, h);
  __syncthreads();
  float* t0 = tile[wave][0];
  float* t1 = tile[wave][1];
  Grad g;
  zero(g);
  float gls[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  double accL = 0.0, accK = 0.0, accC = 0.0;
  const int ntiles = (k.m + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    const int row = batch_row(k, tl * 32 + c, n);   // this lane's sample (both halves h)
    const bool valid = row >= 0;
    float xb[KS1], xt[16], aw[16];
#pragma unroll
    for (int s = 0; s < KS1; s++) { const int kk = 2 * s + h; xb[s] = (valid && kk < D) ? obs[(size_t)row * D + kk] : 0.0f; }
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int rs = __shfl(row, 16 * h + s, 64);   // the row of the tile's sample 16 h + s
      xt[s] = c < D ? (rs >= 0 ? obs[(size_t)rs * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f);
    }
    v16f h1 = bias_tile(sbias[0], h);
    aop(wimg, Q_W1, lane, aw);
#pragma unroll
    for (int s = 0; s < KS1; s++) h1 = TILE_MFMA(aw[s], xb[s], h1);
#pragma unroll
    for (int v = 0; v < 16; v++) h1[v] = tanh_fast(h1[v]);
    v16f h2 = bias_tile(sbias[1], h);
    aop(wimg, Q_W2, lane, aw);
#pragma unroll
    for (int v = 0; v < 16; v++) h2 = TILE_MFMA(aw[v], h1[v], h2);
#pragma unroll
    for (int v = 0; v < 16; v++) h2[v] = tanh_fast(h2[v]);
    v16f wt;
    {
      v16f mu = bias_tile(sbias[2], h);
      aop(wimg, Q_W3, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) mu = TILE_MFMA(aw[v], h2[v], mu);
      const float m4[4] = {mu[0], mu[1], mu[2], mu[3]};
      float w4[4];
      clip_cotangent<A>(k, gs, row, h, m4, w4, gls, accL, accK, accC);
#pragma unroll
      for (int v = 0; v < 16; v++) wt[v] = v < 4 ? w4[v < 4 ? v : 0] : 0.0f;
    }
    reverse_tile(wimg, Q_W2T, Q_W3T, h1, h2, wt, xt, t0, t1, lane, c, h, g);
  }
  const int orow = blockIdx.x * WAVES + wave;
  float* out = partial + (size_t)orow * (S::NP + A);
  store_row<D, A>(g, out, c, h);
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const float s = half_sum32(gls[v]);
    if (c == 0 && v + 4 * h < A) out[S::NP + v + 4 * h] = s;
  }
  accL = wave_sum64(accL); accK = wave_sum64(accK); accC = wave_sum64(accC);
  if (lane == 0) { double* so = stats + (size_t)orow * 3; so[0] = accL; so[1] = accK; so[2] = accC; }
}

}  // namespace w32

// ---------------------------------------------------------------------------------------------------------------- width 128
namespace w128 {
using namespace cassie_pg;

// pg_vjp_kernel with the output layer and the cotangent between its forward and reverse pass.  What the VJP read from memory per tile of
// ANOTHER wavefront (the cotangent transposed for gW3, the observations transposed for gW1) goes through LDS here: the cotangent tile
// scot[u] = [action][sample] and the batch rows srow[u] of the four tiles of the group.  One row of partial sums and statistics per WORKGROUP.
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) clip_grad_kernel(const float* __restrict__ obs, int n, Net th0, Clip k0, float* __restrict__ partial,
                                                              double* __restrict__ stats) {
  typedef Shape<D, A> S;
  static_assert(D < 32 && A <= 8, "a column of ones next to the observations; the cotangent rows in registers 0..3 of the two lane halves");
  constexpr int KS1 = (D + 1) / 2;
  __shared__ alignas(16) float stage[2][WAVES][H * TP];
  __shared__ alignas(16) float scot[WAVES][8 * TP];
  __shared__ int srow[WAVES][32];
  __shared__ Net snet;
  __shared__ Clip sclip;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid == 0) { snet = th0; sclip = k0; }
  v16f gW2[NB], gW1 = zero16(), gW3 = zero16();
#pragma unroll
  for (int b = 0; b < NB; b++) gW2[b] = zero16();
  float gb2 = 0.0f, gb3 = 0.0f, gls[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  double accL = 0.0, accK = 0.0, accC = 0.0;
  Gauss gs;
  gauss_init<A>(gs, k0.ls_new, k0.ls_old, h);
  const int ntiles = (k0.m + 31) / 32, ngroups = (ntiles + WAVES - 1) / WAVES;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    // (pointers re-read from LDS behind the barrier, as in pg_vjp_kernel: no load through them can be hoisted out of the loop)
    __syncthreads();
    const Net th = snet;
    const Clip k = sclip;
    const int gs0 = grp * WAVES * 32;
    const int row = batch_row(k, gs0 + 32 * wave + c, n);
    const bool valid = row >= 0;                                    // a tile past the end runs with w = 0: its G2, G1 are zero
    if (h == 0) srow[wave][c] = row;
    float xb[KS1];
#pragma unroll
    for (int s = 0; s < KS1; s++) { const int kk = 2 * s + h; xb[s] = (valid && kk < D) ? obs[(size_t)row * D + kk] : 0.0f; }
    v16f h1[NB], h2[NB], g2[NB], g1[NB];
    forward_hidden<D>(th, xb, h1, h2, c, h);
    float wt[4];
    {
      v16f mu;
#pragma unroll
      for (int v = 0; v < 16; v++) mu[v] = (v < 4 && v + 4 * h < A) ? th.b3[v + 4 * h] : 0.0f;
#pragma unroll
      for (int kb = 0; kb < NB; kb++) gemm_block(th.W3, H, 0, 32 * kb, c < A, h2[kb], mu, c, h);
      const float m4[4] = {mu[0], mu[1], mu[2], mu[3]};
      clip_cotangent<A>(k, gs, row, h, m4, wt, gls, accL, accK, accC);
    }
#pragma unroll
    for (int v = 0; v < 4; v++) scot[wave][(v + 4 * h) * TP + c] = wt[v];
    // the cotangent rows and the batch rows of the group's four tiles, transposed, from LDS (eight cotangent rows in a tile: lanes c >= A feed zeros)
#define PG_VJP_COT_ROW(u, wa) \
  { wave_get(scot[u], wa, c & 7, h); _Pragma("unroll") for (int e = 0; e < 16; e++) (wa)[e] = c < A ? (wa)[e] : 0.0f; }
#define PG_VJP_OBS_T(u, e, x) { const int rs = srow[u][16 * h + (e)]; (x) = c < D ? (rs >= 0 ? obs[(size_t)rs * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f); }
#include "cassie_pg_vjp.inc"
#undef PG_VJP_COT_ROW
#undef PG_VJP_OBS_T
  }
  float* out = partial + (size_t)blockIdx.x * (S::NP + A);
#include "cassie_pg_vjp_row.inc"
  // g_log_std and the statistics: per wavefront by butterflies, the four wavefronts added in order by wavefront 0 (through LDS)
  __syncthreads();
  double* red = reinterpret_cast<double*>(&stage[0][0][0]);   // [WAVES][16]
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const float s = half_sum32(gls[v]);
    if (c == 0) red[wave * 16 + v + 4 * h] = (double)s;
  }
  accL = wave_sum64(accL); accK = wave_sum64(accK); accC = wave_sum64(accC);
  if (lane == 0) { red[wave * 16 + 8] = accL; red[wave * 16 + 9] = accK; red[wave * 16 + 10] = accC; }
  __syncthreads();
  if (tid < 11) {
    if (tid < 8) {
      float s = 0.0f;
      for (int w = 0; w < WAVES; w++) s += (float)red[w * 16 + tid];
      if (tid < A) out[S::NP + tid] = s;
    } else {
      double s = 0.0;
      for (int w = 0; w < WAVES; w++) s += red[w * 16 + tid];
      stats[(size_t)blockIdx.x * 3 + tid - 8] = s;
    }
  }
}

}  // namespace w128
}  // namespace cassie_ppo

extern "C" {

int CassieTrpoGae(const float* obs_dev, const long long* t_dev, const double* rew_dev, const unsigned char* cut_dev, int T, int n, int obs_dim,
                  const double* coeffs_dev, const double* last_value_dev, double gamma, double lambda, double* returns_dev, double* adv_dev, double* partial_dev,
                  void* stream) {
  if (!obs_dev || !t_dev || !rew_dev || !cut_dev || T <= 0 || n <= 0 || !returns_dev || !adv_dev || !partial_dev) return CASSIE_EINVAL;
  return cassie_tiles::launch_obs3d(obs_dim, [&](auto d) {
    hipLaunchKernelGGL(cassie_ppo::gae_kernel<d()>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, obs_dev, t_dev, rew_dev, cut_dev, T, n, coeffs_dev, last_value_dev,
                       gamma, lambda, returns_dev, adv_dev, partial_dev);
  });
}

int CassieTrpoClipGradRows(int m) { return cassie_ppo::w32::blocks_for(m) * cassie_ppo::w32::WAVES; }
int CassiePgClipGradRows(int m) { return cassie_pg::vjp_blocks(m); }

static bool clip_args_ok(const float* obs_dev, int n, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev, const float* old_mean_dev,
                         const float* log_std_old, const float* log_std_new, const float* partial_dev, const double* stats_dev) {
  if (!obs_dev || n <= 0 || m <= 0 || !act_dev || !adv_dev || !old_mean_dev || !log_std_old || !log_std_new || !partial_dev || !stats_dev) return false;
  return idx_dev || m <= n;   // without an index the minibatch is rows 0 .. m - 1
}

int CassieTrpoClipGrad(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* W3, const float* b3, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev,
                       const float* old_mean_dev, const float* log_std_old, const float* log_std_new, float clip, float scale, float* partial_dev,
                       double* stats_dev, void* stream) {
  using namespace cassie_ppo;
  const cassie_tiles::Net th{W1, b1, W2, b2, W3, b3};
  if (!net_ok(th) || !clip_args_ok(obs_dev, n, idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, partial_dev, stats_dev)) return CASSIE_EINVAL;
  const Clip k{idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, clip, scale};
  return cassie_tiles::launch_shape(obs_dim, act_dim, [&](auto d, auto a) {
    hipLaunchKernelGGL((w32::clip_grad_kernel<d(), a()>), dim3(w32::blocks_for(m)), dim3(64 * w32::WAVES), 0, (hipStream_t)stream, obs_dev, n, th, k, partial_dev, stats_dev);
  });
}

int CassiePgClipGrad(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                     const float* W3, const float* b3, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev,
                     const float* old_mean_dev, const float* log_std_old, const float* log_std_new, float clip, float scale, float* partial_dev,
                     double* stats_dev, void* stream) {
  using namespace cassie_ppo;
  const cassie_tiles::Net th{W1, b1, W2, b2, W3, b3};   // b1, W2, b2, W3 are read as float4
  if (!net_ok16(th) || !clip_args_ok(obs_dev, n, idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, partial_dev, stats_dev)) return CASSIE_EINVAL;
  const Clip k{idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, clip, scale};
  return cassie_tiles::launch_shape(obs_dim, act_dim, [&](auto d, auto a) {
    hipLaunchKernelGGL((w128::clip_grad_kernel<d(), a()>), dim3(cassie_pg::vjp_blocks(m)), dim3(64 * cassie_pg::WAVES), 0, (hipStream_t)stream, obs_dev, n, th, k, partial_dev,
                       stats_dev);
  });
}

}  // extern "C"
