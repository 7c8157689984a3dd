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
// The device functions of the two VJP units are duplicated here, not shared through a header: those units keep compiling to the
// instructions they had (cassie_pg_net.h, which both width-128 units already share, is included as it is).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_pg_net.h"

namespace cassie_ppo {

// ---------------------------------------------------------------------------------------------------------------- GAE
// tu_trpo_baseline.hip's feature arithmetic (float32 as the torch expressions evaluate it, promoted to float64)
__device__ __forceinline__ float clip10(float x) { return fminf(fmaxf(x, -10.0f), 10.0f); }
__device__ __forceinline__ float path_clock(long long t) { return (float)t * (1.0f / 100.0f); }

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
__device__ __forceinline__ int row_of(const Clip& k, int p, int n) {
  if (p >= k.m) return -1;
  if (!k.idx) return p;
  const long long r = k.idx[p];
  return (int)(r < 0 ? 0 : (r >= n ? (long long)n - 1 : r));
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
    gls[v] += on ? ws * (zn[v] * zn[v] - 1.0f) : 0.0f;
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

constexpr int H = 32, TP = 36, WAVES = 4, MAX_BLOCKS = 512;   // tu_trpo.hip's

template <int D, int A> struct Shape {
  static constexpr int NP = H * D + H + H * H + H + A * H + A;
  static constexpr int O_W1 = 0, O_B1 = H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H;
};
struct Net { const float *W1, *b1, *W2, *b2, *W3, *b3; };
typedef float v16f __attribute__((ext_vector_type(16)));
#define PPO_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float tanh_fast(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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
  for (int q = wave; q < Q_N; q += WAVES) {
    float v4[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int st = 4 * (q & 3) + e;
      const int r = (st & 3) + 8 * (st >> 2) + 4 * h;
      const int k1 = 2 * st + h;
      float x = 0.0f;
      if (q < Q_W2) x = (st < KS1 && k1 < D) ? th.W1[c * D + k1] : 0.0f;
      else if (q < Q_W3) x = th.W2[c * H + r];
      else if (q < Q_W2T) x = c < A ? th.W3[c * H + r] : 0.0f;
      else if (q < Q_W3T) x = th.W2[r * H + c];
      else x = (e + 4 * h < A) ? th.W3[(e + 4 * h) * H + c] : 0.0f;
      v4[e] = x;
    }
    wimg[q][lane] = make_float4(v4[0], v4[1], v4[2], v4[3]);
  }
  Gauss gs;
  gauss_init<A>(gs, k.ls_new, k.ls_old, h);
  __syncthreads();
  auto aop = [&](int q0, float (&a)[16]) {
#pragma unroll
    for (int q = 0; q < 4; q++) { const float4 w = wimg[q0 + q][lane]; a[4 * q] = w.x; a[4 * q + 1] = w.y; a[4 * q + 2] = w.z; a[4 * q + 3] = w.w; }
  };
  auto bias_tile = [&](int which) {
    v16f z;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 b = *reinterpret_cast<const float4*>(&sbias[which][8 * g + 4 * h]);
      z[4 * g] = b.x; z[4 * g + 1] = b.y; z[4 * g + 2] = b.z; z[4 * g + 3] = b.w;
    }
    return z;
  };
  float* t0 = tile[wave][0];
  float* t1 = tile[wave][1];
  auto put = [&](float* t, const v16f& x) {
#pragma unroll
    for (int v = 0; v < 16; v++) t[((v & 3) + 8 * (v >> 2) + 4 * h) * TP + c] = x[v];
  };
  auto get = [&](const float* t, float (&y)[16]) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float4 b = *reinterpret_cast<const float4*>(&t[c * TP + 16 * h + 4 * q]);
      y[4 * q] = b.x; y[4 * q + 1] = b.y; y[4 * q + 2] = b.z; y[4 * q + 3] = b.w;
    }
  };
  v16f gW1, gW2, gW3;
#pragma unroll
  for (int v = 0; v < 16; v++) { gW1[v] = 0.0f; gW2[v] = 0.0f; gW3[v] = 0.0f; }
  float gb2 = 0.0f, gb3 = 0.0f, gls[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  double accL = 0.0, accK = 0.0, accC = 0.0;
  const int ntiles = (k.m + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    const int row = row_of(k, tl * 32 + c, n);   // this lane's sample (both halves h)
    const bool valid = row >= 0;
    float xb[KS1], xt[16], aw[16];
#pragma unroll
    for (int s = 0; s < KS1; s++) { const int kk = 2 * s + h; xb[s] = (valid && kk < D) ? obs[(size_t)row * D + kk] : 0.0f; }
#pragma unroll
    for (int s = 0; s < 16; s++) {
      const int rs = __shfl(row, 16 * h + s, 64);   // the row of the tile's sample 16 h + s
      xt[s] = c < D ? (rs >= 0 ? obs[(size_t)rs * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f);
    }
    v16f h1 = bias_tile(0);
    aop(Q_W1, aw);
#pragma unroll
    for (int s = 0; s < KS1; s++) h1 = PPO_MFMA(aw[s], xb[s], h1);
#pragma unroll
    for (int v = 0; v < 16; v++) h1[v] = tanh_fast(h1[v]);
    v16f h2 = bias_tile(1);
    aop(Q_W2, aw);
#pragma unroll
    for (int v = 0; v < 16; v++) h2 = PPO_MFMA(aw[v], h1[v], h2);
#pragma unroll
    for (int v = 0; v < 16; v++) h2[v] = tanh_fast(h2[v]);
    v16f wt;
    {
      v16f mu = bias_tile(2);
      aop(Q_W3, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) mu = PPO_MFMA(aw[v], h2[v], mu);
      const float m4[4] = {mu[0], mu[1], mu[2], mu[3]};
      float w4[4];
      clip_cotangent<A>(k, gs, row, h, m4, w4, gls, accL, accK, accC);
#pragma unroll
      for (int v = 0; v < 16; v++) wt[v] = v < 4 ? w4[v < 4 ? v : 0] : 0.0f;
    }
    // reverse mode: G2 = (W3' w) o (1 - H2^2), G1 = (W2' G2) o (1 - H1^2)
    v16f g2, g1;
#pragma unroll
    for (int v = 0; v < 16; v++) { g2[v] = 0.0f; g1[v] = 0.0f; }
    {
      const float4 w = wimg[Q_W3T][lane];
      g2 = PPO_MFMA(w.x, wt[0], g2); g2 = PPO_MFMA(w.y, wt[1], g2); g2 = PPO_MFMA(w.z, wt[2], g2); g2 = PPO_MFMA(w.w, wt[3], g2);
    }
#pragma unroll
    for (int v = 0; v < 16; v++) g2[v] *= 1.0f - h2[v] * h2[v];
    aop(Q_W2T, aw);
#pragma unroll
    for (int v = 0; v < 16; v++) g1 = PPO_MFMA(aw[v], g2[v], g1);
#pragma unroll
    for (int v = 0; v < 16; v++) g1[v] *= 1.0f - h1[v] * h1[v];
    // parameter gradients: products over the sample index, operands transposed through the wavefront's LDS tiles
    float ta[16], tb[16];
    put(t0, g2); put(t1, h1);
    wave_lds_sync();
    get(t0, ta); get(t1, tb);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; s++) { gW2 = PPO_MFMA(ta[s], tb[s], gW2); gb2 += ta[s]; }
    put(t0, g1);
    wave_lds_sync();
    get(t0, ta);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; s++) gW1 = PPO_MFMA(ta[s], xt[s], gW1);
    put(t0, wt); put(t1, h2);
    wave_lds_sync();
    get(t0, ta); get(t1, tb);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; s++) { gW3 = PPO_MFMA(ta[s], tb[s], gW3); gb3 += ta[s]; }
  }
  const int orow = blockIdx.x * WAVES + wave;
  float* out = partial + (size_t)orow * (S::NP + A);
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = (v & 3) + 8 * (v >> 2) + 4 * h;
    out[S::O_W2 + r * H + c] = gW2[v];
    if (c < D) out[S::O_W1 + r * D + c] = gW1[v];
    if (c == D) out[S::O_B1 + r] = gW1[v];
    if (r < A) out[S::O_W3 + r * H + c] = gW3[v];
  }
  gb2 += __shfl_xor(gb2, 32, 64); gb3 += __shfl_xor(gb3, 32, 64);
  if (h == 0) out[S::O_B2 + c] = gb2;
  if (h == 0 && c < A) out[S::O_B3 + c] = gb3;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const float s = half_sum32(gls[v]);
    if (c == 0 && v + 4 * h < A) out[S::NP + v + 4 * h] = s;
  }
  accL = wave_sum64(accL); accK = wave_sum64(accK); accC = wave_sum64(accC);
  if (lane == 0) { double* so = stats + (size_t)orow * 3; so[0] = accL; so[1] = accK; so[2] = accC; }
}

inline int blocks_for(int n) {
  const int tiles = (n + 31) / 32;
  int b = (tiles + WAVES - 1) / WAVES;
  return b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

}  // namespace w32

// ---------------------------------------------------------------------------------------------------------------- width 128
namespace w128 {
using namespace cassie_pg;

__device__ __forceinline__ void wave_put(float* __restrict__ t, const v16f (&x)[NB], int c, int h) {   // accumulator layout -> [row][sample]
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int v = 0; v < 16; v++) t[(32 * b + (v & 3) + 8 * (v >> 2) + 4 * h) * TP + c] = x[b][v];
}
__device__ __forceinline__ void wave_get(const float* __restrict__ t, float (&y)[16], int c, int h) {   // lane (c, h): row c, samples 16 h .. 16 h + 15
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float4 b = *reinterpret_cast<const float4*>(&t[c * TP + 16 * h + 4 * q]);
    y[4 * q] = b.x; y[4 * q + 1] = b.y; y[4 * q + 2] = b.z; y[4 * q + 3] = b.w;
  }
}

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
    const int row = row_of(k, gs0 + 32 * wave + c, n);
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
    // G2 = (W3' w) o (1 - H2^2): k-step v sums over the cotangent row a = v + 4 h
#pragma unroll
    for (int ob = 0; ob < NB; ob++) {
      v16f y = zero16();
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int a = v + 4 * h;
        y = PG_MFMA(a < A ? th.W3[a * H + 32 * ob + c] : 0.0f, wt[v], y);
      }
#pragma unroll
      for (int v = 0; v < 16; v++) y[v] *= 1.0f - h2[ob][v] * h2[ob][v];
      g2[ob] = y;
    }
    // ---- 1. H1 (slot 0, kept to the third exchange) and H2 (slot 1): gW3[a][32 q + j] += sum_s w[s][a] H2[32 q + j][s]
    wave_put(stage[0][wave], h1, c, h);
    wave_put(stage[1][wave], h2, c, h);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], wa[16];
      wave_get(scot[u], wa, c & 7, h);   // the cotangent row of action c (eight rows in the tile; lanes c >= A feed zeros)
#pragma unroll
      for (int e = 0; e < 16; e++) wa[e] = c < A ? wa[e] : 0.0f;
      wave_get(stage[1][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) { gW3 = PG_MFMA(wa[s], ta[s], gW3); gb3 += wa[s]; }
    }
    // ---- 2. G2 (slot 1): gW2[32 q + i][32 kb + j] += sum_s G2[32 q + i][s] H1[32 kb + j][s]
    __syncthreads();
    wave_put(stage[1][wave], g2, c, h);
    __syncthreads();
    const float* myh1 = stage[0][wave];
#pragma unroll
    for (int ob = 0; ob < NB; ob++) {
      v16f y = zero16();
#pragma unroll
      for (int kb = 0; kb < NB; kb++)
#pragma unroll
        for (int v = 0; v < 16; v++) y = PG_MFMA(th.W2[(size_t)(32 * kb + (v & 3) + 8 * (v >> 2) + 4 * h) * H + 32 * ob + c], g2[kb][v], y);
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const float x = myh1[(32 * ob + (v & 3) + 8 * (v >> 2) + 4 * h) * TP + c];
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
        for (int s = 0; s < 16; s++) gW2[kb] = PG_MFMA(ta[s], tb[s], gW2[kb]);
      }
    }
    // ---- 3. G1 (slot 0): gW1[32 q + i][k] += sum_s G1[32 q + i][s] [obs | 1][s][k]   (column D: gb1)
    __syncthreads();
    wave_put(stage[0][wave], g1, c, h);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], xt[16];
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int rs = srow[u][16 * h + e];
        xt[e] = c < D ? (rs >= 0 ? obs[(size_t)rs * D + c] : 0.0f) : (c == D ? 1.0f : 0.0f);
      }
      wave_get(stage[0][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) gW1 = PG_MFMA(ta[s], xt[s], gW1);
    }
  }
  // ---- this workgroup's row: gW[r(v, h)][c] in register v
  float* out = partial + (size_t)blockIdx.x * (S::NP + A);
  const int q = wave;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = (v & 3) + 8 * (v >> 2) + 4 * h;
#pragma unroll
    for (int kb = 0; kb < NB; kb++) out[S::O_W2 + (32 * q + r) * H + 32 * kb + c] = gW2[kb][v];
    if (c < D) out[S::O_W1 + (32 * q + r) * D + c] = gW1[v];
    if (c == D) out[S::O_B1 + 32 * q + r] = gW1[v];
    if (r < A) out[S::O_W3 + r * H + 32 * q + c] = gW3[v];
  }
  gb2 += __shfl_xor(gb2, 32, 64); gb3 += __shfl_xor(gb3, 32, 64);
  if (h == 0) out[S::O_B2 + 32 * q + c] = gb2;
  if (q == 0 && h == 0 && c < A) out[S::O_B3 + c] = gb3;
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

inline int blocks_for(int m) {
  const int groups = ((m + 31) / 32 + WAVES - 1) / WAVES;
  return groups < 1 ? 1 : (groups > MAX_VJP_BLOCKS ? MAX_VJP_BLOCKS : groups);
}

}  // namespace w128
}  // namespace cassie_ppo

extern "C" {

int CassieTrpoGae(const float* obs_dev, const long long* t_dev, const double* rew_dev, const unsigned char* cut_dev, int T, int n, int obs_dim,
                  const double* coeffs_dev, const double* last_value_dev, double gamma, double lambda, double* returns_dev, double* adv_dev, double* partial_dev,
                  void* stream) {
  if (!obs_dev || !t_dev || !rew_dev || !cut_dev || T <= 0 || n <= 0 || !returns_dev || !adv_dev || !partial_dev) return CASSIE_EINVAL;
  const dim3 grid((n + 255) / 256), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (obs_dim == 26) hipLaunchKernelGGL(cassie_ppo::gae_kernel<26>, grid, block, 0, s, obs_dev, t_dev, rew_dev, cut_dev, T, n, coeffs_dev, last_value_dev, gamma, lambda, returns_dev, adv_dev, partial_dev);
  else if (obs_dim == 17) hipLaunchKernelGGL(cassie_ppo::gae_kernel<17>, grid, block, 0, s, obs_dev, t_dev, rew_dev, cut_dev, T, n, coeffs_dev, last_value_dev, gamma, lambda, returns_dev, adv_dev, partial_dev);
  else return CASSIE_EINVAL;
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieTrpoClipGradRows(int m) { return cassie_ppo::w32::blocks_for(m) * cassie_ppo::w32::WAVES; }
int CassiePgClipGradRows(int m) { return cassie_ppo::w128::blocks_for(m); }

static bool clip_args_ok(const float* obs_dev, int n, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                         const long long* idx_dev, int m, const float* act_dev, const float* adv_dev, const float* old_mean_dev, const float* log_std_old,
                         const float* log_std_new, const float* partial_dev, const double* stats_dev) {
  if (!obs_dev || n <= 0 || m <= 0 || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !act_dev || !adv_dev || !old_mean_dev || !log_std_old || !log_std_new ||
      !partial_dev || !stats_dev)
    return false;
  return idx_dev || m <= n;   // without an index the minibatch is rows 0 .. m - 1
}

int CassieTrpoClipGrad(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* W3, const float* b3, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev,
                       const float* old_mean_dev, const float* log_std_old, const float* log_std_new, float clip, float scale, float* partial_dev,
                       double* stats_dev, void* stream) {
  using namespace cassie_ppo;
  if (!clip_args_ok(obs_dev, n, W1, b1, W2, b2, W3, b3, idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, partial_dev, stats_dev)) return CASSIE_EINVAL;
  const w32::Net th{W1, b1, W2, b2, W3, b3};
  const Clip k{idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, clip, scale};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(w32::blocks_for(m)), block(64 * w32::WAVES);
  if (obs_dim == 26 && act_dim == 6) hipLaunchKernelGGL((w32::clip_grad_kernel<26, 6>), grid, block, 0, s, obs_dev, n, th, k, partial_dev, stats_dev);
  else if (obs_dim == 26 && act_dim == 7) hipLaunchKernelGGL((w32::clip_grad_kernel<26, 7>), grid, block, 0, s, obs_dev, n, th, k, partial_dev, stats_dev);
  else if (obs_dim == 17 && act_dim == 6) hipLaunchKernelGGL((w32::clip_grad_kernel<17, 6>), grid, block, 0, s, obs_dev, n, th, k, partial_dev, stats_dev);
  else if (obs_dim == 17 && act_dim == 7) hipLaunchKernelGGL((w32::clip_grad_kernel<17, 7>), grid, block, 0, s, obs_dev, n, th, k, partial_dev, stats_dev);
  else return CASSIE_EINVAL;
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassiePgClipGrad(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                     const float* W3, const float* b3, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev,
                     const float* old_mean_dev, const float* log_std_old, const float* log_std_new, float clip, float scale, float* partial_dev,
                     double* stats_dev, void* stream) {
  using namespace cassie_ppo;
  if (!clip_args_ok(obs_dev, n, W1, b1, W2, b2, W3, b3, idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, partial_dev, stats_dev)) return CASSIE_EINVAL;
  if (!cassie_pg::aligned16(b1) || !cassie_pg::aligned16(W2) || !cassie_pg::aligned16(b2) || !cassie_pg::aligned16(W3)) return CASSIE_EINVAL;   // read as float4
  const cassie_pg::Net th{W1, b1, W2, b2, W3, b3};
  const Clip k{idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, clip, scale};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(w128::blocks_for(m)), block(64 * cassie_pg::WAVES);
  if (obs_dim == 26 && act_dim == 6) hipLaunchKernelGGL((w128::clip_grad_kernel<26, 6>), grid, block, 0, s, obs_dev, n, th, k, partial_dev, stats_dev);
  else if (obs_dim == 26 && act_dim == 7) hipLaunchKernelGGL((w128::clip_grad_kernel<26, 7>), grid, block, 0, s, obs_dev, n, th, k, partial_dev, stats_dev);
  else if (obs_dim == 17 && act_dim == 6) hipLaunchKernelGGL((w128::clip_grad_kernel<17, 6>), grid, block, 0, s, obs_dev, n, th, k, partial_dev, stats_dev);
  else if (obs_dim == 17 && act_dim == 7) hipLaunchKernelGGL((w128::clip_grad_kernel<17, 7>), grid, block, 0, s, obs_dev, n, th, k, partial_dev, stats_dev);
  else return CASSIE_EINVAL;
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
