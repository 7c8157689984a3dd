// tu_pg3d.hip -- the width-128 policy kernels of PPO at the Cassie3d shape, 45 observations and 10 actions (include/cassie_trpo.h,
// "width-128 policy at 45 x 10"; cassierl_amd/ppo.py): the sampler's policy step and the gradient of the clipped surrogate on one minibatch.
//
// Read tu_pg.hip's and tu_ppo.hip's headers first: the layout (exact float32 v_mfma_f32_32x32x2_f32, a tile of 32 samples per wavefront,
// activations in the accumulator layout, four wavefronts exchanging transposed tiles through two LDS slots) and the contracts
// (CassiePgPolicyStep, CassiePgClipGrad) are theirs.  The forward pass of the hidden layers is cassie_pg_net.h's, generic in D: the first layer
// has 23 k-steps per 32-row block.  Two layout assumptions of the 26-wide kernels do not hold here, and this unit is what replaces them:
//
//   * the action rows.  The padded 32-row output tile has action a on row a, and row_of(v, h) = (v & 3) + 8 (v >> 2) + 4 h puts rows 0..3 in
//     registers 0..3 of half 0, rows 4..7 in registers 0..3 of half 1, rows 8..11 in registers 4..7 of half 0 (rows 12..15: half 1).  Ten
//     actions are therefore registers v < NS = 6 with a = row_of(v, h) < A: six live slots on half 0 (actions 0..3, 8, 9), four on half 1
//     (4..7; its slots 4 and 5 are rows 12 and 13, masked).  Everything that was written `a = v + 4 h, v < 4` -- the per-action constants, the
//     cotangent, g_log_std, the k-steps of G2 = W3' w, the rows of the cotangent tile in LDS (16, of which 10 are read) -- runs over these slots.
//   * [obs | 1] is 46 columns, two 32-column blocks.  [gW1 | gb1] of a wavefront's quarter is two accumulator tiles (columns 0..31 and
//     32..63; column 45 is gb1, 46..63 are fed zeros).  The third exchange of a group runs TWICE over the G1 image in LDS slot 0, once per
//     column block: one pass with both blocks' transposed observations live (32 more registers next to 112 accumulator registers) is what
//     the register budget of this kernel does not have.  G1 is read from LDS twice; the observations are read once per block either way.
//
// The reverse pass is written out here, not taken from cassie_pg_vjp.inc: that text fixes `v < 4` and one gW1 tile, and it is shared as text
// by two kernels at the register limit whose instructions must not change.  For the same reason this is a unit of its own (any new function
// in tu_pg.hip / tu_ppo.hip changes the register allocation of every kernel there) and the small host-visible pieces of tu_ppo.hip (Clip,
// batch_row, the butterflies) are repeated below.  Fixed summation order throughout: a call repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_pg_net.h"

namespace cassie_pg3d {

using namespace cassie_pg;

constexpr int D3 = 45, A3 = 10;

// ---------------------------------------------------------------------------------------------------------------- policy step
// CassiePgPolicyStep's contract; the mean comes out with action a = row_of(v, h) in register v < NS of lane (environment, h).
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ log_std,
                                                                const float* __restrict__ noise, const double* __restrict__ low, const double* __restrict__ high,
                                                                float* __restrict__ obs32, float* __restrict__ mean, float* __restrict__ act, double* __restrict__ env_act) {
  static_assert(A > 8 && A <= 12, "action rows 8.. in registers 4.. of lane half 0");
  constexpr int KS1 = (D + 1) / 2, NS = A - 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  {   // one tile per wavefront (tu_pg.hip: a tile loop makes the compiler hoist a tile's weight loads out of it, and spill)
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
    for (int v = 0; v < 16; v++) mu[v] = (v < NS && row_of(v, h) < A) ? th.b3[row_of(v, h)] : 0.0f;
#pragma unroll
    for (int kb = 0; kb < NB; kb++) gemm_block(th.W3, H, 0, 32 * kb, c < A, h2[kb], mu, c, h);
#pragma unroll
    for (int v = 0; v < NS; v++) {
      const int a = row_of(v, h);
      if (valid && a < A) {
        const size_t o = (size_t)smp * A + a;
        const float val = mu[v] + noise[o] * expf(log_std[a]);
        mean[o] = mu[v]; act[o] = val;
        const double lo = low[a], hi = high[a];
        double e = lo + ((double)val + 1.0) * 0.5 * (hi - lo);
        e = e < lo ? lo : (e > hi ? hi : e);
        env_act[o] = e;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the cotangent
struct Clip {   // what a launch adds to the network's arguments (tu_ppo.hip's)
  const long long* idx;
  int m;
  const float *act, *adv, *old_mean, *ls_old, *ls_new;
  float clip, scale;
};

// batch row of minibatch position p (-1 behind the end of the minibatch); a wild index is clamped into the batch
__device__ __forceinline__ int batch_row(const Clip& k, int p, int n) {
  if (p >= k.m) return -1;
  if (!k.idx) return p;
  const long long r = k.idx[p];
  return (int)(r < 0 ? 0 : (r >= n ? (long long)n - 1 : r));
}

// per-action constants of the two Gaussians for the action slots of this lane half (GaussianMLPPolicy.log_likelihood / .kl of trpo.py)
template <int NS> struct Gauss { float isn[NS], iso[NS], dls[NS], kden[NS], kvar[NS]; };
template <int A, int NS> __device__ __forceinline__ void gauss_init(Gauss<NS>& g, const float* __restrict__ ls_new, const float* __restrict__ ls_old, int h) {
#pragma unroll
  for (int v = 0; v < NS; v++) {
    const int a = row_of(v, h);
    const float ln = a < A ? ls_new[a] : 0.0f, lo = a < A ? ls_old[a] : 0.0f;
    const float sn = expf(ln), so = expf(lo);
    g.isn[v] = 1.0f / sn; g.iso[v] = 1.0f / so; g.dls[v] = ln - lo;
    g.kden[v] = 1.0f / (2.0f * sn * sn + 1e-8f); g.kvar[v] = so * so - sn * sn;
  }
}

// One sample on lanes (c, 0) and (c, 1): mean mu[v] of action a = row_of(v, h) -> cotangent wt[v] = d L / d mean = -scale w z / std, and this
// lane's sums: g_log_std (the actions of its slots), and on the h = 0 lane the sample's loss term, KL and clip flag.  The log-likelihood
// difference is the difference of the two quadratic forms and of the log-stds (tu_ppo.hip: the ratio stays accurate near 1).
template <int A, int NS>
__device__ __forceinline__ void clip_cotangent(const Clip& k, const Gauss<NS>& g, int row, int h, const float (&mu)[NS], float (&wt)[NS], float (&gls)[NS],
                                               double& accL, double& accK, double& accC) {
  const bool valid = row >= 0;
  float ll = 0.0f, kl = 0.0f, zn[NS];
#pragma unroll
  for (int v = 0; v < NS; v++) {
    zn[v] = 0.0f;
    const int a = row_of(v, h);
    if (valid && a < A) {
      const size_t o = (size_t)row * A + a;
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
  for (int v = 0; v < NS; v++) {
    const bool on = row_of(v, h) < A;
    wt[v] = on ? ws * zn[v] * g.isn[v] : 0.0f;
    gls[v] = on ? __builtin_fmaf(__builtin_fmaf(zn[v], zn[v], -1.0f), ws, gls[v]) : gls[v];   // ws (z^2 - 1)
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

// ---------------------------------------------------------------------------------------------------------------- clip gradient
// partial [gridDim.x][NP + A]: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | g_log_std] of this workgroup's tiles, stats [gridDim.x][3].  Wavefront q
// accumulates rows 32 q .. 32 q + 31 of gW1 / gb1 / gW2 / gb2 and columns 32 q .. 32 q + 31 of gW3 from the group's four tiles.
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) clip_grad_kernel(const float* __restrict__ obs, int n, Net th0, Clip k0, float* __restrict__ partial,
                                                              double* __restrict__ stats) {
  typedef Shape<D, A> S;
  static_assert(D >= 32 && D < 64, "[obs | 1] in two 32-column blocks");
  static_assert(A > 8 && A <= 12, "action rows 8.. in registers 4.. of lane half 0; 16 cotangent rows in LDS");
  constexpr int KS1 = (D + 1) / 2, NS = A - 4;
  __shared__ alignas(16) float stage[2][WAVES][H * TP];
  __shared__ alignas(16) float scot[WAVES][16 * TP];
  __shared__ int srow[WAVES][32];
  __shared__ Net snet;
  __shared__ Clip sclip;
  __shared__ Gauss<NS> sgauss[2];   // per lane half; in LDS, not in 30 registers across the group loop
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid == 0) { snet = th0; sclip = k0; }
  v16f gW2[NB], gW1a = zero16(), gW1b = zero16(), gW3 = zero16();
#pragma unroll
  for (int b = 0; b < NB; b++) gW2[b] = zero16();
  float gb2 = 0.0f, gb3 = 0.0f, gls[NS];
#pragma unroll
  for (int v = 0; v < NS; v++) gls[v] = 0.0f;
  double accL = 0.0, accK = 0.0, accC = 0.0;
  if (tid < 2) gauss_init<A, NS>(sgauss[tid], k0.ls_new, k0.ls_old, tid);   // (read by every lane of half h behind the group loop's first barrier)
  const int ntiles = (k0.m + 31) / 32, ngroups = (ntiles + WAVES - 1) / WAVES;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {   // the same trip count for every wavefront of the workgroup
    // (pointers re-read from LDS behind the barrier, as in pg_vjp_kernel: no load through them can be hoisted out of the loop; the barrier
    // also orders this group's first LDS writes after the previous group's last reads)
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
    float wt[NS];
    {
      v16f mu;
#pragma unroll
      for (int v = 0; v < 16; v++) mu[v] = (v < NS && ROW_AT(0, v, h) < A) ? th.b3[ROW_AT(0, v, h)] : 0.0f;
#pragma unroll
      for (int kb = 0; kb < NB; kb++) gemm_block(th.W3, H, 0, 32 * kb, c < A, h2[kb], mu, c, h);
      float ms[NS];
#pragma unroll
      for (int v = 0; v < NS; v++) ms[v] = mu[v];
      const Gauss<NS> gs = sgauss[h];
      clip_cotangent<A, NS>(k, gs, row, h, ms, wt, gls, accL, accK, accC);
    }
#pragma unroll
    for (int v = 0; v < NS; v++) scot[wave][ROW_AT(0, v, h) * TP + c] = wt[v];   // rows 0..13; rows >= A hold zeros
    // G2 = (W3' w) o (1 - H2^2): k-step v sums over the cotangent rows a = row_of(v, 0) and row_of(v, 1)
#pragma unroll
    for (int ob = 0; ob < NB; ob++) {
      v16f y = zero16();
#pragma unroll
      for (int v = 0; v < NS; v++) {
        const int a = ROW_AT(0, v, h);
        y = TILE_MFMA(a < A ? th.W3[a * H + 32 * ob + c] : 0.0f, wt[v], y);
      }
#pragma unroll
      for (int v = 0; v < 16; v++) y[v] *= 1.0f - h2[ob][v] * h2[ob][v];
      g2[ob] = y;
    }
    // Three exchanges through the two LDS slots, so that no more than two 128 x 32 activations of the tile are live in registers:
    // ---- 1. H1 (slot 0, kept to the third exchange) and H2 (slot 1): gW3[a][32 q + j] += sum_s w[s][a] H2[32 q + j][s]
    wave_put(stage[0][wave], h1, c, h);
    wave_put(stage[1][wave], h2, c, h);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], wa[16];
      wave_get(scot[u], wa, c & 15, h);   // cotangent row (action) c at the 16 k-steps; lanes c >= A feed zeros
#pragma unroll
      for (int e = 0; e < 16; e++) wa[e] = c < A ? wa[e] : 0.0f;
      wave_get(stage[1][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) { gW3 = TILE_MFMA(wa[s], ta[s], gW3); gb3 += wa[s]; }
    }
    // ---- 2. G2 (slot 1): gW2[32 q + i][32 kb + j] += sum_s G2[32 q + i][s] H1[32 kb + j][s]
    __syncthreads();
    wave_put(stage[1][wave], g2, c, h);
    __syncthreads();
    // G1 = (W2' G2) o (1 - H1^2) of this wavefront's tile (H1 from its slot-0 image): k-step v of block (ob, kb) reads W2[32 kb + r(v, h)][32 ob + c]
    const float* myh1 = stage[0][wave];
#pragma unroll
    for (int ob = 0; ob < NB; ob++) {
      v16f y = zero16();
#pragma unroll
      for (int kb = 0; kb < NB; kb++)
#pragma unroll
        for (int v = 0; v < 16; v++) y = TILE_MFMA(th.W2[(size_t)ROW_AT(32 * kb, v, h) * H + 32 * ob + c], g2[kb][v], y);
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const float x = myh1[ROW_AT(32 * ob, v, h) * TP + c];
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
        for (int s = 0; s < 16; s++) gW2[kb] = TILE_MFMA(ta[s], tb[s], gW2[kb]);
      }
    }
    // ---- 3. G1 (slot 0): [gW1 | gb1][32 q + i][k] += sum_s G1[32 q + i][s] [obs | 1][s][k], columns k = c and then k = 32 + c (column D: gb1)
    __syncthreads();
    wave_put(stage[0][wave], g1, c, h);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], xt[16];
#pragma unroll
      for (int e = 0; e < 16; e++) { const int rs = srow[u][16 * h + e]; xt[e] = rs >= 0 ? obs[(size_t)rs * D + c] : 0.0f; }
      wave_get(stage[0][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) gW1a = TILE_MFMA(ta[s], xt[s], gW1a);
    }
#pragma unroll 1
    for (int u = 0; u < WAVES; u++) {
      float ta[16], xt[16];
      const int cc = 32 + c;
#pragma unroll
      for (int e = 0; e < 16; e++) { const int rs = srow[u][16 * h + e]; xt[e] = cc < D ? (rs >= 0 ? obs[(size_t)rs * D + cc] : 0.0f) : (cc == D ? 1.0f : 0.0f); }
      wave_get(stage[0][u] + 32 * wave * TP, ta, c, h);
#pragma unroll
      for (int s = 0; s < 16; s++) gW1b = TILE_MFMA(ta[s], xt[s], gW1b);
    }
  }
  // the workgroup's row: gW[row_of(v, h)][c] in register v
  float* out = partial + (size_t)blockIdx.x * (S::NP + A);
  const int q = wave;
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const int r = row_of(v, h);
#pragma unroll
    for (int kb = 0; kb < NB; kb++) out[S::O_W2 + (32 * q + r) * H + 32 * kb + c] = gW2[kb][v];
    out[S::O_W1 + (32 * q + r) * D + c] = gW1a[v];
    if (32 + c < D) out[S::O_W1 + (32 * q + r) * D + 32 + c] = gW1b[v];
    if (32 + c == D) out[S::O_B1 + 32 * q + r] = gW1b[v];
    if (r < A) out[S::O_W3 + r * H + 32 * q + c] = gW3[v];
  }
  gb2 += __shfl_xor(gb2, 32, 64); gb3 += __shfl_xor(gb3, 32, 64);
  if (h == 0) out[S::O_B2 + 32 * q + c] = gb2;
  if (q == 0 && h == 0 && c < A) out[S::O_B3 + c] = gb3;
  // g_log_std and the statistics: per wavefront by butterflies, the four wavefronts added in order by wavefront 0 (through LDS)
  __syncthreads();
  double* red = reinterpret_cast<double*>(&stage[0][0][0]);   // [WAVES][16 + 3]
#pragma unroll
  for (int v = 0; v < NS; v++) {
    const float s = half_sum32(gls[v]);
    if (c == 0 && row_of(v, h) < A) red[wave * 19 + row_of(v, h)] = (double)s;
  }
  accL = wave_sum64(accL); accK = wave_sum64(accK); accC = wave_sum64(accC);
  if (lane == 0) { red[wave * 19 + 16] = accL; red[wave * 19 + 17] = accK; red[wave * 19 + 18] = accC; }
  __syncthreads();
  if (tid < A) {
    float s = 0.0f;
    for (int w = 0; w < WAVES; w++) s += (float)red[w * 19 + tid];
    out[S::NP + tid] = s;
  } else if (tid >= 16 && tid < 19) {
    double s = 0.0;
    for (int w = 0; w < WAVES; w++) s += red[w * 19 + tid];
    stats[(size_t)blockIdx.x * 3 + tid - 16] = s;
  }
}

inline int step_blocks(int n) { return ((n + 31) / 32 + WAVES - 1) / WAVES; }
inline bool shape_ok(int obs_dim, int act_dim) { return obs_dim == D3 && act_dim == A3; }

}  // namespace cassie_pg3d

extern "C" {

int CassiePg3dParamCount(int obs_dim, int act_dim) {
  return cassie_pg3d::shape_ok(obs_dim, act_dim) ? cassie_pg::Shape<cassie_pg3d::D3, cassie_pg3d::A3>::NP : 0;
}
int CassiePg3dClipGradRows(int m) { return cassie_pg::vjp_blocks(m); }

int CassiePg3dPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2,
                         const float* b2, const float* W3, const float* b3, const float* log_std, const float* noise_dev,
                         const double* low_dev, const double* high_dev, float* obs32_dev, float* mean_dev, float* act_dev,
                         double* env_actions_dev, void* stream) {
  using namespace cassie_pg3d;
  const Net th{W1, b1, W2, b2, W3, b3};
  if (!obs_dev || n <= 0 || !net_ok16(th) || !log_std || !noise_dev || !low_dev || !high_dev || !obs32_dev || !mean_dev || !act_dev || !env_actions_dev ||
      !shape_ok(obs_dim, act_dim))
    return CASSIE_EINVAL;
  hipLaunchKernelGGL((policy_step_kernel<D3, A3>), dim3(step_blocks(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, log_std, noise_dev, low_dev, high_dev,
                     obs32_dev, mean_dev, act_dev, env_actions_dev);
  return launched();
}

int CassiePg3dClipGrad(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* W3, const float* b3, const long long* idx_dev, int m, const float* act_dev, const float* adv_dev,
                       const float* old_mean_dev, const float* log_std_old, const float* log_std_new, float clip, float scale, float* partial_dev,
                       double* stats_dev, void* stream) {
  using namespace cassie_pg3d;
  const Net th{W1, b1, W2, b2, W3, b3};   // b1, W2, b2, W3 are read as float4
  if (!net_ok16(th) || !obs_dev || n <= 0 || m <= 0 || !act_dev || !adv_dev || !old_mean_dev || !log_std_old || !log_std_new || !partial_dev || !stats_dev ||
      !(idx_dev || m <= n) || !shape_ok(obs_dim, act_dim))   // without an index the minibatch is rows 0 .. m - 1
    return CASSIE_EINVAL;
  const Clip k{idx_dev, m, act_dev, adv_dev, old_mean_dev, log_std_old, log_std_new, clip, scale};
  hipLaunchKernelGGL((clip_grad_kernel<D3, A3>), dim3(vjp_blocks(m)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, k, partial_dev, stats_dev);
  return launched();
}

}  // extern "C"
