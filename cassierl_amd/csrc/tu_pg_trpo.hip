// tu_pg_trpo.hip -- TRPO's kernels for the width-128 policy (include/cassie_trpo.h, "width-128 policy"): the Fisher-vector product
// (scale) J' S J v of the 128-128 tanh mean network, the line search's surrogate loss and mean KL, and the vector work of one
// conjugate-gradient iteration on the ~20 k-entry parameter vector.  The counterparts of CassieTrpoFvp / CassieTrpoSurrogate /
// CassieTrpoCgUpdate (tu_trpo.hip), which are written for 32 hidden units.
//
// The layout is tu_pg.hip's (cassie_pg_net.h): exact float32 v_mfma_f32_32x32x2_f32, one tile of 32 samples per wavefront, every
// activation in the accumulator layout, the 6- or 7-row output layer padded to 32 rows, A operands straight from global memory.
//
// The product runs in two launches: a forward-mode kernel writes the per-sample cotangent w = scale * prec * (J v) [n][act_dim], and
// CassiePgVjp (tu_pg.hip, unchanged) takes it back to the parameters.  Fusing the two would add the tangents dH1 / dH2 to the VJP's
// registers (256 VGPRs + ~230 AGPRs already) for a saving of one 12.6 MB write and read at 524 288 samples.
// Where the pieces live: the layout primitives, the argument check (net_ok16) and the (obs_dim, act_dim) dispatch (launch_shape) in cassie_tiles.h; the
// forward pass in cassie_pg_net.h; the CG step's kernel (cg_update_kernel<CG_PER>, one body for both widths) in cassie_onpolicy.h.
// Every sum runs in a fixed order: a run repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "cassie_onpolicy.h"   // cg_update_kernel
#include "cassie_pg_net.h"

namespace cassie_pg {

// ---------------------------------------------------------------------------------------------------------------- J v
// Forward mode along the direction (dW1 .. db3) at the weights th, one tile per wavefront (no tile loop: see tu_pg.hip's policy step):
//   dH1 = (1 - H1^2) o (dW1 x + db1),  dH2 = (1 - H2^2) o (W2 dH1 + dW2 H1 + db2),  dmu = W3 dH2 + dW3 H2 + db3,
// and w[s][a] = scale * prec[a] * dmu[s][a].  Layer 2 is one output block at a time and feeds the output layer at once, so only H1, dH1
// and two 32-row blocks of the second layer are live.  The mean itself is not needed.
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) pg_jvp_kernel(const float* __restrict__ obs, int n, Net th, Net dir, const float* __restrict__ prec,
                                                           float scale, float* __restrict__ wout) {
  constexpr int KS1 = (D + 1) / 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  const int smp = (blockIdx.x * WAVES + wave) * 32 + c;
  const bool valid = smp < n;
  float xb[KS1];
#pragma unroll
  for (int s = 0; s < KS1; s++) { const int k = 2 * s + h; xb[s] = (valid && k < D) ? obs[(size_t)smp * D + k] : 0.0f; }
  v16f h1[NB], d1[NB];
#pragma unroll
  for (int ob = 0; ob < NB; ob++) {
    v16f y = bias_tile(th.b1 + 32 * ob, h), dy = bias_tile(dir.b1 + 32 * ob, h);
#pragma unroll
    for (int s = 0; s < KS1; s++) {
      const int k = 2 * s + h;
      const float a = k < D ? th.W1[(32 * ob + c) * D + k] : 0.0f, da = k < D ? dir.W1[(32 * ob + c) * D + k] : 0.0f;
      y = TILE_MFMA(a, xb[s], y);
      dy = TILE_MFMA(da, xb[s], dy);
    }
#pragma unroll
    for (int v = 0; v < 16; v++) { y[v] = tanh_fast(y[v]); dy[v] *= 1.0f - y[v] * y[v]; }
    h1[ob] = y; d1[ob] = dy;
  }
  v16f dmu;
#pragma unroll
  for (int v = 0; v < 16; v++) dmu[v] = (v < 4 && v + 4 * h < A) ? dir.b3[v + 4 * h] : 0.0f;
#pragma unroll
  for (int ob = 0; ob < NB; ob++) {
    v16f y = bias_tile(th.b2 + 32 * ob, h), dy = bias_tile(dir.b2 + 32 * ob, h);
#pragma unroll
    for (int kb = 0; kb < NB; kb++) {
      gemm_block(th.W2, H, 32 * ob, 32 * kb, true, h1[kb], y, c, h);
      gemm_block(th.W2, H, 32 * ob, 32 * kb, true, d1[kb], dy, c, h);
      gemm_block(dir.W2, H, 32 * ob, 32 * kb, true, h1[kb], dy, c, h);
    }
#pragma unroll
    for (int v = 0; v < 16; v++) { y[v] = tanh_fast(y[v]); dy[v] *= 1.0f - y[v] * y[v]; }
    gemm_block(th.W3, H, 0, 32 * ob, c < A, dy, dmu, c, h);
    gemm_block(dir.W3, H, 0, 32 * ob, c < A, y, dmu, c, h);
  }
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int a = v + 4 * h;
    if (valid && a < A) wout[(size_t)smp * A + a] = scale * prec[a] * dmu[v];
  }
}

// ---------------------------------------------------------------------------------------------------------------- line search
// tu_trpo.hip's surrogate_kernel for the 128-128 network: per sample -exp(ll_new - ll_old) adv and KL(old || new), one tile per wavefront,
// the four wavefront sums added in order into one float64 row per workgroup.
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) pg_surrogate_kernel(const float* __restrict__ obs, int n, Net th, const float* __restrict__ ls_new,
                                                                 const float* __restrict__ ls_old, const float* __restrict__ act, const float* __restrict__ adv,
                                                                 const float* __restrict__ old_mean, double* __restrict__ partial) {
  constexpr int KS1 = (D + 1) / 2;
  __shared__ double red[WAVES][2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  float isn[4], iso[4], dls[4], kden[4], kvar[4];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int a = v + 4 * h;
    const float ln = a < A ? ls_new[a] : 0.0f, lo = a < A ? ls_old[a] : 0.0f;
    const float sn = expf(ln), so = expf(lo);
    isn[v] = 1.0f / sn; iso[v] = 1.0f / so; dls[v] = ln - lo;
    kden[v] = 1.0f / (2.0f * sn * sn + 1e-8f); kvar[v] = so * so - sn * sn;
  }
  const int smp = (blockIdx.x * WAVES + wave) * 32 + c;
  const bool valid = smp < n;
  float xb[KS1];
#pragma unroll
  for (int s = 0; s < KS1; s++) { const int k = 2 * s + h; xb[s] = (valid && k < D) ? obs[(size_t)smp * D + k] : 0.0f; }
  float ac[4], om[4];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const bool on = valid && v + 4 * h < A;
    ac[v] = on ? act[(size_t)smp * A + v + 4 * h] : 0.0f; om[v] = on ? old_mean[(size_t)smp * A + v + 4 * h] : 0.0f;
  }
  const float ad = valid ? adv[smp] : 0.0f;
  v16f h1[NB], h2[NB];
  forward_hidden<D>(th, xb, h1, h2, c, h);
  v16f mu;
#pragma unroll
  for (int v = 0; v < 16; v++) mu[v] = (v < 4 && v + 4 * h < A) ? th.b3[v + 4 * h] : 0.0f;
#pragma unroll
  for (int kb = 0; kb < NB; kb++) gemm_block(th.W3, H, 0, 32 * kb, c < A, h2[kb], mu, c, h);
  float ll = 0.0f, kl = 0.0f;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    if (v + 4 * h < A) {
      const float zn = (ac[v] - mu[v]) * isn[v], zo = (ac[v] - om[v]) * iso[v], dm = om[v] - mu[v];
      ll += 0.5f * (zo * zo - zn * zn) - dls[v];
      kl += (dm * dm + kvar[v]) * kden[v] + dls[v];
    }
  }
  ll += __shfl_xor(ll, 32, 64); kl += __shfl_xor(kl, 32, 64);
  double accL = 0.0, accK = 0.0;
  if (h == 0 && valid) { accL = -(double)(expf(ll) * ad); accK = (double)kl; }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { accL += __shfl_xor(accL, m, 64); accK += __shfl_xor(accK, m, 64); }
  if (lane == 0) { red[wave][0] = accL; red[wave][1] = accK; }
  __syncthreads();
  if (tid < 2) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < WAVES; q++) t += red[q][tid];
    partial[(size_t)blockIdx.x * 2 + tid] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------- CG vector step
// cassie_onpolicy.h's cg_update_kernel for a parameter vector of up to CG_MAX entries (the 128-128 network: 20 878 at 26 -> 7): CG_PER entries per thread.
constexpr int CG_PER = 21;
constexpr int CG_MAX = 1024 * CG_PER;

inline int tile_blocks(int n) { return ((n + 31) / 32 + WAVES - 1) / WAVES; }

}  // namespace cassie_pg

extern "C" {

int CassiePgFvp(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* W3, const float* b3, const float* dW1, const float* db1, const float* dW2, const float* db2, const float* dW3,
                const float* db3, const float* prec, float scale, float* work_dev, float* partial_dev, void* stream) {
  using namespace cassie_pg;
  const Net th{W1, b1, W2, b2, W3, b3}, dir{dW1, db1, dW2, db2, dW3, db3};
  if (!obs_dev || n <= 0 || !net_ok16(th) || !net_ok16(dir) || !prec || !work_dev || !partial_dev) return CASSIE_EINVAL;
  const int rc = launch_shape(obs_dim, act_dim, [&](auto d, auto a) {
    hipLaunchKernelGGL((pg_jvp_kernel<d(), a()>), dim3(tile_blocks(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, dir, prec, scale, work_dev);
  });
  if (rc != CASSIE_OK) return rc;
  return CassiePgVjp(obs_dev, n, obs_dim, act_dim, W1, b1, W2, b2, W3, b3, work_dev, partial_dev, stream);
}

int CassiePgSurrogateRows(int n_samples) { return n_samples > 0 ? cassie_pg::tile_blocks(n_samples) : 0; }

int CassiePgSurrogate(const float* obs_dev, int n, int obs_dim, int act_dim, const float* W1, const float* b1, const float* W2, const float* b2,
                      const float* W3, const float* b3, const float* log_std_new, const float* log_std_old, const float* act_dev,
                      const float* adv_dev, const float* old_mean_dev, double* partial_dev, void* stream) {
  using namespace cassie_pg;
  const Net th{W1, b1, W2, b2, W3, b3};
  if (!obs_dev || n <= 0 || !net_ok16(th) || !log_std_new || !log_std_old || !act_dev || !adv_dev || !old_mean_dev || !partial_dev) return CASSIE_EINVAL;
  return launch_shape(obs_dim, act_dim, [&](auto d, auto a) {
    hipLaunchKernelGGL((pg_surrogate_kernel<d(), a()>), dim3(tile_blocks(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, th, log_std_new, log_std_old, act_dev,
                       adv_dev, old_mean_dev, partial_dev);
  });
}

int CassiePgCgUpdate(int n, int ls_off, int n_ls, const float* Ap_mean_dev, const float* hls_dev, float reg, float tol, float* x_dev, float* r_dev, float* p_dev,
                     float* scal_dev, void* stream) {
  if (n <= 0 || n > cassie_pg::CG_MAX || ls_off < 0 || n_ls < 0 || ls_off + n_ls > n || !Ap_mean_dev || !hls_dev || !x_dev || !r_dev || !p_dev || !scal_dev)
    return CASSIE_EINVAL;
  hipLaunchKernelGGL(cassie_onpolicy::cg_update_kernel<cassie_pg::CG_PER>, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, ls_off, n_ls, Ap_mean_dev, hls_dev, reg, tol, x_dev, r_dev, p_dev, scal_dev);
  return cassie_tiles::launched();
}

}  // extern "C"
