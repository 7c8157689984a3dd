// sac_kernels.h -- Soft Actor-Critic's own device code, one copy for every shape (tu_sac.hip: 26 x 6, 26 x 7, 17 x 6, 17 x 7; tu_sac3d.hip: Cassie3d's
// 45 x 10): the squashed-Gaussian head (squash, actor_sample), the critic and actor gradient kernels, the body of the actor's and the temperature's Adam
// step (actor_apply_rows) and the policy step.  tu_sac.hip's header tells the algorithm and the layout of the two heads; everything that is not SAC's
// is mlp32_tiles.h's, and like it this file takes every difference between the shapes from D and A.  The two units keep their entry points, their
// argument checks and the instantiations.
// Every sum runs in a fixed order: a launch repeats bit for bit.
#pragma once
#include "mlp32_tiles.h"

namespace cassie_sac {

using namespace cassie_mlp32;

constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;

// one component of the squashed Gaussian: action, its log-density term, exp(log_std) eps, and whether the clamp lets a gradient through
__device__ __forceinline__ void squash(float mean, float ls_raw, float eps, float& act, float& logp, float& sde, bool& inside) {
  const float ls = fminf(fmaxf(ls_raw, LOG_STD_MIN), LOG_STD_MAX);
  inside = ls_raw >= LOG_STD_MIN && ls_raw <= LOG_STD_MAX;
  sde = expf(ls) * eps;
  const float u = mean + sde, m2u = -2.0f * u;
  act = tanh_fast(u);
  const float softplus = fmaxf(m2u, 0.0f) + log1pf(expf(-fabsf(m2u)));
  logp = (-0.5f * eps * eps - ls - 0.9189385332046727f) - 2.0f * (0.6931471805599453f - u - softplus);
}

// the actor (images at q0, rows sb[0 .. 2]: mlp32_tiles.h, actor_forward) on the first-layer operand xb with the noise eps of the lane's slots:
// hidden activations a1, a2, the squashed action in the slots of act (0 in the dead ones), log pi of the sample (both lane halves hold it)
template <int D, int A>
__device__ __forceinline__ void actor_sample(const float4 (*wimg)[64], int q0, const float (*sb)[32], const float (&xb)[Shape<D, A>::KS1],
                                             const float (&eps)[Shape<D, A>::NS], int lane, int h, v16f& a1, v16f& a2, float (&act)[Shape<D, A>::NS],
                                             float (&sde)[Shape<D, A>::NS], bool (&inside)[Shape<D, A>::NS], float& logpi) {
  typedef Shape<D, A> S;
  v16f z3;
  actor_forward<D, A>(wimg, q0, sb, xb, lane, h, a1, a2, z3);
  float lp = 0.0f;
#pragma unroll
  for (int v = 0; v < S::NS; v++) {
    float l;
    squash(z3[v], z3[v + S::HREG], eps[v], act[v], l, sde[v], inside[v]);
    if (row_of(v, h) < A) lp += l; else act[v] = 0.0f;
  }
  logpi = lp + __shfl_xor(lp, 32, 64);
}

// ---------------------------------------------------------------------------------------------------------------- critic gradients
// twin_critic_grad (mlp32_tiles.h) with  a' = pi(s'_i; eps[b])  and  sub = alpha log pi(a'|s'_i).
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) critic_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net pi, Net tq1, Net tq2, Net q1, Net q2,
                                                                    const float* __restrict__ eps_next, const float* __restrict__ log_alpha, float gamma,
                                                                    float* __restrict__ partial) {
  typedef Shape<D, A> S;
  const float alpha = expf(log_alpha[0]);
  const auto target = [=](const float4 (*wimg)[64], const float (*sb)[32], const float (&xn)[S::KS1], const float (&en)[S::NS], int lane, int h, float (&an)[S::NS]) {
    v16f a1, a2;
    float sde[S::NS], logpi;
    bool inside[S::NS];
    actor_sample<D, A>(wimg, TC_PI, sb, xn, en, lane, h, a1, a2, an, sde, inside, logpi);
    return alpha * logpi;
  };
  twin_critic_grad<D, A, K_HEAD>(pool, idx, n, pi, tq1, tq2, q1, q2, eps_next, gamma, partial, target);
}

// ---------------------------------------------------------------------------------------------------------------- actor gradient
// Gradient of sum_b (alpha log pi(a~_b|s_b) - min(Q1, Q2)(s_b, a~_b)), a~ = pi(s; eps), with respect to the actor, through the live critics.
// Row: [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | sum log pi | sum min Q].
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) actor_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net th, Net q1, Net q2,
                                                                   const float* __restrict__ eps_dev, const float* __restrict__ log_alpha, float* __restrict__ partial) {
  typedef Shape<D, A, 2 * A> S;   // the actor's row with the 2 A output rows
  enum { AG_PI = 0, AG_W2T = S::LA_N, AG_W3T = AG_W2T + 4, AG_Q1 = AG_W3T + S::NQH, AQ_DA = S::LQ_FWD, AQ_N = AQ_DA + 4, AG_Q2 = AG_Q1 + AQ_N, AG_N = AG_Q2 + AQ_N };
  constexpr int NROW = S::NPA + 2, NS = S::NS, NQ1 = S::NQ1, NQA = S::NQA;
  __shared__ alignas(16) float tilemem[tilemem_floats<NROW>()];
  __shared__ alignas(16) float sbias[9][32];   // actor b1 b2 b3;  critics b1 b2 W3 each
  __shared__ float4 wimg[AG_N][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, h = lane >> 5;
  if (tid < 32) {
    sbias[0][tid] = th.b1[tid]; sbias[1][tid] = th.b2[tid]; sbias[2][tid] = out_bias<A, K_HEAD>(th.b3, tid);
    sbias[3][tid] = q1.b1[tid]; sbias[4][tid] = q1.b2[tid]; sbias[5][tid] = q1.W3[tid];
    sbias[6][tid] = q2.b1[tid]; sbias[7][tid] = q2.b2[tid]; sbias[8][tid] = q2.W3[tid];
  }
  {
    const Grp g[13] = {{K_FIRST, th.W1, AG_PI + S::LA_W1, NQ1}, {K_HID, th.W2, AG_PI + S::LA_W2, 4}, {K_HEAD, th.W3, AG_PI + S::LA_W3, 4}, {K_HIDT, th.W2, AG_W2T, 4},
                       {K_HEADT, th.W3, AG_W3T, S::NQH},
                       {K_FIRST, q1.W1, AG_Q1 + S::LQ_W1, NQ1}, {K_HIDQ, q1.W2, AG_Q1 + S::LQ_W2, 4}, {K_ACTIN, q1.W2, AG_Q1 + S::LQ_A, NQA}, {K_DA, q1.W2, AG_Q1 + AQ_DA, 4},
                       {K_FIRST, q2.W1, AG_Q2 + S::LQ_W1, NQ1}, {K_HIDQ, q2.W2, AG_Q2 + S::LQ_W2, 4}, {K_ACTIN, q2.W2, AG_Q2 + S::LQ_A, NQA}, {K_DA, q2.W2, AG_Q2 + AQ_DA, 4}};
    fill_images<D, A>(wimg, g, wave, lane);
  }
  const float b3q1 = q1.b3[0], b3q2 = q2.b3[0], alpha = expf(log_alpha[0]);
  __syncthreads();
  float* t0 = tilemem + (wave * 2) * 32 * TP;
  float* t1 = t0 + 32 * TP;
  ActorAcc<S::NB1> acc;
  zero(acc);
  float slp = 0.0f, sq = 0.0f;
  const int ntiles = (n + 31) / 32;
  for (int tl = blockIdx.x * WAVES + wave; tl < ntiles; tl += gridDim.x * WAVES) {
    Tile<D, A> t;
    gather<false>(pool, idx, n, tl, c, h, t);
    float ep[NS];
    action_slots<A>(eps_dev, t.smp, t.valid, h, ep);
    // ---- actor forward: a~ = tanh(mean + exp(log_std) eps) in the slots
    v16f a1, a2;
    float act[NS], sde[NS], logpi, aw[16];
    bool inside[NS];
    actor_sample<D, A>(wimg, AG_PI, sbias, t.xb, ep, lane, h, a1, a2, act, sde, inside, logpi);
    // ---- both critics at (s, a~);  d min(Q1, Q2) / da = W2a' (W3 o (h2 > 0)) of the smaller one, action a in register v of its slot
    v16f da = zero16();
    float qmin;
    {
      v16f c1, h2a, h2b;
      float wa[16], wb[16];
      w3_row(sbias[5], h, wa); w3_row(sbias[8], h, wb);
      const float qa = critic_forward<D, A>(wimg, AG_Q1, sbias + 3, wa, b3q1, t.xb, act, lane, h, c1, h2a);
      const float qb = critic_forward<D, A>(wimg, AG_Q2, sbias + 6, wb, b3q2, t.xb, act, lane, h, c1, h2b);
      const bool first = qa <= qb;
      qmin = first ? qa : qb;
      aop(wimg, AG_Q1 + AQ_DA, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], (first && h2a[v] > 0.0f) ? wa[v] : 0.0f, da);
      aop(wimg, AG_Q2 + AQ_DA, lane, aw);
#pragma unroll
      for (int v = 0; v < 16; v++) da = TILE_MFMA(aw[v], (!first && h2b[v] > 0.0f) ? wb[v] : 0.0f, da);
    }
    if (h == 0 && t.valid) { slp += logpi; sq += qmin; }
    // cotangents of alpha log pi - min Q on the output layer: d/du = 2 alpha a~ - dQ/da (1 - a~^2) on the mean row, that times
    // exp(log_std) eps, minus alpha, on the log_std row (nothing where the clamp is active)
    v16f wt = zero16();
#pragma unroll
    for (int v = 0; v < NS; v++) {
      const bool on = t.valid && row_of(v, h) < A;
      const float du = 2.0f * alpha * act[v] - da[v] * (1.0f - act[v] * act[v]);
      wt[v] = on ? du : 0.0f;
      wt[v + S::HREG] = (on && inside[v]) ? du * sde[v] - alpha : 0.0f;
    }
    actor_reverse<S::NQH>(wimg, AG_W2T, AG_W3T, a1, a2, wt, t.xt, t0, t1, lane, c, h, acc);   // the output rows of both heads
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) { slp += __shfl_xor(slp, m, 64); sq += __shfl_xor(sq, m, 64); }
  __syncthreads();
  float* red = tilemem + wave * NROW;
  actor_row<S, D, A, K_HEAD>(acc, red, c, h);
  if (lane == 0) { red[S::NPA] = slp; red[S::NPA + 1] = sq; }
  __syncthreads();
  reduce_rows<NROW>(tilemem, partial + (size_t)blockIdx.x * NROW);
}

// ---------------------------------------------------------------------------------------------------------------- apply (actor, temperature)
// The body of a unit's one-workgroup apply kernel (1024 threads).  The actor's Adam step from the pieces of apply_rows (mlp32_tiles.h, which keep
// contraction off), without a target network; the last thread takes log_alpha's Adam step on the gradient -(scale * sum log pi + target_entropy),
// the log pi column added in row order (alpha_m == NULL: the temperature is fixed).
__device__ __forceinline__ void actor_apply_rows(int rows, const float* __restrict__ partial, float scale, const NetRW& live, const int (&off)[7], float* __restrict__ m,
                                                 float* __restrict__ v, float a, float beta1, float beta2, float eps, float* __restrict__ log_alpha,
                                                 float* __restrict__ alpha_m, float* __restrict__ alpha_v, float a_alpha, float target_entropy,
                                                 double* __restrict__ stats) {
  constexpr int NSTAT = 2;
  const int np = off[6], stride = np + NSTAT;
  if ((int)threadIdx.x <= NSTAT && stats) {   // (sum log pi, sum min Q, the summed actor loss at the temperature BEFORE its step)
    double s[NSTAT] = {0.0, 0.0};
    for (int r = 0; r < rows; r++) {
      s[0] += (double)partial[(size_t)r * stride + np]; s[1] += (double)partial[(size_t)r * stride + np + 1];
    }
    stats[threadIdx.x] += threadIdx.x == 0 ? s[0] : (threadIdx.x == 1 ? s[1] : exp((double)log_alpha[0]) * s[0] - s[1]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < np; i += 1024)
    adam_entry(column_sum(partial + i, rows, stride, scale), m + i, v + i, entry_of(live, off, i), a, beta1, beta2, eps);
  if (threadIdx.x == 1023 && alpha_m)
    adam_entry(-(column_sum(partial + np, rows, stride, scale) + target_entropy), alpha_m, alpha_v, log_alpha, a_alpha, beta1, beta2, eps);
}

// ---------------------------------------------------------------------------------------------------------------- policy step
// policy_step (mlp32_tiles.h) with the squashed-Gaussian head: act = tanh(mean + exp(clamp(log_std)) noise), in [-1, 1] by construction.
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ noise,
                                                                    const double* __restrict__ low, const double* __restrict__ high, float* __restrict__ obs32,
                                                                    float* __restrict__ act, double* __restrict__ env_act) {
  policy_step<D, A, K_HEAD>(obs, n, th, low, high, obs32, act, env_act, [&](const v16f& z3, int v, size_t o, int) {
    const float ls = fminf(fmaxf(z3[v + head_reg(A)], LOG_STD_MIN), LOG_STD_MAX);
    return tanh_fast(z3[v] + expf(ls) * noise[o]);
  });
}

}  // namespace cassie_sac
