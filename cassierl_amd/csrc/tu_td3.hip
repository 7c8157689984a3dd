// tu_td3.hip -- fused kernels of TD3 (include/cassie_trpo.h, cassierl_amd/td3.py): the policy step with stateless Gaussian exploration that
// writes straight into the replay pool, the gradient of BOTH critics against a smoothed, clipped target action under the minimum of the two
// target critics in one launch, and both critics' Adam steps and soft updates in one launch of two workgroups.  An update that leaves the actor
// alone is these two launches; a delayed one adds tu_ddpg.hip's CassieDdpgActorGrad (through the first critic) and CassieDdpgApply (actor).
//
// The networks are tu_ddpg.hip's 32 x 32 ReLU networks and every convention is its (mlp32_tiles.h; read tu_ddpg.hip's header first).  Nothing
// here is a new building block, and every block is mlp32_tiles.h's: the target actor's forward pass (actor_forward), the two target critics under
// a minimum and the two live critics one after the other on the same registers (twin_critic_grad, shared with tu_sac.hip), the policy step's body
// (policy_step), the Adam step (apply_rows, which is CassieDdpgApply's body).  What is TD3's own is the target action
//   a' = clip(mu'(s') + clip(policy_noise eps, -noise_clip, noise_clip), -1, 1),
// formed in the registers in which the target actor's output layer leaves mu'(s') and the critics' merge layer takes it.  The noise eps
// arrives as a tensor indexed by the batch position (there is no generator in a kernel).
// Every sum runs in a fixed order: a launch repeats bit for bit.
#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "mlp32_tiles.h"

namespace cassie_td3 {

using namespace cassie_mlp32;

__device__ __forceinline__ float clip(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// ---------------------------------------------------------------------------------------------------------------- critic gradients
// twin_critic_grad (mlp32_tiles.h) with a' as above from eps[b] and nothing subtracted from the minimum.
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 1) critic_grad_kernel(Pool pool, const long long* __restrict__ idx, int n, Net ta, Net tq1, Net tq2, Net q1, Net q2,
                                                                    const float* __restrict__ eps_next, float policy_noise, float noise_clip, float gamma,
                                                                    float* __restrict__ partial) {
  typedef Shape<D, A> S;
  static_assert(S::NS == 4, "the target action below is written for four slots, the action a = v + 4 h in register v < 4 (A <= 8)");
  const auto target = [=](const float4 (*wimg)[64], const float (*sb)[32], const float (&xn)[S::KS1], const float (&en)[4], int lane, int h, float (&an)[4]) {
    v16f a1, a2, mu;
    actor_forward<D, A>(wimg, TC_PI, sb, xn, lane, h, a1, a2, mu);
#pragma unroll
    for (int v = 0; v < 4; v++)   // rows a >= A: W3, b3 and the noise are zeros -> a' = 0, on zero columns of the merge layer's image
      an[v] = clip(tanh_fast(mu[v]) + clip(policy_noise * en[v], -noise_clip, noise_clip), -1.0f, 1.0f);
    return 0.0f;
  };
  twin_critic_grad<D, A, K_OUT>(pool, idx, n, ta, tq1, tq2, q1, q2, eps_next, gamma, partial, target);
}

// ---------------------------------------------------------------------------------------------------------------- apply (both critics)
// Workgroup k is CassieDdpgApply's workgroup on critic k: apply_rows (mlp32_tiles.h) on block k of the partial tensor, with the critic's two
// statistic columns added to stats[2 k], stats[2 k + 1].
struct CriticSide { const float* partial; NetRW live, targ; float *m, *v; double* stats; };
struct CriticPair { CriticSide side[2]; int off[7]; };
__global__ void __launch_bounds__(1024) critic_apply_kernel(int rows, float scale, CriticPair pair, float a, float beta1, float beta2, float eps, float tau) {
  const CriticSide& s = pair.side[blockIdx.x];
  apply_rows(rows, 2, s.partial, scale, s.live, s.targ, pair.off, s.m, s.v, a, beta1, beta2, eps, tau, s.stats);
}

// ---------------------------------------------------------------------------------------------------------------- policy step
// policy_step (mlp32_tiles.h) with stateless exploration: act = clip(mu(s) + sigma noise, -1, 1).
template <int D, int A>
__global__ void __launch_bounds__(64 * WAVES, 2) policy_step_kernel(const double* __restrict__ obs, int n, Net th, const float* __restrict__ noise, float sigma,
                                                                    const double* __restrict__ low, const double* __restrict__ high, float* __restrict__ obs32,
                                                                    float* __restrict__ act, double* __restrict__ env_act) {
  policy_step<D, A, K_OUT>(obs, n, th, low, high, obs32, act, env_act,
                           [&](const v16f& z3, int v, size_t o, int) { return clip(tanh_fast(z3[v]) + sigma * noise[o], -1.0f, 1.0f); });
}

}  // namespace cassie_td3

extern "C" {

int CassieTd3PolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, float sigma, const double* low_dev,
                        const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream) {
  using namespace cassie_td3;
  if (!obs_dev || n <= 0 || !net_ok(actor) || !noise_dev || !low_dev || !high_dev || !pool_obs_row_dev || !pool_act_row_dev || !env_actions_dev) return CASSIE_EINVAL;
  MLP32_LAUNCH_STEP(policy_step_kernel, obs_dim, act_dim, policy_step_grid(n), stream, obs_dev, n, net_of(actor), noise_dev, sigma, low_dev, high_dev, pool_obs_row_dev,
                    pool_act_row_dev, env_actions_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieTd3CriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                        long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* target_actor,
                        const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                        const float* eps_next_dev, float policy_noise, float noise_clip, float discount, float* partial_dev, void* stream) {
  using namespace cassie_td3;
  const Pool pool{pool_obs, pool_act, pool_rew, pool_term, pool_next_obs, pool_capacity};
  if (!pool_ok(pool) || !idx_dev || batch <= 0 || !eps_next_dev || !(noise_clip >= 0.0f) || !partial_dev || !aligned4(partial_dev)) return CASSIE_EINVAL;
  if (!net_ok(target_actor) || !net_ok(target_qf1) || !net_ok(target_qf2) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  MLP32_LAUNCH(critic_grad_kernel, obs_dim, act_dim, blocks_for(batch), stream, pool, idx_dev, batch, net_of(target_actor), net_of(target_qf1), net_of(target_qf2),
               net_of(qf1), net_of(qf2), eps_next_dev, policy_noise, noise_clip, discount, partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieTd3CriticApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* qf1, float* const* qf2, float* const* target_qf1,
                         float* const* target_qf2, float* m1_dev, float* v1_dev, float* m2_dev, float* v2_dev, int t, float lr, float beta1, float beta2, float eps,
                         float tau, double* stats_dev, void* stream) {
  using namespace cassie_td3;
  const int np = CassieDdpgParamCount(obs_dim, act_dim, CASSIE_DDPG_CRITIC);
  if (np == 0 || rows <= 0 || !partial_dev || !m1_dev || !v1_dev || !m2_dev || !v2_dev || t < 1) return CASSIE_EINVAL;
  if (!net_ok(qf1) || !net_ok(qf2) || !net_ok(target_qf1) || !net_ok(target_qf2)) return CASSIE_EINVAL;
  CriticPair pair;
  pair.side[0] = CriticSide{partial_dev, net_rw(qf1), net_rw(target_qf1), m1_dev, v1_dev, stats_dev};
  pair.side[1] = CriticSide{partial_dev + (size_t)rows * (np + 2), net_rw(qf2), net_rw(target_qf2), m2_dev, v2_dev, stats_dev ? stats_dev + 2 : nullptr};
  critic_offsets(obs_dim, act_dim, pair.off);   // the critic's row, as CassieDdpgApply lays it out
  hipLaunchKernelGGL(critic_apply_kernel, dim3(2), dim3(1024), 0, (hipStream_t)stream, rows, scale, pair, adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, tau);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
