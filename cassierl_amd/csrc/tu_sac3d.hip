// tu_sac3d.hip -- Soft Actor-Critic's entry points at the Cassie3d shape, 45 observations and 10 actions (include/cassie_trpo.h, "SAC at 45 x 10";
// cassierl_amd/sac.py with env="cassie3d").  The contracts, the algorithm, the order of one update -- five launches -- and the kernels are
// tu_sac.hip's (read its header first): sac_kernels.h and mlp32_tiles.h are generic in (D, A), and this unit instantiates them at <45, 10>.  What
// the shape changes follows from those two numbers there: six action slots per lane half, the two heads on image rows a and 16 + a, the merge
// layer's six k-steps, the 23 k-steps of the first layer and [gW1 | gb1] as two accumulator tiles.  This unit keeps the six entry points with
// their argument checks (stricter than the 26-wide ones: the shape and the alignment of every pointer) and the critic's apply kernel (at 26 x 6
// that step is CassieDdpgApply, which refuses this shape).  It is a unit of its own so that the 45 x 10 kernels compile beside the others.
// CassieDdpgPoolCommit and CassieDdpgPartialRows are shape-free and are used as they are.
#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "sac_kernels.h"

namespace cassie_sac3d {

using namespace cassie_sac;

constexpr int D3 = 45, A3 = 10;
inline bool shape_ok3(int obs_dim, int act_dim) { return obs_dim == D3 && act_dim == A3; }

// a critic: apply_rows (mlp32_tiles.h), as tu_ddpg.hip's apply_kernel
__global__ void __launch_bounds__(1024) critic_apply_kernel(int rows, const float* __restrict__ partial, float scale, NetRW live, NetRW targ, Offsets off,
                                                            float* __restrict__ m, float* __restrict__ v, float a, float beta1, float beta2, float eps, float tau,
                                                            double* __restrict__ stats) {
  apply_rows(rows, 2, partial, scale, live, targ, off.o, m, v, a, beta1, beta2, eps, tau, stats);
}
// the actor and the temperature: actor_apply_rows (sac_kernels.h), as tu_sac.hip's apply_kernel
__global__ void __launch_bounds__(1024) actor_apply_kernel(int rows, const float* __restrict__ partial, float scale, NetRW live, Offsets off, float* __restrict__ m,
                                                           float* __restrict__ v, float a, float beta1, float beta2, float eps, float* __restrict__ log_alpha,
                                                           float* __restrict__ alpha_m, float* __restrict__ alpha_v, float a_alpha, float target_entropy,
                                                           double* __restrict__ stats) {
  actor_apply_rows(rows, partial, scale, live, off.o, m, v, a, beta1, beta2, eps, log_alpha, alpha_m, alpha_v, a_alpha, target_entropy, stats);
}

}  // namespace cassie_sac3d

extern "C" {

int CassieSac3dParamCount(int obs_dim, int act_dim, int which) {
  using namespace cassie_sac3d;
  typedef Shape<D3, A3, 2 * A3> S;
  if (!shape_ok3(obs_dim, act_dim)) return 0;
  return which == CASSIE_DDPG_ACTOR ? S::NPA : (which == CASSIE_DDPG_CRITIC ? S::NPQ : 0);
}

int CassieSac3dPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, const double* low_dev,
                          const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream) {
  using namespace cassie_sac3d;
  if (!shape_ok3(obs_dim, act_dim) || !obs_dev || n <= 0 || !net_ok(actor) || !noise_dev || !low_dev || !high_dev || !pool_obs_row_dev || !pool_act_row_dev ||
      !env_actions_dev)
    return CASSIE_EINVAL;
  if (!aligned4(noise_dev) || !aligned4(pool_obs_row_dev) || !aligned4(pool_act_row_dev) || ((uintptr_t)obs_dev & 7) || ((uintptr_t)env_actions_dev & 7) ||
      ((uintptr_t)low_dev & 7) || ((uintptr_t)high_dev & 7))
    return CASSIE_EINVAL;
  hipLaunchKernelGGL((policy_step_kernel<D3, A3>), dim3(policy_step_grid(n)), dim3(64 * WAVES), 0, (hipStream_t)stream, obs_dev, n, net_of(actor), noise_dev, low_dev, high_dev,
                     pool_obs_row_dev, pool_act_row_dev, env_actions_dev);
  return launched();
}

int CassieSac3dCriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                          long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                          const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                          const float* eps_next_dev, const float* log_alpha_dev, float discount, float* partial_dev, void* stream) {
  using namespace cassie_sac3d;
  const Pool pool{pool_obs, pool_act, pool_rew, pool_term, pool_next_obs, pool_capacity};
  if (!shape_ok3(obs_dim, act_dim) || !pool_ok(pool) || !idx_dev || batch <= 0 || !eps_next_dev || !log_alpha_dev || !partial_dev) return CASSIE_EINVAL;
  if (!aligned4(partial_dev) || !aligned4(eps_next_dev) || !aligned4(log_alpha_dev) || ((uintptr_t)idx_dev & 7)) return CASSIE_EINVAL;
  if (!net_ok(actor) || !net_ok(target_qf1) || !net_ok(target_qf2) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  hipLaunchKernelGGL((critic_grad_kernel<D3, A3>), dim3(blocks_for(batch)), dim3(64 * WAVES), 0, (hipStream_t)stream, pool, idx_dev, batch, net_of(actor), net_of(target_qf1),
                     net_of(target_qf2), net_of(qf1), net_of(qf2), eps_next_dev, log_alpha_dev, discount, partial_dev);
  return launched();
}

int CassieSac3dActorGrad(const float* pool_obs, long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                         const float* const* qf1, const float* const* qf2, const float* eps_dev, const float* log_alpha_dev, float* partial_dev, void* stream) {
  using namespace cassie_sac3d;
  if (!shape_ok3(obs_dim, act_dim) || !pool_obs || pool_capacity <= 0 || !idx_dev || batch <= 0 || !eps_dev || !log_alpha_dev || !partial_dev) return CASSIE_EINVAL;
  if (!aligned4(partial_dev) || !aligned4(eps_dev) || !aligned4(log_alpha_dev) || ((uintptr_t)idx_dev & 7)) return CASSIE_EINVAL;
  if (!net_ok(actor) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  const Pool pool{pool_obs, nullptr, nullptr, nullptr, nullptr, pool_capacity};
  hipLaunchKernelGGL((actor_grad_kernel<D3, A3>), dim3(blocks_for(batch)), dim3(64 * WAVES), 0, (hipStream_t)stream, pool, idx_dev, batch, net_of(actor), net_of(qf1), net_of(qf2),
                     eps_dev, log_alpha_dev, partial_dev);
  return launched();
}

int CassieSac3dCriticApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* live, float* const* target, float* m_dev,
                           float* v_dev, int t, float lr, float beta1, float beta2, float eps, float tau, double* stats_dev, void* stream) {
  using namespace cassie_sac3d;
  if (!shape_ok3(obs_dim, act_dim) || rows <= 0 || !partial_dev || !aligned4(partial_dev) || !net_ok(live) || !net_ok(target) || !m_dev || !v_dev || t < 1)
    return CASSIE_EINVAL;
  Offsets off;
  critic_offsets(obs_dim, act_dim, off.o);
  hipLaunchKernelGGL(critic_apply_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, partial_dev, scale, net_rw(live), net_rw(target), off, m_dev, v_dev,
                     adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, tau, stats_dev);
  return launched();
}

int CassieSac3dActorApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* actor, float* m_dev, float* v_dev, int t, float lr,
                          float beta1, float beta2, float eps, float* log_alpha_dev, float* alpha_m_dev, float* alpha_v_dev, int alpha_t, float alpha_lr,
                          float target_entropy, double* stats_dev, void* stream) {
  using namespace cassie_sac3d;
  if (!shape_ok3(obs_dim, act_dim) || rows <= 0 || !partial_dev || !aligned4(partial_dev) || !net_ok(actor) || !m_dev || !v_dev || t < 1 || !log_alpha_dev)
    return CASSIE_EINVAL;
  if (alpha_m_dev && (!alpha_v_dev || alpha_t < 1)) return CASSIE_EINVAL;
  Offsets off;
  actor_offsets(obs_dim, 2 * act_dim, off.o);
  hipLaunchKernelGGL(actor_apply_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, partial_dev, scale, net_rw(actor), off, m_dev, v_dev,
                     adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, log_alpha_dev, alpha_m_dev, alpha_v_dev,
                     alpha_m_dev ? adam_step_size(alpha_lr, beta1, beta2, alpha_t) : 0.0f, target_entropy, stats_dev);
  return launched();
}

}  // extern "C"
