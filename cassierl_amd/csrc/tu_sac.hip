// tu_sac.hip -- fused kernels of Soft Actor-Critic (include/cassie_trpo.h, cassierl_amd/sac.py): the policy step that samples the squashed
// Gaussian and writes straight into the replay pool, the gradient of BOTH critics in one launch, the actor's gradient through the minimum of
// the two critics and through log pi, and the actor's Adam step with the temperature's.  One update is five launches (critic gradient,
// CassieDdpgApply for each critic, actor gradient, CassieSacApply) where the torch statement (sac.sac_update_torch_) is well over a hundred.
//
// The networks are tu_ddpg.hip's 32 x 32 ReLU networks and every convention is its (mlp32_tiles.h; read tu_ddpg.hip's header first).  The
// critics ARE DDPG's critics, so their Adam step and soft update are CassieDdpgApply.  What is new:
//   * the actor's output layer has 2 A rows, mean [0, A) and log_std [A, 2 A).  Its A-operand image permutes them: image row a holds mean a,
//     image row 2 HREG + a holds log_std a (HREG = 4 for A <= 8, 8 above: cassie_tiles.h, head_reg).  In the accumulator layout the lane
//     (sample, h) then holds, for the action of its slot v, the mean in register v and log_std in register v + HREG: the sample
//     u = mean + exp(log_std) eps, a = tanh(u) and log pi need no data movement, the action sits where the critic's merge layer takes it
//     (tu_ddpg.hip), and the cotangents of both heads sit where the reverse pass takes them (HREG / 2 quads of k-steps instead of DDPG's one);
//   * log pi(a|s) = sum_k (-eps_k^2 / 2 - log_std_k - log(2 pi) / 2) - sum_k 2 (log 2 - u_k - softplus(-2 u_k)); its derivative with respect
//     to u_k is 2 tanh(u_k), with respect to log_std_k directly -1; the clamp of log_std to [-20, 2] passes no gradient outside;
//   * the noise eps arrives as a tensor indexed by the batch position (there is no generator in a kernel); the temperature as a device
//     pointer to log_alpha, so that no launch waits for a read-back;
//   * the critic kernel computes y once per sample and runs the two live critics one after the other on the same registers; each critic
//     has its own block [rows][NPq + 2] of the partial tensor, which is CassieDdpgApply's row format.  Its body is twin_critic_grad of
//     mlp32_tiles.h, shared with tu_td3.hip: SAC gives it the target action and the entropy term.
// SAC's device code -- the squashed-Gaussian head (squash, actor_sample), the cotangents of its actor kernel, the temperature's Adam step and
// its statistics -- is sac_kernels.h's, shared with tu_sac3d.hip (the same kernels at 45 x 10); everything else is mlp32_tiles.h's.  This unit
// keeps the entry points at 26 x 6, 26 x 7, 17 x 6, 17 x 7 and their instantiations; it refuses every other shape.
// Every sum runs in a fixed order: a launch repeats bit for bit.
#include "../../include/cassie_trpo.h"
#include "../../include/cassie_vec.h"
#include "sac_kernels.h"

namespace cassie_sac {

// the actor and the temperature: actor_apply_rows (sac_kernels.h).  One workgroup.
__global__ void __launch_bounds__(1024) apply_kernel(int rows, const float* __restrict__ partial, float scale, NetRW live, Offsets off, float* __restrict__ m,
                                                     float* __restrict__ v, float a, float beta1, float beta2, float eps, float* __restrict__ log_alpha,
                                                     float* __restrict__ alpha_m, float* __restrict__ alpha_v, float a_alpha, float target_entropy,
                                                     double* __restrict__ stats) {
  actor_apply_rows(rows, partial, scale, live, off.o, m, v, a, beta1, beta2, eps, log_alpha, alpha_m, alpha_v, a_alpha, target_entropy, stats);
}

}  // namespace cassie_sac

extern "C" {

int CassieSacParamCount(int obs_dim, int act_dim) {
  if (!cassie_sac::shape_ok(obs_dim, act_dim)) return 0;
  int off[7];
  cassie_sac::actor_offsets(obs_dim, 2 * act_dim, off);
  return off[6];
}

int CassieSacPolicyStep(const double* obs_dev, int n, int obs_dim, int act_dim, const float* const* actor, const float* noise_dev, const double* low_dev,
                        const double* high_dev, float* pool_obs_row_dev, float* pool_act_row_dev, double* env_actions_dev, void* stream) {
  using namespace cassie_sac;
  if (!obs_dev || n <= 0 || !net_ok(actor) || !noise_dev || !low_dev || !high_dev || !pool_obs_row_dev || !pool_act_row_dev || !env_actions_dev) return CASSIE_EINVAL;
  MLP32_LAUNCH_STEP(policy_step_kernel, obs_dim, act_dim, policy_step_grid(n), stream, obs_dev, n, net_of(actor), noise_dev, low_dev, high_dev, pool_obs_row_dev,
                    pool_act_row_dev, env_actions_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieSacCriticGrad(const float* pool_obs, const float* pool_act, const float* pool_rew, const float* pool_term, const float* pool_next_obs,
                        long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                        const float* const* target_qf1, const float* const* target_qf2, const float* const* qf1, const float* const* qf2,
                        const float* eps_next_dev, const float* log_alpha_dev, float discount, float* partial_dev, void* stream) {
  using namespace cassie_sac;
  const Pool pool{pool_obs, pool_act, pool_rew, pool_term, pool_next_obs, pool_capacity};
  if (!pool_ok(pool) || !idx_dev || batch <= 0 || !eps_next_dev || !log_alpha_dev || !partial_dev || !aligned4(partial_dev)) return CASSIE_EINVAL;
  if (!net_ok(actor) || !net_ok(target_qf1) || !net_ok(target_qf2) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  MLP32_LAUNCH(critic_grad_kernel, obs_dim, act_dim, blocks_for(batch), stream, pool, idx_dev, batch, net_of(actor), net_of(target_qf1), net_of(target_qf2), net_of(qf1),
               net_of(qf2), eps_next_dev, log_alpha_dev, discount, partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieSacActorGrad(const float* pool_obs, long long pool_capacity, const long long* idx_dev, int batch, int obs_dim, int act_dim, const float* const* actor,
                       const float* const* qf1, const float* const* qf2, const float* eps_dev, const float* log_alpha_dev, float* partial_dev, void* stream) {
  using namespace cassie_sac;
  if (!pool_obs || pool_capacity <= 0 || !idx_dev || batch <= 0 || !eps_dev || !log_alpha_dev || !partial_dev || !aligned4(partial_dev)) return CASSIE_EINVAL;
  if (!net_ok(actor) || !net_ok(qf1) || !net_ok(qf2)) return CASSIE_EINVAL;
  const Pool pool{pool_obs, nullptr, nullptr, nullptr, nullptr, pool_capacity};
  MLP32_LAUNCH(actor_grad_kernel, obs_dim, act_dim, blocks_for(batch), stream, pool, idx_dev, batch, net_of(actor), net_of(qf1), net_of(qf2), eps_dev, log_alpha_dev,
               partial_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

int CassieSacApply(int rows, int obs_dim, int act_dim, const float* partial_dev, float scale, float* const* actor, float* m_dev, float* v_dev, int t, float lr,
                   float beta1, float beta2, float eps, float* log_alpha_dev, float* alpha_m_dev, float* alpha_v_dev, int alpha_t, float alpha_lr,
                   float target_entropy, double* stats_dev, void* stream) {
  using namespace cassie_sac;
  if (CassieSacParamCount(obs_dim, act_dim) == 0 || rows <= 0 || !partial_dev || !net_ok(actor) || !m_dev || !v_dev || t < 1 || !log_alpha_dev) return CASSIE_EINVAL;
  if (alpha_m_dev && (!alpha_v_dev || alpha_t < 1)) return CASSIE_EINVAL;
  Offsets off;
  actor_offsets(obs_dim, 2 * act_dim, off.o);
  hipLaunchKernelGGL(apply_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, partial_dev, scale, net_rw(actor), off, m_dev, v_dev,
                     adam_step_size(lr, beta1, beta2, t), beta1, beta2, eps, log_alpha_dev, alpha_m_dev, alpha_v_dev,
                     alpha_m_dev ? adam_step_size(alpha_lr, beta1, beta2, alpha_t) : 0.0f, target_entropy, stats_dev);
  return hipGetLastError() == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

}  // extern "C"
