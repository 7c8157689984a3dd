"""Vanilla policy gradient over the batched environment: counterpart of rllab/envs/vpg_cassie.py:15-48.

  policy     GaussianMLPPolicy(hidden_sizes=(128, 128), init_std=1.0)            vpg_cassie.py
             (tanh hidden units, state-independent learned log-std)
  baseline   LinearFeatureBaseline                                               vpg_cassie.py
  algorithm  VPG: batch_size=10000, max_path_length=1000, n_itr=1000, discount=0.99   vpg_cassie.py
  env        normalize(Cassie2dEnv())                                            vpg_cassie.py

What rllab's VPG does with these [external: rllab's published source, not on this machine]:
  * the loss is -mean(logli(a | theta) * adv), with center_adv=True and gae_lambda=1 (BatchPolopt's defaults, as for TRPO);
  * the optimiser is FirstOrderOptimizer(batch_size=None, max_epochs=1) with lasagne.updates.adam and learning_rate=1e-3: ONE
    full-batch Adam step per iteration, the Adam state (m, v, t) kept across iterations;
  * Lasagne's Adam: t += 1; a = lr sqrt(1 - beta2^t) / (1 - beta1^t); m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2;
    theta -= a m / (sqrt(v) + eps), beta1 = 0.9, beta2 = 0.999, eps = 1e-8 -- eps outside the bias correction, which is NOT what
    torch.optim.Adam does (it adds eps to the bias-corrected sqrt(v_hat));
  * vpg_cassie.py's step_size=0.005 and use_gpu=True are swallowed by BatchPolopt's **kwargs: rllab's VPG never reads them.

The sampler, the exploration noise keyed by the global env id, the baseline kernels, advantage centring and the snapshot machinery
are sampler.OnPolicy's, shared with TRPO and PPO.  The hot paths of the width-128 policy are HIP kernels (csrc/tu_pg.hip): the policy
step of the sampler, the policy gradient J' w, and the Adam step.
"""
import torch
import torch.distributed as dist

from .adam import FlatAdam, adam_step_, fused_adam_step_   # (the two steps: tests and tools call Lasagne's Adam as vpg.adam_step_ / vpg.fused_adam_step_)
from .comm import _world, all_mean_
from .fisher import FusedFisher, PgFisher
from .policy import _MEAN_ORDER, _two_layer_tanh, closed_form_grad, flat_grad, flat_params, hidden_sizes_of, set_flat_params   # (_MEAN_ORDER: as vpg._MEAN_ORDER in tests)
from .sampler import OnPolicy, broadcast_initial_policy, gaussian_policy_nets, make_cassie_algo


class PolicyGradKernels:
    """The policy gradient of one batch: width 32 -> CassieTrpoVjp (FusedFisher.vjp), width 128 -> CassiePgVjp (PgFisher.vjp), each in closed
    form; CPU, other shapes or fused=False -> autograd of the surrogate.  `kind` says which ("trpo_vjp", "pg_vjp" or "autograd")."""

    def __init__(self, policy, obs, fused=True):
        self.policy, self.obs = policy, obs
        self.kind, self._vjp = "autograd", None
        if not fused or _two_layer_tanh(policy) is None or not obs.is_cuda or obs.dtype != torch.float32:
            return
        cls, kind = {(32, 32): (FusedFisher, "trpo_vjp"), (128, 128): (PgFisher, "pg_vjp")}.get(hidden_sizes_of(policy), (None, None))
        try:
            if cls is not None:
                self._vjp, self.kind = cls(policy, obs).vjp, kind
        except (ValueError, OSError):
            pass
        self._pg_vjp = self._vjp   # (the name the width-128 tests and tools/ab_vpg_policy.py call J' w by)

    def grad(self, act, old_mean, old_lstd, adv):
        """This rank's gradient of -mean(logli adv) (flat, parameter order)."""
        if self._vjp is not None:
            return closed_form_grad(self.policy, self._vjp, act, old_mean, old_lstd, adv)
        mean, log_std = self.policy.dist_info(self.obs)
        loss = -(self.policy.log_likelihood(act, mean, log_std) * adv).mean()
        return flat_grad(loss, self.policy).detach()


class VPG(FlatAdam, OnPolicy):
    """rllab's VPG on OnPolicy's sampler and baseline.  Switches (attributes, default True) that tests set to force the torch path:
    fused_policy_step (the sampler's policy step), fused_grad (PolicyGradKernels), fused_adam (CassiePgAdam)."""
    ALGO = "vpg"

    def __init__(self, env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size=10000, max_path_length=1000, discount=0.99,
                 learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, log_kl=False, seed=1, env_reset_masked=None, env_id0=None):
        super().__init__(env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size=batch_size, max_path_length=max_path_length,
                         discount=discount, seed=seed, env_reset_masked=env_reset_masked, env_id0=env_id0)
        self._adam_init(learning_rate, beta1, beta2, epsilon)
        self.log_kl = log_kl
        self.last_grad_kind = None

    # the sampler's policy step (CassiePgPolicyStep for a 128-128 policy, CassieTrpoPolicyStep for 32 x 32) is OnPolicy._fused_policy_step

    def optimize(self, d):
        pol = self.policy
        obs, act, adv, old_mean, old_lstd = d["obs"], d["act"], d["adv"], d["mean"], d["log_std"]
        pk = PolicyGradKernels(pol, obs, fused=getattr(self, "fused_grad", True))
        self.last_grad_kind = pk.kind
        g = all_mean_(pk.grad(act, old_mean, old_lstd, adv).contiguous(), "gradient_all_reduce")
        theta = flat_params(pol).contiguous()
        before = theta.clone()
        self.adam_step(theta, g.to(theta.dtype))
        set_flat_params(pol, theta)
        vals = [g.double().norm(), (theta - before).double().norm()]
        if self.log_kl:   # rllab's logged MeanKL / MaxKL / LossAfter: one more forward pass over the batch
            with torch.no_grad():
                mean, log_std = pol.dist_info(obs)
                kl = pol.kl(old_mean, old_lstd, mean, log_std)
                loss_after = -(pol.log_likelihood(act, mean, log_std) * adv).mean()
                mk = kl.max().double().reshape(1).clone()
                if _world() > 1:
                    dist.all_reduce(mk, op=dist.ReduceOp.MAX)
                vals += [all_mean_(kl.mean().double().reshape(1).clone(), "stats_all_reduce")[0], mk[0],
                         all_mean_(loss_after.double().reshape(1).clone(), "stats_all_reduce")[0]]
        vals = torch.stack(vals).tolist()   # one read-back
        st = dict(grad_norm=vals[0], step_norm=vals[1])
        if self.log_kl:
            st.update(mean_kl=vals[2], max_kl=vals[3], loss_after=vals[4])
        return st

    # ---- snapshot: Sampler's, plus the algorithm, the policy shape, the learning rate and the Adam state
    def _snapshot_fields(self):
        return dict(super()._snapshot_fields(), learning_rate=float(self.learning_rate), **self._adam_snapshot())

    def _load_fields(self, ck):
        super()._load_fields(ck)
        self._adam_load(ck)


def make_cassie_vpg(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, hidden_sizes=(128, 128), init_std=1.0,
                    learning_rate=1e-3, terrain=None, sync_policy=True, **kw):
    """vpg_cassie.py:15-48 on the batched MI355X environment; the counterpart of trpo.make_cassie_trpo (same env, terrain and sync_policy rules)."""
    return make_cassie_algo(VPG, gaussian_policy_nets(hidden_sizes, init_std), broadcast_initial_policy, n_envs, kind, control_mode, device, trajectory, seed,
                            terrain, sync_policy, learning_rate=learning_rate, **kw)
