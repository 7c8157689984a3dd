"""TRPO outer loop over the batched environment: counterpart of rllab/envs/trpo_cassie.py:12-55.

The reference drives ONE environment through rllab's TRPO (Theano).  Here the rollout is N resident environments stepped by
one kernel launch per Env.step, and the optimiser is written directly against torch tensors on the same device:

  policy     GaussianMLPPolicy(hidden_sizes=(32, 32), init_std=2.0)            trpo_cassie.py:21-27
             (tanh hidden units, state-independent learned log-std -- rllab's defaults [external])
  baseline   LinearFeatureBaseline: ridge regression on [o, o^2, t, t^2, t^3, 1]  trpo_cassie.py:29 [external]
  algorithm  TRPO: batch_size env-steps per iteration, max_path_length=1000, discount=0.99, step_size (mean KL) 0.005,
             conjugate gradient (10 iterations, damping 1e-5) + backtracking line search (0.8, 15)   trpo_cassie.py:31-42
  env        normalize(Cassie2dEnv()): actions in [-1, 1] mapped affinely to the action box and clipped  trpo_cassie.py:13

Multi-GPU: one process per GPU, each with its own shard of environments; the policy gradient, every Fisher-vector
product, the baseline's normal equations and the line-search statistics are averaged with all_reduce (RCCL on MI355X, gloo in
the CPU tests), so all ranks take the identical step.  Episode returns are gathered once per batch (rollout.gather_returns).

This module is TRPO alone: the sampler, the baseline and the snapshot are sampler.OnPolicy's; the policy, the Fisher-vector products, the
collectives and the environment builder live in policy.py, fisher.py, comm.py and sampler.py.
"""
import math

import torch

from .comm import all_mean_
from .fisher import AnalyticFisher, FusedFisher, PgFisher, conjugate_gradient
from .policy import closed_form_grad, flat_grad, flat_params, set_flat_params
from .sampler import OnPolicy, broadcast_initial_policy, gaussian_policy_nets, make_cassie_algo

COMM = None   # the slot of comm.CommTimer: bench.py sets `trpo.COMM = CommTimer()` around its timed iterations; every collective looks it up here


class TRPO(OnPolicy):
    ALGO = "trpo"   # (a plain TRPO snapshot has no "algo" entry)

    def __init__(self, env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size=15000, max_path_length=1000,
                 discount=0.99, step_size=0.005, cg_iters=10, reg_coeff=1e-5, backtrack_ratio=0.8, max_backtracks=15, seed=1,
                 env_reset_masked=None, env_id0=None):
        """The environment's functions, batch_size and the sampler's arguments: sampler.Sampler; the deviations from rllab's sampler: sampler.OnPolicy."""
        super().__init__(env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size=batch_size, max_path_length=max_path_length,
                         discount=discount, seed=seed, env_reset_masked=env_reset_masked, env_id0=env_id0)
        self.step_size = step_size
        self.cg_iters, self.reg_coeff = cg_iters, reg_coeff
        self.backtrack_ratio, self.max_backtracks = backtrack_ratio, max_backtracks

    # ---- constrained update
    def optimize(self, d):
        pol = self.policy
        obs, act, adv, old_mean, old_lstd = d["obs"], d["act"], d["adv"], d["mean"], d["log_std"]
        old_ll = None

        def surrogate():
            nonlocal old_ll
            if old_ll is None:
                old_ll = pol.log_likelihood(act, old_mean, old_lstd)
            mean, log_std = pol.dist_info(obs)
            lr = (pol.log_likelihood(act, mean, log_std) - old_ll).exp()
            return -(lr * adv).mean(), pol.kl(old_mean, old_lstd, mean, log_std).mean()

        # Fisher-vector products: closed form for the tanh-MLP Gaussian policy -- FusedFisher = the product as ONE launch on the matrix
        # cores (csrc/tu_trpo.hip: 0.16 ms against 0.66 ms per product for the torch operations of AnalyticFisher at 524 288 samples,
        # r04), PgFisher its counterpart for the 128 x 128 policy (csrc/tu_pg_trpo.hip), AnalyticFisher where no kernel applies (CPU, other
        # shapes); otherwise double backprop through ONE graph of grad(KL) (the KL and its gradient do not depend on v: only the second
        # backward pass is repeated per product).  last_fisher_kind says which ran: "trpo_fvp", "pg_fvp", "analytic" or "autograd".
        gk = kl0 = None
        fisher = None
        if getattr(self, "analytic_fisher", True):
            for cls in ((FusedFisher, PgFisher, AnalyticFisher) if getattr(self, "fused_fisher", True) else (AnalyticFisher,)):
                try:
                    fisher = cls(pol, obs)
                    break
                except (ValueError, OSError):
                    fisher = None
        self.last_fisher_kind = "autograd" if fisher is None else fisher.kind
        if fisher is not None:
            # policy gradient in closed form too (closed_form_grad): at theta = theta_old the likelihood ratio is 1, loss = -mean(adv), and
            # J' (d loss / d mean) comes from the Fisher object's reverse pass (r04: 3.9 ms of autograd -> 0.5 ms at 524 288 samples).
            # ASSUMES the batch is exactly on-policy -- old_mean / old_lstd were produced by the CURRENT parameters (true for this
            # sampler: optimize() runs right after the rollout that recorded them) -- and a state-independent log_std; a caller that
            # reuses an older batch must set analytic_fisher = False (the autograd gradient below makes neither assumption).
            g = closed_form_grad(pol, fisher.vjp, act, old_mean, old_lstd, adv)
            loss = -adv.mean()
            g = all_mean_(g, "gradient_all_reduce")
        else:
            loss, _ = surrogate()
            g = all_mean_(flat_grad(loss, pol), "gradient_all_reduce")
            _, kl0 = surrogate()
            gk = flat_grad(kl0, pol, retain_graph=True, create_graph=True)

        def Fvp(v):
            hv = fisher(v) if fisher is not None else flat_grad(gk @ v, pol, retain_graph=True)
            return all_mean_(hv, "fvp_all_reduce") + self.reg_coeff * v

        descent = fisher.conjugate_gradient(g, self.cg_iters, self.reg_coeff) if isinstance(fisher, FusedFisher) and getattr(self, "fused_cg", True) else None
        if descent is None:
            descent = conjugate_gradient(Fvp, g, self.cg_iters)
        shs = 0.5 * (descent @ Fvp(descent))
        if isinstance(fisher, FusedFisher):   # the line search evaluates loss and KL in one launch each (CassieTrpoSurrogate / CassiePgSurrogate)
            ff, old_ls_vec = fisher, old_lstd[0].detach().clone()
            surrogate = lambda: ff.surrogate(pol, act, adv, old_mean, old_ls_vec)
        del gk, kl0, fisher
        step = torch.sqrt(self.step_size / (shs + 1e-8)) * descent
        if not torch.isfinite(step).all():
            return dict(loss_before=float(loss), loss_after=float(loss), kl=0.0, backtracks=-1)
        theta = flat_params(pol)
        loss_before = float(all_mean_(loss.detach().clone().view(1), "line_search_all_reduce"))
        for k in range(self.max_backtracks + 1):
            set_flat_params(pol, theta - (self.backtrack_ratio ** k) * step)
            with torch.no_grad():
                l_new, kl_new = surrogate()
            l_new, kl_new = all_mean_(torch.stack([l_new.detach().double().reshape(()), kl_new.detach().double().reshape(())]), "line_search_all_reduce").tolist()   # one read-back
            if math.isfinite(l_new) and l_new < loss_before and kl_new <= self.step_size:
                return dict(loss_before=loss_before, loss_after=l_new, kl=kl_new, backtracks=k)
        set_flat_params(pol, theta)  # line search failed: keep the old policy
        return dict(loss_before=loss_before, loss_after=loss_before, kl=0.0, backtracks=self.max_backtracks + 1)


def make_cassie_trpo(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, sync_policy=True, terrain=None, hidden_sizes=(32, 32),
                     init_std=2.0, **kw):
    """trpo_cassie.py:12-42 on the batched MI355X environment (make_cassie_algo: env, terrain and sync_policy rules).  hidden_sizes / init_std: the
    policy (trpo_cassie.py's 32 x 32 and 2.0 by default; (128, 128) runs on the kernels of csrc/tu_pg*.hip)."""
    return make_cassie_algo(TRPO, gaussian_policy_nets(hidden_sizes, init_std), broadcast_initial_policy, n_envs, kind, control_mode, device, trajectory, seed,
                            terrain, sync_policy, **kw)


# bench.py, tests/ and tools/ reach these names as trpo.<name>, from when this module held them: exactly the ones they use and that the imports
# above do not already bind (tests/test_learning_layer_cpu.py keeps the list to that).  Code of this package imports them from their own modules.
from ._lib import Kernels, available  # noqa: E402,F401
from .adam import FlatAdam, adam_step_, fused_adam_step_  # noqa: E402,F401
from .baseline import BaselineKernels, LinearFeatureBaseline, discounted_returns, gram  # noqa: E402,F401
from .comm import CommTimer  # noqa: E402,F401
from .policy import GaussianMLPPolicy, NormalizedActions, _MEAN_ORDER, _two_layer_tanh, add_to_log_std_slot_, hidden_sizes_of  # noqa: E402,F401
