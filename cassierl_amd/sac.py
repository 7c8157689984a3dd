"""Soft Actor-Critic over the batched environment, on DDPG's machinery (cassierl_amd/ddpg.py: replay pool, sampler state, schedule, snapshot).

The reference ships no SAC script; this docstring is the contract [external: the published algorithm (Haarnoja et al., 2018, the version with
twin critics and a learned temperature), from memory; no SAC source is on this machine.  Where a published implementation would disagree with
this paragraph, this paragraph wins]:
  * actor  SquashedGaussianMLPPolicy(hidden_sizes=(32, 32)): out = W3 relu(W2 relu(W1 s + b1) + b2) + b3 with 2 A rows, mean = out[:, :A],
    log_std = clamp(out[:, A:], -20, 2);  a sample is u = mean + exp(log_std) eps, a = tanh(u), eps ~ N(0, 1);
      log pi(a|s) = sum_k (-eps_k^2 / 2 - log_std_k - log(2 pi) / 2) - sum_k 2 (log 2 - u_k - softplus(-2 u_k))
    -- the softplus form of log(1 - tanh^2 u), which float32 and the kernels can follow at |u| of 4 and more.  Initialised as DDPG's networks;
    the deterministic action is tanh(mean);
  * critics  two ddpg.ContinuousMLPQFunction, qf1 and qf2, each with a target copy; there is no target actor;
  * one update on the batch (s, a, r, terminal, s') with the noises eps_s, eps_s2 [batch, A], in this order:
      1. a' = pi(s'; eps_s2);  y = r + (1 - terminal) discount (min(Q1', Q2')(s', a') - alpha log pi(a'|s')), no gradient;
      2. each critic: loss mean((Q_i(s, a) - y)^2), one Adam step at qf_learning_rate, its own m, v, t;
      3. a~ = pi(s; eps_s);  actor loss mean(alpha log pi(a~|s) - min(Q1, Q2)(s, a~)) through the critics AFTER their step (the module family's
         convention), one Adam step at policy_learning_rate;
      4. temperature: log_alpha is a parameter with the gradient -mean(log pi(a~|s) + target_entropy), log pi from step 3 (before the actor
         moved); one Adam step at alpha_learning_rate; target_entropy defaults to -A.  The alpha of steps 1 and 3 is the value from before
         this update.  fixed_alpha=<float> sets alpha to that value and switches step 4 off;
      5. both target critics: target <- (1 - tau) target + tau live.
    Adam is vpg.adam_step_; every gradient, log_alpha's included, is averaged over ranks before its Adam step.

With N environments it is DDPG's module (ddpg.py, "With N environments", rules 1-5 and 7; truncation keeps the true s' with terminal = 0; the same
train_step / train_iteration / updates_per_step, one read-back per epoch).  What differs:
  * exploration is the actor's own sample: every rank draws the job's [n_envs_global][A] normals from the sampler's generator and keeps its
    shard's rows, as DDPG does for its OU noise; there is no OU state;
  * after sample_indices() the update's two noise tensors come from the same generator: torch.randn((2, batch_local, A), generator=idx_gen),
    eps_s first -- the run is reproducible and the snapshot carries everything;
  * defaults: batch_size 256, the three learning rates 3e-4, soft_target_tau 0.005, discount 0.99, scale_reward 1.0, init_alpha 1.0;
    max_path_length, epoch_length, min_pool_size and replay_pool_size are DDPG's, so that the two can be compared line for line.

Hot paths are HIP kernels (csrc/tu_sac.hip, include/cassie_trpo.h): CassieSacPolicyStep and CassieDdpgPoolCommit per vector step, and per update
CassieSacCriticGrad (both critics, one launch), CassieDdpgApply for each critic, CassieSacActorGrad, CassieSacApply (actor and log_alpha): five
launches.  Each has its torch statement in this module (SquashedGaussianMLPPolicy.sample, sac_update_torch_); CPU tensors, other shapes or a
library without the entry points run those.
"""
import copy
import ctypes as ct
import math

import torch
import torch.distributed as dist
from torch import nn
from torch.nn import functional as F

from . import terrain as terrain_lib
from .ddpg import CRITIC, DDPG, ContinuousMLPQFunction, ReplayPool, _NoBaseline, _adam_on, _init_hidden, _init_output, _ptrs, default_pool_size, new_adam, soft_update_
from .trpo import TRPO, NormalizedActions, _world, all_mean_, all_sum_, flat_params, set_flat_params
from .vpg import adam_step_

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0


class SquashedGaussianMLPPolicy(nn.Module):
    """mean, log_std = split(W3 relu(W2 relu(W1 s + b1) + b2) + b3), log_std clamped to [-20, 2]; parameters in the kernels' order W1, b1, W2, b2, W3, b3."""

    def __init__(self, obs_dim, act_dim, hidden_sizes=(32, 32), dtype=torch.float32):
        super().__init__()
        h1, h2 = hidden_sizes
        self.l1, self.l2, self.l3 = nn.Linear(obs_dim, h1), nn.Linear(h1, h2), nn.Linear(h2, 2 * act_dim)
        _init_hidden(self.l1); _init_hidden(self.l2); _init_output(self.l3)
        self.obs_dim, self.act_dim, self.hidden_sizes = obs_dim, act_dim, (h1, h2)
        self.to(dtype)

    def forward(self, obs):
        out = self.l3(torch.relu(self.l2(torch.relu(self.l1(obs)))))
        return out[..., :self.act_dim], out[..., self.act_dim:].clamp(LOG_STD_MIN, LOG_STD_MAX)

    dist_info = forward   # (mean, log_std) of the Gaussian BEFORE the squashing; the deterministic action is tanh(mean)

    @staticmethod
    def log_prob(eps, log_std, u):
        """log pi of a = tanh(u), u = mean + exp(log_std) eps: the Gaussian's density of u minus log |da/du| in its softplus form."""
        return (-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1) - (2.0 * (math.log(2.0) - u - F.softplus(-2.0 * u))).sum(-1)

    def sample(self, obs, eps):
        """(a, log pi(a|s)) for the standard normals eps [n, A] (reparameterised: differentiable in the parameters)."""
        mean, log_std = self(obs)
        u = mean + log_std.exp() * eps
        return torch.tanh(u), self.log_prob(eps, log_std, u)


def new_alpha_adam(log_alpha):
    return dict(t=0, m=torch.zeros_like(log_alpha), v=torch.zeros_like(log_alpha))


def sac_update_torch_(actor, qf1, qf2, target_qf1, target_qf2, log_alpha, adam_pi, adam_q1, adam_q2, adam_alpha, batch, eps_s, eps_s2, discount=0.99,
                      qf_lr=3e-4, policy_lr=3e-4, alpha_lr=3e-4, tau=0.005, target_entropy=None, learn_alpha=True, beta1=0.9, beta2=0.999, eps=1e-8):
    """One SAC update (the module docstring's steps 1-5) on batch = (s, a, r, terminal, s') in the networks' dtype: the specification of
    CassieSacCriticGrad / CassieDdpgApply x 2 / CassieSacActorGrad / CassieSacApply.  log_alpha: tensor [1], stepped in place.  Gradients are
    averaged over ranks before their Adam step.  Returns (qf1_loss, qf2_loss, policy_loss, mean log pi, alpha), alpha from before the update."""
    s, a, r, term, s2 = batch
    if target_entropy is None:
        target_entropy = -float(actor.act_dim)
    alpha = log_alpha.detach().exp().clone()   # steps 1 and 3 see the temperature from before this update
    with torch.no_grad():
        a2, logp2 = actor.sample(s2, eps_s2)
        y = r + (1.0 - term) * discount * (torch.min(target_qf1(s2, a2), target_qf2(s2, a2)) - alpha * logp2)
    losses = []
    for qf, adam in ((qf1, adam_q1), (qf2, adam_q2)):
        loss = ((qf(s, a) - y) ** 2).mean()
        g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(qf.parameters()))])
        _adam_on(qf, all_mean_(g.contiguous(), "gradient_all_reduce"), adam, qf_lr, beta1, beta2, eps)
        losses.append(loss.detach())
    at, logp = actor.sample(s, eps_s)
    policy_loss = (alpha * logp - torch.min(qf1(s, at), qf2(s, at))).mean()   # the critics AFTER their step; only the actor moves
    g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(policy_loss, list(actor.parameters()))])
    _adam_on(actor, all_mean_(g.contiguous(), "gradient_all_reduce"), adam_pi, policy_lr, beta1, beta2, eps)
    avg_logp = logp.detach().mean()
    if learn_alpha:
        g = all_mean_((-(avg_logp + target_entropy)).reshape(1).contiguous(), "gradient_all_reduce")
        adam_alpha["t"] += 1
        adam_step_(log_alpha, g.to(log_alpha.dtype), adam_alpha["m"], adam_alpha["v"], adam_alpha["t"], alpha_lr, beta1, beta2, eps)
    soft_update_(target_qf1, qf1, tau)
    soft_update_(target_qf2, qf2, tau)
    return losses[0], losses[1], policy_loss.detach(), avg_logp, alpha.reshape(())


def kernels_cover(actor, qf1, qf2):
    """The kernels' shapes: float32 CUDA networks, hidden 32 x 32, D 26 or 17, A 6 or 7."""
    if not isinstance(actor, SquashedGaussianMLPPolicy) or not all(isinstance(q, ContinuousMLPQFunction) for q in (qf1, qf2)):
        return False
    if not all(p.is_cuda and p.dtype == torch.float32 for p in (next(m.parameters()) for m in (actor, qf1, qf2))):
        return False
    return actor.hidden_sizes == (32, 32) and actor.obs_dim in (26, 17) and actor.act_dim in (6, 7) \
        and all(q.hidden_sizes == (32, 32) and (q.obs_dim, q.act_dim) == (actor.obs_dim, actor.act_dim) for q in (qf1, qf2))


class SacKernels:
    """The five launches of one update (csrc/tu_sac.hip, tu_ddpg.hip's apply) on the networks' own storage.  ValueError / OSError / AttributeError
    where they do not apply."""

    def __init__(self, actor, qf1, qf2, target_qf1, target_qf2, log_alpha):
        from . import _lib
        if not kernels_cover(actor, qf1, qf2):
            raise ValueError("SacKernels: float32 CUDA networks with 32 x 32 hidden units, obs_dim 26 or 17, act_dim 6 or 7")
        self.L = L = _lib.load()
        self.fn = dict(rows=L.CassieDdpgPartialRows, critic_grad=L.CassieSacCriticGrad, actor_grad=L.CassieSacActorGrad, apply=L.CassieSacApply,
                       critic_apply=L.CassieDdpgApply)
        self.D, self.A = actor.obs_dim, actor.act_dim
        self.np_pi, self.np_q = L.CassieSacParamCount(self.D, self.A), L.CassieDdpgParamCount(self.D, self.A, CRITIC)
        if self.np_pi == 0 or self.np_q == 0:
            raise ValueError("SacKernels: unsupported shape %d -> %d" % (self.D, self.A))
        for net in (actor, qf1, qf2, target_qf1, target_qf2):
            if not all(p.is_contiguous() for p in net.parameters()):
                raise ValueError("SacKernels: contiguous parameters")
        if not (log_alpha.is_cuda and log_alpha.dtype == torch.float32 and log_alpha.numel() == 1):
            raise ValueError("SacKernels: log_alpha must be a float32 CUDA tensor of one element")
        self.actor, self.qf, self.target_qf, self.log_alpha = actor, (qf1, qf2), (target_qf1, target_qf2), log_alpha
        self.dev = next(actor.parameters()).device
        self._partial = {}

    def _stream(self):
        return ct.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _rows(self, which, batch):
        key = (which, batch)
        if key not in self._partial:
            rows = self.fn["rows"](batch)
            shape = (2, rows, self.np_q + 2) if which == "critic" else (rows, self.np_pi + 2)
            self._partial[key] = torch.empty(shape, dtype=torch.float32, device=self.dev)
        return self._partial[key]

    def _check_noise(self, noise, idx):
        if noise.shape != (idx.numel(), self.A) or noise.dtype != torch.float32 or not noise.is_contiguous() or noise.device != self.dev:
            raise ValueError("SacKernels: the noise must be a contiguous float32 tensor [batch, act_dim] on the networks' device")

    def critic_grad(self, pool, idx, eps_s2, discount):
        """partial [2][rows][NPq + 2] of the batch idx: for each critic the gradient of SUM (Q - y)^2, the sum itself, SUM Q."""
        P = lambda t: ct.c_void_p(t.data_ptr())
        self._check_noise(eps_s2, idx)
        out = self._rows("critic", idx.numel())
        rc = self.fn["critic_grad"](P(pool.obs), P(pool.act), P(pool.rew), P(pool.term), P(pool.nobs), ct.c_longlong(pool.capacity), P(idx), idx.numel(), self.D, self.A,
                                    _ptrs(self.actor), _ptrs(self.target_qf[0]), _ptrs(self.target_qf[1]), _ptrs(self.qf[0]), _ptrs(self.qf[1]), P(eps_s2),
                                    P(self.log_alpha), ct.c_float(discount), P(out), self._stream())
        if rc != 0:
            raise RuntimeError("CassieSacCriticGrad failed (%d)" % rc)
        return out

    def actor_grad(self, pool, idx, eps_s):
        """partial [rows][NPpi + 2]: gradient of SUM (alpha log pi(a~|s) - min Q(s, a~)) with respect to the actor, SUM log pi, SUM min Q."""
        P = lambda t: ct.c_void_p(t.data_ptr())
        self._check_noise(eps_s, idx)
        out = self._rows("actor", idx.numel())
        rc = self.fn["actor_grad"](P(pool.obs), ct.c_longlong(pool.capacity), P(idx), idx.numel(), self.D, self.A, _ptrs(self.actor), _ptrs(self.qf[0]),
                                   _ptrs(self.qf[1]), P(eps_s), P(self.log_alpha), P(out), self._stream())
        if rc != 0:
            raise RuntimeError("CassieSacActorGrad failed (%d)" % rc)
        return out

    def critic_apply(self, k, partial, scale, adam, lr, beta1, beta2, eps, tau, stats=None):
        """CassieDdpgApply on critic k: rows added in order, Adam, soft update of its target.  stats [2] float64: += (sum (Q - y)^2, sum Q)."""
        adam["t"] += 1
        rc = self.fn["critic_apply"](partial.shape[0], self.D, self.A, CRITIC, ct.c_void_p(partial.data_ptr()), ct.c_float(scale), _ptrs(self.qf[k]),
                                     _ptrs(self.target_qf[k]), ct.c_void_p(adam["m"].data_ptr()), ct.c_void_p(adam["v"].data_ptr()), int(adam["t"]), ct.c_float(lr),
                                     ct.c_float(beta1), ct.c_float(beta2), ct.c_float(eps), ct.c_float(tau), None if stats is None else ct.c_void_p(stats.data_ptr()),
                                     self._stream())
        if rc != 0:
            raise RuntimeError("CassieDdpgApply failed (%d)" % rc)

    def actor_apply(self, partial, scale, adam, lr, beta1, beta2, eps, adam_alpha, alpha_lr, target_entropy, stats=None):
        """Rows added in order, Adam on the actor, log_alpha's Adam step (adam_alpha None: fixed temperature): one launch.
        stats [3] float64: += (sum log pi, sum min Q, summed actor loss)."""
        adam["t"] += 1
        if adam_alpha is not None:
            adam_alpha["t"] += 1
        P = lambda t: ct.c_void_p(t.data_ptr())
        rc = self.fn["apply"](partial.shape[0], self.D, self.A, P(partial), ct.c_float(scale), _ptrs(self.actor), P(adam["m"]), P(adam["v"]), int(adam["t"]),
                              ct.c_float(lr), ct.c_float(beta1), ct.c_float(beta2), ct.c_float(eps), P(self.log_alpha),
                              None if adam_alpha is None else P(adam_alpha["m"]), None if adam_alpha is None else P(adam_alpha["v"]),
                              0 if adam_alpha is None else int(adam_alpha["t"]), ct.c_float(alpha_lr), ct.c_float(target_entropy),
                              None if stats is None else P(stats), self._stream())
        if rc != 0:
            raise RuntimeError("CassieSacApply failed (%d)" % rc)

    def update(self, pool, idx, eps_s, eps_s2, discount, qf_lr, policy_lr, alpha_lr, tau, target_entropy, adam_pi, adam_q1, adam_q2, adam_alpha, beta1=0.9,
               beta2=0.999, eps=1e-8, stats=None):
        """sac_update_torch_ on the rows idx of the pool, five launches (world == 1); with several ranks the host adds the rows, averages them over
        ranks and applies one row.  adam_alpha None: fixed temperature.  stats [7] float64: += (sum e1^2, sum Q1, sum e2^2, sum Q2, sum log pi,
        sum min Q, summed actor loss)."""
        scale = 1.0 / idx.numel()
        many = _world() > 1
        part = self.critic_grad(pool, idx, eps_s2, discount)
        if many:
            part = all_mean_(part.sum(1, keepdim=True).contiguous(), "gradient_all_reduce")
        for k, adam in enumerate((adam_q1, adam_q2)):
            self.critic_apply(k, part[k], scale, adam, qf_lr, beta1, beta2, eps, tau, None if stats is None else stats[2 * k:])
        part = self.actor_grad(pool, idx, eps_s)   # the actor sees the critics after their step
        if many:
            part = all_mean_(part.sum(0, keepdim=True).contiguous(), "gradient_all_reduce")
        self.actor_apply(part, scale, adam_pi, policy_lr, beta1, beta2, eps, adam_alpha, alpha_lr, target_entropy, None if stats is None else stats[4:])


class SAC(DDPG):
    """Soft Actor-Critic on DDPG's sampler state, pool, schedule and snapshot rules.  Switches (attributes, default True) that tests set to force the
    torch statements: fused_policy_step (CassieSacPolicyStep + CassieDdpgPoolCommit), fused_update (the five update launches), fused_sampler_step
    (TRPO's).  last_update_kind says which update ran: "sac_kernels" or "torch"."""

    _REW = 7   # _stats: sum e1^2, sum Q1, sum e2^2, sum Q2, sum log pi, sum min Q, summed actor loss, summed mean reward

    def __init__(self, env_step, env_reset, policy, qf1, qf2, n_envs, obs_dim, act_map, batch_size=256, max_path_length=100, epoch_length=1000,
                 min_pool_size=10000, replay_pool_size=1000000, discount=0.99, scale_reward=1.0, qf_learning_rate=3e-4, policy_learning_rate=3e-4,
                 alpha_learning_rate=3e-4, soft_target_tau=0.005, updates_per_step=1, init_alpha=1.0, fixed_alpha=None, target_entropy=None, beta1=0.9,
                 beta2=0.999, epsilon=1e-8, seed=1, env_reset_masked=None, env_id0=None, snapshot_pool=True):
        TRPO.__init__(self, env_step, env_reset, policy, _NoBaseline(), n_envs, obs_dim, act_map, batch_size=batch_size, max_path_length=max_path_length,
                      discount=discount, seed=seed, env_reset_masked=env_reset_masked, env_id0=env_id0)
        self.qf1, self.qf2 = qf1, qf2
        self.target_qf1, self.target_qf2 = copy.deepcopy(qf1), copy.deepcopy(qf2)
        for p in list(self.target_qf1.parameters()) + list(self.target_qf2.parameters()):
            p.requires_grad_(False)
        dev, dt = self._init_off_policy("SAC", policy.act_dim, batch_size, epoch_length, min_pool_size, replay_pool_size, scale_reward, qf_learning_rate,
                                        policy_learning_rate, soft_target_tau, updates_per_step, beta1, beta2, epsilon, seed, snapshot_pool)
        self.alpha_learning_rate = alpha_learning_rate
        self.fixed_alpha = None if fixed_alpha is None else float(fixed_alpha)
        self.target_entropy = -float(self.act_dim) if target_entropy is None else float(target_entropy)
        self.log_alpha = torch.full((1,), math.log(init_alpha if fixed_alpha is None else fixed_alpha), dtype=dt, device=dev)
        self.adam_pi, self.adam_q1, self.adam_q2, self.adam_alpha = new_adam(policy), new_adam(qf1), new_adam(qf2), new_alpha_adam(self.log_alpha)

    @property
    def alpha(self):
        return float(self.log_alpha.exp())

    # ---- kernels
    def _update_kernels(self):
        if not getattr(self, "fused_update", True) or not kernels_cover(self.policy, self.qf1, self.qf2):
            return None
        if self._kernels is None:
            try:
                self._kernels = SacKernels(self.policy, self.qf1, self.qf2, self.target_qf1, self.target_qf2, self.log_alpha)
            except (ValueError, OSError, AttributeError):
                self._kernels = False
        return self._kernels or None

    def _fused_step(self, dev):
        """(policy step, pool commit) as one launch each, or None: DDPG's conditions."""
        if not getattr(self, "fused_policy_step", True) or dev.type != "cuda" or not kernels_cover(self.policy, self.qf1, self.qf2) or self.obs_dim != 26 \
                or self.policy.obs_dim != 26 or not isinstance(self.act_map, NormalizedActions):
            return None
        low, high, n, D, A = self.act_map.low, self.act_map.high, self.n_envs, self.obs_dim, self.act_dim
        if not all(t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == A for t in (low, high)):
            return None
        try:
            from . import _lib
            L = _lib.load()
            step_fn, commit_fn = L.CassieSacPolicyStep, L.CassieDdpgPoolCommit
        except (OSError, AttributeError):
            return None
        if not hasattr(self, "_env_actions") or self._env_actions.shape != (n, A):
            self._env_actions = torch.empty((n, A), dtype=torch.float64, device=dev)
        P = lambda t: ct.c_void_p(t.data_ptr())
        pool = self.pool
        stream = lambda: ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def step(obs, noise, top):
            if obs.dtype != torch.float64 or not obs.is_contiguous():
                raise TypeError("CassieSacPolicyStep: observations must be a contiguous float64 tensor (got %s)" % obs.dtype)
            assert noise.is_contiguous() and noise.dtype == torch.float32 and noise.shape == (n, A)
            assert 0 <= top and top + n <= pool.capacity
            rc = step_fn(P(obs), n, D, A, _ptrs(self.policy), P(noise), P(low), P(high), P(pool.obs[top]), P(pool.act[top]), P(self._env_actions), stream())
            if rc != 0:
                raise RuntimeError("CassieSacPolicyStep failed (%d)" % rc)
        return step, self._pool_commit(commit_fn, stream)

    def _explore(self, o, noise):
        return self.policy.sample(o, noise)[0]

    # ---- one update
    def sample_noise(self):
        """The update's two noise tensors (eps_s, eps_s2), drawn after sample_indices() from the same generator."""
        return torch.randn((2, self.batch_local, self.act_dim), generator=self.idx_gen, device=self.pool.obs.device, dtype=self.pool.obs.dtype)

    def update(self, idx, noise=None):
        """One SAC update on the pool rows idx (this rank's share of the batch) with noise [2, batch_local, A].  DDPG.train_step passes the indices
        alone: the noise is then drawn here, after them, from the same generator."""
        if noise is None:
            noise = self.sample_noise()
        learn = self.fixed_alpha is None
        k = self._update_kernels()
        if k is not None:
            k.update(self.pool, idx.contiguous(), noise[0], noise[1], self.discount, self.qf_learning_rate, self.policy_learning_rate, self.alpha_learning_rate,
                     self.tau, self.target_entropy, self.adam_pi, self.adam_q1, self.adam_q2, self.adam_alpha if learn else None, self.beta1, self.beta2,
                     self.epsilon, self._stats)
            self.last_update_kind = "sac_kernels"
        else:
            s, a, r, term, s2 = batch = self.pool.sample(idx)
            with torch.no_grad():
                q = torch.stack([self.qf1(s, a).mean(), self.qf2(s, a).mean()]).double()   # before the step, as the kernels record it
            with torch.enable_grad():
                l1, l2, ploss, logp, alpha = sac_update_torch_(self.policy, self.qf1, self.qf2, self.target_qf1, self.target_qf2, self.log_alpha, self.adam_pi,
                                                               self.adam_q1, self.adam_q2, self.adam_alpha, batch, noise[0], noise[1], self.discount,
                                                               self.qf_learning_rate, self.policy_learning_rate, self.alpha_learning_rate, self.tau,
                                                               self.target_entropy, learn, self.beta1, self.beta2, self.epsilon)
            n = idx.numel()
            l1, l2, ploss, logp, alpha = (x.double() for x in (l1, l2, ploss, logp, alpha))
            self._stats[:7] += torch.stack([l1, q[0], l2, q[1], logp, alpha * logp - ploss, ploss]) * n
            self.last_update_kind = "torch"
        self.n_updates += 1

    def train_iteration(self):
        """epoch_length vector steps; one read-back."""
        timing = getattr(self, "timing", False)
        if timing:
            import time
            torch.cuda.synchronize(); t0 = time.perf_counter()
        self._ep.zero_(); self._stats.zero_()
        updates = 0
        for _ in range(self.epoch_length):
            updates += self.train_step()
        ep = all_sum_(self._ep.clone(), "stats_all_reduce")
        st = all_mean_(self._stats.clone(), "stats_all_reduce")
        v = torch.cat([ep, st, self.log_alpha.double().exp()]).tolist()   # the one read-back
        per = max(1, updates) * self.batch_local
        nan = float("nan")
        avg = lambda x: x / per if updates else nan
        out = dict(itr=self.itr, env_steps=self.epoch_length * self.n_envs * _world(), updates=updates, pool_size=self.pool.size * _world(),
                   avg_reward=v[9] / self.epoch_length, episodes=int(v[0]), avg_return=v[1] / v[0] if v[0] > 0 else nan,
                   qf_loss=avg(0.5 * (v[2] + v[4])), avg_q=avg(0.5 * (v[3] + v[5])), qf1_loss=avg(v[2]), qf2_loss=avg(v[4]), policy_loss=avg(v[8]),
                   avg_log_pi=avg(v[6]), avg_min_q=avg(v[7]), alpha=v[10], update_kind=self.last_update_kind)
        if timing:
            torch.cuda.synchronize()
            out["seconds_epoch"] = time.perf_counter() - t0
        self.itr += 1
        return out

    # ---- snapshot: DDPG's, with SAC's networks and optimiser states
    def _snapshot_fields(self):
        sd = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
        ad = lambda a: dict(t=int(a["t"]), m=a["m"].detach().cpu(), v=a["v"].detach().cpu())
        return dict(algo="sac", hidden_sizes=list(self.policy.hidden_sizes), qf1=sd(self.qf1), qf2=sd(self.qf2), target_qf1=sd(self.target_qf1),
                    target_qf2=sd(self.target_qf2), log_alpha=self.log_alpha.detach().cpu(), adam_pi=ad(self.adam_pi), adam_q1=ad(self.adam_q1),
                    adam_q2=ad(self.adam_q2), adam_alpha=ad(self.adam_alpha), idx_gen_state=self.idx_gen.get_state(), n_updates=int(self.n_updates),
                    pool=self.pool.state() if self.snapshot_pool else None)

    def _load_fields(self, ck):
        algo = ck.get("algo", "trpo")
        if algo != "sac":
            raise ValueError("SAC.load: the snapshot was written by %s, this run is sac" % algo)
        for name in ("qf1", "qf2", "target_qf1", "target_qf2"):
            getattr(self, name).load_state_dict(ck[name])
        self.log_alpha.copy_(ck["log_alpha"])   # in place: the kernels read it through its pointer
        for mine, theirs in ((self.adam_pi, ck["adam_pi"]), (self.adam_q1, ck["adam_q1"]), (self.adam_q2, ck["adam_q2"]), (self.adam_alpha, ck["adam_alpha"])):
            mine["t"] = int(theirs["t"])
            mine["m"].copy_(theirs["m"]); mine["v"].copy_(theirs["v"])
        self.n_updates = int(ck.get("n_updates", 0))
        self._pending = ck

    def load(self, path, restore_sampler=True):
        """DDPG.load without an OU state: the index / noise generator and the pool come back only where the sampler did."""
        extra, restored = TRPO.load(self, path, restore_sampler)
        ck, self._pending = self._pending, None
        self.pool_restored = False
        if restored:
            self.idx_gen.set_state(ck["idx_gen_state"])
            if ck.get("pool") is not None:
                self.pool.load_state(ck["pool"])
                self.pool_restored = True
            else:
                self.pool.top = self.pool.size = 0
                print("SAC.load: the snapshot carries no replay pool; this run restarts with an empty one", flush=True)
        return extra, restored


def broadcast_initial_networks(algo):
    """Rank 0's initial actor, critics and log_alpha are authoritative; the targets are the critics' copies (a collective: every rank must call it)."""
    if dist.is_initialized() and dist.get_world_size() > 1:
        for net, tgt in ((algo.policy, None), (algo.qf1, algo.target_qf1), (algo.qf2, algo.target_qf2)):
            theta = flat_params(net)
            dist.broadcast(theta, 0)
            set_flat_params(net, theta)
            if tgt is not None:
                set_flat_params(tgt, theta)
        dist.broadcast(algo.log_alpha, 0)


def make_cassie_sac(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, terrain=None, sync_policy=True, replay_pool_size=None, **kw):
    """SAC on the batched MI355X environment; the counterpart of ddpg.make_cassie_ddpg (same env, terrain and sync_policy rules).
    replay_pool_size: rows of this rank's pool (default: 1 000 000 rounded up to a multiple of n_envs; a row is 4 (2 D + A + 2) bytes)."""
    from .vec_env import CassieVecEnv
    env = CassieVecEnv(n_envs, kind=kind, control_mode=control_mode, n_substeps=10, auto_reset=True, device=device, trajectory=trajectory)
    env.use_torch_stream()
    dev = "cuda:%d" % device
    bufs = env.alloc()
    torch.manual_seed(seed)
    obs_w = env.observation_space.shape[0]
    policy = SquashedGaussianMLPPolicy(obs_w, env.adim).to(dev)
    qf1, qf2 = ContinuousMLPQFunction(obs_w, env.adim).to(dev), ContinuousMLPQFunction(obs_w, env.adim).to(dev)
    act_map = NormalizedActions(env.action_space.low, env.action_space.high, dev)
    algo = SAC(lambda a: env.step(a, bufs), lambda: env.reset(bufs), policy, qf1, qf2, n_envs, obs_w, act_map, seed=seed,
               replay_pool_size=default_pool_size(n_envs) if replay_pool_size is None else replay_pool_size,
               env_reset_masked=lambda m: env.reset(bufs, mask=m), **kw)
    algo.env = env
    algo.terrain_spec = terrain
    if terrain is not None:
        env.set_terrain_library(terrain_lib.library_of_spec(terrain), terrain_lib.DEFAULT_SIZE[:2])
        env.set_terrain_ids(terrain_lib.assign_terrains(terrain["seed"], algo.env_ids, len(terrain["files"])).to(dev))
    if sync_policy:
        broadcast_initial_networks(algo)
    return algo
