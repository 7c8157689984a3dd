"""Soft Actor-Critic over the batched environment, on the off-policy base (cassierl_amd/offpolicy.py: replay pool, sampler state, schedule, snapshot).

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
    Adam is adam.adam_step_; every gradient, log_alpha's included, is averaged over ranks before its Adam step.

With N environments it is the off-policy base (offpolicy.py, "With N environments", rules 1-5 and 7; truncation keeps the true s' with terminal = 0;
the same train_step / train_iteration / updates_per_step, one read-back per epoch).  What differs from DDPG:
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

On Cassie3d (make_cassie_sac(n, env="cassie3d", control_mode="PD" | "Torque", kp=.., kd=..): 45 observations, 10 actions, the standing reset) the
same 32 x 32 networks run on the same kernels (csrc/sac_kernels.h, instantiated at <45, 10> by csrc/tu_sac3d.hip) -- CassieSac3dPolicyStep,
CassieSac3dCriticGrad, CassieSac3dCriticApply for each critic, CassieSac3dActorGrad, CassieSac3dActorApply, still five launches per update -- and
everything above holds unchanged: target_entropy defaults to -10, and a pool row is 4 (2 D + A + 2) = 408 bytes, so the default pool of
1 000 000 rows is 408 MB per rank.
"""
import ctypes as ct
import math

import torch
import torch.distributed as dist
from torch import nn
from torch.nn import functional as F

from .adam import adam_step_
from .comm import all_mean_
from .ddpg import ACTOR, CRITIC, ContinuousMLPQFunction, _init_hidden, _init_output
from .offpolicy import OffPolicy, PoolKernels, _F, _P, _adam_on, _ptrs, broadcast_initial_networks, make_cassie_offpolicy, new_adam, soft_update_

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


SHAPE3D = (45, 10)   # Cassie3d: the entry points of csrc/tu_sac3d.hip


def kernels_cover(actor, qf1, qf2):
    """The kernels' shapes: float32 CUDA networks, hidden 32 x 32, D 26 or 17 with A 6 or 7, or Cassie3d's (45, 10)."""
    if not isinstance(actor, SquashedGaussianMLPPolicy) or not all(isinstance(q, ContinuousMLPQFunction) for q in (qf1, qf2)):
        return False
    if not all(p.is_cuda and p.dtype == torch.float32 for p in (next(m.parameters()) for m in (actor, qf1, qf2))):
        return False
    return actor.hidden_sizes == (32, 32) and ((actor.obs_dim in (26, 17) and actor.act_dim in (6, 7)) or (actor.obs_dim, actor.act_dim) == SHAPE3D) \
        and all(q.hidden_sizes == (32, 32) and (q.obs_dim, q.act_dim) == (actor.obs_dim, actor.act_dim) for q in (qf1, qf2))


class SacKernels(PoolKernels):
    """The five launches of one update (csrc/tu_sac.hip, tu_ddpg.hip's apply; at 45 x 10 csrc/tu_sac3d.hip, ENTRY3D) on the networks' own storage.
    ValueError / OSError / AttributeError where they do not apply."""

    ENTRY = dict(PartialRows="CassieDdpgPartialRows", ParamCount="CassieDdpgParamCount", SacParamCount="CassieSacParamCount", SacCriticGrad="CassieSacCriticGrad",
                 SacActorGrad="CassieSacActorGrad", SacApply="CassieSacApply", Apply="CassieDdpgApply")
    ENTRY3D = dict(PartialRows="CassieDdpgPartialRows", ParamCount="CassieSac3dParamCount", SacCriticGrad="CassieSac3dCriticGrad",
                   SacActorGrad="CassieSac3dActorGrad", SacApply="CassieSac3dActorApply", Apply="CassieSac3dCriticApply")

    def __init__(self, actor, qf1, qf2, target_qf1, target_qf2, log_alpha):
        if not kernels_cover(actor, qf1, qf2):
            raise ValueError("SacKernels: float32 CUDA networks with 32 x 32 hidden units, obs_dim 26 or 17 and act_dim 6 or 7, or 45 x 10")
        self.D, self.A = actor.obs_dim, actor.act_dim
        self.is3d = (self.D, self.A) == SHAPE3D
        if self.is3d:
            self.ENTRY = self.ENTRY3D   # the entry table of this shape
        super().__init__((actor, qf1, qf2, target_qf1, target_qf2))
        self.np_pi = self.fn["ParamCount"](self.D, self.A, ACTOR) if self.is3d else self.fn["SacParamCount"](self.D, self.A)
        self.np_q = self.fn["ParamCount"](self.D, self.A, CRITIC)
        self._which = () if self.is3d else (CRITIC,)   # CassieDdpgApply serves both of DDPG's networks; CassieSac3dCriticApply is the critic's
        if self.np_pi == 0 or self.np_q == 0:
            raise ValueError("SacKernels: unsupported shape %d -> %d" % (self.D, self.A))
        if not (log_alpha.is_cuda and log_alpha.dtype == torch.float32 and log_alpha.numel() == 1):
            raise ValueError("SacKernels: log_alpha must be a float32 CUDA tensor of one element")
        self.actor, self.qf, self.target_qf, self.log_alpha = actor, (qf1, qf2), (target_qf1, target_qf2), log_alpha

    def critic_grad(self, pool, idx, eps_s2, discount):
        """partial [2][rows][NPq + 2] of the batch idx: for each critic the gradient of SUM (Q - y)^2, the sum itself, SUM Q."""
        self._check_noise(eps_s2, idx)
        out = self._rows("critic", idx.numel(), 2, -1, self.np_q + 2)
        self._call("SacCriticGrad", _P(pool.obs), _P(pool.act), _P(pool.rew), _P(pool.term), _P(pool.nobs), ct.c_longlong(pool.capacity), _P(idx), idx.numel(), self.D,
                   self.A, _ptrs(self.actor), _ptrs(self.target_qf[0]), _ptrs(self.target_qf[1]), _ptrs(self.qf[0]), _ptrs(self.qf[1]), _P(eps_s2),
                   _P(self.log_alpha), ct.c_float(discount), _P(out), self._stream())
        return out

    def actor_grad(self, pool, idx, eps_s):
        """partial [rows][NPpi + 2]: gradient of SUM (alpha log pi(a~|s) - min Q(s, a~)) with respect to the actor, SUM log pi, SUM min Q."""
        self._check_noise(eps_s, idx)
        out = self._rows("actor", idx.numel(), -1, self.np_pi + 2)
        self._call("SacActorGrad", _P(pool.obs), ct.c_longlong(pool.capacity), _P(idx), idx.numel(), self.D, self.A, _ptrs(self.actor), _ptrs(self.qf[0]),
                   _ptrs(self.qf[1]), _P(eps_s), _P(self.log_alpha), _P(out), self._stream())
        return out

    def critic_apply(self, k, partial, scale, adam, lr, beta1, beta2, eps, tau, stats=None):
        """CassieDdpgApply (45 x 10: CassieSac3dCriticApply) on critic k: rows added in order, Adam, soft update of its target.  stats [2] float64: += (sum (Q - y)^2, sum Q)."""
        adam["t"] += 1
        self._call("Apply", partial.shape[0], self.D, self.A, *self._which, _P(partial), ct.c_float(scale), _ptrs(self.qf[k]), _ptrs(self.target_qf[k]), _P(adam["m"]),
                   _P(adam["v"]), int(adam["t"]), *_F(lr, beta1, beta2, eps, tau), None if stats is None else _P(stats), self._stream())

    def actor_apply(self, partial, scale, adam, lr, beta1, beta2, eps, adam_alpha, alpha_lr, target_entropy, stats=None):
        """Rows added in order, Adam on the actor, log_alpha's Adam step (adam_alpha None: fixed temperature): one launch.
        stats [3] float64: += (sum log pi, sum min Q, summed actor loss)."""
        adam["t"] += 1
        if adam_alpha is not None:
            adam_alpha["t"] += 1
        alpha = (None, None, 0) if adam_alpha is None else (_P(adam_alpha["m"]), _P(adam_alpha["v"]), int(adam_alpha["t"]))
        self._call("SacApply", partial.shape[0], self.D, self.A, _P(partial), ct.c_float(scale), _ptrs(self.actor), _P(adam["m"]), _P(adam["v"]), int(adam["t"]),
                   *_F(lr, beta1, beta2, eps), _P(self.log_alpha), *alpha, *_F(alpha_lr, target_entropy), None if stats is None else _P(stats), self._stream())

    def update(self, pool, idx, eps_s, eps_s2, discount, qf_lr, policy_lr, alpha_lr, tau, target_entropy, adam_pi, adam_q1, adam_q2, adam_alpha, beta1=0.9,
               beta2=0.999, eps=1e-8, stats=None):
        """sac_update_torch_ on the rows idx of the pool, five launches (world == 1); with several ranks the host adds the rows, averages them over
        ranks and applies one row.  adam_alpha None: fixed temperature.  stats [7] float64: += (sum e1^2, sum Q1, sum e2^2, sum Q2, sum log pi,
        sum min Q, summed actor loss)."""
        scale = 1.0 / idx.numel()
        part = self._over_ranks(self.critic_grad(pool, idx, eps_s2, discount), 1)
        for k, adam in enumerate((adam_q1, adam_q2)):
            self.critic_apply(k, part[k], scale, adam, qf_lr, beta1, beta2, eps, tau, None if stats is None else stats[2 * k:])
        part = self._over_ranks(self.actor_grad(pool, idx, eps_s))   # the actor sees the critics after their step
        self.actor_apply(part, scale, adam_pi, policy_lr, beta1, beta2, eps, adam_alpha, alpha_lr, target_entropy, None if stats is None else stats[4:])


class SAC(OffPolicy):
    """Soft Actor-Critic on OffPolicy's sampler state, pool, schedule and snapshot.  Kernels: CassieSacPolicyStep + CassieDdpgPoolCommit per vector step,
    the five update launches; last_update_kind is "sac_kernels" or "torch"."""

    ALGO, STEP_ENTRY = "sac", {26: "CassieSacPolicyStep", 45: "CassieSac3dPolicyStep"}
    CASSIE3D = True
    NETS = (("policy", None), ("qf1", "target_qf1"), ("qf2", "target_qf2"))   # there is no target actor
    ADAMS = ("adam_pi", "adam_q1", "adam_q2", "adam_alpha")
    _REW = 7   # _stats: sum e1^2, sum Q1, sum e2^2, sum Q2, sum log pi, sum min Q, summed actor loss, summed mean reward

    def __init__(self, env_step, env_reset, policy, qf1, qf2, n_envs, obs_dim, act_map, batch_size=256, max_path_length=100, epoch_length=1000,
                 min_pool_size=10000, replay_pool_size=1000000, discount=0.99, scale_reward=1.0, qf_learning_rate=3e-4, policy_learning_rate=3e-4,
                 alpha_learning_rate=3e-4, soft_target_tau=0.005, updates_per_step=1, init_alpha=1.0, fixed_alpha=None, target_entropy=None, beta1=0.9,
                 beta2=0.999, epsilon=1e-8, seed=1, env_reset_masked=None, env_id0=None, snapshot_pool=True):
        self.qf1, self.qf2 = qf1, qf2
        super().__init__(env_step, env_reset, policy, n_envs, obs_dim, act_map, batch_size, max_path_length, epoch_length, min_pool_size, replay_pool_size, discount,
                         scale_reward, qf_learning_rate, policy_learning_rate, soft_target_tau, updates_per_step, beta1, beta2, epsilon, seed, env_reset_masked,
                         env_id0, snapshot_pool)
        self.alpha_learning_rate = alpha_learning_rate
        self.fixed_alpha = None if fixed_alpha is None else float(fixed_alpha)
        self.target_entropy = -float(self.act_dim) if target_entropy is None else float(target_entropy)
        self.log_alpha = torch.full((1,), math.log(init_alpha if fixed_alpha is None else fixed_alpha), dtype=self.pool.obs.dtype, device=self.pool.obs.device)
        self.adam_pi, self.adam_q1, self.adam_q2, self.adam_alpha = new_adam(policy), new_adam(qf1), new_adam(qf2), new_alpha_adam(self.log_alpha)

    @property
    def alpha(self):
        return float(self.log_alpha.exp())

    def _covered(self):
        return kernels_cover(self.policy, self.qf1, self.qf2)

    def _new_kernels(self):
        return SacKernels(self.policy, self.qf1, self.qf2, self.target_qf1, self.target_qf2, self.log_alpha)

    def _policy_step_call(self, fn, head, noise, tail):
        return fn(*head, _ptrs(self.policy), noise, *tail)

    def _explore(self, o, noise):
        return self.policy.sample(o, noise)[0]

    # ---- one update
    def sample_noise(self):
        """The update's two noise tensors (eps_s, eps_s2), drawn after sample_indices() from the same generator."""
        return torch.randn((2, self.batch_local, self.act_dim), generator=self.idx_gen, device=self.pool.obs.device, dtype=self.pool.obs.dtype)

    def update(self, idx, noise=None):
        """One SAC update on the pool rows idx (this rank's share of the batch) with noise [2, batch_local, A].  OffPolicy.train_step passes the
        indices alone: the noise is then drawn here, after them, from the same generator."""
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

    def _readback_extra(self):
        return [self.log_alpha.double().exp()]

    def _report(self, v, updates):
        avg = lambda x: self._per_sample(x, updates)
        return dict(qf_loss=avg(0.5 * (v[2] + v[4])), avg_q=avg(0.5 * (v[3] + v[5])), qf1_loss=avg(v[2]), qf2_loss=avg(v[4]), policy_loss=avg(v[8]),
                    avg_log_pi=avg(v[6]), avg_min_q=avg(v[7]), alpha=v[10])

    # ---- snapshot: the base's, with log_alpha; there is no OU state
    def _snapshot_extra(self):
        return dict(log_alpha=self.log_alpha.detach().cpu())

    def _load_extra(self, ck):
        self.log_alpha.copy_(ck["log_alpha"])   # in place: the kernels read it through its pointer

    def _broadcast_extra(self):
        dist.broadcast(self.log_alpha, 0)


def make_cassie_sac(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, terrain=None, sync_policy=True, replay_pool_size=None, **kw):
    """SAC on the batched MI355X environment: offpolicy.make_cassie_offpolicy with SAC's networks.  env="cassie3d" (with control_mode and, through **kw,
    kp / kd) runs it on Cassie3dVecEnv: sampler.make_cassie_algo.  replay_pool_size defaults to 1 000 000 rows per rank: 240 MB on Cassie2d, 408 MB
    on Cassie3d (a row is 4 (2 D + A + 2) bytes)."""
    make_nets = lambda D, A: (SquashedGaussianMLPPolicy(D, A), ContinuousMLPQFunction(D, A), ContinuousMLPQFunction(D, A))
    return make_cassie_offpolicy(SAC, make_nets, n_envs, kind, control_mode, device, trajectory, seed, terrain, sync_policy, replay_pool_size, **kw)
