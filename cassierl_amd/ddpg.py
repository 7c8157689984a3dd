"""DDPG over the batched environment: counterpart of rllab/envs/ddpg_cassie.py:14-51.

  policy     DeterministicMLPPolicy(hidden_sizes=(32, 32))                       ddpg_cassie.py:20-24
  qf         ContinuousMLPQFunction (defaults)                                   ddpg_cassie.py:28
  es         OUStrategy (defaults)                                               ddpg_cassie.py:26
  algorithm  DDPG: batch_size=32, max_path_length=100, epoch_length=1000, min_pool_size=10000, n_epochs=1000, discount=0.99,
             scale_reward=0.01, qf_learning_rate=1e-3, policy_learning_rate=1e-4                                     ddpg_cassie.py:30-45
  env        normalize(Cassie2dEnv())                                            ddpg_cassie.py:18

What rllab's DDPG does with these [external: rllab's published source, from memory; rllab is not on this machine.  Where rllab's real source
would disagree with this paragraph, this paragraph is the contract of this module]:
  * actor  mu(s) = tanh(W3 relu(W2 relu(W1 s + b1) + b2) + b3);  critic  Q(s, a) = W3 relu(W2 [relu(W1 s + b1); a] + b2) + b3 -- the action joins
    at the second hidden layer (action_merge_layer=-2).  Hidden weights HeUniform (+-sqrt(6 / fan_in)), hidden biases zero, output weights
    and biases uniform in +-3e-3;
  * exploration: Ornstein-Uhlenbeck state x per environment and action component, x <- x + theta (mu - x) + sigma n, n ~ N(0, 1), theta 0.15,
    sigma 0.3, mu 0; x = mu when a path starts; the action is clip(mu(s) + x, -1, 1), then normalize()'s affine map to the action box;
  * one environment step: act, step, the path clock advances, a live path that reaches max_path_length ends; the transition
    (s, a, scale_reward r, terminal) goes into the pool; then, if the pool holds min_pool_size transitions, n_updates_per_sample (1) updates
    run, each on batch_size transitions drawn uniformly with replacement;
  * one update: y = r + (1 - terminal) discount Q'(s', mu'(s'));  critic loss mean((Q(s, a) - y)^2), one Adam step at qf_learning_rate;  actor
    loss -mean(Q(s, mu(s))) with the critic AFTER its step, one Adam step at policy_learning_rate;  target <- (1 - tau) target + tau live for
    both networks, tau = 0.001.  Adam is Lasagne's (adam.adam_step_), each network with its own m, v, t.  No weight decay; replay_pool_size
    1 000 000.

With N environments: the rules of every algorithm on the replay pool, offpolicy.py, "With N environments" (rule 6: the OU noise's normals).

Hot paths are HIP kernels (csrc/tu_ddpg.hip, include/cassie_trpo.h): CassieDdpgPolicyStep (one launch per vector step, writes the pool's rows),
CassieDdpgPoolCommit (one launch after Env.step), and per update CassieDdpgCriticGrad, CassieDdpgApply, CassieDdpgActorGrad, CassieDdpgApply.  Each
has a torch statement in this module that is its specification (OUStrategy.evolve + DeterministicMLPPolicy, offpolicy.ReplayPool.write,
ddpg_update_torch_); CPU tensors, other shapes or a library without the entry points run those.
"""
import ctypes as ct
import math

import torch
from torch import nn

from .comm import all_mean_
from .offpolicy import OffPolicy, PoolKernels, ReplayPool, _F, _P, _adam_on, _ptrs, broadcast_initial_networks, default_pool_size, \
    make_cassie_offpolicy, new_adam, soft_update_   # the moved names stay reachable as ddpg.<name> (tools, tests)

ACTOR, CRITIC = 0, 1   # CASSIE_DDPG_ACTOR / CASSIE_DDPG_CRITIC


def _init_hidden(lin):
    b = math.sqrt(6.0 / lin.in_features)   # HeUniform [external]
    nn.init.uniform_(lin.weight, -b, b)
    nn.init.zeros_(lin.bias)


def _init_output(lin):
    nn.init.uniform_(lin.weight, -3e-3, 3e-3)
    nn.init.uniform_(lin.bias, -3e-3, 3e-3)


class DeterministicMLPPolicy(nn.Module):
    """mu(s) = tanh(W3 relu(W2 relu(W1 s + b1) + b2) + b3); parameters in the kernels' order W1, b1, W2, b2, W3, b3."""

    def __init__(self, obs_dim, act_dim, hidden_sizes=(32, 32), dtype=torch.float32):
        super().__init__()
        h1, h2 = hidden_sizes
        self.l1, self.l2, self.l3 = nn.Linear(obs_dim, h1), nn.Linear(h1, h2), nn.Linear(h2, act_dim)
        _init_hidden(self.l1); _init_hidden(self.l2); _init_output(self.l3)
        self.obs_dim, self.act_dim, self.hidden_sizes = obs_dim, act_dim, (h1, h2)
        self.to(dtype)

    def forward(self, obs):
        return torch.tanh(self.l3(torch.relu(self.l2(torch.relu(self.l1(obs))))))


class ContinuousMLPQFunction(nn.Module):
    """Q(s, a) = W3 relu(W2 [relu(W1 s + b1); a] + b2) + b3: the action joins at the second hidden layer."""

    def __init__(self, obs_dim, act_dim, hidden_sizes=(32, 32), dtype=torch.float32):
        super().__init__()
        h1, h2 = hidden_sizes
        self.l1, self.l2, self.l3 = nn.Linear(obs_dim, h1), nn.Linear(h1 + act_dim, h2), nn.Linear(h2, 1)
        _init_hidden(self.l1); _init_hidden(self.l2); _init_output(self.l3)
        self.obs_dim, self.act_dim, self.hidden_sizes = obs_dim, act_dim, (h1, h2)
        self.to(dtype)

    def first_hidden(self, obs):
        return torch.relu(self.l1(obs))

    def forward(self, obs, act):
        h2 = torch.relu(self.l2(torch.cat([self.first_hidden(obs), act], dim=-1)))
        return self.l3(h2).squeeze(-1)


class OUStrategy:
    """rllab's OUStrategy: per environment and action component x <- x + theta (mu - x) + sigma n; x = mu where a path starts."""

    def __init__(self, n_envs, act_dim, device="cpu", dtype=torch.float32, theta=0.15, sigma=0.3, mu=0.0):
        self.theta, self.sigma, self.mu = theta, sigma, mu
        self.state = torch.full((n_envs, act_dim), mu, dtype=dtype, device=device)

    def evolve(self, noise, fresh=None):
        """One step with the standard normals `noise` [n, A]; `fresh` [n] bool: paths that start here (their state is mu first)."""
        x = self.state
        if fresh is not None:
            x = torch.where(fresh.unsqueeze(-1), torch.full_like(x, self.mu), x)
        self.state = x + self.theta * (self.mu - x) + self.sigma * noise.to(x.dtype)
        return self.state

    def get_action(self, mean, noise, fresh=None):
        return (mean + self.evolve(noise, fresh)).clamp(-1.0, 1.0)


def ddpg_update_torch_(actor, critic, target_actor, target_critic, adam_mu, adam_q, batch, discount=0.99, qf_lr=1e-3, policy_lr=1e-4, tau=1e-3,
                       beta1=0.9, beta2=0.999, eps=1e-8):
    """One DDPG update on batch = (s, a, r, terminal, s') in the networks' dtype: the specification of CassieDdpgCriticGrad / CassieDdpgApply /
    CassieDdpgActorGrad / CassieDdpgApply.  Gradients are averaged over ranks before their Adam step.  Returns (qf_loss, policy_surr, mean Q)."""
    s, a, r, term, s2 = batch
    with torch.no_grad():
        y = r + (1.0 - term) * discount * target_critic(s2, target_actor(s2))
    q = critic(s, a)
    qf_loss = ((q - y) ** 2).mean()
    g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(qf_loss, list(critic.parameters()))])
    _adam_on(critic, all_mean_(g.contiguous(), "gradient_all_reduce"), adam_q, qf_lr, beta1, beta2, eps)
    surr = -critic(s, actor(s)).mean()   # the critic AFTER its step; only the actor moves
    g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(surr, list(actor.parameters()))])
    _adam_on(actor, all_mean_(g.contiguous(), "gradient_all_reduce"), adam_mu, policy_lr, beta1, beta2, eps)
    soft_update_(target_critic, critic, tau)
    soft_update_(target_actor, actor, tau)
    return qf_loss.detach(), surr.detach(), q.detach().mean()


def kernels_cover(actor, critic):
    """The update kernels' shapes: float32 CUDA networks, hidden 32 x 32, D 26 or 17, A 6 or 7."""
    if not isinstance(actor, DeterministicMLPPolicy) or not isinstance(critic, ContinuousMLPQFunction):
        return False
    p = next(actor.parameters())
    if not p.is_cuda or p.dtype != torch.float32 or next(critic.parameters()).dtype != torch.float32:
        return False
    return actor.hidden_sizes == (32, 32) and critic.hidden_sizes == (32, 32) and actor.obs_dim in (26, 17) and actor.act_dim in (6, 7) \
        and (critic.obs_dim, critic.act_dim) == (actor.obs_dim, actor.act_dim)


class DdpgKernels(PoolKernels):
    """The four launches of one update (csrc/tu_ddpg.hip) on the networks' own storage.  ValueError / OSError / AttributeError where they do not apply."""

    ENTRY = {k: "CassieDdpg" + k for k in ("ParamCount", "PartialRows", "CriticGrad", "ActorGrad", "Apply")}

    def __init__(self, actor, critic, target_actor, target_critic):
        if not kernels_cover(actor, critic):
            raise ValueError("DdpgKernels: float32 CUDA networks with 32 x 32 hidden units, obs_dim 26 or 17, act_dim 6 or 7")
        super().__init__((actor, critic, target_actor, target_critic))
        self.D, self.A = actor.obs_dim, actor.act_dim
        self.np = {which: self.fn["ParamCount"](self.D, self.A, which) for which in (ACTOR, CRITIC)}
        if 0 in self.np.values():
            raise ValueError("DdpgKernels: unsupported shape %d -> %d" % (self.D, self.A))
        self.nets = dict(actor=actor, critic=critic, target_actor=target_actor, target_critic=target_critic)

    def critic_grad(self, pool, idx, discount):
        """partial [rows][NPq + 2] of the batch idx: gradient of SUM (Q - y)^2, the sum itself, SUM Q."""
        n = self.nets
        out = self._rows(CRITIC, idx.numel(), -1, self.np[CRITIC] + 2)
        self._call("CriticGrad", _P(pool.obs), _P(pool.act), _P(pool.rew), _P(pool.term), _P(pool.nobs), ct.c_longlong(pool.capacity), _P(idx), idx.numel(), self.D,
                   self.A, _ptrs(n["target_actor"]), _ptrs(n["target_critic"]), _ptrs(n["critic"]), ct.c_float(discount), _P(out), self._stream())
        return out

    def actor_grad(self, pool, idx):
        """partial [rows][NPmu + 1]: gradient of -SUM Q(s, mu(s)) with respect to the actor, SUM Q(s, mu(s))."""
        n = self.nets
        out = self._rows(ACTOR, idx.numel(), -1, self.np[ACTOR] + 1)
        self._call("ActorGrad", _P(pool.obs), ct.c_longlong(pool.capacity), _P(idx), idx.numel(), self.D, self.A, _ptrs(n["actor"]), _ptrs(n["critic"]), _P(out),
                   self._stream())
        return out

    def apply(self, which, partial, scale, adam, lr, beta1, beta2, eps, tau, stats=None):
        """Rows added in order, Adam on the live network, soft update of its target: one launch.  stats: float64 device tensor the summed extra
        columns are added to."""
        n = self.nets
        live, targ = (n["actor"], n["target_actor"]) if which == ACTOR else (n["critic"], n["target_critic"])
        adam["t"] += 1
        self._call("Apply", partial.shape[0], self.D, self.A, which, _P(partial), ct.c_float(scale), _ptrs(live), _ptrs(targ), _P(adam["m"]), _P(adam["v"]),
                   int(adam["t"]), *_F(lr, beta1, beta2, eps, tau), None if stats is None else _P(stats), self._stream())

    def update(self, pool, idx, discount, qf_lr, policy_lr, tau, adam_mu, adam_q, beta1=0.9, beta2=0.999, eps=1e-8, stats=None):
        """ddpg_update_torch_ on the rows idx of the pool, four launches (world == 1); with several ranks the host adds the rows, averages them
        over ranks and applies one row.  stats [3] float64: += (sum (Q - y)^2, sum Q(s, a), sum Q(s, mu(s)))."""
        scale = 1.0 / idx.numel()
        for which, adam, lr, off in ((CRITIC, adam_q, qf_lr, 0), (ACTOR, adam_mu, policy_lr, 2)):
            part = self.critic_grad(pool, idx, discount) if which == CRITIC else self.actor_grad(pool, idx)   # the actor sees the critic after its step
            self.apply(which, self._over_ranks(part), scale, adam, lr, beta1, beta2, eps, tau, None if stats is None else stats[off:])


class DDPG(OffPolicy):
    """rllab's DDPG on OffPolicy's sampler state, pool, schedule and snapshot.  Kernels: CassieDdpgPolicyStep + CassieDdpgPoolCommit per vector step,
    the four update launches; last_update_kind is "ddpg_kernels" or "torch"."""

    ALGO, STEP_ENTRY = "ddpg", {26: "CassieDdpgPolicyStep"}
    NETS = (("policy", "target_policy"), ("qf", "target_qf"))
    ADAMS = ("adam_mu", "adam_q")
    _REW = 3   # _stats: sum (Q - y)^2, sum Q(s, a), sum Q(s, mu(s)), summed mean reward

    def __init__(self, env_step, env_reset, policy, qf, n_envs, obs_dim, act_map, batch_size=32, max_path_length=100, epoch_length=1000,
                 min_pool_size=10000, replay_pool_size=1000000, discount=0.99, scale_reward=0.01, qf_learning_rate=1e-3, policy_learning_rate=1e-4,
                 soft_target_tau=1e-3, updates_per_step=1, ou_theta=0.15, ou_sigma=0.3, ou_mu=0.0, beta1=0.9, beta2=0.999, epsilon=1e-8, seed=1,
                 env_reset_masked=None, env_id0=None, snapshot_pool=True):
        self.qf = qf
        super().__init__(env_step, env_reset, policy, n_envs, obs_dim, act_map, batch_size, max_path_length, epoch_length, min_pool_size, replay_pool_size, discount,
                         scale_reward, qf_learning_rate, policy_learning_rate, soft_target_tau, updates_per_step, beta1, beta2, epsilon, seed, env_reset_masked,
                         env_id0, snapshot_pool)
        self.ou = OUStrategy(n_envs, self.act_dim, self.pool.obs.device, self.pool.obs.dtype, ou_theta, ou_sigma, ou_mu)
        self.adam_mu, self.adam_q = new_adam(policy), new_adam(qf)

    def _covered(self):
        return kernels_cover(self.policy, self.qf)

    def _new_kernels(self):
        return DdpgKernels(self.policy, self.qf, self.target_policy, self.target_qf)

    def _policy_step_call(self, fn, head, noise, tail):
        ou = self.ou
        assert ou.state.is_contiguous() and self.path_t.dtype == torch.int64
        return fn(*head, *[ct.c_void_p(p) for p in _ptrs(self.policy)], noise, _P(self.path_t), *_F(ou.theta, ou.sigma, ou.mu), _P(ou.state), *tail)

    def _explore(self, o, noise):
        """The exploring action in [-1, 1] for the float32 observations o and this step's normals (the torch statement of the policy-step kernel)."""
        return self.ou.get_action(self.policy(o), noise, self.path_t == 0)

    def update(self, idx):
        """One DDPG update on the pool rows idx (this rank's share of the batch)."""
        k = self._update_kernels()
        if k is not None:
            k.update(self.pool, idx.contiguous(), self.discount, self.qf_learning_rate, self.policy_learning_rate, self.tau, self.adam_mu, self.adam_q,
                     self.beta1, self.beta2, self.epsilon, self._stats)
            self.last_update_kind = "ddpg_kernels"
        else:
            with torch.enable_grad():
                loss, surr, q = ddpg_update_torch_(self.policy, self.qf, self.target_policy, self.target_qf, self.adam_mu, self.adam_q, self.pool.sample(idx),
                                                   self.discount, self.qf_learning_rate, self.policy_learning_rate, self.tau, self.beta1, self.beta2, self.epsilon)
            n = idx.numel()
            self._stats[:3] += torch.stack([loss.double() * n, q.double() * n, -surr.double() * n])
            self.last_update_kind = "torch"
        self.n_updates += 1

    def _report(self, v, updates):
        avg = lambda x: self._per_sample(x, updates)
        return dict(qf_loss=avg(v[2]), avg_q=avg(v[3]), policy_surr=avg(-v[4]))

    def _snapshot_extra(self):
        return dict(ou_state=self.ou.state.cpu())

    def _load_sampler_extra(self, ck, dev):
        self.ou.state = ck["ou_state"].to(dev)


def make_cassie_ddpg(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, terrain=None, sync_policy=True, replay_pool_size=None, **kw):
    """ddpg_cassie.py:14-51 on the batched MI355X environment: offpolicy.make_cassie_offpolicy with DDPG's networks."""
    make_nets = lambda D, A: (DeterministicMLPPolicy(D, A), ContinuousMLPQFunction(D, A))
    return make_cassie_offpolicy(DDPG, make_nets, n_envs, kind, control_mode, device, trajectory, seed, terrain, sync_policy, replay_pool_size, **kw)
