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
    both networks, tau = 0.001.  Adam is Lasagne's (vpg.adam_step_), each network with its own m, v, t.  No weight decay; replay_pool_size
    1 000 000.

With N environments ("DDPG"):
  1. a pool row is (s [D], a [A], r, terminal, s' [D]), float32, structure of arrays on the device; a is the clipped action in [-1, 1], r is
     already scaled.  rllab's pool finds s' at ring index + 1, which only works for one environment;
  2. one vector step appends exactly N rows at ring positions [top, top + N), environment i at top + i; the capacity is a multiple of N
     (ValueError otherwise), so an append never wraps inside a step; size = min(size + N, capacity); every rank owns the pool of its own
     environments;
  3. a live path cut at max_path_length is stored with terminal = 0 and its true s' (the observation Env.step returned, before the masked
     reset).  rllab drops that transition because its ring cannot hold it; that is not reproduced.  A real done is stored with terminal = 1;
     its s' is whatever the auto-reset returned and is multiplied by zero in the target;
  4. `updates_per_step` (1) updates of `batch_size` (32) rows follow every vector step: with N = 1 this is rllab's loop; at large N one sets
     both (e.g. batch_size = 65536, updates_per_step = 1) -- no scaling rule is invented;
  5. batch indices: torch.randint(0, size, (batch,)) from a generator on the device seeded from (seed, rank).  With world > 1 each rank draws
     batch_size / world indices from its own pool and both gradients are averaged over ranks before their Adam step: parameters, targets and
     Adam state stay identical on all ranks, and the result depends on the number of ranks;
  6. OU noise is drawn as TRPO's exploration noise: every rank draws the [n_envs_global][A] normals of the job and keeps its shard's rows;
  7. float32 arithmetic.  The update kernels cover D 26 or 17, A 6 or 7, hidden 32 x 32; the policy-step kernel the environment's 26-wide rows.

Hot paths are HIP kernels (csrc/tu_ddpg.hip, include/cassie_trpo.h): CassieDdpgPolicyStep (one launch per vector step, writes the pool's rows),
CassieDdpgPoolCommit (one launch after Env.step), and per update CassieDdpgCriticGrad, CassieDdpgApply, CassieDdpgActorGrad, CassieDdpgApply.  Each
has a torch statement in this module that is its specification (OUStrategy.evolve + DeterministicMLPPolicy, ReplayPool.write,
ddpg_update_torch_); CPU tensors, other shapes or a library without the entry points run those.
"""
import ctypes as ct
import math

import torch
import torch.distributed as dist
from torch import nn

from . import terrain as terrain_lib
from .trpo import TRPO, NormalizedActions, _world, all_mean_, all_sum_, flat_params, set_flat_params
from .vpg import adam_step_

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


class ReplayPool:
    """Device ring of transitions (s, a, r, terminal, s'), structure of arrays; one vector step appends n_envs rows at [top, top + n_envs)."""

    def __init__(self, capacity, n_envs, obs_dim, act_dim, device="cpu", dtype=torch.float32):
        if capacity <= 0 or capacity % n_envs != 0:
            raise ValueError("ReplayPool: the capacity (%d) must be a positive multiple of the number of environments (%d)" % (capacity, n_envs))
        self.capacity, self.n_envs, self.obs_dim, self.act_dim = capacity, n_envs, obs_dim, act_dim
        z = lambda *shape: torch.zeros(shape, dtype=dtype, device=device)
        self.obs, self.act, self.rew, self.term, self.nobs = z(capacity, obs_dim), z(capacity, act_dim), z(capacity), z(capacity), z(capacity, obs_dim)
        self.top, self.size = 0, 0

    BYTES_PER_ROW = staticmethod(lambda obs_dim, act_dim: 4 * (2 * obs_dim + act_dim + 2))

    def write(self, top, obs32, act, rew, terminal, next_obs32):
        n = self.n_envs
        self.obs[top:top + n], self.act[top:top + n], self.nobs[top:top + n] = obs32, act, next_obs32
        self.rew[top:top + n], self.term[top:top + n] = rew, terminal

    def advance(self):
        """The rows [top, top + n_envs) have been written."""
        self.top = (self.top + self.n_envs) % self.capacity
        self.size = min(self.size + self.n_envs, self.capacity)

    def append(self, obs32, act, rew, terminal, next_obs32):
        self.write(self.top, obs32, act, rew.to(self.rew.dtype), terminal.to(self.term.dtype), next_obs32)
        self.advance()

    def sample(self, idx):
        return self.obs[idx], self.act[idx], self.rew[idx], self.term[idx], self.nobs[idx]

    def state(self):
        s = self.size
        return dict(size=int(self.size), top=int(self.top), capacity=int(self.capacity), obs=self.obs[:s].cpu(), act=self.act[:s].cpu(), rew=self.rew[:s].cpu(),
                    term=self.term[:s].cpu(), nobs=self.nobs[:s].cpu())

    def load_state(self, st):
        if st["capacity"] != self.capacity:
            raise ValueError("ReplayPool: the snapshot's pool holds %d rows, this run's %d" % (st["capacity"], self.capacity))
        s = st["size"]
        for k in ("obs", "act", "rew", "term", "nobs"):
            getattr(self, k)[:s] = st[k].to(self.obs.device)
        self.size, self.top = s, st["top"]


def new_adam(net):
    theta = flat_params(net)
    return dict(t=0, m=torch.zeros_like(theta), v=torch.zeros_like(theta))


def _adam_on(net, g, adam, lr, beta1, beta2, eps):
    theta = flat_params(net).contiguous()
    adam["t"] += 1
    adam_step_(theta, g.to(theta.dtype), adam["m"], adam["v"], adam["t"], lr, beta1, beta2, eps)
    set_flat_params(net, theta)


def soft_update_(target, live, tau):
    with torch.no_grad():
        for pt, p in zip(target.parameters(), live.parameters()):
            pt.mul_(1.0 - tau).add_(p, alpha=tau)


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


def _ptrs(net):
    """Host array of the six device pointers {W1, b1, W2, b2, W3, b3} of a network."""
    ps = [net.l1.weight, net.l1.bias, net.l2.weight, net.l2.bias, net.l3.weight, net.l3.bias]
    return (ct.c_void_p * 6)(*[p.data_ptr() for p in ps])


def kernels_cover(actor, critic):
    """The update kernels' shapes: float32 CUDA networks, hidden 32 x 32, D 26 or 17, A 6 or 7."""
    if not isinstance(actor, DeterministicMLPPolicy) or not isinstance(critic, ContinuousMLPQFunction):
        return False
    p = next(actor.parameters())
    if not p.is_cuda or p.dtype != torch.float32 or next(critic.parameters()).dtype != torch.float32:
        return False
    return actor.hidden_sizes == (32, 32) and critic.hidden_sizes == (32, 32) and actor.obs_dim in (26, 17) and actor.act_dim in (6, 7) \
        and (critic.obs_dim, critic.act_dim) == (actor.obs_dim, actor.act_dim)


class DdpgKernels:
    """The four launches of one update (csrc/tu_ddpg.hip) on the networks' own storage.  ValueError / OSError / AttributeError where they do not apply."""

    def __init__(self, actor, critic, target_actor, target_critic):
        from . import _lib
        if not kernels_cover(actor, critic):
            raise ValueError("DdpgKernels: float32 CUDA networks with 32 x 32 hidden units, obs_dim 26 or 17, act_dim 6 or 7")
        self.L = L = _lib.load()
        self.fn = {k: getattr(L, "CassieDdpg" + k) for k in ("ParamCount", "PartialRows", "CriticGrad", "ActorGrad", "Apply")}
        self.D, self.A = actor.obs_dim, actor.act_dim
        self.np = {ACTOR: L.CassieDdpgParamCount(self.D, self.A, ACTOR), CRITIC: L.CassieDdpgParamCount(self.D, self.A, CRITIC)}
        if 0 in self.np.values():
            raise ValueError("DdpgKernels: unsupported shape %d -> %d" % (self.D, self.A))
        for net in (actor, critic, target_actor, target_critic):
            if not all(p.is_contiguous() for p in net.parameters()):
                raise ValueError("DdpgKernels: contiguous parameters")
        self.nets = dict(actor=actor, critic=critic, target_actor=target_actor, target_critic=target_critic)
        self.dev = next(actor.parameters()).device
        self._partial = {}

    def _stream(self):
        return ct.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _rows(self, which, batch):
        key = (which, batch)
        if key not in self._partial:
            rows = self.fn["PartialRows"](batch)
            self._partial[key] = torch.empty((rows, self.np[which] + (1 if which == ACTOR else 2)), dtype=torch.float32, device=self.dev)
        return self._partial[key]

    def critic_grad(self, pool, idx, discount):
        """partial [rows][NPq + 2] of the batch idx: gradient of SUM (Q - y)^2, the sum itself, SUM Q."""
        P = lambda t: ct.c_void_p(t.data_ptr())
        n = self.nets
        out = self._rows(CRITIC, idx.numel())
        rc = self.fn["CriticGrad"](P(pool.obs), P(pool.act), P(pool.rew), P(pool.term), P(pool.nobs), ct.c_longlong(pool.capacity), P(idx), idx.numel(), self.D, self.A,
                                   _ptrs(n["target_actor"]), _ptrs(n["target_critic"]), _ptrs(n["critic"]), ct.c_float(discount), P(out), self._stream())
        if rc != 0:
            raise RuntimeError("CassieDdpgCriticGrad failed (%d)" % rc)
        return out

    def actor_grad(self, pool, idx):
        """partial [rows][NPmu + 1]: gradient of -SUM Q(s, mu(s)) with respect to the actor, SUM Q(s, mu(s))."""
        P = lambda t: ct.c_void_p(t.data_ptr())
        n = self.nets
        out = self._rows(ACTOR, idx.numel())
        rc = self.fn["ActorGrad"](P(pool.obs), ct.c_longlong(pool.capacity), P(idx), idx.numel(), self.D, self.A, _ptrs(n["actor"]), _ptrs(n["critic"]), P(out),
                                  self._stream())
        if rc != 0:
            raise RuntimeError("CassieDdpgActorGrad failed (%d)" % rc)
        return out

    def apply(self, which, partial, scale, adam, lr, beta1, beta2, eps, tau, stats=None):
        """Rows added in order, Adam on the live network, soft update of its target: one launch.  stats: float64 device tensor the summed extra
        columns are added to."""
        n = self.nets
        live, targ = (n["actor"], n["target_actor"]) if which == ACTOR else (n["critic"], n["target_critic"])
        adam["t"] += 1
        rc = self.fn["Apply"](partial.shape[0], self.D, self.A, which, ct.c_void_p(partial.data_ptr()), ct.c_float(scale), _ptrs(live), _ptrs(targ),
                              ct.c_void_p(adam["m"].data_ptr()), ct.c_void_p(adam["v"].data_ptr()), int(adam["t"]), ct.c_float(lr), ct.c_float(beta1),
                              ct.c_float(beta2), ct.c_float(eps), ct.c_float(tau), None if stats is None else ct.c_void_p(stats.data_ptr()), self._stream())
        if rc != 0:
            raise RuntimeError("CassieDdpgApply failed (%d)" % rc)

    def update(self, pool, idx, discount, qf_lr, policy_lr, tau, adam_mu, adam_q, beta1=0.9, beta2=0.999, eps=1e-8, stats=None):
        """ddpg_update_torch_ on the rows idx of the pool, four launches (world == 1); with several ranks the host adds the rows, averages them
        over ranks and applies one row.  stats [3] float64: += (sum (Q - y)^2, sum Q(s, a), sum Q(s, mu(s)))."""
        scale = 1.0 / idx.numel()
        for which, adam, lr, off in ((CRITIC, adam_q, qf_lr, 0), (ACTOR, adam_mu, policy_lr, 2)):
            part = self.critic_grad(pool, idx, discount) if which == CRITIC else self.actor_grad(pool, idx)   # the actor sees the critic after its step
            if _world() > 1:
                part = all_mean_(part.sum(0, keepdim=True).contiguous(), "gradient_all_reduce")
            self.apply(which, part, scale, adam, lr, beta1, beta2, eps, tau, None if stats is None else stats[off:])


class _NoBaseline:
    coeffs = None


class DDPG(TRPO):
    """rllab's DDPG on TRPO's sampler state (path clocks, exploration-noise generator, truncation, snapshot).  Switches (attributes, default True)
    that tests set to force the torch statements: fused_policy_step (CassieDdpgPolicyStep + CassieDdpgPoolCommit), fused_update (the four update
    launches), fused_sampler_step (TRPO's).  last_update_kind says which update ran: "ddpg_kernels" or "torch"."""

    _REW = 3   # _stats: sum (Q - y)^2, sum Q(s, a), sum Q(s, mu(s)), summed mean reward

    def __init__(self, env_step, env_reset, policy, qf, n_envs, obs_dim, act_map, batch_size=32, max_path_length=100, epoch_length=1000,
                 min_pool_size=10000, replay_pool_size=1000000, discount=0.99, scale_reward=0.01, qf_learning_rate=1e-3, policy_learning_rate=1e-4,
                 soft_target_tau=1e-3, updates_per_step=1, ou_theta=0.15, ou_sigma=0.3, ou_mu=0.0, beta1=0.9, beta2=0.999, epsilon=1e-8, seed=1,
                 env_reset_masked=None, env_id0=None, snapshot_pool=True):
        import copy
        super().__init__(env_step, env_reset, policy, _NoBaseline(), n_envs, obs_dim, act_map, batch_size=batch_size, max_path_length=max_path_length,
                         discount=discount, seed=seed, env_reset_masked=env_reset_masked, env_id0=env_id0)
        self.qf = qf
        self.target_policy, self.target_qf = copy.deepcopy(policy), copy.deepcopy(qf)
        for p in list(self.target_policy.parameters()) + list(self.target_qf.parameters()):
            p.requires_grad_(False)
        dev, dt = self._init_off_policy("DDPG", policy.l3.out_features, batch_size, epoch_length, min_pool_size, replay_pool_size, scale_reward, qf_learning_rate,
                                        policy_learning_rate, soft_target_tau, updates_per_step, beta1, beta2, epsilon, seed, snapshot_pool)
        self.ou = OUStrategy(n_envs, self.act_dim, dev, dt, ou_theta, ou_sigma, ou_mu)
        self.adam_mu, self.adam_q = new_adam(policy), new_adam(qf)

    def _init_off_policy(self, name, act_dim, batch_size, epoch_length, min_pool_size, replay_pool_size, scale_reward, qf_learning_rate, policy_learning_rate,
                         soft_target_tau, updates_per_step, beta1, beta2, epsilon, seed, snapshot_pool):
        """What every algorithm on the replay pool sets up after TRPO.__init__ (DDPG, SAC): this rank's share of the batch, the schedule, the pool, the
        index generator's seeding and the per-iteration accumulators.  Returns the policy's (device, dtype)."""
        world = _world()
        if batch_size % world != 0:
            raise ValueError("%s: batch_size (%d) must be divisible by the number of ranks (%d)" % (name, batch_size, world))
        p0 = next(self.policy.parameters())
        dev, dt = p0.device, p0.dtype
        self.batch_size, self.batch_local = batch_size, batch_size // world
        self.epoch_length, self.min_pool_size, self.updates_per_step = epoch_length, min_pool_size, updates_per_step
        self.scale_reward, self.qf_learning_rate, self.policy_learning_rate, self.tau = scale_reward, qf_learning_rate, policy_learning_rate, soft_target_tau
        self.beta1, self.beta2, self.epsilon = beta1, beta2, epsilon
        self.act_dim = act_dim
        self.pool = ReplayPool(replay_pool_size, self.n_envs, self.obs_dim, act_dim, dev, dt)
        rank = dist.get_rank() if dist.is_initialized() else 0
        self.idx_gen = torch.Generator(device=dev)
        self.idx_gen.manual_seed(seed * 1000003 + 7919 * (rank + 1))
        self.snapshot_pool = snapshot_pool
        self.n_updates = 0
        self.last_update_kind = None
        self.last_policy_step_fused = None
        self._ep = torch.zeros(2, dtype=torch.float64, device=dev)        # finished paths, their summed returns (this iteration)
        self._stats = torch.zeros(self._REW + 1, dtype=torch.float64, device=dev)   # the update's sums (see _REW), then the summed mean reward
        self._rows = None
        self._kernels = None
        return dev, dt

    # ---- kernels
    def _update_kernels(self):
        if not getattr(self, "fused_update", True) or not kernels_cover(self.policy, self.qf):
            return None
        if self._kernels is None:
            try:
                self._kernels = DdpgKernels(self.policy, self.qf, self.target_policy, self.target_qf)
            except (ValueError, OSError, AttributeError):
                self._kernels = False
        return self._kernels or None

    def _fused_step(self, dev):
        """(policy step, pool commit) as one launch each, or None: CUDA float32 networks of a supported shape on the environment's 26-wide rows,
        rllab's normalize() action map with float64 bounds."""
        if not getattr(self, "fused_policy_step", True) or dev.type != "cuda" or not kernels_cover(self.policy, self.qf) or self.obs_dim != 26 \
                or self.policy.obs_dim != 26 or not isinstance(self.act_map, NormalizedActions):
            return None
        low, high, n, D, A = self.act_map.low, self.act_map.high, self.n_envs, self.obs_dim, self.act_dim
        if not all(t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == A for t in (low, high)):
            return None
        try:
            from . import _lib
            L = _lib.load()
            step_fn, commit_fn = L.CassieDdpgPolicyStep, L.CassieDdpgPoolCommit
        except (OSError, AttributeError):
            return None
        if not hasattr(self, "_env_actions") or self._env_actions.shape != (n, A):
            self._env_actions = torch.empty((n, A), dtype=torch.float64, device=dev)
        P = lambda t: ct.c_void_p(t.data_ptr())
        pool, ou = self.pool, self.ou
        stream = lambda: ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def step(obs, noise, top):
            if obs.dtype != torch.float64 or not obs.is_contiguous():
                raise TypeError("CassieDdpgPolicyStep: observations must be a contiguous float64 tensor (got %s)" % obs.dtype)
            assert noise.is_contiguous() and noise.dtype == torch.float32 and ou.state.is_contiguous() and self.path_t.dtype == torch.int64
            assert 0 <= top and top + n <= pool.capacity
            rc = step_fn(P(obs), n, D, A, *[ct.c_void_p(p) for p in _ptrs(self.policy)], P(noise), P(self.path_t), ct.c_float(ou.theta), ct.c_float(ou.sigma), ct.c_float(ou.mu),
                         P(ou.state), P(low), P(high), P(pool.obs[top]), P(pool.act[top]), P(self._env_actions), stream())
            if rc != 0:
                raise RuntimeError("CassieDdpgPolicyStep failed (%d)" % rc)

        return step, self._pool_commit(commit_fn, stream)

    def _pool_commit(self, commit_fn, stream):
        """CassieDdpgPoolCommit on the rows the policy step opened."""
        P = lambda t: ct.c_void_p(t.data_ptr())
        pool, n, D = self.pool, self.n_envs, self.obs_dim

        def commit(rew, done, nobs, top):
            assert rew.is_contiguous() and done.is_contiguous() and nobs.is_contiguous() and nobs.dtype == torch.float64
            assert 0 <= top and top + n <= pool.capacity
            rc = commit_fn(P(rew), P(done), P(nobs), n, D, ct.c_double(self.scale_reward), P(pool.rew[top:]), P(pool.term[top:]), P(pool.nobs[top]), stream())
            if rc != 0:
                raise RuntimeError("CassieDdpgPoolCommit failed (%d)" % rc)
        return commit

    def _explore(self, o, noise):
        """The exploring action in [-1, 1] for the float32 observations o and this step's normals (the torch statement of the policy-step kernel)."""
        return self.ou.get_action(self.policy(o), noise, self.path_t == 0)

    # ---- one vector step and its updates
    @torch.no_grad()
    def env_step_into_pool(self):
        """Act, step, store: N rows at [top, top + N).  The torch branch is the specification of CassieDdpgPolicyStep / CassieDdpgPoolCommit."""
        if self.obs is None:
            self.obs = self.env_reset().clone()
        N, A, pool = self.n_envs, self.act_dim, self.pool
        dev, dt = self.obs.device, pool.obs.dtype
        noise = torch.randn((self.n_envs_global, A), dtype=dt, device=dev, generator=self.gen)[self.env_id0:self.env_id0 + N]
        self.noise_step += 1
        top = pool.top
        fused = self._fused_step(dev)
        if self._rows is None:
            self._rows = (torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.bool, device=dev))
        if fused is not None:
            fused[0](self.obs, noise.contiguous(), top)
            nobs, rew, done = self.env_step(self._env_actions)
        else:
            o = self.obs.to(dt)
            a = self._explore(o, noise)
            nobs, rew, done = self.env_step(self.act_map(a))
        self.last_policy_step_fused = fused is not None
        if fused is not None and rew.dtype == torch.float64 and done.dtype == torch.uint8:
            fused[1](rew, done, nobs, top)   # next to CassieTrpoSamplerStep, not fused with it: DESIGN.md, "DDPG"
        else:
            if fused is not None:
                o, a = pool.obs[top:top + N], pool.act[top:top + N]
            pool.write(top, o, a, (self.scale_reward * rew.double()).to(dt), (done != 0).to(dt), nobs.to(dt))
        pool.advance()
        self._stats[self._REW] += rew.mean()
        book = self._fused_sampler_step(dev)
        cut, done = self._book_step(book, rew, done, *self._rows, self._ep)
        nobs = self._reset_truncated(cut, done, nobs)   # after the commit: a truncated path keeps its true s'
        self.obs = nobs.clone()

    def sample_indices(self):
        return torch.randint(0, self.pool.size, (self.batch_local,), generator=self.idx_gen, device=self.pool.obs.device)

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

    def train_step(self):
        """One vector step plus its updates; returns the number of updates that ran."""
        self.env_step_into_pool()
        if self.pool.size * _world() < self.min_pool_size:
            return 0
        for _ in range(self.updates_per_step):
            self.update(self.sample_indices())
        return self.updates_per_step

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
        v = torch.cat([ep, st]).tolist()   # the one read-back
        per = max(1, updates) * self.batch_local
        nan = float("nan")
        out = dict(itr=self.itr, env_steps=self.epoch_length * self.n_envs * _world(), updates=updates, pool_size=self.pool.size * _world(),
                   avg_reward=v[5] / self.epoch_length, episodes=int(v[0]), avg_return=v[1] / v[0] if v[0] > 0 else nan,
                   qf_loss=v[2] / per if updates else nan, avg_q=v[3] / per if updates else nan, policy_surr=-v[4] / per if updates else nan,
                   update_kind=self.last_update_kind)
        if timing:
            torch.cuda.synchronize()
            out["seconds_epoch"] = time.perf_counter() - t0
        self.itr += 1
        return out

    # ---- snapshot: TRPO's (actor under "policy", sampler state, env records) plus everything else a resumed run needs to BE the interrupted run
    def _snapshot_fields(self):
        sd = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
        ad = lambda a: dict(t=int(a["t"]), m=a["m"].detach().cpu(), v=a["v"].detach().cpu())
        return dict(algo="ddpg", hidden_sizes=list(self.policy.hidden_sizes), qf=sd(self.qf), target_policy=sd(self.target_policy), target_qf=sd(self.target_qf),
                    adam_mu=ad(self.adam_mu), adam_q=ad(self.adam_q), ou_state=self.ou.state.cpu(), idx_gen_state=self.idx_gen.get_state(),
                    n_updates=int(self.n_updates), pool=self.pool.state() if self.snapshot_pool else None)

    def _load_fields(self, ck):
        algo = ck.get("algo", "trpo")
        if algo != "ddpg":
            raise ValueError("DDPG.load: the snapshot was written by %s, this run is ddpg" % algo)
        self.qf.load_state_dict(ck["qf"])
        self.target_policy.load_state_dict(ck["target_policy"])
        self.target_qf.load_state_dict(ck["target_qf"])
        for mine, theirs in ((self.adam_mu, ck["adam_mu"]), (self.adam_q, ck["adam_q"])):
            mine["t"] = int(theirs["t"])
            mine["m"].copy_(theirs["m"]); mine["v"].copy_(theirs["v"])   # in place: the kernels hold no pointers, but the tensors stay the run's own
        self.n_updates = int(ck.get("n_updates", 0))
        self._pending = ck

    def load(self, path, restore_sampler=True):
        """TRPO.load, then -- only where the sampler came back, i.e. this IS the interrupted run -- the OU state, the index generator and the pool.
        A snapshot written without its pool (snapshot_pool=False) restarts with an empty one; `pool_restored` says which."""
        extra, restored = super().load(path, restore_sampler)
        ck, self._pending = self._pending, None
        dev = next(self.policy.parameters()).device
        self.pool_restored = False
        if restored:
            self.ou.state = ck["ou_state"].to(dev)
            self.idx_gen.set_state(ck["idx_gen_state"])
            if ck.get("pool") is not None:
                self.pool.load_state(ck["pool"])
                self.pool_restored = True
            else:
                self.pool.top = self.pool.size = 0
                print("DDPG.load: the snapshot carries no replay pool; this run restarts with an empty one", flush=True)
        return extra, restored


def default_pool_size(n_envs, target=1000000):
    """rllab's replay_pool_size rounded up to a multiple of the environment count."""
    return ((target + n_envs - 1) // n_envs) * n_envs


def broadcast_initial_networks(algo):
    """Rank 0's initial actor and critic are authoritative; the targets are their copies (a collective: every rank must call it)."""
    if dist.is_initialized() and dist.get_world_size() > 1:
        for net, tgt in ((algo.policy, algo.target_policy), (algo.qf, algo.target_qf)):
            theta = flat_params(net)
            dist.broadcast(theta, 0)
            set_flat_params(net, theta)
            set_flat_params(tgt, theta)


def make_cassie_ddpg(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, terrain=None, sync_policy=True, replay_pool_size=None, **kw):
    """ddpg_cassie.py:14-51 on the batched MI355X environment; the counterpart of vpg.make_cassie_vpg (same env, terrain and sync_policy rules).
    replay_pool_size: rows of this rank's pool (default: rllab's 1 000 000 rounded up to a multiple of n_envs; a row is 4 (2 D + A + 2) bytes)."""
    from .vec_env import CassieVecEnv
    env = CassieVecEnv(n_envs, kind=kind, control_mode=control_mode, n_substeps=10, auto_reset=True, device=device, trajectory=trajectory)
    env.use_torch_stream()
    dev = "cuda:%d" % device
    bufs = env.alloc()
    torch.manual_seed(seed)
    obs_w = env.observation_space.shape[0]
    policy = DeterministicMLPPolicy(obs_w, env.adim).to(dev)
    qf = ContinuousMLPQFunction(obs_w, env.adim).to(dev)
    act_map = NormalizedActions(env.action_space.low, env.action_space.high, dev)
    algo = DDPG(lambda a: env.step(a, bufs), lambda: env.reset(bufs), policy, qf, n_envs, obs_w, act_map, seed=seed,
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
