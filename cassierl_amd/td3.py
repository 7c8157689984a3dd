"""TD3 (twin delayed DDPG) over the batched environment, on DDPG's machinery (cassierl_amd/ddpg.py: networks, replay pool, sampler state, schedule,
snapshot) and in the shape of cassierl_amd/sac.py.

The reference ships no TD3 script; this docstring is the contract [external: the published algorithm (Fujimoto et al., 2018), from memory; no TD3
source is on this machine.  Where a published implementation would disagree with this paragraph, this paragraph wins]:
  * actor  ddpg.DeterministicMLPPolicy with a target copy;  critics  two ddpg.ContinuousMLPQFunction, qf1 and qf2, each with a target copy;
  * one update on the batch (s, a, r, terminal, s') with the smoothing normals eps2 [batch, A], in this order:
      1. a' = clip(mu'(s') + clip(policy_noise eps2, -noise_clip, noise_clip), -1, 1);  y = r + (1 - terminal) discount min(Q1', Q2')(s', a'),
         no gradient;
      2. each critic: loss mean((Q_k(s, a) - y)^2), one Adam step at qf_learning_rate, its own m, v, t;
      3. only when n_updates % policy_delay == policy_delay - 1 (n_updates counts the updates made before this one): the actor's loss
         -mean(Q1(s, mu(s))) through qf1 AFTER its step, one Adam step at policy_learning_rate; then all three targets
         target <- (1 - tau) target + tau live.  On every other update the actor and ALL targets stay as they are: the critics regress towards
         targets that stand still between two actor steps, which is what the delay is for.
    Adam is vpg.adam_step_; every gradient is averaged over ranks before its Adam step.

With N environments it is DDPG's module (ddpg.py, "With N environments", rules 1-5 and 7; truncation keeps the true s' with terminal = 0; the same
train_step / train_iteration / updates_per_step, one read-back per epoch).  What differs:
  * exploration is clip(mu(s) + exploration_sigma n, -1, 1) with the per-step normals DDPG draws for its OU noise (every rank draws the job's
    [n_envs_global][A] normals from the sampler's generator and keeps its shard's rows); there is no OU state;
  * the update's smoothing normals come from a generator of their own, torch.randn((batch_local, A), generator=noise_gen), seeded from
    (seed, rank) like the index generator; the snapshot carries both;
  * defaults: policy_noise 0.2, noise_clip 0.5, policy_delay 2, exploration_sigma 0.1, soft_target_tau 0.005; batch_size 256, both learning
    rates 3e-4, discount 0.99, scale_reward 1.0 and the pool sizes are SAC's.

Hot paths are HIP kernels (csrc/tu_td3.hip, include/cassie_trpo.h): CassieTd3PolicyStep and CassieDdpgPoolCommit per vector step, and per update
CassieTd3CriticGrad (both critics, one launch) and CassieTd3CriticApply (both critics' Adam steps and soft updates, one launch); a delayed update
adds DDPG's CassieDdpgActorGrad through qf1 and CassieDdpgApply on the actor: two launches, or four.  Each has its torch statement in this module
(TD3._explore, td3_update_torch_); CPU tensors, other shapes or a library without the entry points run those.
"""
import copy
import ctypes as ct

import torch
import torch.distributed as dist

from . import terrain as terrain_lib
from .ddpg import ACTOR, CRITIC, DDPG, ContinuousMLPQFunction, DdpgKernels, DeterministicMLPPolicy, _NoBaseline, _adam_on, _ptrs, default_pool_size, \
    kernels_cover as ddpg_kernels_cover, new_adam, soft_update_
from .trpo import TRPO, NormalizedActions, _world, all_mean_, all_sum_, flat_params, set_flat_params


def delayed(n_updates, policy_delay):
    """Whether the update that follows n_updates earlier ones also steps the actor and moves the targets."""
    return n_updates % policy_delay == policy_delay - 1


def smoothed_target_action(target_actor, s2, eps2, policy_noise, noise_clip):
    return (target_actor(s2) + (policy_noise * eps2).clamp(-noise_clip, noise_clip)).clamp(-1.0, 1.0)


def td3_update_torch_(actor, qf1, qf2, target_actor, target_qf1, target_qf2, adam_mu, adam_q1, adam_q2, batch, eps2, n_updates, policy_delay=2, policy_noise=0.2,
                      noise_clip=0.5, discount=0.99, qf_lr=3e-4, policy_lr=3e-4, tau=5e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """One TD3 update (the module docstring's steps 1-3) on batch = (s, a, r, terminal, s') in the networks' dtype: the specification of
    CassieTd3CriticGrad / CassieTd3CriticApply / CassieDdpgActorGrad / CassieDdpgApply.  n_updates: the updates made before this one (the delay's
    phase).  Gradients are averaged over ranks before their Adam step.  Returns (qf1_loss, qf2_loss, mean Q1, mean Q2, policy_surr), the Q means
    from before the step, policy_surr None on an update that leaves the actor alone."""
    s, a, r, term, s2 = batch
    with torch.no_grad():
        a2 = smoothed_target_action(target_actor, s2, eps2, policy_noise, noise_clip)
        y = r + (1.0 - term) * discount * torch.min(target_qf1(s2, a2), target_qf2(s2, a2))
    out = []
    for qf, adam in ((qf1, adam_q1), (qf2, adam_q2)):
        q = qf(s, a)
        loss = ((q - y) ** 2).mean()
        g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(qf.parameters()))])
        _adam_on(qf, all_mean_(g.contiguous(), "gradient_all_reduce"), adam, qf_lr, beta1, beta2, eps)
        out.append((loss.detach(), q.detach().mean()))
    surr = None
    if delayed(n_updates, policy_delay):
        surr = -qf1(s, actor(s)).mean()   # the first critic AFTER its step; only the actor moves
        g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(surr, list(actor.parameters()))])
        _adam_on(actor, all_mean_(g.contiguous(), "gradient_all_reduce"), adam_mu, policy_lr, beta1, beta2, eps)
        surr = surr.detach()
        for tgt, live in ((target_qf1, qf1), (target_qf2, qf2), (target_actor, actor)):
            soft_update_(tgt, live, tau)
    return out[0][0], out[1][0], out[0][1], out[1][1], surr


def kernels_cover(actor, qf1, qf2):
    """The kernels' shapes: DDPG's for the actor and each critic."""
    return ddpg_kernels_cover(actor, qf1) and ddpg_kernels_cover(actor, qf2)


class Td3Kernels:
    """The launches of one update on the networks' own storage: csrc/tu_td3.hip for the critics, DdpgKernels (actor, qf1) for the delayed actor
    step.  Every library call goes through the dict `fn`.  ValueError / OSError / AttributeError where they do not apply."""

    def __init__(self, actor, qf1, qf2, target_actor, target_qf1, target_qf2):
        if not kernels_cover(actor, qf1, qf2):
            raise ValueError("Td3Kernels: float32 CUDA networks with 32 x 32 hidden units, obs_dim 26 or 17, act_dim 6 or 7")
        self.actor_kernels = DdpgKernels(actor, qf1, target_actor, target_qf1)   # CassieDdpgActorGrad through qf1, CassieDdpgApply on the actor
        self.L = L = self.actor_kernels.L
        self.fn = self.actor_kernels.fn
        self.fn.update(Td3CriticGrad=L.CassieTd3CriticGrad, Td3CriticApply=L.CassieTd3CriticApply)
        self.D, self.A, self.np_q = actor.obs_dim, actor.act_dim, self.actor_kernels.np[CRITIC]
        for net in (qf2, target_qf2):
            if not all(p.is_contiguous() for p in net.parameters()):
                raise ValueError("Td3Kernels: contiguous parameters")
        self.target_actor, self.qf, self.target_qf = target_actor, (qf1, qf2), (target_qf1, target_qf2)
        self.dev = self.actor_kernels.dev
        self._partial = {}

    def _stream(self):
        return ct.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def critic_grad(self, pool, idx, eps2, policy_noise, noise_clip, discount):
        """partial [2][rows][NPq + 2] of the batch idx: for each critic the gradient of SUM (Q - y)^2, the sum itself, SUM Q."""
        P = lambda t: ct.c_void_p(t.data_ptr())
        batch = idx.numel()
        if eps2.shape != (batch, self.A) or eps2.dtype != torch.float32 or not eps2.is_contiguous() or eps2.device != self.dev:
            raise ValueError("Td3Kernels: the noise must be a contiguous float32 tensor [batch, act_dim] on the networks' device")
        if batch not in self._partial:
            self._partial[batch] = torch.empty((2, self.fn["PartialRows"](batch), self.np_q + 2), dtype=torch.float32, device=self.dev)
        out = self._partial[batch]
        rc = self.fn["Td3CriticGrad"](P(pool.obs), P(pool.act), P(pool.rew), P(pool.term), P(pool.nobs), ct.c_longlong(pool.capacity), P(idx), batch, self.D, self.A,
                                      _ptrs(self.target_actor), _ptrs(self.target_qf[0]), _ptrs(self.target_qf[1]), _ptrs(self.qf[0]), _ptrs(self.qf[1]), P(eps2),
                                      ct.c_float(policy_noise), ct.c_float(noise_clip), ct.c_float(discount), P(out), self._stream())
        if rc != 0:
            raise RuntimeError("CassieTd3CriticGrad failed (%d)" % rc)
        return out

    def critic_apply(self, partial, scale, adam_q1, adam_q2, lr, beta1, beta2, eps, tau, stats=None):
        """Both critics in one launch: block k's rows added in order, Adam, soft update of target k (tau = 0: the target keeps its bits).
        stats [4] float64: += (sum e1^2, sum Q1, sum e2^2, sum Q2)."""
        P = lambda t: ct.c_void_p(t.data_ptr())
        if adam_q1["t"] != adam_q2["t"]:
            raise ValueError("Td3Kernels: the two critics step together (t %d and %d)" % (adam_q1["t"], adam_q2["t"]))
        # the kernel finds block 1 at rows * (NPq + 2) floats behind block 0
        if partial.dim() != 3 or partial.shape[0] != 2 or partial.shape[1] < 1 or partial.shape[2] != self.np_q + 2 or partial.dtype != torch.float32 \
                or not partial.is_contiguous() or partial.device != self.dev:
            raise ValueError("Td3Kernels: partial must be a contiguous float32 tensor [2, rows, %d] on the networks' device" % (self.np_q + 2))
        adam_q1["t"] += 1
        adam_q2["t"] += 1
        rc = self.fn["Td3CriticApply"](partial.shape[1], self.D, self.A, P(partial), ct.c_float(scale), _ptrs(self.qf[0]), _ptrs(self.qf[1]), _ptrs(self.target_qf[0]),
                                       _ptrs(self.target_qf[1]), P(adam_q1["m"]), P(adam_q1["v"]), P(adam_q2["m"]), P(adam_q2["v"]), int(adam_q1["t"]), ct.c_float(lr),
                                       ct.c_float(beta1), ct.c_float(beta2), ct.c_float(eps), ct.c_float(tau), None if stats is None else P(stats), self._stream())
        if rc != 0:
            raise RuntimeError("CassieTd3CriticApply failed (%d)" % rc)

    def update(self, pool, idx, eps2, with_actor, policy_noise, noise_clip, discount, qf_lr, policy_lr, tau, adam_mu, adam_q1, adam_q2, beta1=0.9, beta2=0.999,
               eps=1e-8, stats=None):
        """td3_update_torch_ on the rows idx of the pool: two launches, four where with_actor (world == 1); with several ranks the host adds the
        rows, averages them over ranks and applies one row.  stats [5] float64: += (sum e1^2, sum Q1, sum e2^2, sum Q2, sum Q1(s, mu(s)))."""
        scale = 1.0 / idx.numel()
        many = _world() > 1
        part = self.critic_grad(pool, idx, eps2, policy_noise, noise_clip, discount)
        if many:
            part = all_mean_(part.sum(1, keepdim=True).contiguous(), "gradient_all_reduce")
        self.critic_apply(part, scale, adam_q1, adam_q2, qf_lr, beta1, beta2, eps, tau if with_actor else 0.0, stats)
        if with_actor:
            part = self.actor_kernels.actor_grad(pool, idx)   # the actor sees qf1 after its step
            if many:
                part = all_mean_(part.sum(0, keepdim=True).contiguous(), "gradient_all_reduce")
            self.actor_kernels.apply(ACTOR, part, scale, adam_mu, policy_lr, beta1, beta2, eps, tau, None if stats is None else stats[4:])


class TD3(DDPG):
    """TD3 on DDPG's sampler state, pool, schedule and snapshot rules.  Switches (attributes, default True) that tests set to force the torch
    statements: fused_policy_step (CassieTd3PolicyStep + CassieDdpgPoolCommit), fused_update (the update launches), fused_sampler_step (TRPO's).
    last_update_kind says which update ran: "td3_kernels" or "torch"."""

    _REW = 5   # _stats: sum e1^2, sum Q1, sum e2^2, sum Q2, sum Q1(s, mu(s)) over the delayed updates, summed mean reward

    def __init__(self, env_step, env_reset, policy, qf1, qf2, n_envs, obs_dim, act_map, batch_size=256, max_path_length=100, epoch_length=1000,
                 min_pool_size=10000, replay_pool_size=1000000, discount=0.99, scale_reward=1.0, qf_learning_rate=3e-4, policy_learning_rate=3e-4,
                 soft_target_tau=0.005, updates_per_step=1, policy_noise=0.2, noise_clip=0.5, policy_delay=2, exploration_sigma=0.1, beta1=0.9, beta2=0.999,
                 epsilon=1e-8, seed=1, env_reset_masked=None, env_id0=None, snapshot_pool=True):
        if policy_delay < 1:
            raise ValueError("TD3: policy_delay (%d) must be at least 1" % policy_delay)
        TRPO.__init__(self, env_step, env_reset, policy, _NoBaseline(), n_envs, obs_dim, act_map, batch_size=batch_size, max_path_length=max_path_length,
                      discount=discount, seed=seed, env_reset_masked=env_reset_masked, env_id0=env_id0)
        self.qf1, self.qf2 = qf1, qf2
        self.target_policy, self.target_qf1, self.target_qf2 = copy.deepcopy(policy), copy.deepcopy(qf1), copy.deepcopy(qf2)
        for net in (self.target_policy, self.target_qf1, self.target_qf2):
            for p in net.parameters():
                p.requires_grad_(False)
        dev, _ = self._init_off_policy("TD3", policy.act_dim, batch_size, epoch_length, min_pool_size, replay_pool_size, scale_reward, qf_learning_rate,
                                       policy_learning_rate, soft_target_tau, updates_per_step, beta1, beta2, epsilon, seed, snapshot_pool)
        self.policy_noise, self.noise_clip, self.policy_delay, self.exploration_sigma = policy_noise, noise_clip, policy_delay, exploration_sigma
        rank = dist.get_rank() if dist.is_initialized() else 0
        self.noise_gen = torch.Generator(device=dev)   # the smoothing normals: a stream of its own beside idx_gen
        self.noise_gen.manual_seed(seed * 1000003 + 104729 * (rank + 1))
        self.adam_mu, self.adam_q1, self.adam_q2 = new_adam(policy), new_adam(qf1), new_adam(qf2)

    @property
    def actor_updates(self):
        """Delayed updates among the n_updates made so far."""
        return self.n_updates // self.policy_delay

    # ---- kernels
    def _update_kernels(self):
        if not getattr(self, "fused_update", True) or not kernels_cover(self.policy, self.qf1, self.qf2):
            return None
        if self._kernels is None:
            try:
                self._kernels = Td3Kernels(self.policy, self.qf1, self.qf2, self.target_policy, self.target_qf1, self.target_qf2)
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
            step_fn, commit_fn = L.CassieTd3PolicyStep, L.CassieDdpgPoolCommit
        except (OSError, AttributeError):
            return None
        if not hasattr(self, "_env_actions") or self._env_actions.shape != (n, A):
            self._env_actions = torch.empty((n, A), dtype=torch.float64, device=dev)
        P = lambda t: ct.c_void_p(t.data_ptr())
        pool = self.pool
        stream = lambda: ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def step(obs, noise, top):
            if obs.dtype != torch.float64 or not obs.is_contiguous():
                raise TypeError("CassieTd3PolicyStep: observations must be a contiguous float64 tensor (got %s)" % obs.dtype)
            assert noise.is_contiguous() and noise.dtype == torch.float32 and noise.shape == (n, A)
            assert 0 <= top and top + n <= pool.capacity
            rc = step_fn(P(obs), n, D, A, _ptrs(self.policy), P(noise), ct.c_float(self.exploration_sigma), P(low), P(high), P(pool.obs[top]), P(pool.act[top]),
                         P(self._env_actions), stream())
            if rc != 0:
                raise RuntimeError("CassieTd3PolicyStep failed (%d)" % rc)
        return step, self._pool_commit(commit_fn, stream)

    def _explore(self, o, noise):
        return (self.policy(o) + self.exploration_sigma * noise).clamp(-1.0, 1.0)

    # ---- one update
    def sample_noise(self):
        """The update's smoothing normals eps2 [batch_local, A], from their own generator."""
        return torch.randn((self.batch_local, self.act_dim), generator=self.noise_gen, device=self.pool.obs.device, dtype=self.pool.obs.dtype)

    def update(self, idx, noise=None):
        """One TD3 update on the pool rows idx (this rank's share of the batch) with the smoothing normals noise [batch_local, A].  DDPG.train_step
        passes the indices alone: the noise is then drawn here."""
        if noise is None:
            noise = self.sample_noise()
        with_actor = delayed(self.n_updates, self.policy_delay)
        k = self._update_kernels()
        if k is not None:
            k.update(self.pool, idx.contiguous(), noise, with_actor, self.policy_noise, self.noise_clip, self.discount, self.qf_learning_rate,
                     self.policy_learning_rate, self.tau, self.adam_mu, self.adam_q1, self.adam_q2, self.beta1, self.beta2, self.epsilon, self._stats)
            self.last_update_kind = "td3_kernels"
        else:
            with torch.enable_grad():
                l1, l2, q1, q2, surr = td3_update_torch_(self.policy, self.qf1, self.qf2, self.target_policy, self.target_qf1, self.target_qf2, self.adam_mu,
                                                         self.adam_q1, self.adam_q2, self.pool.sample(idx), noise, self.n_updates, self.policy_delay,
                                                         self.policy_noise, self.noise_clip, self.discount, self.qf_learning_rate, self.policy_learning_rate,
                                                         self.tau, self.beta1, self.beta2, self.epsilon)
            n = idx.numel()
            self._stats[:4] += torch.stack([l1, q1, l2, q2]).double() * n
            if surr is not None:
                self._stats[4] -= surr.double() * n
            self.last_update_kind = "torch"
        self.n_updates += 1

    def train_iteration(self):
        """epoch_length vector steps; one read-back."""
        timing = getattr(self, "timing", False)
        if timing:
            import time
            torch.cuda.synchronize(); t0 = time.perf_counter()
        self._ep.zero_(); self._stats.zero_()
        updates, actor_before = 0, self.actor_updates
        for _ in range(self.epoch_length):
            updates += self.train_step()
        actor_updates = self.actor_updates - actor_before
        ep = all_sum_(self._ep.clone(), "stats_all_reduce")
        st = all_mean_(self._stats.clone(), "stats_all_reduce")
        v = torch.cat([ep, st]).tolist()   # the one read-back
        nan = float("nan")
        avg = lambda x: x / (updates * self.batch_local) if updates else nan
        out = dict(itr=self.itr, env_steps=self.epoch_length * self.n_envs * _world(), updates=updates, actor_updates=actor_updates, pool_size=self.pool.size * _world(),
                   avg_reward=v[7] / self.epoch_length, episodes=int(v[0]), avg_return=v[1] / v[0] if v[0] > 0 else nan, qf1_loss=avg(v[2]), qf2_loss=avg(v[4]),
                   avg_q1=avg(v[3]), avg_q2=avg(v[5]), policy_surr=-v[6] / (actor_updates * self.batch_local) if actor_updates else nan,
                   update_kind=self.last_update_kind)
        if timing:
            torch.cuda.synchronize()
            out["seconds_epoch"] = time.perf_counter() - t0
        self.itr += 1
        return out

    # ---- snapshot: DDPG's, with TD3's networks, optimiser states and both generators; n_updates fixes the delay's phase
    def _snapshot_fields(self):
        sd = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
        ad = lambda a: dict(t=int(a["t"]), m=a["m"].detach().cpu(), v=a["v"].detach().cpu())
        return dict(algo="td3", hidden_sizes=list(self.policy.hidden_sizes), qf1=sd(self.qf1), qf2=sd(self.qf2), target_policy=sd(self.target_policy),
                    target_qf1=sd(self.target_qf1), target_qf2=sd(self.target_qf2), adam_mu=ad(self.adam_mu), adam_q1=ad(self.adam_q1), adam_q2=ad(self.adam_q2),
                    idx_gen_state=self.idx_gen.get_state(), noise_gen_state=self.noise_gen.get_state(), n_updates=int(self.n_updates),
                    pool=self.pool.state() if self.snapshot_pool else None)

    def _load_fields(self, ck):
        algo = ck.get("algo", "trpo")
        if algo != "td3":
            raise ValueError("TD3.load: the snapshot was written by %s, this run is td3" % algo)
        for name in ("qf1", "qf2", "target_policy", "target_qf1", "target_qf2"):
            getattr(self, name).load_state_dict(ck[name])
        for mine, theirs in ((self.adam_mu, ck["adam_mu"]), (self.adam_q1, ck["adam_q1"]), (self.adam_q2, ck["adam_q2"])):
            mine["t"] = int(theirs["t"])
            mine["m"].copy_(theirs["m"]); mine["v"].copy_(theirs["v"])
        self.n_updates = int(ck.get("n_updates", 0))
        self._pending = ck

    def load(self, path, restore_sampler=True):
        """DDPG.load without an OU state: both generators and the pool come back only where the sampler did."""
        extra, restored = TRPO.load(self, path, restore_sampler)
        ck, self._pending = self._pending, None
        self.pool_restored = False
        if restored:
            self.idx_gen.set_state(ck["idx_gen_state"])
            self.noise_gen.set_state(ck["noise_gen_state"])
            if ck.get("pool") is not None:
                self.pool.load_state(ck["pool"])
                self.pool_restored = True
            else:
                self.pool.top = self.pool.size = 0
                print("TD3.load: the snapshot carries no replay pool; this run restarts with an empty one", flush=True)
        return extra, restored


def broadcast_initial_networks(algo):
    """Rank 0's initial actor and critics are authoritative; the three targets are their copies (a collective: every rank must call it)."""
    if dist.is_initialized() and dist.get_world_size() > 1:
        for net, tgt in ((algo.policy, algo.target_policy), (algo.qf1, algo.target_qf1), (algo.qf2, algo.target_qf2)):
            theta = flat_params(net)
            dist.broadcast(theta, 0)
            set_flat_params(net, theta)
            set_flat_params(tgt, theta)


def make_cassie_td3(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, terrain=None, sync_policy=True, replay_pool_size=None, **kw):
    """TD3 on the batched MI355X environment; the counterpart of sac.make_cassie_sac (same env, terrain and sync_policy rules).
    replay_pool_size: rows of this rank's pool (default: 1 000 000 rounded up to a multiple of n_envs; a row is 4 (2 D + A + 2) bytes)."""
    from .vec_env import CassieVecEnv
    env = CassieVecEnv(n_envs, kind=kind, control_mode=control_mode, n_substeps=10, auto_reset=True, device=device, trajectory=trajectory)
    env.use_torch_stream()
    dev = "cuda:%d" % device
    bufs = env.alloc()
    torch.manual_seed(seed)
    obs_w = env.observation_space.shape[0]
    policy = DeterministicMLPPolicy(obs_w, env.adim).to(dev)
    qf1, qf2 = ContinuousMLPQFunction(obs_w, env.adim).to(dev), ContinuousMLPQFunction(obs_w, env.adim).to(dev)
    act_map = NormalizedActions(env.action_space.low, env.action_space.high, dev)
    algo = TD3(lambda a: env.step(a, bufs), lambda: env.reset(bufs), policy, qf1, qf2, n_envs, obs_w, act_map, seed=seed,
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
