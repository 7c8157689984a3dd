"""TD3 (twin delayed DDPG) over the batched environment, on the off-policy base (cassierl_amd/offpolicy.py: replay pool, sampler state, schedule,
snapshot) with DDPG's networks (cassierl_amd/ddpg.py), in the shape of cassierl_amd/sac.py.

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
    Adam is adam.adam_step_; every gradient is averaged over ranks before its Adam step.

With N environments it is the off-policy base (offpolicy.py, "With N environments", rules 1-5 and 7; truncation keeps the true s' with terminal = 0;
the same train_step / train_iteration / updates_per_step, one read-back per epoch).  What differs from DDPG:
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
import ctypes as ct

import torch

from .comm import all_mean_
from .ddpg import ACTOR, CRITIC, ContinuousMLPQFunction, DdpgKernels, DeterministicMLPPolicy, kernels_cover as ddpg_kernels_cover
from .offpolicy import OffPolicy, PoolKernels, _F, _P, _adam_on, _ptrs, broadcast_initial_networks, make_cassie_offpolicy, new_adam, soft_update_


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


class Td3Kernels(PoolKernels):
    """The launches of one update on the networks' own storage: csrc/tu_td3.hip for the critics, DdpgKernels (actor, qf1) for the delayed actor
    step, which shares this object's `fn`.  ValueError / OSError / AttributeError where they do not apply."""

    ENTRY = dict(Td3CriticGrad="CassieTd3CriticGrad", Td3CriticApply="CassieTd3CriticApply")

    def __init__(self, actor, qf1, qf2, target_actor, target_qf1, target_qf2):
        if not kernels_cover(actor, qf1, qf2):
            raise ValueError("Td3Kernels: float32 CUDA networks with 32 x 32 hidden units, obs_dim 26 or 17, act_dim 6 or 7")
        self.actor_kernels = DdpgKernels(actor, qf1, target_actor, target_qf1)   # CassieDdpgActorGrad through qf1, CassieDdpgApply on the actor
        super().__init__((actor, qf2, target_qf2), self.actor_kernels.fn)
        self.D, self.A, self.np_q = actor.obs_dim, actor.act_dim, self.actor_kernels.np[CRITIC]
        self.target_actor, self.qf, self.target_qf = target_actor, (qf1, qf2), (target_qf1, target_qf2)

    def critic_grad(self, pool, idx, eps2, policy_noise, noise_clip, discount):
        """partial [2][rows][NPq + 2] of the batch idx: for each critic the gradient of SUM (Q - y)^2, the sum itself, SUM Q."""
        self._check_noise(eps2, idx)
        out = self._rows("critic", idx.numel(), 2, -1, self.np_q + 2)
        self._call("Td3CriticGrad", _P(pool.obs), _P(pool.act), _P(pool.rew), _P(pool.term), _P(pool.nobs), ct.c_longlong(pool.capacity), _P(idx), idx.numel(), self.D,
                   self.A, _ptrs(self.target_actor), _ptrs(self.target_qf[0]), _ptrs(self.target_qf[1]), _ptrs(self.qf[0]), _ptrs(self.qf[1]), _P(eps2),
                   *_F(policy_noise, noise_clip, discount), _P(out), self._stream())
        return out

    def critic_apply(self, partial, scale, adam_q1, adam_q2, lr, beta1, beta2, eps, tau, stats=None):
        """Both critics in one launch: block k's rows added in order, Adam, soft update of target k (tau = 0: the target keeps its bits).
        stats [4] float64: += (sum e1^2, sum Q1, sum e2^2, sum Q2)."""
        if adam_q1["t"] != adam_q2["t"]:
            raise ValueError("Td3Kernels: the two critics step together (t %d and %d)" % (adam_q1["t"], adam_q2["t"]))
        # the kernel finds block 1 at rows * (NPq + 2) floats behind block 0
        if partial.dim() != 3 or partial.shape[0] != 2 or partial.shape[1] < 1 or partial.shape[2] != self.np_q + 2 or partial.dtype != torch.float32 \
                or not partial.is_contiguous() or partial.device != self.dev:
            raise ValueError("Td3Kernels: partial must be a contiguous float32 tensor [2, rows, %d] on the networks' device" % (self.np_q + 2))
        adam_q1["t"] += 1
        adam_q2["t"] += 1
        self._call("Td3CriticApply", partial.shape[1], self.D, self.A, _P(partial), ct.c_float(scale), _ptrs(self.qf[0]), _ptrs(self.qf[1]), _ptrs(self.target_qf[0]),
                   _ptrs(self.target_qf[1]), _P(adam_q1["m"]), _P(adam_q1["v"]), _P(adam_q2["m"]), _P(adam_q2["v"]), int(adam_q1["t"]),
                   *_F(lr, beta1, beta2, eps, tau), None if stats is None else _P(stats), self._stream())

    def update(self, pool, idx, eps2, with_actor, policy_noise, noise_clip, discount, qf_lr, policy_lr, tau, adam_mu, adam_q1, adam_q2, beta1=0.9, beta2=0.999,
               eps=1e-8, stats=None):
        """td3_update_torch_ on the rows idx of the pool: two launches, four where with_actor (world == 1); with several ranks the host adds the
        rows, averages them over ranks and applies one row.  stats [5] float64: += (sum e1^2, sum Q1, sum e2^2, sum Q2, sum Q1(s, mu(s)))."""
        scale = 1.0 / idx.numel()
        part = self._over_ranks(self.critic_grad(pool, idx, eps2, policy_noise, noise_clip, discount), 1)
        self.critic_apply(part, scale, adam_q1, adam_q2, qf_lr, beta1, beta2, eps, tau if with_actor else 0.0, stats)
        if with_actor:
            part = self._over_ranks(self.actor_kernels.actor_grad(pool, idx))   # the actor sees qf1 after its step
            self.actor_kernels.apply(ACTOR, part, scale, adam_mu, policy_lr, beta1, beta2, eps, tau, None if stats is None else stats[4:])


class TD3(OffPolicy):
    """TD3 on OffPolicy's sampler state, pool, schedule and snapshot.  Kernels: CassieTd3PolicyStep + CassieDdpgPoolCommit per vector step, the
    update launches; last_update_kind is "td3_kernels" or "torch"."""

    ALGO, STEP_ENTRY = "td3", {26: "CassieTd3PolicyStep"}
    NETS = (("policy", "target_policy"), ("qf1", "target_qf1"), ("qf2", "target_qf2"))
    ADAMS = ("adam_mu", "adam_q1", "adam_q2")
    COUNTS = ("actor_updates",)
    _REW = 5   # _stats: sum e1^2, sum Q1, sum e2^2, sum Q2, sum Q1(s, mu(s)) over the delayed updates, summed mean reward

    def __init__(self, env_step, env_reset, policy, qf1, qf2, n_envs, obs_dim, act_map, batch_size=256, max_path_length=100, epoch_length=1000,
                 min_pool_size=10000, replay_pool_size=1000000, discount=0.99, scale_reward=1.0, qf_learning_rate=3e-4, policy_learning_rate=3e-4,
                 soft_target_tau=0.005, updates_per_step=1, policy_noise=0.2, noise_clip=0.5, policy_delay=2, exploration_sigma=0.1, beta1=0.9, beta2=0.999,
                 epsilon=1e-8, seed=1, env_reset_masked=None, env_id0=None, snapshot_pool=True):
        if policy_delay < 1:
            raise ValueError("TD3: policy_delay (%d) must be at least 1" % policy_delay)
        self.qf1, self.qf2 = qf1, qf2
        super().__init__(env_step, env_reset, policy, n_envs, obs_dim, act_map, batch_size, max_path_length, epoch_length, min_pool_size, replay_pool_size, discount,
                         scale_reward, qf_learning_rate, policy_learning_rate, soft_target_tau, updates_per_step, beta1, beta2, epsilon, seed, env_reset_masked,
                         env_id0, snapshot_pool)
        self.policy_noise, self.noise_clip, self.policy_delay, self.exploration_sigma = policy_noise, noise_clip, policy_delay, exploration_sigma
        self.noise_gen = self._rank_generator(self.pool.obs.device, seed, 104729)   # the smoothing normals: a stream of its own beside idx_gen
        self.adam_mu, self.adam_q1, self.adam_q2 = new_adam(policy), new_adam(qf1), new_adam(qf2)

    @property
    def actor_updates(self):
        """Delayed updates among the n_updates made so far."""
        return self.n_updates // self.policy_delay

    def _covered(self):
        return kernels_cover(self.policy, self.qf1, self.qf2)

    def _new_kernels(self):
        return Td3Kernels(self.policy, self.qf1, self.qf2, self.target_policy, self.target_qf1, self.target_qf2)

    def _policy_step_call(self, fn, head, noise, tail):
        return fn(*head, _ptrs(self.policy), noise, ct.c_float(self.exploration_sigma), *tail)

    def _explore(self, o, noise):
        return (self.policy(o) + self.exploration_sigma * noise).clamp(-1.0, 1.0)

    # ---- one update
    def sample_noise(self):
        """The update's smoothing normals eps2 [batch_local, A], from their own generator."""
        return torch.randn((self.batch_local, self.act_dim), generator=self.noise_gen, device=self.pool.obs.device, dtype=self.pool.obs.dtype)

    def update(self, idx, noise=None):
        """One TD3 update on the pool rows idx (this rank's share of the batch) with the smoothing normals noise [batch_local, A].
        OffPolicy.train_step passes the indices alone: the noise is then drawn here."""
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

    def _report(self, v, updates):
        avg = lambda x: self._per_sample(x, updates)
        actor_updates = self.actor_updates - (self.n_updates - updates) // self.policy_delay   # the delayed ones among this epoch's updates
        return dict(actor_updates=actor_updates, qf1_loss=avg(v[2]), qf2_loss=avg(v[4]), avg_q1=avg(v[3]), avg_q2=avg(v[5]),
                    policy_surr=-v[6] / (actor_updates * self.batch_local) if actor_updates else float("nan"))

    # ---- snapshot: the base's, with the smoothing normals' generator; n_updates fixes the delay's phase
    def _snapshot_extra(self):
        return dict(noise_gen_state=self.noise_gen.get_state())

    def _load_sampler_extra(self, ck, dev):
        self.noise_gen.set_state(ck["noise_gen_state"])


def make_cassie_td3(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, terrain=None, sync_policy=True, replay_pool_size=None, **kw):
    """TD3 on the batched MI355X environment: offpolicy.make_cassie_offpolicy with TD3's networks."""
    make_nets = lambda D, A: (DeterministicMLPPolicy(D, A), ContinuousMLPQFunction(D, A), ContinuousMLPQFunction(D, A))
    return make_cassie_offpolicy(TD3, make_nets, n_envs, kind, control_mode, device, trajectory, seed, terrain, sync_policy, replay_pool_size, **kw)
