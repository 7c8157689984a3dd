"""What the algorithms on the replay pool share (ddpg.py, sac.py, td3.py): the pool, Adam and target helpers, the base of their kernel-call classes
and OffPolicy, the class they derive from -- sampler state, schedule, fused policy step, epoch report and snapshot.  This module imports none of them.

With N environments ("DDPG"):
  1. a pool row is (s [D], a [A], r, terminal, s' [D]), float32, structure of arrays on the device; a is the clipped action in [-1, 1], r is
     already scaled.  rllab's pool finds s' at ring index + 1, which only works for one environment;
  2. one vector step appends exactly N rows at ring positions [top, top + N), environment i at top + i; the capacity is a multiple of N
     (ValueError otherwise), so an append never wraps inside a step; size = min(size + N, capacity); every rank owns the pool of its own
     environments;
  3. a live path cut at max_path_length is stored with terminal = 0 and its true s' (the observation Env.step returned, before the masked
     reset).  rllab drops that transition because its ring cannot hold it; that is not reproduced.  A real done is stored with terminal = 1;
     its s' is whatever the auto-reset returned and is multiplied by zero in the target;
  4. `updates_per_step` (1) updates of `batch_size` rows follow every vector step: with N = 1 this is rllab's loop; at large N one sets
     both (e.g. batch_size = 65536, updates_per_step = 1) -- no scaling rule is invented;
  5. batch indices: torch.randint(0, size, (batch,)) from a generator on the device seeded from (seed, rank).  With world > 1 each rank draws
     batch_size / world indices from its own pool and every gradient is averaged over ranks before its Adam step: parameters, targets and
     Adam state stay identical on all ranks, and the result depends on the number of ranks;
  6. the per-step exploration normals (DDPG's OU noise) are drawn as TRPO's exploration noise: every rank draws the [n_envs_global][A] normals
     of the job and keeps its shard's rows;
  7. float32 arithmetic.  The update kernels cover D 26 or 17, A 6 or 7, hidden 32 x 32; the policy-step kernels the environment's 26-wide rows.
     SAC's also cover Cassie3d's 45 x 10 (sac.py; DDPG and TD3 do not run on env="cassie3d").

A new algorithm on the pool: DESIGN.md, "Off-policy family".
"""
import copy
import ctypes as ct

import torch
import torch.distributed as dist

from ._lib import Kernels, available, ptr as _P
from .adam import adam_step_
from .comm import _world, all_mean_, all_sum_
from .policy import NormalizedActions, flat_params, set_flat_params
from .sampler import Sampler, make_cassie_algo


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


def _ptrs(net):
    """Host array of the six device pointers {W1, b1, W2, b2, W3, b3} of a network."""
    ps = [net.l1.weight, net.l1.bias, net.l2.weight, net.l2.bias, net.l3.weight, net.l3.bias]
    return (ct.c_void_p * 6)(*[p.data_ptr() for p in ps])


def _F(*xs):
    return [ct.c_float(x) for x in xs]


class PoolKernels(Kernels):
    """Base of DdpgKernels, SacKernels and Td3Kernels: the library calls of one update on the networks' own storage (_lib.Kernels: ENTRY, `fn`,
    _call; the call sites pass the stream themselves, where the kernel takes one)."""

    STREAM_LAST = False

    def __init__(self, nets, fn=None):
        super().__init__(next(nets[0].parameters()).device, fn)   # Td3Kernels shares the dict of the DdpgKernels it embeds
        for net in nets:
            if not all(p.is_contiguous() for p in net.parameters()):
                raise ValueError("%s: contiguous parameters" % type(self).__name__)
        self._partial = {}

    def _rows(self, key, batch, *shape):
        """The cached buffer `key` of partial sums for this batch size: shape with -1 standing for the rows CassieDdpgPartialRows gives."""
        if (key, batch) not in self._partial:
            rows = self.fn["PartialRows"](batch)
            self._partial[key, batch] = torch.empty([rows if s == -1 else s for s in shape], dtype=torch.float32, device=self.dev)
        return self._partial[key, batch]

    def _check_noise(self, noise, idx):
        if noise.shape != (idx.numel(), self.A) or noise.dtype != torch.float32 or not noise.is_contiguous() or noise.device != self.dev:
            raise ValueError("%s: the noise must be a contiguous float32 tensor [batch, act_dim] on the networks' device" % type(self).__name__)

    @staticmethod
    def _over_ranks(part, rows_dim=0):
        """With several ranks the host adds the workgroups' rows and averages the one row that is left over ranks."""
        if _world() > 1:
            part = all_mean_(part.sum(rows_dim, keepdim=True).contiguous(), "gradient_all_reduce")
        return part


class OffPolicy(Sampler):
    """An algorithm on the replay pool, on Sampler's state (path clocks, exploration-noise generator, truncation, snapshot).  Switches
    (attributes, default True) that tests set to force the torch statements: fused_policy_step (the policy-step kernel + CassieDdpgPoolCommit),
    fused_update (the update launches), fused_sampler_step (Sampler's).  last_update_kind says which update ran.  A subclass supplies the class
    attributes and hooks below, _explore, update and its own constructor arguments ("Off-policy family")."""

    ALGO = None         # the snapshot's "algo" entry
    STEP_ENTRY = {}     # width of the environment's rows -> exported name of the policy-step kernel for it (26; SAC: 45 as well)
    NETS = ()           # (live, target or None) attribute names, the actor ("policy") first: targets are made, saved and broadcast from this
    ADAMS = ()          # attribute names of the Adam states
    COUNTS = ()         # keys of _report() that follow "updates" in the epoch's dict; the others follow "avg_return"
    _REW = 0            # _stats: the update's sums, then (at this index) the summed mean reward

    def __init__(self, env_step, env_reset, policy, n_envs, obs_dim, act_map, batch_size, max_path_length, epoch_length, min_pool_size, replay_pool_size, discount,
                 scale_reward, qf_learning_rate, policy_learning_rate, soft_target_tau, updates_per_step, beta1, beta2, epsilon, seed, env_reset_masked, env_id0,
                 snapshot_pool):
        """The live networks besides the policy are attributes already (NETS names them).  Sets up the targets, this rank's share of the batch, the
        schedule, the pool, the index generator's seeding and the per-iteration accumulators."""
        super().__init__(env_step, env_reset, policy, n_envs, obs_dim, act_map, batch_size=batch_size, max_path_length=max_path_length,
                         discount=discount, seed=seed, env_reset_masked=env_reset_masked, env_id0=env_id0)
        for live, target in self.NETS:
            if target is not None:
                setattr(self, target, copy.deepcopy(getattr(self, live)))
                for p in getattr(self, target).parameters():
                    p.requires_grad_(False)
        world = _world()
        if batch_size % world != 0:
            raise ValueError("%s: batch_size (%d) must be divisible by the number of ranks (%d)" % (type(self).__name__, batch_size, world))
        p0 = next(self.policy.parameters())
        dev, dt = p0.device, p0.dtype
        self.batch_size, self.batch_local = batch_size, batch_size // world
        self.epoch_length, self.min_pool_size, self.updates_per_step = epoch_length, min_pool_size, updates_per_step
        self.scale_reward, self.qf_learning_rate, self.policy_learning_rate, self.tau = scale_reward, qf_learning_rate, policy_learning_rate, soft_target_tau
        self.beta1, self.beta2, self.epsilon = beta1, beta2, epsilon
        self.act_dim = policy.act_dim
        self.pool = ReplayPool(replay_pool_size, self.n_envs, self.obs_dim, self.act_dim, dev, dt)
        self.idx_gen = self._rank_generator(dev, seed, 7919)
        self.snapshot_pool = snapshot_pool
        self.n_updates = 0
        self.last_update_kind = None
        self.last_policy_step_fused = None
        self._ep = torch.zeros(2, dtype=torch.float64, device=dev)        # finished paths, their summed returns (this iteration)
        self._stats = torch.zeros(self._REW + 1, dtype=torch.float64, device=dev)   # the update's sums (see _REW), then the summed mean reward
        self._rows = None
        self._kernels = None

    @staticmethod
    def _rank_generator(dev, seed, prime):
        rank = dist.get_rank() if dist.is_initialized() else 0
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed * 1000003 + prime * (rank + 1))
        return gen

    # ---- hooks
    def _covered(self):
        """Whether the networks have the kernels' shapes (the module's kernels_cover)."""
        raise NotImplementedError

    def _new_kernels(self):
        """The module's kernels object on this run's networks."""
        raise NotImplementedError

    def _policy_step_call(self, fn, head, noise, tail):
        """Calls the policy-step entry fn(*head, <the actor and what else the algorithm passes>, *tail) and returns its code.  head: obs, n, D, A;
        noise: this step's normals; tail: low, high, the pool's obs and act rows, the environment's actions, the stream."""
        raise NotImplementedError

    def _report(self, v, updates):
        """The algorithm's entries of the epoch's dict from the read-back v = [episodes, returns, _stats..., _readback_extra...]."""
        raise NotImplementedError

    def _readback_extra(self):
        """Device tensors (float64, 1-d) appended to the epoch's one read-back."""
        return []

    def _snapshot_extra(self):
        return {}

    def _load_extra(self, ck):
        """Entries of _snapshot_extra that come back with every load."""

    def _load_sampler_extra(self, ck, dev):
        """Entries of _snapshot_extra that come back only where the sampler did."""

    def _broadcast_extra(self):
        """What broadcast_initial_networks sends besides the networks."""

    # ---- kernels
    def _update_kernels(self):
        if not getattr(self, "fused_update", True) or not self._covered():
            return None
        if self._kernels is None:
            try:
                self._kernels = self._new_kernels()
            except (ValueError, OSError, AttributeError):
                self._kernels = False
        return self._kernels or None

    def _fused_step(self, dev):
        """(policy step, pool commit) as one launch each, or None: CUDA float32 networks of a supported shape on the environment's own rows (26 wide;
        45 wide where the algorithm has a step entry for it), rllab's normalize() action map with float64 bounds."""
        entry = self.STEP_ENTRY.get(self.obs_dim)
        if not getattr(self, "fused_policy_step", True) or dev.type != "cuda" or not self._covered() or entry is None or self.policy.obs_dim != self.obs_dim \
                or not isinstance(self.act_map, NormalizedActions):
            return None
        low, high, n, D, A = self.act_map.low, self.act_map.high, self.n_envs, self.obs_dim, self.act_dim
        if not all(t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == A for t in (low, high)):
            return None
        if not available(entry, "CassieDdpgPoolCommit"):
            return None
        k = Kernels(dev, entry={"Step": entry, "Commit": "CassieDdpgPoolCommit"})
        step_fn, commit_fn = k.fn["Step"], k.fn["Commit"]
        if not hasattr(self, "_env_actions") or self._env_actions.shape != (n, A):
            self._env_actions = torch.empty((n, A), dtype=torch.float64, device=dev)
        pool = self.pool
        stream = lambda: ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def step(obs, noise, top):
            if obs.dtype != torch.float64 or not obs.is_contiguous():
                raise TypeError("%s: observations must be a contiguous float64 tensor (got %s)" % (entry, obs.dtype))
            assert noise.is_contiguous() and noise.dtype == torch.float32 and noise.shape == (n, A)
            assert 0 <= top and top + n <= pool.capacity
            rc = self._policy_step_call(step_fn, (_P(obs), n, D, A), _P(noise),
                                        (_P(low), _P(high), _P(pool.obs[top]), _P(pool.act[top]), _P(self._env_actions), stream()))
            if rc != 0:
                raise RuntimeError("%s failed (%d)" % (entry, rc))
        return step, self._pool_commit(commit_fn, stream)

    def _pool_commit(self, commit_fn, stream):
        """CassieDdpgPoolCommit on the rows the policy step opened."""
        pool, n, D = self.pool, self.n_envs, self.obs_dim

        def commit(rew, done, nobs, top):
            assert rew.is_contiguous() and done.is_contiguous() and nobs.is_contiguous() and nobs.dtype == torch.float64
            assert 0 <= top and top + n <= pool.capacity
            rc = commit_fn(_P(rew), _P(done), _P(nobs), n, D, ct.c_double(self.scale_reward), _P(pool.rew[top:]), _P(pool.term[top:]), _P(pool.nobs[top]), stream())
            if rc != 0:
                raise RuntimeError("CassieDdpgPoolCommit failed (%d)" % rc)
        return commit

    # ---- one vector step and its updates
    @torch.no_grad()
    def env_step_into_pool(self):
        """Act, step, store: N rows at [top, top + N).  The torch branch is the specification of the policy-step kernel / CassieDdpgPoolCommit."""
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

    def train_step(self):
        """One vector step plus its updates (update(idx): the subclass's); returns the number of updates that ran."""
        self.env_step_into_pool()
        if self.pool.size * _world() < self.min_pool_size:
            return 0
        for _ in range(self.updates_per_step):
            self.update(self.sample_indices())
        return self.updates_per_step

    def _per_sample(self, x, updates):
        """A sum over the epoch's update batches as a mean per sample (nan for an epoch without updates): for _report."""
        return x / (updates * self.batch_local) if updates else float("nan")

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
        v = torch.cat([ep, st, *self._readback_extra()]).tolist()   # the one read-back
        own = self._report(v, updates)
        out = dict(itr=self.itr, env_steps=self.epoch_length * self.n_envs * _world(), updates=updates, **{k: own.pop(k) for k in self.COUNTS},
                   pool_size=self.pool.size * _world(), avg_reward=v[2 + self._REW] / self.epoch_length, episodes=int(v[0]),
                   avg_return=v[1] / v[0] if v[0] > 0 else float("nan"), **own, update_kind=self.last_update_kind)
        if timing:
            torch.cuda.synchronize()
            out["seconds_epoch"] = time.perf_counter() - t0
        self.itr += 1
        return out

    # ---- snapshot: Sampler's (actor under "policy", sampler state, env records) plus everything else a resumed run needs to BE the interrupted run
    def _saved_nets(self):
        return [name for pair in self.NETS for name in pair if name not in (None, "policy")]

    def _snapshot_fields(self):
        sd = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
        ad = lambda a: dict(t=int(a["t"]), m=a["m"].detach().cpu(), v=a["v"].detach().cpu())
        return dict(algo=self.ALGO, hidden_sizes=list(self.policy.hidden_sizes), **{n: sd(getattr(self, n)) for n in self._saved_nets()},
                    **{a: ad(getattr(self, a)) for a in self.ADAMS}, **self._snapshot_extra(), idx_gen_state=self.idx_gen.get_state(),
                    n_updates=int(self.n_updates), pool=self.pool.state() if self.snapshot_pool else None)

    def _load_fields(self, ck):
        algo = ck.get("algo", "trpo")
        if algo != self.ALGO:
            raise ValueError("%s.load: the snapshot was written by %s, this run is %s" % (type(self).__name__, algo, self.ALGO))
        self._check_env_family(ck)   # before the first network comes back: the other family's networks have other shapes
        for name in self._saved_nets():
            getattr(self, name).load_state_dict(ck[name])
        for name in self.ADAMS:
            mine, theirs = getattr(self, name), ck[name]
            mine["t"] = int(theirs["t"])
            mine["m"].copy_(theirs["m"]); mine["v"].copy_(theirs["v"])   # in place: the kernels hold no pointers, but the tensors stay the run's own
        self._load_extra(ck)
        self.n_updates = int(ck.get("n_updates", 0))
        self._pending = ck

    def load(self, path, restore_sampler=True):
        """Sampler.load, then -- only where the sampler came back, i.e. this IS the interrupted run -- the index generator, _load_sampler_extra and the
        pool.  A snapshot written without its pool (snapshot_pool=False) restarts with an empty one; `pool_restored` says which."""
        extra, restored = super().load(path, restore_sampler)
        ck, self._pending = self._pending, None
        self.pool_restored = False
        if restored:
            self.idx_gen.set_state(ck["idx_gen_state"])
            self._load_sampler_extra(ck, next(self.policy.parameters()).device)
            if ck.get("pool") is not None:
                self.pool.load_state(ck["pool"])
                self.pool_restored = True
            else:
                self.pool.top = self.pool.size = 0
                print("%s.load: the snapshot carries no replay pool; this run restarts with an empty one" % type(self).__name__, flush=True)
        return extra, restored


def default_pool_size(n_envs, target=1000000):
    """rllab's replay_pool_size rounded up to a multiple of the environment count."""
    return ((target + n_envs - 1) // n_envs) * n_envs


def broadcast_initial_networks(algo):
    """Rank 0's initial live networks (and what _broadcast_extra names) are authoritative; the targets are their copies (a collective: every rank
    must call it)."""
    if dist.is_initialized() and dist.get_world_size() > 1:
        for live, target in algo.NETS:
            theta = flat_params(getattr(algo, live))
            dist.broadcast(theta, 0)
            set_flat_params(getattr(algo, live), theta)
            if target is not None:
                set_flat_params(getattr(algo, target), theta)
        algo._broadcast_extra()


def make_cassie_offpolicy(cls, make_nets, n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, terrain=None, sync_policy=True,
                          replay_pool_size=None, **kw):
    """cls on the batched MI355X environment (sampler.make_cassie_algo: env, terrain and sync_policy rules).  make_nets(obs_dim, act_dim) -> the networks
    of cls's constructor, the policy first, built after torch.manual_seed(seed).  replay_pool_size: rows of this rank's pool (default: rllab's
    1 000 000 rounded up to a multiple of n_envs; a row is 4 (2 D + A + 2) bytes)."""
    return make_cassie_algo(cls, lambda D, A, dev: [net.to(dev) for net in make_nets(D, A)], broadcast_initial_networks, n_envs, kind, control_mode, device,
                            trajectory, seed, terrain, sync_policy, replay_pool_size=default_pool_size(n_envs) if replay_pool_size is None else replay_pool_size, **kw)
