"""What every algorithm on the batched environment shares, and what the on-policy ones share on top of it.

  Sampler    the resident environments and their bookkeeping -- exploration noise keyed by the global environment id, path clocks and returns,
             truncation at max_path_length, the gather of returns -- and the snapshot (snapshot_mode="last").  The base of OffPolicy
             (offpolicy.py: DDPG, SAC, TD3) and of ES.
  OnPolicy   Sampler plus the LinearFeatureBaseline: the rollout batch (collect), returns / advantages / the baseline's fit (process) and the
             iteration around a subclass's optimize().  The base of TRPO, VPG and PPO.
  make_cassie_algo   any of them on CassieVecEnv or Cassie3dVecEnv: what every make_cassie_* is.
"""
import ctypes as ct
import math

import torch
import torch.distributed as dist

from . import terrain as terrain_lib
from ._lib import Kernels, available, ptr
from .baseline import BaselineKernels, LinearFeatureBaseline, discounted_returns
from .comm import _world, all_mean_, all_sum_
from .policy import GaussianMLPPolicy, NormalizedActions, _two_layer_tanh, flat_params, hidden_sizes_of, set_flat_params


class Sampler:
    ALGO = None        # the snapshot's "algo" entry ("trpo": a plain TRPO snapshot has none)
    CASSIE3D = False   # whether make_cassie_algo builds this algorithm on Cassie3d (env="cassie3d"): PPO, SAC and ES

    def __init__(self, env_step, env_reset, policy, n_envs, obs_dim, act_map, batch_size, max_path_length=1000, discount=0.99, seed=1, env_reset_masked=None,
                 env_id0=None):
        """env_step(actions[N, adim] float64) -> (obs[N, obs_dim], reward[N], done[N] uint8/bool), auto-resetting;
        env_reset() -> obs; env_reset_masked(mask uint8[N]) -> obs with the masked envs reset (used when a path is truncated
        at max_path_length, where rllab's sampler calls env.reset()).  batch_size counts env-steps over ALL ranks, as
        rllab's batch_size does."""
        self.env_step, self.env_reset, self.env_reset_masked = env_step, env_reset, env_reset_masked
        # Host-side lower bound of the Env.steps left before ANY path can reach max_path_length (path_t <= max_path_length -
        # _steps_to_trunc holds for every env): while it is positive no truncation mask can be non-empty, so collect() launches no
        # masked reset at all; when it reaches zero the device-side maximum of path_t re-arms it (one scalar read-back per
        # max_path_length steps at most -- r02 launched the masked-reset kernel on EVERY step once 1000 steps had elapsed).
        self._steps_to_trunc = max_path_length
        self.policy, self.act_map = policy, act_map
        self.n_envs, self.obs_dim = n_envs, obs_dim
        self.horizon = max(1, int(math.ceil(batch_size / (n_envs * _world()))))
        self.max_path_length, self.discount = max_path_length, discount
        dev = next(policy.parameters()).device
        # Exploration noise that does not depend on the number of ranks the envs are sharded over: every rank draws the noise of
        # ALL environments of the job from an identically seeded generator -- one randn kernel per Env.step, 3 M numbers at
        # 512k envs -- and keeps the rows of its own shard [env_id0, env_id0 + n_envs).  (r03 first used a counter-based hash keyed
        # by the global env id, rollout.counter_normal: ~55 elementwise launches per step, a third of the rollout's wall-clock.)
        rank = dist.get_rank() if dist.is_initialized() else 0
        self.seed = seed
        self.env_id0 = rank * n_envs if env_id0 is None else env_id0
        self.n_envs_global = n_envs * _world()
        self.env_ids = torch.arange(n_envs, dtype=torch.int64, device=dev) + self.env_id0
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed * 1000003)
        self.noise_step = 0
        self.obs = None
        self.path_t = torch.zeros(n_envs, dtype=torch.int64, device=dev)
        self.path_ret = torch.zeros(n_envs, dtype=torch.float64, device=dev)
        self.itr = 0

    def _fused_sampler_step(self, dev):
        """The sampler's per-step bookkeeping as one launch (include/cassie_trpo.h: CassieTrpoSamplerStep), or None."""
        if not getattr(self, "fused_sampler_step", True) or dev.type != "cuda" or not available():
            return None
        k = Kernels(dev, entry={"Rows": "CassieTrpoSamplerRows", "Step": "CassieTrpoSamplerStep"})
        n, P = self.n_envs, ptr
        if not hasattr(self, "_book_partial") or self._book_partial.shape[0] != k.fn["Rows"](n):
            self._book_partial = torch.empty((k.fn["Rows"](n), 2), dtype=torch.float64, device=dev)

        def book(rew, done, rew_row, t_row, cut_row):
            assert rew.is_contiguous() and done.is_contiguous() and rew_row.is_contiguous() and t_row.is_contiguous() and cut_row.is_contiguous()
            assert self.path_t.dtype == torch.int64 and self.path_ret.dtype == torch.float64
            k._call("Step", P(rew), P(done), n, ct.c_longlong(int(self.max_path_length)), P(self.path_t), P(self.path_ret), P(rew_row), P(t_row), P(cut_row),
                    P(self._book_partial))
        return book

    def _book_step(self, book, rew, done, rew_row, t_row, cut_row, ep):
        """Clocks, returns, truncation and episode statistics of one Env.step (shared with ddpg.DDPG): this step's rows rew_row / t_row / cut_row
        are written, ep += (finished paths, their summed returns).  Returns (cut, done)."""
        if book is not None and rew.dtype == torch.float64 and done.dtype == torch.uint8:
            # clocks, returns, truncation and episode statistics of this step in ONE launch (CassieTrpoSamplerStep)
            book(rew, done, rew_row, t_row, cut_row)
            ep += self._book_partial.sum(0)
            return cut_row, done
        done = done.bool().clone()
        rew_row[:], t_row[:] = rew, self.path_t
        self.path_ret += rew
        self.path_t += 1
        cut = done | (self.path_t >= self.max_path_length)  # rllab truncates paths at max_path_length
        cut_row[:] = cut
        ep[0] += cut.sum()
        ep[1] += torch.where(cut, self.path_ret, torch.zeros_like(self.path_ret)).sum()
        self.path_ret = torch.where(cut, torch.zeros_like(self.path_ret), self.path_ret)
        self.path_t = torch.where(cut, torch.zeros_like(self.path_t), self.path_t)
        return cut, done

    def _reset_truncated(self, cut, done, nobs):
        """The masked reset of paths cut at max_path_length while their env is alive (armed by _steps_to_trunc); returns the next observation."""
        self._steps_to_trunc -= 1
        if self.env_reset_masked is not None and self._steps_to_trunc <= 0:
            # a path may have been truncated at max_path_length while its env is still alive: rllab resets the env there
            trunc = cut & ~done.bool()
            if bool(trunc.any()):
                nobs = self.env_reset_masked(trunc.to(torch.uint8))
            self._steps_to_trunc = self.max_path_length - int(self.path_t.max())  # re-arm from the oldest live path
        return nobs

    @staticmethod
    def _gather_returns(per_env):
        from . import rollout as R
        from . import trpo   # the timer's slot is trpo.COMM, read at call time: comm._all_reduce_sum says why
        if trpo.COMM is None or _world() == 1:
            return R.gather_returns(per_env)
        box = []
        trpo.COMM.run("returns_all_gather", lambda: box.append(R.gather_returns(per_env)), per_env)
        return box[0]

    # ---- snapshot_mode="last" (trpo_cassie.py:9-19,50; sim_policy.py:19-23): everything a resumed run needs to BE the
    # interrupted run -- policy, baseline, iteration, and per rank the sampler state (action-noise generator, current
    # observation, path clocks/returns) and the resident env state records.  Rank 0 writes `path`, rank r > 0 `path.rank<r>`.
    def _rank_path(self, path):
        r = dist.get_rank() if dist.is_initialized() else 0
        return path if r == 0 else "%s.rank%d" % (path, r)

    def _baseline_coeffs(self):
        """The snapshot's "baseline" entry: an algorithm without a baseline writes None (OnPolicy: the regression's coefficients)."""
        return None

    def _load_baseline_coeffs(self, coeffs, dev):
        """Takes the snapshot's "baseline" entry back (OnPolicy); nothing to take here."""

    def save(self, path, extra=None):
        """Tensors and plain Python values only (loaded with weights_only=True), written to `path.tmp` and renamed into place so
        that a crash during the write never corrupts the one snapshot_mode='last' file."""
        import io
        import os
        env = getattr(self, "env", None)
        if extra is not None:   # `extra` must survive the weights_only load of load(): refuse at save time what could not be read back
            buf = io.BytesIO()
            torch.save(dict(extra=extra), buf)
            buf.seek(0)
            try:
                torch.load(buf, map_location="cpu", weights_only=True)
            except Exception as ex:
                raise TypeError("TRPO.save: `extra` must be tensors / plain Python values (weights_only round trip failed: %r)" % (ex,))
        n_global = self.n_envs * (dist.get_world_size() if dist.is_initialized() else 1)
        coeffs = self._baseline_coeffs()
        ck = dict(n_envs_global=int(n_global), policy={k: v.detach().cpu() for k, v in self.policy.state_dict().items()},
                  baseline=None if coeffs is None else coeffs.detach().cpu(), itr=int(self.itr), extra=extra,
                  noise_step=int(self.noise_step), noise_seed=int(self.seed), gen_state=self.gen.get_state(), obs=None if self.obs is None else self.obs.cpu(),
                  path_t=self.path_t.cpu(), path_ret=self.path_ret.cpu(), steps_to_trunc=int(self._steps_to_trunc),
                  env_state=None if env is None or not hasattr(env, "get_full_state_host") else torch.from_numpy(env.get_full_state_host()),
                  terrain=terrain_lib.spec_key(getattr(self, "terrain_spec", None)), **self._env_family_fields())
        ck.update(self._snapshot_fields())
        mine = self._rank_path(path)
        torch.save(ck, mine + ".tmp")
        os.replace(mine + ".tmp", mine)

    def _env_family_fields(self):
        """The environment family of the run -- "cassie2d" (also: no make_cassie_algo, as the CPU tests' toy environments) or "cassie3d", then
        with what Cassie3dVecEnv was configured with (make_cassie_algo sets env_family / env_config)."""
        return dict(env_family=getattr(self, "env_family", "cassie2d"), env_config=getattr(self, "env_config", None))

    def _check_env_family(self, ck):
        """A snapshot continues on the family (and, for Cassie3d, the control mode and gains) it was written on; one written before the
        entry existed is Cassie2d's."""
        name, mine, theirs = type(self).__name__, self._env_family_fields(), dict(env_family=ck.get("env_family", "cassie2d"), env_config=ck.get("env_config"))
        if theirs["env_family"] != mine["env_family"]:
            raise ValueError("%s.load: the snapshot was written on %s, this run is on %s" % (name, theirs["env_family"], mine["env_family"]))
        if theirs["env_config"] != mine["env_config"]:
            raise ValueError("%s.load: the snapshot's %s was configured with %r, this run's with %r" % (name, mine["env_family"], theirs["env_config"], mine["env_config"]))

    @property
    def hidden_sizes(self):
        return hidden_sizes_of(self.policy)

    def _snapshot_fields(self):
        """Entries of the snapshot beyond the common ones: the algorithm (but for TRPO itself) and the policy's hidden sizes; a subclass adds
        its hyper-parameters and optimiser state."""
        return dict({} if self.ALGO == "trpo" else dict(algo=self.ALGO), hidden_sizes=list(self.hidden_sizes))

    def _load_fields(self, ck):
        """Called with the loaded snapshot before anything is restored: refuses a snapshot that is not this run's (a subclass also takes
        back its _snapshot_fields()).  A plain TRPO run continues any GaussianMLPPolicy snapshot (its own, VPG's, PPO's, ES's) but not the
        deterministic / squashed-Gaussian actors of ddpg, sac and td3; every other algorithm takes back only its own.  The policy's hidden
        sizes must match (a snapshot without them was written by a 32 x 32 run)."""
        name, algo = type(self).__name__, ck.get("algo", "trpo")
        if algo != self.ALGO and (self.ALGO != "trpo" or algo in ("ddpg", "sac", "td3")):
            raise ValueError("%s.load: the snapshot was written by %s, this run is %s" % (name, algo, self.ALGO))
        theirs, mine = tuple(ck.get("hidden_sizes", (32, 32))), self.hidden_sizes
        if theirs != mine:
            raise ValueError("%s.load: the snapshot's policy has hidden sizes %r, this run's has %r" % (name, theirs, mine))

    def load(self, path, restore_sampler=True):
        """Returns (extra, sampler_restored): policy / baseline / iteration always come back; the sampler state (env records,
        noise counter, observation, path clocks) only from this rank's own file with a matching batch shape -- the second value
        says whether that happened, so a run that merely LOOKS resumed can be told from the interrupted run continued."""
        import os
        dev = next(self.policy.parameters()).device
        mine = self._rank_path(path)
        ck = torch.load(mine if os.path.exists(mine) else path, map_location="cpu", weights_only=True)
        self._load_fields(ck)
        self._check_env_family(ck)
        # the ground is part of the run: resuming on other terrain would silently be a different run (snapshots without the key: flat floor)
        mine_spec, theirs = terrain_lib.spec_key(getattr(self, "terrain_spec", None)), ck.get("terrain")
        if mine_spec != theirs:
            raise ValueError("TRPO.load: the snapshot was written on terrain %r, this job runs on %r" % (theirs, mine_spec))
        self.policy.load_state_dict(ck["policy"])
        self._load_baseline_coeffs(ck["baseline"], dev)
        self.itr = ck["itr"]
        env = getattr(self, "env", None)
        restored = False
        n_global = self.n_envs * (dist.get_world_size() if dist.is_initialized() else 1)
        # the sampler comes back only if the snapshot carries all of it and was written by a job of the same shape: the noise stream is
        # drawn over the job's GLOBAL env range, so a different world size would silently change it (snapshots written before the
        # noise counter existed have no "noise_step": policy / baseline only, restored = False)
        complete = all(k in ck for k in ("noise_step", "obs", "path_t", "path_ret")) and ck.get("n_envs_global", n_global) == n_global
        if restore_sampler and complete and os.path.exists(mine) and ck.get("env_state") is not None and env is not None \
                and tuple(ck["env_state"].shape) == (self.n_envs, getattr(env, "FULL_STATE_WIDTH", 88)):   # (88: the Cassie2d record)
            env.set_full_state_host(ck["env_state"].numpy())
            self.noise_step, self.seed = ck["noise_step"], ck.get("noise_seed", self.seed)
            if ck.get("gen_state") is not None:
                self.gen.set_state(ck["gen_state"])
            self.obs = None if ck["obs"] is None else ck["obs"].to(dev)
            self.path_t, self.path_ret = ck["path_t"].to(dev), ck["path_ret"].to(dev)
            self._steps_to_trunc = ck.get("steps_to_trunc", 0)
            restored = True
        self.sampler_restored = restored
        return ck.get("extra"), restored


class OnPolicy(Sampler):
    """Deviations from rllab's batch sampler, on purpose: paths cut by the end of the batch are bootstrapped with the baseline's
    value of the next observation (rllab's batch sampler discards/truncates the tail instead; with 65 536 envs x few steps
    per iteration nearly every path is cut, so dropping the tail would bias every return); the policy runs in float32.
    A subclass supplies optimize(processed batch) -> the iteration's statistics."""

    def __init__(self, env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size, max_path_length=1000, discount=0.99, seed=1,
                 env_reset_masked=None, env_id0=None):
        super().__init__(env_step, env_reset, policy, n_envs, obs_dim, act_map, batch_size, max_path_length, discount, seed, env_reset_masked, env_id0)
        self.baseline = baseline

    def _baseline_coeffs(self):
        return self.baseline.coeffs

    def _load_baseline_coeffs(self, coeffs, dev):
        self.baseline.coeffs = None if coeffs is None else coeffs.to(dev)

    def _fused_policy_step(self, dev, pol_dtype):
        """The fused policy-step launcher (include/cassie_trpo.h: CassieTrpoPolicyStep for 32 x 32 hidden units, CassiePgPolicyStep for
        128 x 128) when it applies -- CUDA, float32 two-layer tanh policy of a supported shape, rllab's normalize() action map -- else None
        (the torch operations below)."""
        if not getattr(self, "fused_policy_step", True) or dev.type != "cuda" or pol_dtype != torch.float32 or not isinstance(self.act_map, NormalizedActions):
            return None
        lin = _two_layer_tanh(self.policy)
        if lin is None:
            return None
        D, A = lin[0].in_features, lin[2].out_features
        hs = (lin[0].out_features, lin[1].out_features)
        if (D, A) == (45, 10):   # Cassie3d: the width-128 kernel of csrc/tu_pg3d.hip
            entry = "CassiePg3dPolicyStep" if hs == (128, 128) else None
        else:
            entry = {(32, 32): "CassieTrpoPolicyStep", (128, 128): "CassiePgPolicyStep"}.get(hs) if (D, A) in ((26, 6), (26, 7)) else None
        if entry is None or self.obs_dim != D or not available(entry):
            return None
        if not hasattr(self, "_env_actions") or self._env_actions.shape != (self.n_envs, A):
            self._env_actions = torch.empty((self.n_envs, A), dtype=torch.float64, device=dev)
        P = ptr
        w = [P(lin[0].weight), P(lin[0].bias), P(lin[1].weight), P(lin[1].bias), P(lin[2].weight), P(lin[2].bias), P(self.policy.log_std)]
        low, high, n = self.act_map.low, self.act_map.high, self.n_envs
        # the kernel reads the bounds as `const double*`: anything else (NormalizedActions takes a dtype) goes the torch way
        if not all(t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == A for t in (low, high)):
            return None
        k = Kernels(dev, entry={"PolicyStep": entry})
        self.policy_step_entry = entry

        def step(obs, noise, obs32, mean, act):
            if obs.dtype != torch.float64 or not obs.is_contiguous():
                raise TypeError("%s: observations must be a contiguous float64 tensor (got %s)" % (entry, obs.dtype))
            assert noise.is_contiguous() and obs32.is_contiguous()
            k._call("PolicyStep", P(obs), n, D, A, *w, P(noise), P(low), P(high), P(obs32), P(mean), P(act), P(self._env_actions))
        return step

    # ---- sampling: T vectorised Env.steps, everything stays on the device
    @torch.no_grad()
    def collect(self):
        from . import rollout as R
        pol_dtype = next(self.policy.parameters()).dtype
        if self.obs is None:
            self.obs = self.env_reset().clone()
        T, N = self.horizon, self.n_envs
        dev = self.obs.device
        obs_b = torch.empty((T, N, self.obs_dim), dtype=pol_dtype, device=dev)
        act_b = torch.empty((T, N, self.policy.log_std.numel()), dtype=pol_dtype, device=dev)
        mean_b, lstd_b = torch.empty_like(act_b), torch.empty_like(act_b)
        rew_b = torch.empty((T, N), dtype=torch.float64, device=dev)
        done_b = torch.empty((T, N), dtype=torch.bool, device=dev)
        t_b = torch.empty((T, N), dtype=torch.int64, device=dev)
        ep = torch.zeros(2, dtype=torch.float64, device=dev)   # finished episodes / their summed returns, kept on the device:
        fused = self._fused_policy_step(dev, pol_dtype)          # boolean-mask indexing would synchronise every step
        book = self._fused_sampler_step(dev) if fused is not None else None
        if fused is not None:
            lstd_b[:] = self.policy.log_std.detach()
        for t in range(T):
            noise = torch.randn((self.n_envs_global, self.policy.log_std.numel()), dtype=pol_dtype, device=dev,
                                generator=self.gen)[self.env_id0:self.env_id0 + N]
            self.noise_step += 1
            if fused is not None:
                # float32 view of the observation, mean network, noise and the normalize() action map in ONE launch (csrc/tu_trpo.hip),
                # written straight into this step's rows of the batch buffers
                fused(self.obs, noise, obs_b[t], mean_b[t], act_b[t])
                nobs, rew, done = self.env_step(self._env_actions)
            else:
                o = self.obs.to(pol_dtype)
                a, mean, log_std = self.policy.get_actions(o, noise=noise)
                nobs, rew, done = self.env_step(self.act_map(a))
                obs_b[t], act_b[t], mean_b[t], lstd_b[t] = o, a, mean, log_std
            cut, done = self._book_step(book, rew, done, rew_b[t], t_b[t], done_b[t], ep)
            nobs = self._reset_truncated(cut, done, nobs)
            self.obs = nobs.clone()
        return dict(obs=obs_b, act=act_b, mean=mean_b, log_std=lstd_b, rew=rew_b, done=done_b, t=t_b,
                    episode_count=ep[0], episode_return_sum=ep[1])

    def _baseline_kernels(self, obs):
        """BaselineKernels for this batch (float32 CUDA observations of a supported width, LinearFeatureBaseline) or None."""
        if not getattr(self, "fused_baseline", True) or not obs.is_cuda or obs.dtype != torch.float32 or type(self.baseline) is not LinearFeatureBaseline:
            return None
        bk = getattr(self, "_bk", None)
        if bk is None or bk.D != obs.shape[-1] or bk.dev != obs.device:
            try:
                bk = BaselineKernels(obs.device, obs.shape[-1])
            except (ValueError, OSError):
                bk = None
            self._bk = bk
        return bk

    def _advantages(self, bk, batch, obs, tt):
        """process()'s hook: (returns [T, N], advantages [T, N], [sum adv, sum adv^2] or None for process to take them) of the batch.  bk: the
        BaselineKernels or None (the torch statements); obs, tt: the flat views.  TRPO: gae_lambda = 1; unfinished paths are bootstrapped
        with the baseline of the next observation (0 at iteration 0)."""
        T, N = batch["rew"].shape
        if bk is not None:
            # value of every sample, return-to-go and advantage in one pass over the batch (csrc/tu_trpo_baseline.hip)
            coeffs = self.baseline.coeffs
            last_v = None if coeffs is None else bk.predict(self.obs.to(obs.dtype), self.path_t, coeffs)
            return bk.returns_advantages(batch["obs"], batch["t"], batch["rew"], batch["done"], coeffs, last_v, self.discount)
        last_v = self.baseline.predict(self.obs.to(obs.dtype), self.path_t)
        returns = discounted_returns(batch["rew"], batch["done"], self.discount, last_v)
        return returns, returns - self.baseline.predict(obs, tt).view(T, N), None

    def process(self, batch):
        T, N = batch["rew"].shape
        flat = lambda x: x.reshape(T * N, *x.shape[2:])
        obs, tt = flat(batch["obs"]), flat(batch["t"])
        bk = self._baseline_kernels(obs)
        returns, adv, sums = self._advantages(bk, batch, obs, tt)
        adv = flat(adv)
        if sums is None:
            sums = torch.stack([adv.sum(), (adv * adv).sum()])
        n = torch.tensor([adv.numel()], dtype=torch.float64, device=adv.device)
        s12 = all_sum_(sums.clone(), "advantage_all_reduce"); n = all_sum_(n, "advantage_all_reduce")
        mean = s12[0] / n
        std = (s12[1] / n - mean * mean).clamp_min(0).sqrt()
        adv = ((adv - mean) / (std + 1e-8)).to(obs.dtype)  # center_adv
        if bk is not None:
            # the regression's normal equations on the FP64 matrix cores: no feature matrix in memory
            A, b = bk.gram(obs, tt, flat(returns))
            self.baseline.fit_normal_equations(A, b, bk.ridge_solve if getattr(self, "fused_solve", True) else None)
        else:
            self.baseline.fit(obs, tt, flat(returns))
        return dict(obs=obs, act=flat(batch["act"]), mean=flat(batch["mean"]), log_std=flat(batch["log_std"]), adv=adv, **self._processed_extras())

    def _processed_extras(self):
        """process()'s hook: further entries of the processed batch (PPO with a value network: its value targets); none by default."""
        return {}

    def train_iteration(self):
        from . import rollout as R
        timing = getattr(self, "timing", False)  # synchronising timers: rollout (policy forward + Env.step) vs TRPO update
        if timing:
            import time
            torch.cuda.synchronize(); t0 = time.perf_counter()
        batch = self.collect()
        if timing:
            torch.cuda.synchronize(); t1 = time.perf_counter()
        stats = self.optimize(self.process(batch))
        if timing:
            torch.cuda.synchronize(); t2 = time.perf_counter()
            stats.update(seconds_rollout=t1 - t0, seconds_update=t2 - t1)
        cnt = all_sum_(torch.stack([batch["episode_count"], batch["episode_return_sum"]]), "stats_all_reduce")
        per_env = batch["rew"].sum(0)                       # the one gather of the rollout batch (N per rank)
        stats.update(itr=self.itr, env_steps=batch["rew"].numel() * _world(), episodes=int(cnt[0]),
                     avg_return=float(cnt[1] / cnt[0]) if cnt[0] > 0 else float("nan"),
                     avg_reward=float(all_mean_(batch["rew"].mean().view(1).clone(), "stats_all_reduce")),
                     gathered=int(self._gather_returns(per_env).numel()))
        self.itr += 1
        return stats


def broadcast_initial_policy(algo):
    """Rank 0's initial parameters are authoritative (a collective: every rank must call it)."""
    if dist.is_initialized() and dist.get_world_size() > 1:
        theta = flat_params(algo.policy)
        dist.broadcast(theta, 0)
        set_flat_params(algo.policy, theta)


def make_cassie_algo(cls, make_nets, broadcast, n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, terrain=None, sync_policy=True,
                     terrain_ids=None, env="cassie2d", kp=10.0, kd=5.0, **kw):
    """cls on the batched MI355X environment: what every make_cassie_* is.  env: the environment family -- "cassie2d" (CassieVecEnv: kind, trajectory,
    terrain) or "cassie3d" (Cassie3dVecEnv(n_envs, control_mode, kp, kd): standing reset, 45 observations, 10 actions; no terrain, gait or kind, and
    only for an algorithm with CASSIE3D set -- PPO, SAC and ES; the others refuse rather than run untested on their torch paths).  make_nets(obs_dim, act_dim, dev) -> the constructor's arguments between
    env_reset and n_envs (the policy first), built right after torch.manual_seed(seed): every rank builds the same initial networks, and with
    sync_policy `broadcast(algo)` makes rank 0's authoritative anyway.  sync_policy=False: NOTHING collective happens in here (the env, its
    workspaces, the networks are local allocations that can fail on one rank alone); the caller agrees on success across ranks first and then
    broadcasts (bench.py's TRPO stage).  terrain: None (the flat floor) or a spec of terrain.terrain_spec -- every environment on its own field of
    the spec's library, drawn by terrain.assign_terrains over terrain_ids(the GLOBAL env ids) (default: the ids themselves); snapshots record it."""
    if env not in ("cassie2d", "cassie3d"):
        raise ValueError("make_cassie_algo: env must be 'cassie2d' or 'cassie3d', got %r" % (env,))
    family, env_config = env, None
    if family == "cassie3d":   # (checked before any device is touched)
        if not cls.CASSIE3D:
            raise ValueError("%s does not run on env='cassie3d': PPO (ppo.make_cassie_ppo), SAC (sac.make_cassie_sac) and ES (es.make_cassie_es) are the algorithms built for the 45 x 10 shape" % cls.__name__)
        if terrain is not None or trajectory is not None or kind != "walk":
            raise ValueError("env='cassie3d' has no terrain, reference gait or kind (got terrain=%r, trajectory %s, kind=%r): it is the standing-reset Cassie3d"
                             % (terrain, "given" if trajectory is not None else "None", kind))
        if control_mode not in ("PD", "Torque"):
            raise ValueError("env='cassie3d' has the control modes 'PD' and 'Torque', not %r" % (control_mode,))
        import numpy as np
        from .vec_env3d import NU, Cassie3dVecEnv
        env_config = dict(control_mode=control_mode, kp=np.broadcast_to(np.asarray(kp, dtype=np.float64), (NU,)).tolist(),
                          kd=np.broadcast_to(np.asarray(kd, dtype=np.float64), (NU,)).tolist())
        env = Cassie3dVecEnv(n_envs, control_mode=control_mode, n_substeps=10, auto_reset=True, kp=kp, kd=kd, device=device)
    else:
        from .vec_env import CassieVecEnv
        env = CassieVecEnv(n_envs, kind=kind, control_mode=control_mode, n_substeps=10, auto_reset=True, device=device, trajectory=trajectory)
    env.use_torch_stream()
    dev = "cuda:%d" % device
    bufs = env.alloc()
    torch.manual_seed(seed)  # trpo_cassie.py:53 seed=1
    obs_w = env.observation_space.shape[0]  # what step() emits (26 for both kinds); the networks are sized from the env, as trpo_cassie.py does through env.spec
    nets = make_nets(obs_w, env.adim if family == "cassie2d" else len(env.action_space.low), dev)
    act_map = NormalizedActions(env.action_space.low, env.action_space.high, dev)
    algo = cls(lambda a: env.step(a, bufs), lambda: env.reset(bufs), *nets, n_envs, obs_w, act_map, seed=seed, env_reset_masked=lambda m: env.reset(bufs, mask=m), **kw)
    algo.env = env
    algo.env_family, algo.env_config = family, env_config
    algo.terrain_spec = terrain
    if terrain is not None:
        ids = algo.env_ids if terrain_ids is None else terrain_ids(algo.env_ids)
        env.set_terrain_library(terrain_lib.library_of_spec(terrain), terrain_lib.DEFAULT_SIZE[:2])
        env.set_terrain_ids(terrain_lib.assign_terrains(terrain["seed"], ids, len(terrain["files"])).to(dev))
    if sync_policy:
        broadcast(algo)
    return algo


def gaussian_policy_nets(hidden_sizes, init_std):
    """make_nets of the on-policy family: a GaussianMLPPolicy and a LinearFeatureBaseline."""
    return lambda obs_dim, act_dim, dev: (GaussianMLPPolicy(obs_dim, act_dim, tuple(hidden_sizes), init_std=init_std).to(dev), LinearFeatureBaseline())
