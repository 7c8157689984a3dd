"""DDPG (cassierl_amd/ddpg.py, counterpart of rllab/envs/ddpg_cassie.py) on CPU: the networks, the OU strategy, the replay pool, the torch statement
of the update against an independent autograd statement, rllab's schedule at N = 1, learning on a toy env, the world-size-2 (gloo) run, snapshot /
resume and the refusal of foreign snapshots."""
import copy
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cassierl_amd import ddpg as G
from cassierl_amd import trpo as T
from cassierl_amd import vpg as V
from test_trpo_cpu import SnapshotToyEnv, ToyVecEnv

AMAP = lambda: T.NormalizedActions([-1, -1], [1, 1], "cpu")


def test_network_shapes_counts_and_initial_ranges():
    torch.manual_seed(0)
    pol, qf = G.DeterministicMLPPolicy(26, 6), G.ContinuousMLPQFunction(26, 6)
    assert [tuple(p.shape) for p in pol.parameters()] == [(32, 26), (32,), (32, 32), (32,), (6, 32), (6,)]
    assert [tuple(p.shape) for p in qf.parameters()] == [(32, 26), (32,), (32, 38), (32,), (1, 32), (1,)]
    assert sum(p.numel() for p in pol.parameters()) == 2118 and sum(p.numel() for p in qf.parameters()) == 2145
    for net in (pol, qf):
        for lin in (net.l1, net.l2):
            b = math.sqrt(6.0 / lin.in_features)
            assert lin.weight.abs().max().item() <= b and lin.weight.abs().max().item() > 0.8 * b and (lin.bias == 0).all()
        assert net.l3.weight.abs().max().item() <= 3e-3 and net.l3.bias.abs().max().item() <= 3e-3 and net.l3.weight.abs().max().item() > 0
    obs, a1, a2 = torch.randn(5, 26), torch.rand(5, 6) * 2 - 1, torch.rand(5, 6) * 2 - 1
    assert pol(obs).shape == (5, 6) and pol(obs).abs().max().item() < 1 and qf(obs, a1).shape == (5,)
    # the action enters at layer 2: h1 does not see it, q does
    assert torch.equal(qf.first_hidden(obs), torch.relu(qf.l1(obs)))
    assert not torch.equal(qf(obs, a1), qf(obs, a2))
    h2 = torch.relu(qf.l2(torch.cat([qf.first_hidden(obs), a1], 1)))
    assert torch.equal(qf(obs, a1), qf.l3(h2).squeeze(-1))


def test_ou_recurrence_reset_and_clipping():
    rng = np.random.default_rng(0)
    n, A, theta, sigma, mu = 3, 2, 0.15, 0.3, 0.0
    noise = rng.normal(size=(10, n, A))
    fresh = np.zeros((10, n), dtype=bool)
    fresh[0] = True; fresh[4, 1] = True; fresh[7, 2] = True
    x = np.full((n, A), 5.0)   # overwritten by the path start at step 0
    ref = []
    for t in range(10):
        x = np.where(fresh[t][:, None], mu, x)
        x = x + theta * (mu - x) + sigma * noise[t]
        ref.append(x.copy())
    ou = G.OUStrategy(n, A, dtype=torch.float64)
    ou.state = torch.full((n, A), 5.0, dtype=torch.float64)
    for t in range(10):
        got = ou.evolve(torch.tensor(noise[t]), torch.tensor(fresh[t]))
        np.testing.assert_allclose(got.numpy(), ref[t], rtol=0, atol=1e-15)
    act = ou.get_action(torch.full((n, A), 0.95, dtype=torch.float64), torch.tensor(noise[0]) * 10)
    assert act.min().item() >= -1 and act.max().item() <= 1 and (act.abs() == 1).any()
    assert (G.OUStrategy(2, 2).theta, G.OUStrategy(2, 2).sigma, G.OUStrategy(2, 2).mu) == (0.15, 0.3, 0.0)


def test_pool_append_order_wrap_and_saturation():
    with pytest.raises(ValueError, match="multiple"):
        G.ReplayPool(10, 4, 3, 2)
    pool = G.ReplayPool(12, 4, 3, 2, dtype=torch.float64)
    assert G.ReplayPool.BYTES_PER_ROW(26, 6) == 240
    for k in range(4):
        base = 100.0 * k + torch.arange(4, dtype=torch.float64)
        top = pool.top
        pool.append(base[:, None].expand(4, 3), -base[:, None].expand(4, 2), base + 0.5, (torch.arange(4) % 2 == 0), base[:, None].expand(4, 3) + 0.25)
        assert top == (4 * k) % 12 and pool.top == (4 * (k + 1)) % 12 and pool.size == min(4 * (k + 1), 12)
        assert torch.equal(pool.obs[top:top + 4, 0], base) and torch.equal(pool.act[top:top + 4, 1], -base)   # environment i at top + i
        assert torch.equal(pool.rew[top:top + 4], base + 0.5) and torch.equal(pool.nobs[top:top + 4, 2], base + 0.25)
        assert pool.term[top:top + 4].tolist() == [1.0, 0.0, 1.0, 0.0]
    assert pool.obs[0, 0].item() == 300.0 and pool.obs[4, 0].item() == 100.0   # the fourth append wrapped onto the first
    s, a, r, term, s2 = pool.sample(torch.tensor([5, 5, 0]))
    assert s[:, 0].tolist() == [101.0, 101.0, 300.0] and r.tolist() == [101.5, 101.5, 300.5]


class _ClockEnv:
    """obs = (env id, steps since reset, 0, 1); env 0 is done at every 3rd step of its episode; masked resets restart the clock."""

    def __init__(self, n):
        self.n, self.t = n, torch.zeros(n, dtype=torch.float64)

    def _obs(self):
        return torch.stack([torch.arange(self.n, dtype=torch.float64), self.t, torch.zeros(self.n, dtype=torch.float64), torch.ones(self.n, dtype=torch.float64)], 1)

    def reset(self, mask=None):
        self.t = torch.zeros(self.n, dtype=torch.float64) if mask is None else torch.where(mask.bool(), torch.zeros_like(self.t), self.t)
        return self._obs()

    def step(self, a):
        self.t = self.t + 1
        done = (self.t >= 3) & (torch.arange(self.n) == 0)
        self.t = torch.where(done, torch.zeros_like(self.t), self.t)   # auto-reset
        return self._obs(), torch.ones(self.n, dtype=torch.float64), done.to(torch.uint8)


def test_truncated_path_keeps_its_next_observation_and_a_done_is_terminal():
    env = _ClockEnv(2)
    torch.manual_seed(0)
    algo = G.DDPG(env.step, env.reset, G.DeterministicMLPPolicy(4, 2, dtype=torch.float64), G.ContinuousMLPQFunction(4, 2, dtype=torch.float64), 2, 4, AMAP(),
                  batch_size=2, max_path_length=5, min_pool_size=10 ** 9, replay_pool_size=40, scale_reward=0.01, env_reset_masked=lambda m: env.reset(m))
    for _ in range(6):
        algo.train_step()
    pool = algo.pool
    clock = lambda rows: pool.obs[rows, 1].tolist()
    # env 1 (rows 1, 3, 5, ...): never done; its path is cut at step 5 -> terminal 0, s' = the observation Env.step returned (clock 5), and the
    # row after it starts from the masked reset (clock 0)
    assert clock([1, 3, 5, 7, 9, 11]) == [0.0, 1.0, 2.0, 3.0, 4.0, 0.0]
    assert pool.term[[1, 3, 5, 7, 9, 11]].tolist() == [0.0] * 6
    assert pool.nobs[9, 1].item() == 5.0 and pool.nobs[9, 0].item() == 1.0
    # env 0: done at its 3rd step -> terminal 1, s' is what the auto-reset returned (clock 0)
    assert pool.term[[0, 2, 4, 6, 8, 10]].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    assert pool.nobs[4, 1].item() == 0.0 and clock([6]) == [0.0]
    assert torch.allclose(pool.rew[:12], torch.full((12,), 0.01, dtype=torch.float64))   # scale_reward * r
    assert pool.act[:12].abs().max().item() <= 1.0


# ---- the update
def _fresh(seed, D=5, A=3):
    torch.manual_seed(seed)
    nets = [G.DeterministicMLPPolicy(D, A, dtype=torch.float64), G.ContinuousMLPQFunction(D, A, dtype=torch.float64)]
    with torch.no_grad():
        for net in nets:
            net.l3.weight.uniform_(-0.5, 0.5)
            for lin in (net.l1, net.l2):
                lin.bias.normal_(0, 0.1)
    tg = [copy.deepcopy(n) for n in nets]
    with torch.no_grad():
        for net in tg:
            for p in net.parameters():
                p.add_(0.05 * torch.randn_like(p))
    return nets + tg


def _independent_update(pol, qf, tpol, tqf, st, batch, gamma, qf_lr, pol_lr, tau, old_critic_for_actor=False):
    """The issue's update written against autograd and nn.Module copies: y, critic loss, Adam; actor loss through the NEW critic, Adam; soft updates."""
    s, a, r, term, s2 = batch
    y = (r + (1 - term) * gamma * tqf(s2, tpol(s2))).detach()
    critic_for_actor = copy.deepcopy(qf) if old_critic_for_actor else qf
    qf.zero_grad()
    ((qf(s, a) - y) ** 2).mean().backward()
    th = T.flat_params(qf)
    st["tq"] += 1
    V.adam_step_(th, torch.cat([p.grad.reshape(-1) for p in qf.parameters()]), st["mq"], st["vq"], st["tq"], qf_lr)
    T.set_flat_params(qf, th)
    pol.zero_grad()
    (-critic_for_actor(s, pol(s)).mean()).backward()
    th = T.flat_params(pol)
    st["tp"] += 1
    V.adam_step_(th, torch.cat([p.grad.reshape(-1) for p in pol.parameters()]), st["mp"], st["vp"], st["tp"], pol_lr)
    T.set_flat_params(pol, th)
    with torch.no_grad():
        for tgt, live in ((tpol, pol), (tqf, qf)):
            for pt, p in zip(tgt.parameters(), live.parameters()):
                pt.copy_((1 - tau) * pt + tau * p)


def test_update_statement_matches_an_independent_autograd_statement():
    nets = _fresh(1)
    mine, ref, wrong = [copy.deepcopy(n) for n in nets], [copy.deepcopy(n) for n in nets], [copy.deepcopy(n) for n in nets]
    adam_mu, adam_q = G.new_adam(mine[0]), G.new_adam(mine[1])
    z = lambda n: torch.zeros(n, dtype=torch.float64)
    st = [dict(tq=0, tp=0, mq=z(T.flat_params(nets[1]).numel()), vq=z(T.flat_params(nets[1]).numel()), mp=z(T.flat_params(nets[0]).numel()),
               vp=z(T.flat_params(nets[0]).numel())) for _ in range(2)]
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        n = 40
        batch = (torch.randn(n, 5, dtype=torch.float64, generator=g), torch.rand(n, 3, dtype=torch.float64, generator=g) * 2 - 1,
                 torch.randn(n, dtype=torch.float64, generator=g), (torch.rand(n, generator=g) < 0.3).double(), torch.randn(n, 5, dtype=torch.float64, generator=g))
        loss, surr, q = G.ddpg_update_torch_(mine[0], mine[1], mine[2], mine[3], adam_mu, adam_q, batch, 0.97, 1e-2, 1e-3, 0.05)
        assert loss.item() > 0 and math.isfinite(surr.item()) and math.isfinite(q.item())
        _independent_update(*ref, st[0], batch, 0.97, 1e-2, 1e-3, 0.05)
        _independent_update(*wrong, st[1], batch, 0.97, 1e-2, 1e-3, 0.05, old_critic_for_actor=True)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    for a, b in zip(mine, ref):
        assert rel(T.flat_params(a), T.flat_params(b)) < 1e-12
    for a, b in ((adam_mu["m"], st[0]["mp"]), (adam_mu["v"], st[0]["vp"]), (adam_q["m"], st[0]["mq"]), (adam_q["v"], st[0]["vq"])):
        assert rel(a, b) < 1e-12
    assert adam_mu["t"] == adam_q["t"] == 3
    # the order matters: an actor step through the critic BEFORE its step gives another actor
    assert rel(T.flat_params(mine[0]), T.flat_params(wrong[0])) > 1e-6


def test_one_environment_with_the_defaults_runs_rllabs_schedule():
    env = ToyVecEnv(1, 0)
    torch.manual_seed(0)
    algo = G.DDPG(env.step, env.reset, G.DeterministicMLPPolicy(4, 2, dtype=torch.float64), G.ContinuousMLPQFunction(4, 2, dtype=torch.float64), 1, 4, AMAP(),
                  replay_pool_size=G.default_pool_size(1))
    assert (algo.batch_size, algo.max_path_length, algo.epoch_length, algo.min_pool_size, algo.discount, algo.scale_reward, algo.qf_learning_rate,
            algo.policy_learning_rate, algo.tau, algo.updates_per_step, algo.pool.capacity) == (32, 100, 1000, 10000, 0.99, 0.01, 1e-3, 1e-4, 1e-3, 1, 1000000)
    algo.min_pool_size = 50   # the schedule, not the 10 000 steps
    seen = []
    real = algo.update
    algo.update = lambda idx: (seen.append(idx.clone()), real(idx))
    ran = [algo.train_step() for _ in range(60)]
    assert ran == [0] * 49 + [1] * 11 and len(seen) == 11 and algo.n_updates == 11
    for k, idx in enumerate(seen):
        assert idx.shape == (32,) and idx.dtype == torch.int64 and idx.min().item() >= 0 and idx.max().item() < 50 + k
    assert algo.last_update_kind == "torch"
    assert G.default_pool_size(65536) == 16 * 65536 and G.default_pool_size(4096) % 4096 == 0 and G.default_pool_size(4096) >= 1000000


class _BanditEnv:
    """One step per path: obs = (s0, s1, 0, 1) drawn afresh, reward = -(a0 - c s0)^2."""

    def __init__(self, n, seed, c=0.8):
        self.n, self.c, self.g = n, c, torch.Generator().manual_seed(seed)
        self.reset()

    def reset(self):
        self.s = torch.rand(self.n, 2, generator=self.g, dtype=torch.float64) * 2 - 1
        return torch.cat([self.s, torch.zeros(self.n, 1, dtype=torch.float64), torch.ones(self.n, 1, dtype=torch.float64)], 1)

    def step(self, a):
        r = -(a[:, 0].clamp(-1, 1) - self.c * self.s[:, 0]) ** 2
        return self.reset(), r, torch.ones(self.n, dtype=torch.uint8)


def test_ddpg_improves_reward_on_toy_env():
    env = _BanditEnv(64, 3)
    torch.manual_seed(3)
    algo = G.DDPG(env.step, env.reset, G.DeterministicMLPPolicy(4, 2, dtype=torch.float64), G.ContinuousMLPQFunction(4, 2, dtype=torch.float64), 64, 4, AMAP(),
                  batch_size=64, max_path_length=100, epoch_length=25, min_pool_size=64, replay_pool_size=64 * 50, scale_reward=1.0, qf_learning_rate=1e-2,
                  policy_learning_rate=1e-3, soft_target_tau=0.05, ou_sigma=0.2, seed=3)

    def policy_reward():   # mean reward of mu(s), without exploration noise
        g = torch.Generator().manual_seed(11)
        s = torch.rand(4096, 2, generator=g, dtype=torch.float64) * 2 - 1
        o = torch.cat([s, torch.zeros(4096, 1, dtype=torch.float64), torch.ones(4096, 1, dtype=torch.float64)], 1)
        with torch.no_grad():
            return -((algo.policy(o)[:, 0] - 0.8 * s[:, 0]) ** 2).mean().item()

    first = policy_reward()
    for _ in range(40):
        last = algo.train_iteration()
    for k in ("itr", "env_steps", "updates", "pool_size", "avg_reward", "episodes", "avg_return", "qf_loss", "policy_surr", "avg_q", "update_kind"):
        assert k in last
    assert last["env_steps"] == 64 * 25 and last["updates"] == 25 and last["pool_size"] == 64 * 50 and last["episodes"] == 64 * 25
    after = policy_reward()
    assert after > first + 0.05, (first, after)


# ---- data-parallel: identical parameters on both ranks, equal to a one-process emulation of the two shards
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _shard_batch(rank, k, n=24, D=5, A=3):
    g = torch.Generator().manual_seed(1000 * rank + k)
    return (torch.randn(n, D, dtype=torch.float64, generator=g), torch.rand(n, A, dtype=torch.float64, generator=g) * 2 - 1,
            torch.randn(n, dtype=torch.float64, generator=g), (torch.rand(n, generator=g) < 0.3).double(), torch.randn(n, D, dtype=torch.float64, generator=g))


def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nets = _fresh(7)
    adam_mu, adam_q = G.new_adam(nets[0]), G.new_adam(nets[1])
    for k in range(5):
        G.ddpg_update_torch_(*nets, adam_mu, adam_q, _shard_batch(rank, k), 0.97, 1e-2, 1e-3, 0.05)
    q.put((rank, [T.flat_params(n).numpy() for n in nets]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_process_ddpg_keeps_identical_parameters_and_equals_the_emulation():
    # one process: both shards' gradients, averaged, then the same Adam steps and soft updates
    nets = _fresh(7)
    pol, qf, tpol, tqf = nets
    adam_mu, adam_q = G.new_adam(pol), G.new_adam(qf)
    for k in range(5):
        shards = [_shard_batch(r, k) for r in range(2)]
        gq = 0
        for s, a, r, term, s2 in shards:
            with torch.no_grad():
                y = r + (1 - term) * 0.97 * tqf(s2, tpol(s2))
            gq = gq + T.flat_grad(((qf(s, a) - y) ** 2).mean(), qf) / 2
        G._adam_on(qf, gq, adam_q, 1e-2, 0.9, 0.999, 1e-8)
        gp = sum(T.flat_grad(-qf(s, pol(s)).mean(), pol) / 2 for s, _, _, _, _ in shards)
        G._adam_on(pol, gp, adam_mu, 1e-3, 0.9, 0.999, 1e-8)
        G.soft_update_(tqf, qf, 0.05); G.soft_update_(tpol, pol, 0.05)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for a, b, ref in zip(got[0], got[1], nets):
        assert np.array_equal(a, b) and np.isfinite(a).all()
        np.testing.assert_allclose(a, T.flat_params(ref).numpy(), rtol=0, atol=1e-12)


def test_batch_must_divide_over_ranks_and_pool_over_envs():
    env = ToyVecEnv(4, 0)
    mk = lambda **kw: G.DDPG(env.step, env.reset, G.DeterministicMLPPolicy(4, 2, dtype=torch.float64), G.ContinuousMLPQFunction(4, 2, dtype=torch.float64), 4, 4,
                             AMAP(), **kw)
    with pytest.raises(ValueError, match="multiple"):
        mk(replay_pool_size=1000001)
    assert mk(replay_pool_size=1000).batch_local == 32


# ---- snapshot / resume
def _snap_ddpg(seed, **kw):
    env = SnapshotToyEnv(8, seed)
    env.g = None
    torch.manual_seed(seed)
    algo = G.DDPG(env.step, env.reset, G.DeterministicMLPPolicy(4, 2, dtype=torch.float64), G.ContinuousMLPQFunction(4, 2, dtype=torch.float64), 8, 4, AMAP(),
                  batch_size=16, max_path_length=1000, epoch_length=4, min_pool_size=16, replay_pool_size=8 * 6, seed=seed, **kw)
    algo.env = env
    return algo


def _state(a):
    return [T.flat_params(n).clone() for n in (a.policy, a.qf, a.target_policy, a.target_qf)] + \
        [a.adam_mu["m"], a.adam_mu["v"], a.adam_q["m"], a.adam_q["v"], a.ou.state, a.pool.obs, a.pool.act, a.pool.rew, a.pool.term, a.pool.nobs, a.path_t, a.obs]


def test_resumed_ddpg_run_is_the_interrupted_run(tmp_path):
    """k epochs, save, load in a fresh object, k more epochs == 2k uninterrupted epochs, bit for bit, the pool (which wraps) included."""
    a = _snap_ddpg(2)
    a.env.g = torch.Generator().manual_seed(2); a.env.reset(); a.obs = None
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ck = torch.load(p, weights_only=True)
    assert ck["algo"] == "ddpg" and ck["adam_q"]["t"] == a.adam_q["t"] == 7 and ck["pool"]["size"] == 48 and ck["pool"]["top"] == a.pool.top
    ref = [a.train_iteration() for _ in range(2)]
    b = _snap_ddpg(7)
    b.env.g = torch.Generator().manual_seed(99)
    _, restored = b.load(p)
    assert restored and b.pool_restored and b.adam_q["t"] == 7 and b.pool.size == 48 and b.itr == 2
    got = [b.train_iteration() for _ in range(2)]
    assert repr(got) == repr(ref)   # (nan where no path ended: compared as text)
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert (a.pool.top, a.pool.size, a.n_updates) == (b.pool.top, b.pool.size, b.n_updates)


def test_snapshot_without_its_pool_restarts_with_an_empty_one(tmp_path, capsys):
    a = _snap_ddpg(2, snapshot_pool=False)
    a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    assert torch.load(p, weights_only=True)["pool"] is None
    b = _snap_ddpg(7)
    _, restored = b.load(p)
    assert restored and not b.pool_restored and b.pool.size == 0 and b.pool.top == 0
    assert "no replay pool" in capsys.readouterr().out
    assert torch.equal(T.flat_params(a.qf), T.flat_params(b.qf)) and torch.equal(T.flat_params(a.target_policy), T.flat_params(b.target_policy))
    assert b.train_step() == 0   # 8 rows < min_pool_size again


def test_load_refuses_foreign_snapshots(tmp_path):
    env = ToyVecEnv(8, 0)
    torch.manual_seed(0)
    pol = T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=torch.float64)
    trpo = T.TRPO(env.step, env.reset, pol, T.LinearFeatureBaseline(), 8, 4, AMAP(), batch_size=8 * 2)
    vpg = V.VPG(env.step, env.reset, T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=torch.float64), T.LinearFeatureBaseline(), 8, 4, AMAP(), batch_size=8 * 2)
    d = _snap_ddpg(1)
    trpo.train_iteration(); vpg.train_iteration(); d.train_iteration()
    pt, pv, pd = (str(tmp_path / n) for n in ("trpo.pt", "vpg.pt", "ddpg.pt"))
    trpo.save(pt); vpg.save(pv); d.save(pd)
    before = T.flat_params(d.policy).clone()
    with pytest.raises(ValueError, match="trpo.*ddpg"):
        d.load(pt)
    with pytest.raises(ValueError, match="vpg.*ddpg"):
        d.load(pv)
    assert torch.equal(T.flat_params(d.policy), before)
    with pytest.raises(ValueError, match="ddpg.*trpo"):
        trpo.load(pd)
    with pytest.raises(ValueError, match="ddpg.*vpg"):
        vpg.load(pd)


def test_cpu_networks_run_the_torch_statements():
    assert not G.kernels_cover(G.DeterministicMLPPolicy(26, 6), G.ContinuousMLPQFunction(26, 6))
    a = _snap_ddpg(3)
    assert a._update_kernels() is None and a._fused_step(torch.device("cpu")) is None
