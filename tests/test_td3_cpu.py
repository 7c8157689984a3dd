"""TD3 (cassierl_amd/td3.py) on CPU, test for test as tests/test_sac_cpu.py: the torch statement of the update against an independent autograd
statement (the delay included), the two clips of the target action, exploration and the pool rules, the schedule at N = 1, learning on a toy env, the
world-size-2 (gloo) run, snapshot / resume and the refusal of foreign snapshots."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cassierl_amd import ddpg as G
from cassierl_amd import td3 as D3
from cassierl_amd import trpo as T
from cassierl_amd import vpg as V
from test_ddpg_cpu import AMAP, _BanditEnv, _ClockEnv, _free_port
from test_trpo_cpu import SnapshotToyEnv, ToyVecEnv

F64 = torch.float64


def _mk(env, n, seed=0, **kw):
    torch.manual_seed(seed)
    nets = (G.DeterministicMLPPolicy(4, 2, dtype=F64), G.ContinuousMLPQFunction(4, 2, dtype=F64), G.ContinuousMLPQFunction(4, 2, dtype=F64))
    kw.setdefault("seed", seed or 1)
    return D3.TD3(env.step, env.reset, *nets, n, 4, AMAP(), **kw)


# ---- the update
def _fresh(seed, D=5, A=3):
    """actor, qf1, qf2, target actor, target_qf1, target_qf2; the targets are perturbed copies."""
    torch.manual_seed(seed)
    nets = [G.DeterministicMLPPolicy(D, A, dtype=F64), G.ContinuousMLPQFunction(D, A, dtype=F64), G.ContinuousMLPQFunction(D, A, dtype=F64)]
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


def _batch(g, n=40, D=5, A=3):
    return (torch.randn(n, D, dtype=F64, generator=g), torch.rand(n, A, dtype=F64, generator=g) * 2 - 1, torch.randn(n, dtype=F64, generator=g),
            (torch.rand(n, generator=g) < 0.3).double(), torch.randn(n, D, dtype=F64, generator=g)), torch.randn(n, A, dtype=F64, generator=g)


def _adam(st, key, net, lr, b1=0.9, b2=0.999, eps=1e-8):
    """Lasagne's Adam written out per parameter tensor, out of place (not vpg.adam_step_, which ddpg._adam_on takes its step through):
    a_t = lr sqrt(1 - b2^t) / (1 - b1^t),  m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,  theta = theta - a_t m / (sqrt(v) + eps)."""
    ps = list(net.parameters())
    a = st.setdefault(key, dict(t=0, m=[torch.zeros_like(p) for p in ps], v=[torch.zeros_like(p) for p in ps]))
    a["t"] += 1
    step = lr * (1.0 - b2 ** a["t"]) ** 0.5 / (1.0 - b1 ** a["t"])
    with torch.no_grad():
        for i, p in enumerate(ps):
            a["m"][i] = b1 * a["m"][i] + (1.0 - b1) * p.grad
            a["v"][i] = b2 * a["v"][i] + (1.0 - b2) * p.grad * p.grad
            p.copy_(p - step * a["m"][i] / (a["v"][i] ** 0.5 + eps))


def _flat(xs):
    return torch.cat([x.reshape(-1) for x in xs])


def _independent_update(pi, q1, q2, tpi, t1, t2, st, batch, e2, k, delay, sigma, c, gamma, qf_lr, pi_lr, tau, wrong=None):
    """The issue's update written against nn.Module copies, .backward() and min / max in place of clamp; k: the updates made before this one."""
    s, a, r, term, s2 = batch
    with torch.no_grad():
        off = torch.minimum(torch.maximum(sigma * e2, torch.full_like(e2, -c)), torch.full_like(e2, c))
        a2 = torch.minimum(torch.maximum(torch.tanh(tpi.l3(torch.relu(tpi.l2(torch.relu(tpi.l1(s2)))))) + off, -torch.ones_like(e2)), torch.ones_like(e2))
        y = r + (1 - term) * gamma * torch.minimum(t1(s2, a2), t2(s2, a2))
    old_q1 = copy.deepcopy(q1)
    for key, q in (("q1", q1), ("q2", q2)):
        q.zero_grad()
        ((q(s, a) - y) ** 2).mean().backward()
        _adam(st, key, q, qf_lr)
    moves = k % delay == delay - 1
    if moves:
        pi.zero_grad()
        (-(old_q1 if wrong == "old_critic" else q1)(s, pi(s)).mean()).backward()
        _adam(st, "pi", pi, pi_lr)
    if moves or wrong == "targets_every_step":
        with torch.no_grad():
            for tgt, live in ((t1, q1), (t2, q2)) + (((tpi, pi),) if moves else ()):
                for pt, p in zip(tgt.parameters(), live.parameters()):
                    pt.copy_((1 - tau) * pt + tau * p)


def test_update_statement_matches_an_independent_autograd_statement():
    """Four consecutive updates with policy_delay 2: networks, targets and Adam states agree with the independent statement to 1e-12; updates 1 and 3
    leave the actor, its Adam state and all three targets with the bits they had."""
    nets = _fresh(1)
    runs = {k: [copy.deepcopy(n) for n in nets] for k in ("mine", "ref", "old_critic", "targets_every_step")}
    mine = runs["mine"]
    adams = [G.new_adam(mine[0]), G.new_adam(mine[1]), G.new_adam(mine[2])]
    st = {k: {} for k in runs}
    g = torch.Generator().manual_seed(3)
    hp = dict(policy_delay=2, policy_noise=0.3, noise_clip=0.4, discount=0.97, qf_lr=1e-2, policy_lr=1e-3, tau=0.05)
    for k in range(4):
        batch, e2 = _batch(g)
        still = [T.flat_params(n).clone() for n in (mine[0], mine[3], mine[4], mine[5])] + [adams[0]["m"].clone(), adams[0]["v"].clone()]
        t_before = adams[0]["t"]
        l1, l2, q1, q2, surr = D3.td3_update_torch_(*mine, *adams, batch, e2, k, **hp)
        assert l1.item() > 0 and l2.item() > 0 and math.isfinite(q1.item()) and math.isfinite(q2.item())
        now = [T.flat_params(n) for n in (mine[0], mine[3], mine[4], mine[5])] + [adams[0]["m"], adams[0]["v"]]
        if k % 2 == 0:
            assert surr is None and adams[0]["t"] == t_before
            for x, y in zip(still, now):
                assert torch.equal(x, y)
        else:
            assert math.isfinite(surr.item()) and adams[0]["t"] == t_before + 1
            for x, y in zip(still, now):
                assert not torch.equal(x, y)
        for w in ("ref", "old_critic", "targets_every_step"):
            _independent_update(*runs[w], st[w], batch, e2, k, 2, 0.3, 0.4, 0.97, 1e-2, 1e-3, 0.05, wrong=None if w == "ref" else w)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    for a, b in zip(mine, runs["ref"]):
        assert rel(T.flat_params(a), T.flat_params(b)) < 1e-12
    for adam, key, t in zip(adams, ("pi", "q1", "q2"), (2, 4, 4)):
        assert rel(adam["m"], _flat(st["ref"][key]["m"])) < 1e-12 and rel(adam["v"], _flat(st["ref"][key]["v"])) < 1e-12 and adam["t"] == st["ref"][key]["t"] == t
    # the order and the delay matter: an actor step through qf1 BEFORE its step, or critic targets that move on every update, give other networks
    assert rel(T.flat_params(mine[0]), T.flat_params(runs["old_critic"][0])) > 1e-6
    assert rel(T.flat_params(mine[4]), T.flat_params(runs["targets_every_step"][4])) > 1e-6


def test_target_action_takes_both_clips_and_no_noise_gives_ddpgs_target():
    pi, q1, q2, tpi, t1, t2 = _fresh(2)
    g = torch.Generator().manual_seed(4)
    (s, a, r, term, s2), e2 = _batch(g, n=400)
    with torch.no_grad():
        mu = tpi(s2)
        # policy_noise 10, noise_clip 0.5: |10 eps| < 0.5 only where |eps| < 0.05, about 4 % of the components
        a2 = D3.smoothed_target_action(tpi, s2, e2, 10.0, 0.5)
        off = (10.0 * e2).clamp(-0.5, 0.5)
        assert ((off.abs() == 0.5).double().mean().item()) > 0.9 and off.abs().max().item() == 0.5
        inner = (mu + off).abs() < 1
        assert torch.equal(a2[inner], (mu + off)[inner]) and a2.abs().max().item() <= 1.0
        # the output bias at +-5: mu' = tanh(+-5 + O(1)) lies beyond +-0.5 on nearly every component, and there every offset of 0.5 that points
        # outwards ends exactly at +-1; an offset that points inwards stays inside, and nothing lies beyond
        sat = copy.deepcopy(tpi)
        sign = torch.tensor([1.0, -1.0, 1.0], dtype=F64)
        sat.l3.bias.copy_(5.0 * sign)
        mu = sat(s2)
        strong = mu * sign >= 0.5
        assert strong.double().mean().item() > 0.95
        a2 = D3.smoothed_target_action(sat, s2, e2, 10.0, 0.5)
        outwards = (off * sign == 0.5) & strong
        assert outwards.double().mean().item() > 0.4 and torch.equal(a2[outwards], sign.expand_as(a2)[outwards]) and a2.abs().max().item() == 1.0
        assert ((a2 * sign)[off * sign == -0.5] < 0.51).all()
        # policy_noise 0: the target action is mu'(s') and y is DDPG's target under the minimum of the two target critics
        assert torch.equal(D3.smoothed_target_action(tpi, s2, e2, 0.0, 0.5), tpi(s2))
        y = r + (1 - term) * 0.97 * torch.min(t1(s2, tpi(s2)), t2(s2, tpi(s2)))
    mine, ref = [copy.deepcopy(n) for n in (pi, q1, q2, tpi, t1, t2)], [copy.deepcopy(q1), copy.deepcopy(q2)]
    D3.td3_update_torch_(*mine, G.new_adam(pi), G.new_adam(q1), G.new_adam(q2), (s, a, r, term, s2), e2, 0, policy_noise=0.0, discount=0.97, qf_lr=1e-2)
    for q, got in zip(ref, mine[1:3]):
        G._adam_on(q, T.flat_grad(((q(s, a) - y) ** 2).mean(), q), G.new_adam(q), 1e-2, 0.9, 0.999, 1e-8)
        assert torch.equal(T.flat_params(q), T.flat_params(got))


# ---- exploration, schedule and pool
def test_truncated_path_keeps_its_next_observation_and_actions_are_the_clipped_noisy_mean():
    env = _ClockEnv(2)
    algo = _mk(env, 2, batch_size=2, max_path_length=5, min_pool_size=10 ** 9, replay_pool_size=40, scale_reward=0.01, exploration_sigma=0.7,
               env_reset_masked=lambda m: env.reset(m))
    with torch.no_grad():
        algo.policy.l3.weight.uniform_(-0.5, 0.5)   # mu(s) of order 1: with sigma 0.7 the clip is active on some components
    gen = torch.Generator(); gen.set_state(algo.gen.get_state())
    for _ in range(6):
        algo.train_step()
    pool = algo.pool
    assert pool.obs[[1, 3, 5, 7, 9, 11], 1].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 0.0] and pool.term[[1, 3, 5, 7, 9, 11]].tolist() == [0.0] * 6
    assert pool.nobs[9, 1].item() == 5.0 and pool.nobs[9, 0].item() == 1.0   # cut at step 5: terminal 0 and the true s'
    assert pool.term[[0, 2, 4, 6, 8, 10]].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 1.0] and pool.nobs[4, 1].item() == 0.0
    assert torch.allclose(pool.rew[:12], torch.full((12,), 0.01, dtype=F64)) and pool.top == 12 and pool.size == 12
    for k in range(6):   # the action is clip(mu + sigma n, -1, 1) with the sampler generator's normals
        n = torch.randn((2, 2), dtype=F64, generator=gen)
        with torch.no_grad():
            assert torch.equal(pool.act[2 * k:2 * k + 2], (algo.policy(pool.obs[2 * k:2 * k + 2]) + 0.7 * n).clamp(-1, 1))
    assert pool.act[:12].abs().max().item() == 1.0 and not hasattr(algo, "ou")


def test_one_environment_with_the_defaults_runs_the_delayed_schedule():
    env = ToyVecEnv(1, 0)
    algo = _mk(env, 1, replay_pool_size=G.default_pool_size(1))
    assert (algo.batch_size, algo.max_path_length, algo.epoch_length, algo.min_pool_size, algo.discount, algo.scale_reward, algo.qf_learning_rate,
            algo.policy_learning_rate, algo.tau, algo.updates_per_step, algo.pool.capacity, algo.policy_noise, algo.noise_clip, algo.policy_delay,
            algo.exploration_sigma) == (256, 100, 1000, 10000, 0.99, 1.0, 3e-4, 3e-4, 0.005, 1, 1000000, 0.2, 0.5, 2, 0.1)
    algo.min_pool_size = 50
    seen = []
    real = algo.update
    algo.update = lambda idx, noise=None: (seen.append((idx.clone(), algo.noise_gen.get_state(), algo.idx_gen.get_state())), real(idx, noise))
    actor0, target0 = T.flat_params(algo.policy).clone(), T.flat_params(algo.target_qf1).clone()
    ran = []
    for step in range(60):
        ran.append(algo.train_step())
        k = sum(ran)
        assert algo.n_updates == k and algo.actor_updates == k // 2 == algo.adam_mu["t"] and algo.adam_q1["t"] == algo.adam_q2["t"] == k
        if k == 1:   # the first update is not a delayed one
            assert torch.equal(T.flat_params(algo.policy), actor0) and torch.equal(T.flat_params(algo.target_qf1), target0)
    assert ran == [0] * 49 + [1] * 11 and len(seen) == 11 and algo.last_update_kind == "torch"
    assert not torch.equal(T.flat_params(algo.policy), actor0) and not torch.equal(T.flat_params(algo.target_qf1), target0)
    for k, (idx, _, _) in enumerate(seen):
        assert idx.shape == (256,) and idx.dtype == torch.int64 and idx.min().item() >= 0 and idx.max().item() < 50 + k
    # the smoothing normals come from their own generator: drawing them leaves the index generator alone
    gen = torch.Generator(); gen.set_state(seen[3][1])
    algo.noise_gen.set_state(seen[3][1]); algo.idx_gen.set_state(seen[3][2])
    noise = algo.sample_noise()
    assert noise.shape == (256, 2) and noise.dtype == F64 and torch.equal(noise, torch.randn((256, 2), generator=gen, dtype=F64))
    assert torch.equal(algo.idx_gen.get_state(), seen[3][2])


def test_batch_must_divide_over_ranks_pool_over_envs_and_the_delay_is_positive():
    env = ToyVecEnv(4, 0)
    with pytest.raises(ValueError, match="multiple"):
        _mk(env, 4, replay_pool_size=1000001)
    with pytest.raises(ValueError, match="policy_delay"):
        _mk(env, 4, replay_pool_size=1000, policy_delay=0)
    assert _mk(env, 4, replay_pool_size=1000).batch_local == 256


def test_td3_improves_reward_on_toy_env():
    """tests/test_sac_cpu.py's toy test: the same environment, budget (40 epochs of 25 steps, 64 environments, batch 64) and criterion."""
    env = _BanditEnv(64, 3)
    algo = _mk(env, 64, seed=3, batch_size=64, max_path_length=100, epoch_length=25, min_pool_size=64, replay_pool_size=64 * 50, qf_learning_rate=1e-2,
               policy_learning_rate=1e-3, soft_target_tau=0.05)

    def policy_reward():   # mean reward of mu(s), without exploration noise
        g = torch.Generator().manual_seed(11)
        s = torch.rand(4096, 2, generator=g, dtype=F64) * 2 - 1
        o = torch.cat([s, torch.zeros(4096, 1, dtype=F64), torch.ones(4096, 1, dtype=F64)], 1)
        with torch.no_grad():
            return -((algo.policy(o)[:, 0] - 0.8 * s[:, 0]) ** 2).mean().item()

    first = policy_reward()
    for _ in range(40):
        last = algo.train_iteration()
    assert set(last) == {"itr", "env_steps", "updates", "actor_updates", "pool_size", "avg_reward", "episodes", "avg_return", "qf1_loss", "qf2_loss", "avg_q1", "avg_q2",
                         "policy_surr", "update_kind"}
    assert last["env_steps"] == 64 * 25 and last["updates"] == 25 and last["actor_updates"] in (12, 13) and last["pool_size"] == 64 * 50
    assert last["episodes"] == 64 * 25 and last["update_kind"] == "torch" and algo.n_updates == 1000 and algo.actor_updates == 500
    assert last["qf1_loss"] > 0 and last["qf2_loss"] > 0 and all(math.isfinite(last[k]) for k in ("avg_q1", "avg_q2", "policy_surr"))
    after = policy_reward()
    assert after > first + 0.05, (first, after)


# ---- data-parallel: identical parameters on both ranks, equal to a one-process emulation of the two shards
def _shard(rank, k):
    return _batch(torch.Generator().manual_seed(1000 * rank + k), n=24)


HP = dict(policy_delay=2, policy_noise=0.3, noise_clip=0.4, discount=0.97, qf_lr=1e-2, policy_lr=1e-3, tau=0.05)


def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nets = _fresh(7)
    adams = [G.new_adam(nets[0]), G.new_adam(nets[1]), G.new_adam(nets[2])]
    for k in range(5):
        batch, e2 = _shard(rank, k)
        D3.td3_update_torch_(*nets, *adams, batch, e2, k, **HP)
    q.put((rank, [T.flat_params(n).numpy() for n in nets]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_process_td3_keeps_identical_parameters_and_equals_the_emulation():
    pi, q1, q2, tpi, t1, t2 = nets = _fresh(7)
    adams = [G.new_adam(pi), G.new_adam(q1), G.new_adam(q2)]
    for k in range(5):
        shards = [_shard(r, k) for r in range(2)]
        gq = [0, 0]
        for (s, a, r, term, s2), e2 in shards:
            with torch.no_grad():
                a2 = (tpi(s2) + (0.3 * e2).clamp(-0.4, 0.4)).clamp(-1, 1)
                y = r + (1 - term) * 0.97 * torch.min(t1(s2, a2), t2(s2, a2))
            for i, q in enumerate((q1, q2)):
                gq[i] = gq[i] + T.flat_grad(((q(s, a) - y) ** 2).mean(), q) / 2
        for i, q in enumerate((q1, q2)):
            G._adam_on(q, gq[i], adams[1 + i], 1e-2, 0.9, 0.999, 1e-8)
        if k % 2 == 1:
            gp = sum(T.flat_grad(-q1(s, pi(s)).mean(), pi) / 2 for (s, _, _, _, _), _ in shards)
            G._adam_on(pi, gp, adams[0], 1e-3, 0.9, 0.999, 1e-8)
            G.soft_update_(t1, q1, 0.05); G.soft_update_(t2, q2, 0.05); G.soft_update_(tpi, pi, 0.05)
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


# ---- snapshot / resume
def _snap_td3(seed, **kw):
    env = SnapshotToyEnv(8, seed)
    env.g = None
    algo = _mk(env, 8, seed=seed, batch_size=16, max_path_length=1000, epoch_length=4, min_pool_size=16, replay_pool_size=8 * 6, **kw)
    algo.env = env
    return algo


def _state(a):
    return [T.flat_params(n).clone() for n in (a.policy, a.qf1, a.qf2, a.target_policy, a.target_qf1, a.target_qf2)] + \
        [x[k] for x in (a.adam_mu, a.adam_q1, a.adam_q2) for k in ("m", "v")] + [a.pool.obs, a.pool.act, a.pool.rew, a.pool.term, a.pool.nobs, a.path_t, a.obs]


@pytest.mark.parametrize("epochs", [2, 1])
def test_resumed_td3_run_is_the_interrupted_run(tmp_path, epochs):
    """k epochs, save, load in a fresh object, 2 more epochs == k + 2 uninterrupted epochs, bit for bit, the pool (which wraps) included.  Two epochs
    stop after 7 updates, one after 3: an odd n_updates both times, so the update after the resume must be a delayed one."""
    a = _snap_td3(2)
    a.env.g = torch.Generator().manual_seed(2); a.env.reset(); a.obs = None
    for _ in range(epochs):
        a.train_iteration()
    n = 4 * epochs - 1
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ck = torch.load(p, weights_only=True)
    assert ck["algo"] == "td3" and ck["n_updates"] == a.n_updates == n and n % 2 == 1 and ck["adam_q1"]["t"] == ck["adam_q2"]["t"] == n
    assert ck["adam_mu"]["t"] == a.adam_mu["t"] == n // 2 and ck["pool"]["size"] == min(48, 32 * epochs) and ck["pool"]["top"] == a.pool.top
    assert "ou_state" not in ck and "log_alpha" not in ck and "noise_gen_state" in ck and "idx_gen_state" in ck and "target_policy" in ck
    ref = [a.train_iteration() for _ in range(2)]
    b = _snap_td3(7)
    b.env.g = torch.Generator().manual_seed(99)
    _, restored = b.load(p)
    assert restored and b.pool_restored and b.n_updates == n and b.adam_q2["t"] == n and b.adam_mu["t"] == n // 2 and b.itr == epochs
    actor = T.flat_params(b.policy).clone()
    b.train_step()
    assert b.n_updates == n + 1 and b.adam_mu["t"] == n // 2 + 1 and not torch.equal(T.flat_params(b.policy), actor)   # the delay's phase came back
    c = _snap_td3(9)
    c.env.g = torch.Generator().manual_seed(5)
    c.load(p)
    got = [c.train_iteration() for _ in range(2)]
    assert repr(got) == repr(ref)
    for x, y in zip(_state(a), _state(c)):
        assert torch.equal(x, y)
    assert (a.pool.top, a.pool.size, a.n_updates) == (c.pool.top, c.pool.size, c.n_updates)
    assert torch.equal(a.noise_gen.get_state(), c.noise_gen.get_state()) and torch.equal(a.idx_gen.get_state(), c.idx_gen.get_state())


def test_resume_without_the_pool_restarts_with_an_empty_one_and_is_reproducible(tmp_path, capsys):
    a = _snap_td3(2, snapshot_pool=False)
    a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    assert torch.load(p, weights_only=True)["pool"] is None
    runs = []
    for seed in (7, 9):   # two fresh objects resumed from the pool-less snapshot run the same run, bit for bit
        b = _snap_td3(seed)
        _, restored = b.load(p)
        assert restored and not b.pool_restored and b.pool.size == 0 and b.pool.top == 0 and b.n_updates == 3
        assert "TD3.load: the snapshot carries no replay pool" in capsys.readouterr().out
        assert torch.equal(T.flat_params(a.qf2), T.flat_params(b.qf2)) and torch.equal(T.flat_params(a.target_policy), T.flat_params(b.target_policy))
        assert b.train_step() == 0   # 8 rows < min_pool_size again
        runs.append((repr([b.train_iteration() for _ in range(2)]), _state(b)))
    assert runs[0][0] == runs[1][0]
    for x, y in zip(runs[0][1], runs[1][1]):
        assert torch.equal(x, y)


def test_load_refuses_foreign_snapshots(tmp_path):
    from cassierl_amd import sac as S
    env = ToyVecEnv(8, 0)
    torch.manual_seed(0)
    trpo = T.TRPO(env.step, env.reset, T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=F64), T.LinearFeatureBaseline(), 8, 4, AMAP(), batch_size=8 * 2)
    vpg = V.VPG(env.step, env.reset, T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=F64), T.LinearFeatureBaseline(), 8, 4, AMAP(), batch_size=8 * 2)
    kw = dict(batch_size=16, epoch_length=4, min_pool_size=16, replay_pool_size=48)
    env2, env3 = SnapshotToyEnv(8, 1), SnapshotToyEnv(8, 1)
    torch.manual_seed(1)
    d = G.DDPG(env2.step, env2.reset, G.DeterministicMLPPolicy(4, 2, dtype=F64), G.ContinuousMLPQFunction(4, 2, dtype=F64), 8, 4, AMAP(), **kw)
    s = S.SAC(env3.step, env3.reset, S.SquashedGaussianMLPPolicy(4, 2, dtype=F64), G.ContinuousMLPQFunction(4, 2, dtype=F64), G.ContinuousMLPQFunction(4, 2, dtype=F64),
              8, 4, AMAP(), **kw)
    t = _snap_td3(1)
    others = dict(trpo=trpo, vpg=vpg, ddpg=d, sac=s)
    paths = {name: str(tmp_path / (name + ".pt")) for name in list(others) + ["td3"]}
    for name, algo in list(others.items()) + [("td3", t)]:
        algo.train_iteration()
        algo.save(paths[name])
    before = T.flat_params(t.policy).clone()
    for name in others:
        with pytest.raises(ValueError, match="TD3.load: the snapshot was written by %s, this run is td3" % name):
            t.load(paths[name])
    assert torch.equal(T.flat_params(t.policy), before)
    for name, other in others.items():
        with pytest.raises(ValueError, match="td3.*%s" % name):
            other.load(paths["td3"])


def test_cpu_networks_run_the_torch_statements():
    assert not D3.kernels_cover(G.DeterministicMLPPolicy(26, 6), G.ContinuousMLPQFunction(26, 6), G.ContinuousMLPQFunction(26, 6))
    a = _snap_td3(3)
    assert a._update_kernels() is None and a._fused_step(torch.device("cpu")) is None
    a.train_iteration()
    assert a.last_update_kind == "torch" and a.last_policy_step_fused is False and a.n_updates == 3


def test_entry_points_refuse_other_shapes_before_any_launch():
    """obs_dim 26 or 17, act_dim 6 or 7 (the policy step: obs_dim 26); anything else, a null pointer or a negative noise clip is CASSIE_EINVAL (-1)."""
    import ctypes as ct
    from cassierl_amd import _lib
    L = _lib.load()
    buf = (ct.c_double * 64)()
    p = ct.cast(buf, ct.c_void_p)
    net = (ct.c_void_p * 6)(*[p.value] * 6)
    f = ct.c_float
    for D, A in ((5, 3), (26, 8), (32, 6), (17, 5)):
        assert L.CassieTd3CriticGrad(p, p, p, p, p, ct.c_longlong(8), p, 4, D, A, net, net, net, net, net, p, f(0.2), f(0.5), f(0.99), p, None) == -1
        assert L.CassieTd3CriticApply(1, D, A, p, f(1.0), net, net, net, net, p, p, p, p, 1, f(1e-3), f(0.9), f(0.999), f(1e-8), f(5e-3), None, None) == -1
    for D, A in ((17, 6), (17, 7), (5, 3)):
        assert L.CassieTd3PolicyStep(p, 4, D, A, net, p, f(0.1), p, p, p, p, p, None) == -1
    assert L.CassieTd3CriticGrad(p, p, p, p, p, ct.c_longlong(8), p, 4, 26, 6, net, net, net, net, net, p, f(0.2), f(-0.5), f(0.99), p, None) == -1
    assert L.CassieTd3CriticGrad(p, p, p, p, p, ct.c_longlong(8), p, 4, 26, 6, net, None, net, net, net, p, f(0.2), f(0.5), f(0.99), p, None) == -1
    assert L.CassieTd3CriticApply(1, 26, 6, p, f(1.0), net, net, net, net, p, p, p, p, 0, f(1e-3), f(0.9), f(0.999), f(1e-8), f(5e-3), None, None) == -1
