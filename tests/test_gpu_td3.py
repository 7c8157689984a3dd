"""TD3's kernels (csrc/tu_td3.hip) against the torch statements of cassierl_amd/td3.py, and train_td3.py / sim_policy.py on the GPU.  -m gpu only.

The reference of every gradient comparison is FLOAT64 torch autograd of td3.py's own statement on networks and data cast up; the bounds and the "4x"
rule are tests/test_gpu_offpolicy_edges.py's (its _check prints which of the two held): a gradient max|g_kernel - g_64| < 2e-4 max|g_64|, a statistic
column 1e-5 relative, an action 5e-6 (1 + max|a_64|).  Pools are built by rejection on the LIVE critics' ReLU margins at (s, a) only: nothing else
carries a gradient in the critic step (the target action's clips, the minimum and the target networks' ReLUs are continuous in y).

Networks, pools and kernel objects are built once per shape and kind (lru_cache) and are never written to."""
import copy
import functools
import os
import sys

import numpy as np
import pytest

import test_gpu_offpolicy_edges as TE
from test_gpu_ddpg import _free_port, _run, _small

pytestmark = pytest.mark.gpu

GAMMA = 0.99
REGIMES = {"rare": (0.2, 0.5), "clipped": (10.0, 0.5), "none": (0.0, 0.5)}   # the noise clip rarely active, active on almost every component, no noise
CASES = TE.CASES_A + [(1000, 26, 7)]


def _nets(D, A, seed, out_bias=None):
    """Actor, two critics and a target of each with test_gpu_ddpg._nets' scaling (HeUniform hidden weights, biases N(0, 0.1), output weights +-0.3, the
    critics' output bias 0.5); the targets are other draws.  out_bias [A]: the target actor's output bias."""
    import torch
    from cassierl_amd import ddpg as G
    torch.manual_seed(seed)
    nets = [G.DeterministicMLPPolicy(D, A), G.ContinuousMLPQFunction(D, A), G.ContinuousMLPQFunction(D, A),
            G.DeterministicMLPPolicy(D, A), G.ContinuousMLPQFunction(D, A), G.ContinuousMLPQFunction(D, A)]
    with torch.no_grad():
        for net in nets:
            for lin in (net.l1, net.l2, net.l3):
                lin.bias.copy_(0.1 * torch.randn_like(lin.bias))
            net.l3.weight.uniform_(-0.3, 0.3)
        for qf in nets[1:3] + nets[4:]:
            qf.l3.bias.fill_(0.5)
        if out_bias is not None:
            nets[3].l3.bias.copy_(torch.as_tensor(out_bias, dtype=torch.float32))
    return [n.cuda() for n in nets]   # actor, qf1, qf2, target actor, target_qf1, target_qf2


def _pool_with_margin(qf1, qf2, D, A, candidates=40000, seed=11, eps=1e-4):
    """test_gpu_ddpg._pool_with_margin's candidates, kept where both live critics' hidden pre-activations at (s, a) keep |z| >= eps (float64)."""
    import torch
    from cassierl_amd import ddpg as G
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = 0.7 * torch.randn(candidates, D, device="cuda", generator=g)
    act = torch.rand(candidates, A, device="cuda", generator=g) * 2 - 1
    keep = torch.ones(candidates, dtype=torch.bool, device="cuda")
    with torch.no_grad():
        for q in (qf1, qf2):
            q = copy.deepcopy(q).double()
            y1 = q.l1(obs.double())
            y2 = q.l2(torch.cat([y1.relu(), act.double()], 1))
            keep &= (y1.abs() >= eps).all(1) & (y2.abs() >= eps).all(1)
    dropped = 1.0 - keep.float().mean().item()
    obs, act = obs[keep], act[keep]
    m = obs.shape[0]
    pool = G.ReplayPool(m, 1, D, A, "cuda")
    pool.obs.copy_(obs); pool.act.copy_(act)
    pool.rew.copy_(torch.randn(m, device="cuda", generator=g) * 0.1)
    pool.term.copy_((torch.rand(m, device="cuda", generator=g) < 0.2).float())
    pool.nobs.copy_(0.7 * torch.randn(m, D, device="cuda", generator=g))
    pool.size = m
    return pool, dropped


@functools.lru_cache(maxsize=None)
def _td3(D, A, kind="plain"):
    """(nets, nets in float64, pool, share of candidates dropped, kernels) of one shape and kind of target networks."""
    from cassierl_amd import td3 as D3
    nets = _nets(D, A, 3, out_bias=[5.0 if a % 2 == 0 else -5.0 for a in range(A)] if kind == "saturated" else None)
    if kind == "tied":   # the second target critic is the first: the minimum is a tie on every row
        nets[5] = copy.deepcopy(nets[4])
    pool, dropped = _pool_with_margin(nets[1], nets[2], D, A)
    return nets, [copy.deepcopy(m).double() for m in nets], pool, dropped, D3.Td3Kernels(*nets)


def _ref(nets, data, eps2, policy_noise, noise_clip):
    """td3_update_torch_'s critic losses in the dtype of the arguments: [(critic k's gradient, loss, mean Q)] and the target action."""
    import torch
    from cassierl_amd import td3 as D3
    _, qf1, qf2, tpol, tq1, tq2 = nets
    s, a, r, term, s2 = data
    with torch.no_grad():
        a2 = D3.smoothed_target_action(tpol, s2, eps2, policy_noise, noise_clip)
        y = r + (1.0 - term) * GAMMA * torch.min(tq1(s2, a2), tq2(s2, a2))
    out = []
    for qf in (qf1, qf2):
        q = qf(s, a)
        loss = ((q - y) ** 2).mean()
        out.append((TE._flat_grad(loss, qf), loss.detach().double(), q.detach().double().mean()))
    return out, a2, y


def _critic_case(batch, D, A, regime, kind="plain"):
    """CassieTd3CriticGrad (both blocks, both statistic columns, launched twice) on one batch against float64 and float32 autograd."""
    import torch
    nets, nets64, pool, dropped, k = _td3(D, A, kind)
    print("ReLU margins of the live critics at (s, a) (%s): %.2f %% of the candidate rows dropped" % (kind, 100 * dropped))
    assert dropped <= 0.03
    policy_noise, noise_clip = REGIMES[regime]
    idx, g = TE._indices(pool, batch)
    eps2 = torch.randn(batch, A, device="cuda", generator=g)
    data = pool.sample(idx)
    c64, a2, _ = _ref(nets64, [t.double() for t in data], eps2.double(), policy_noise, noise_clip)
    c32, _, _ = _ref(nets, data, eps2, policy_noise, noise_clip)
    part = k.critic_grad(pool, idx, eps2, policy_noise, noise_clip, GAMMA).clone()
    NP = c64[0][0].numel()
    assert part.shape == (2, TE._rows_ok(k, part, batch), NP + 2)
    for i in range(2):
        tot = part[i].double().sum(0) / batch
        TE._check("critic %d gradient" % (i + 1), tot[:NP], c64[i][0], c32[i][0], 2e-4)
        TE._check("critic %d loss" % (i + 1), tot[NP], c64[i][1], c32[i][1], 1e-5)
        TE._check("critic %d mean Q" % (i + 1), tot[NP + 1], c64[i][2], c32[i][2], 1e-5)
    assert torch.equal(part, k.critic_grad(pool, idx, eps2, policy_noise, noise_clip, GAMMA))   # fixed-order sums: the same bits twice
    off = (policy_noise * eps2.double()).clamp(-noise_clip, noise_clip)
    print("batch %d (%d, %d) %s / %s: noise clip active on %.1f %% of the components, a' exactly +-1 on %.1f %%" %
          (batch, D, A, regime, kind, 100 * (off.abs() == noise_clip).double().mean().item(), 100 * (a2.abs() == 1).double().mean().item()))
    return nets, nets64, pool, idx, eps2, data, off, a2, part


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("batch,obs_dim,act_dim", CASES)
def test_td3_critic_gradients_match_float64_autograd(batch, obs_dim, act_dim, regime):
    """Batches of a tile or less up to the grid-stride loop with a ragged last tile, both shapes, indices with repeats, in the three noise regimes."""
    import torch
    nets, _, pool, idx, eps2, data, off, _, part = _critic_case(batch, obs_dim, act_dim, regime)
    if regime == "clipped" and batch >= 127:
        assert (off.abs() == 0.5).double().mean().item() > 0.9
    if regime == "rare" and batch >= 127:
        assert (off.abs() == 0.5).double().mean().item() < 0.05
    if regime == "none":   # policy_noise = 0 is the unsmoothed target: whatever the noise tensor holds, the same bits
        k = _td3(obs_dim, act_dim)[-1]
        assert torch.equal(part, k.critic_grad(pool, idx, torch.zeros_like(eps2), 0.0, 0.5, GAMMA))
        assert torch.equal(part, k.critic_grad(pool, idx, 7.0 * eps2, 0.0, 0.0, GAMMA))


@pytest.mark.parametrize("obs_dim,act_dim", [(26, 6), (17, 7)])
def test_td3_critic_gradients_with_a_saturated_target_action(obs_dim, act_dim):
    """The target actor's output bias at +5 (even actions) and -5 (odd ones), noise 10 clipped at 0.5: the outer clip ends at exactly +-1 wherever the
    offset points outwards."""
    _, _, _, _, _, _, off, a2, _ = _critic_case(1000, obs_dim, act_dim, "clipped", "saturated")
    assert (a2.abs() == 1).double().mean().item() > 0.4 and a2.abs().max().item() == 1.0


def test_td3_critic_gradients_with_tied_target_critics():
    """target_qf2 is a copy of target_qf1: the minimum is a tie on every row, and no gradient depends on which side it takes."""
    import torch
    nets, _, _, _, eps2, data, _, _, _ = _critic_case(1000, 26, 6, "rare", "tied")
    from cassierl_amd import td3 as D3
    with torch.no_grad():
        a2 = D3.smoothed_target_action(nets[3], data[4], eps2, 0.2, 0.5)
        assert torch.equal(nets[4](data[4], a2), nets[5](data[4], a2))


@pytest.mark.parametrize("obs_dim,act_dim", [(26, 6), (17, 7)])
def test_td3_critic_gradient_clamps_wild_rows(obs_dim, act_dim):
    """Row numbers outside [0, capacity) give, bit for bit, the rows of the index clamped on the host."""
    import torch
    pool, g = TE._random_pool(obs_dim, act_dim)
    cap = pool.capacity
    idx = torch.tensor([-7, 0, 3, cap - 1, cap, cap + 1000, 2 ** 40, 17, 17], dtype=torch.int64, device="cuda")
    k = _td3(obs_dim, act_dim)[-1]
    eps2 = torch.randn(idx.numel(), act_dim, device="cuda", generator=g)
    a = k.critic_grad(pool, idx, eps2, 0.2, 0.5, GAMMA).clone()
    b = k.critic_grad(pool, idx.clamp(0, cap - 1), eps2, 0.2, 0.5, GAMMA).clone()
    assert torch.isfinite(a).all() and a.abs().max().item() > 0
    assert torch.equal(a, b)


@pytest.mark.parametrize("rows", [1, 64])
def test_td3_critic_apply_equals_two_ddpg_applies_bit_for_bit(rows):
    """Five steps on gradients spanning 1e-4 .. 1: both critics, their targets, both Adam states and the four statistics against CassieDdpgApply on the
    same blocks; then a step with tau = 0, which leaves the targets' bits."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import td3 as D3
    from cassierl_amd import trpo as T
    nets = _nets(26, 6, 4)
    ref = [copy.deepcopy(n) for n in nets]
    k = D3.Td3Kernels(*nets)
    kd = [G.DdpgKernels(ref[0], ref[1 + i], ref[3], ref[4 + i]) for i in range(2)]
    adam, adam_r = [G.new_adam(nets[1]), G.new_adam(nets[2])], [G.new_adam(ref[1]), G.new_adam(ref[2])]
    NQ = T.flat_params(nets[1]).numel()
    stats, want = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    lr, scale = 1e-3, 1.0 / 37
    torch.manual_seed(5)
    for t in range(1, 7):
        tau = 5e-3 if t < 6 else 0.0
        part = torch.randn(2, rows, NQ + 2, device="cuda") * 10.0 ** torch.randint(-4, 1, (NQ + 2,), device="cuda").float()   # gradients spanning 1e-4 .. 1
        targets = [T.flat_params(n).clone() for n in nets[4:]]
        k.critic_apply(part, scale, adam[0], adam[1], lr, 0.9, 0.999, 1e-8, tau, stats)
        for i in range(2):
            kd[i].apply(G.CRITIC, part[i], scale, adam_r[i], lr, 0.9, 0.999, 1e-8, tau, want[2 * i:])
        assert adam[0]["t"] == adam[1]["t"] == adam_r[0]["t"] == t
        for i in range(2):
            assert (T.flat_params(nets[4 + i]) != targets[i]).any().item() == (tau != 0.0)
            if tau == 0.0:
                assert torch.equal(T.flat_params(nets[4 + i]), targets[i])
            for a, b in ((nets[1 + i], ref[1 + i]), (nets[4 + i], ref[4 + i])):
                assert torch.equal(T.flat_params(a), T.flat_params(b)), (t, i)
            assert torch.equal(adam[i]["m"], adam_r[i]["m"]) and torch.equal(adam[i]["v"], adam_r[i]["v"]), (t, i)
        assert torch.equal(stats, want) and stats.abs().min().item() > 0
    assert not torch.equal(T.flat_params(nets[1]), T.flat_params(nets[2])) and torch.equal(T.flat_params(nets[0]), T.flat_params(ref[0]))


def test_td3_critic_apply_refuses_before_it_changes_anything():
    """Adam counters that differ, or a partial that is not one contiguous [2][rows][NPq + 2] block, raise ValueError with both counters, the
    Adam states and the critics as they were."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import td3 as D3
    from cassierl_amd import trpo as T
    nets = _nets(26, 6, 6)
    k = D3.Td3Kernels(*nets)
    adam = [G.new_adam(nets[1]), G.new_adam(nets[2])]
    NQ = T.flat_params(nets[1]).numel()
    before = [T.flat_params(n).clone() for n in nets]
    good = torch.randn(2, 3, NQ + 2, device="cuda")
    wide = torch.randn(2, 3, NQ + 3, device="cuda")
    bad = [wide[:, :, :NQ + 2], good[:, :, :NQ + 1].contiguous(), good[0], good.double(), good.cpu()]
    for part in bad:
        with pytest.raises(ValueError):
            k.critic_apply(part, 1.0, adam[0], adam[1], 1e-3, 0.9, 0.999, 1e-8, 5e-3)
    adam[1]["t"] = 1
    with pytest.raises(ValueError):
        k.critic_apply(good, 1.0, adam[0], adam[1], 1e-3, 0.9, 0.999, 1e-8, 5e-3)
    assert adam[0]["t"] == 0 and adam[1]["t"] == 1
    for a in adam:
        assert not a["m"].any().item() and not a["v"].any().item()
    for n, b in zip(nets, before):
        assert torch.equal(T.flat_params(n), b)
    adam[1]["t"] = 0
    k.critic_apply(good, 1.0, adam[0], adam[1], 1e-3, 0.9, 0.999, 1e-8, 5e-3)
    assert adam[0]["t"] == adam[1]["t"] == 1 and not torch.equal(T.flat_params(nets[1]), before[1])


@pytest.mark.parametrize("sigma", [0.1, 3.0])
@pytest.mark.parametrize("n", [33, 1000])
@pytest.mark.parametrize("control_mode,adim", [("PD", 6), ("OSC", 7)])
def test_td3_policy_step_matches_the_torch_statement(control_mode, adim, n, sigma):
    """CassieTd3PolicyStep as test_gpu_sac.test_sac_policy_step_matches_the_torch_statement; sigma 3 puts the clip to work on many components."""
    import torch
    from cassierl_amd import td3 as D3
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env import action_space
    pol, qf1, qf2, _, _, _ = _nets(26, adim, 7)
    pol64 = copy.deepcopy(pol).double()
    box = action_space(control_mode)
    amap = T.NormalizedActions(box.low, box.high, "cuda")
    algo = D3.TD3(None, None, pol, qf1, qf2, n, 26, amap, replay_pool_size=3 * n, exploration_sigma=sigma)
    fused = algo._fused_step(torch.device("cuda:0"))
    assert fused is not None
    step = fused[0]
    pool = algo.pool
    lo, hi = torch.as_tensor(box.low, device="cuda"), torch.as_tensor(box.high, device="cuda")
    exact = 0
    for top in (n, 2 * n, 0):   # the middle of the ring, an append that ends exactly at capacity, the next one at 0
        for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs):
            t.copy_(torch.randn_like(t))
        before = [t.clone() for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs)]
        obs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
        noise = torch.randn(n, adim, device="cuda")
        with torch.no_grad():
            a32 = algo._explore(obs.float(), noise)
            a64 = (pol64(obs.float().double()) + sigma * noise.double()).clamp(-1, 1)   # the statement's input is the float32 observation
        step(obs, noise, top)
        act = pool.act[top:top + n]
        assert torch.equal(pool.obs[top:top + n], obs.float())
        TE._check("policy step n %d A %d top %d sigma %g, actions" % (n, adim, top, sigma), act, a64, a32, 5e-6, plus=1.0)
        assert act.min().item() >= -1.0 and act.max().item() <= 1.0
        assert (algo._env_actions - amap(act)).abs().max().item() < 1e-12
        assert (algo._env_actions >= lo).all() and (algo._env_actions <= hi).all()
        rest = torch.ones(pool.capacity, dtype=torch.bool, device="cuda")
        rest[top:top + n] = False
        for now, was in zip((pool.obs, pool.act), before[:2]):
            assert torch.equal(now[rest], was[rest])
        for now, was in zip((pool.rew, pool.term, pool.nobs), before[2:]):   # the policy step opens the rows; the commit fills these
            assert torch.equal(now, was)
        exact += int((act.abs() == 1).sum().item())
    print("policy step n %d A %d sigma %g: %d of %d actions exactly +-1" % (n, adim, sigma, exact, 3 * n * adim))
    if sigma == 3.0:   # |mu + 3 n| >= 1 wherever |n| >= 2 / 3 at the least: about half of the components
        assert exact > 0.3 * 3 * n * adim


def test_fused_update_equals_the_torch_update_on_stand_data():
    """1024 stand environments, Torque mode, 8 vector steps into the pool, then four updates of batch 1024 with policy_delay 2 by the kernels and by
    td3_update_torch_ from the same state, indices and noises.  The kernels make 2 library calls on an update that leaves the actor alone and 4 on a
    delayed one, and the former leaves the actor and all three targets with the bits they had."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import td3 as D3
    from cassierl_amd import trpo as T
    from cassierl_amd.trajectory import default_gait
    algo = D3.make_cassie_td3(1024, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, replay_pool_size=1024 * 8, batch_size=1024,
                              min_pool_size=10 ** 9, policy_delay=2)
    for _ in range(8):
        assert algo.train_step() == 0
    assert algo.last_policy_step_fused and algo.pool.size == 1024 * 8 and algo.pool.top == 0
    assert torch.isfinite(algo.pool.obs).all() and torch.isfinite(algo.pool.nobs).all() and torch.isfinite(algo.pool.rew).all()
    assert algo.pool.act.abs().max().item() <= 1.0 and algo.pool.act.std().item() > 0.05
    nets = (algo.policy, algo.qf1, algo.qf2, algo.target_policy, algo.target_qf1, algo.target_qf2)
    state0 = [copy.deepcopy(n.state_dict()) for n in nets]
    theta0 = [T.flat_params(n).clone() for n in nets]
    draws = [(algo.sample_indices(), algo.sample_noise()) for _ in range(4)]
    calls = []

    def reset():
        for n, sd in zip(nets, state0):
            n.load_state_dict(sd)
        algo.adam_mu, algo.adam_q1, algo.adam_q2 = G.new_adam(algo.policy), G.new_adam(algo.qf1), G.new_adam(algo.qf2)
        algo.n_updates = 0

    reset()
    for idx, noise in draws[:2]:   # the partial-sum buffers of this batch size exist from here on
        algo.update(idx, noise)
    k = algo._update_kernels()
    for name, fn in list(k.fn.items()):
        k.fn[name] = (lambda name, fn: lambda *a: (calls.append(name), fn(*a))[1])(name, fn)
    res = {}
    for fused in (True, False):
        reset()
        algo.fused_update = fused
        for u, (idx, noise) in enumerate(draws):
            still = [T.flat_params(n).clone() for n in (nets[0], nets[3], nets[4], nets[5])]
            del calls[:]
            algo.update(idx, noise)
            assert algo.last_update_kind == ("td3_kernels" if fused else "torch") and algo.n_updates == u + 1
            if fused:
                assert calls == (["Td3CriticGrad", "Td3CriticApply"] if u % 2 == 0 else ["Td3CriticGrad", "Td3CriticApply", "ActorGrad", "Apply"]), calls
            same = [torch.equal(a, T.flat_params(n)) for a, n in zip(still, (nets[0], nets[3], nets[4], nets[5]))]
            assert same == [u % 2 == 0] * 4, (fused, u, same)
        assert algo.adam_mu["t"] == 2 and algo.adam_q1["t"] == algo.adam_q2["t"] == 4
        res[fused] = [T.flat_params(n).clone() for n in nets]
    rels = [((a - b).norm() / b.norm()).item() for a, b in zip(res[True], res[False])]
    moved = [(a - t0).norm().item() for a, t0 in zip(res[False], theta0)]
    print("fused vs torch update, relative difference (actor, qf1, qf2, target actor, target_qf1, target_qf2): %s; moved by %s" % (rels, moved))
    assert all(m > 0 for m in moved)
    assert all(r < 1e-5 for r in rels), rels
    algo.env.close()


# ------------------------------------------------------------------------------------------------------------------ front ends
NP_ALL = 2 * 2118 + 4 * 2145   # actor, two critics and a target of each
LOSSES = ("avg_reward", "qf1_loss", "qf2_loss", "avg_q1", "avg_q2", "policy_surr", "episodes", "actor_updates")


def test_train_td3_runs_the_kernels_and_the_torch_update():
    from conftest import ROOT
    script = os.path.join(ROOT, "train_td3.py")
    for extra, kind in (([], "td3_kernels"), (["--torch-update"], "torch")):
        st = _run([sys.executable, script, "--n-epochs", "2"] + extra + _small(256))
        assert len(st) == 2 and st[-1]["update_kind"] == kind and st[0]["updates"] == 5 and st[-1]["updates"] == 6
        assert st[0]["actor_updates"] == 2 and st[-1]["actor_updates"] == 3   # updates 1 and 3 of the first five, then 5, 7 and 9
        for key in LOSSES:
            assert np.isfinite(st[-1][key]), (key, st[-1])
        assert st[-1]["qf1_loss"] > 0 and st[-1]["qf2_loss"] > 0


def test_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    """train_td3.py: two epochs, snapshot, one more epoch in a fresh process == three epochs uninterrupted, bit for bit (the ring wraps at 8 steps,
    paths are truncated at 10; the snapshot is taken after 11 updates, an odd number)."""
    from conftest import ROOT
    script = os.path.join(ROOT, "train_td3.py")
    small = _small(1024)
    snap, b, c = str(tmp_path / "snap.pt"), str(tmp_path / "b.npy"), str(tmp_path / "c.npy")
    _run([sys.executable, script, "--n-epochs", "2", "--snapshot", snap] + small)
    sb = _run([sys.executable, script, "--n-epochs", "1", "--load-policy", snap, "--dump-params", b] + small)
    sc = _run([sys.executable, script, "--n-epochs", "3", "--dump-params", c] + small)
    assert sb[0]["sampler_restored"] and sb[0]["pool_restored"] and sb[0]["pool_size"] == 1024 * 8
    last_b, last_c = sb[-1], sc[-1]
    assert last_b["itr"] == last_c["itr"] == 2 and last_b["updates"] == last_c["updates"] == 6 and last_c["update_kind"] == "td3_kernels"
    for key in LOSSES:
        assert last_b[key] == last_c[key], (key, last_b[key], last_c[key])
    tb, tc = np.load(b), np.load(c)
    assert tb.size == NP_ALL and np.isfinite(tc).all()
    assert np.array_equal(tb, tc)


def test_two_rank_td3_keeps_identical_parameters(tmp_path):
    """train_td3.py on two ranks with 1024 envs each (both on device 0, gloo): finite, identical parameters on both ranks."""
    from conftest import ROOT
    script = os.path.join(ROOT, "train_td3.py")
    out = str(tmp_path / "two.npy")
    env = dict(os.environ, CASSIE_DEVICE_MAP="0,0", CASSIE_BACKEND="gloo")
    args = _small(2048)   # the batch is counted over the two ranks
    st = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
               script, "--n-epochs", "2", "--dump-params", out] + args, timeout=900, env=env)
    assert len(st) == 2 and st[-1]["updates"] == 6 and st[-1]["env_steps"] == 2 * 1024 * 6 and st[-1]["update_kind"] == "td3_kernels"
    t0, t1 = np.load(out), np.load(out + ".rank1.npy")
    assert t0.size == NP_ALL and np.isfinite(t0).all() and np.isfinite(t1).all()
    assert np.array_equal(t0, t1)


def test_sim_policy_rolls_out_a_td3_snapshot(tmp_path):
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    _run([sys.executable, os.path.join(ROOT, "train_td3.py"), "--envs-per-gpu", "512", "--batch-size", "512", "--pool-size", "4096", "--min-pool-size", "1024",
          "--epoch-length", "4", "--n-epochs", "2", "--kind", "stand", "--control-mode", "Torque", "--snapshot", snap])
    assert os.path.exists(snap)
    r = _run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "256", "--max-path-length", "60", "--kind", "stand", "--control-mode", "Torque"])[-1]
    assert r["itr"] == 2 and r["envs"] == 256 and r["deterministic"] and 0 < r["avg_path_length"] <= 60 and np.isfinite(r["avg_return"])
    assert np.isfinite(r["min_return"]) and np.isfinite(r["max_return"])
