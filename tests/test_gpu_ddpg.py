"""DDPG's kernels (csrc/tu_ddpg.hip) against the torch statements of cassierl_amd/ddpg.py, and train_ddpg.py / sim_policy.py on the GPU.  -m gpu only.

Tolerances are those of tests/test_gpu_vpg.py for the same kind of comparison: float32 rounding bounds, not measurements."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _nets(D, A, seed, dtype=None):
    """Actor, critic and their targets: HeUniform hidden weights, biases N(0, 0.1); output layers wide enough (+-0.3) that mu(s) and dQ/da are not
    rounding noise, the critic's output bias at 0.5 so that mean Q is O(1); the targets are other draws."""
    import torch
    from cassierl_amd import ddpg as G
    torch.manual_seed(seed)
    out = []
    for k in range(2):
        pol, qf = G.DeterministicMLPPolicy(D, A), G.ContinuousMLPQFunction(D, A)
        with torch.no_grad():
            for net in (pol, qf):
                for lin in (net.l1, net.l2, net.l3):
                    lin.bias.copy_(0.1 * torch.randn_like(lin.bias))
                net.l3.weight.uniform_(-0.3, 0.3)
            qf.l3.bias.fill_(0.5)
        out += [pol.cuda(), qf.cuda()]
    return out   # actor, critic, target actor, target critic


def _margin_ok(pol, qf, obs, act, eps=1e-4):
    """Rows whose hidden pre-activations (float64 reference: live actor, live critic at (s, a) and at (s, mu(s))) all keep |z| >= eps: a
    pre-activation within rounding of zero can take different sides in the kernel and in torch, which changes that sample's gradient by O(1)."""
    import copy
    import torch
    p, q = copy.deepcopy(pol).double(), copy.deepcopy(qf).double()
    o, a = obs.double(), act.double()
    with torch.no_grad():
        z1 = p.l1(o); z2 = p.l2(z1.relu())
        mu = torch.tanh(p.l3(z2.relu()))
        y1 = q.l1(o)
        y2 = q.l2(torch.cat([y1.relu(), a], 1)); y2m = q.l2(torch.cat([y1.relu(), mu], 1))
        return torch.stack([(z.abs() >= eps).all(1) for z in (z1, z2, y1, y2, y2m)]).all(0)


def _pool_with_margin(pol, qf, D, A, candidates=40000, seed=11):
    """A full ReplayPool built by rejection (the ReLU condition above); returns (pool, fraction dropped)."""
    import torch
    from cassierl_amd import ddpg as G
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = 0.7 * torch.randn(candidates, D, device="cuda", generator=g)
    act = torch.rand(candidates, A, device="cuda", generator=g) * 2 - 1
    keep = _margin_ok(pol, qf, obs, act)
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


def _algo(n, control_mode, adim, cap_steps=3, seed=7):
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env import action_space
    pol, qf, _, _ = _nets(26, adim, seed)
    box = action_space(control_mode)
    amap = T.NormalizedActions(box.low, box.high, "cuda")
    return G.DDPG(None, None, pol, qf, n, 26, amap, replay_pool_size=cap_steps * n), box, amap


@pytest.mark.parametrize("n", [5000, 65536])
@pytest.mark.parametrize("control_mode,adim", [("PD", 6), ("OSC", 7)])
def test_ddpg_policy_step_matches_the_torch_statement(control_mode, adim, n):
    import torch
    from cassierl_amd import ddpg as G
    algo, box, amap = _algo(n, control_mode, adim)
    fused = algo._fused_step(torch.device("cuda:0"))
    assert fused is not None
    step = fused[0]
    pool = algo.pool
    lo, hi = torch.as_tensor(box.low, device="cuda"), torch.as_tensor(box.high, device="cuda")
    for top in (n, 2 * n, 0):   # the middle of the ring, an append that ends exactly at capacity, the next one at 0
        for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs):
            t.copy_(torch.randn_like(t))
        before = [t.clone() for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs)]
        obs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
        noise = torch.randn(n, adim, device="cuda")
        algo.path_t = torch.randint(0, 3, (n,), device="cuda", dtype=torch.int64)
        algo.ou.state = 0.3 * torch.randn(n, adim, device="cuda")
        ref = G.OUStrategy(n, adim, "cuda")
        ref.state = algo.ou.state.clone()
        a_ref = ref.get_action(algo.policy(obs.float()), noise, algo.path_t == 0)
        step(obs, noise, top)
        act = pool.act[top:top + n]
        assert torch.equal(pool.obs[top:top + n], obs.float())
        assert (act - a_ref).abs().max().item() < 5e-6 * (1 + a_ref.abs().max().item())
        assert act.min().item() >= -1.0 and act.max().item() <= 1.0
        assert (algo.ou.state - ref.state).abs().max().item() < 5e-6
        assert (algo._env_actions - amap(act)).abs().max().item() < 1e-12
        assert (algo._env_actions >= lo).all() and (algo._env_actions <= hi).all()
        rest = torch.ones(pool.capacity, dtype=torch.bool, device="cuda")
        rest[top:top + n] = False
        for now, was in zip((pool.obs, pool.act), before[:2]):
            assert torch.equal(now[rest], was[rest])
        for now, was in zip((pool.rew, pool.term, pool.nobs), before[2:]):   # the policy step opens the rows; the commit fills these
            assert torch.equal(now, was)


@pytest.mark.parametrize("n", [5000, 65536])
def test_ddpg_pool_commit_matches_the_torch_statement(n):
    import torch
    from cassierl_amd import ddpg as G
    algo, _, _ = _algo(n, "PD", 6)
    commit = algo._fused_step(torch.device("cuda:0"))[1]
    pool = algo.pool
    for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs):
        t.copy_(torch.randn_like(t))
    before = [t.clone() for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs)]
    rew = torch.randn(n, dtype=torch.float64, device="cuda") * 3
    done = (torch.rand(n, device="cuda") < 0.3).to(torch.uint8)
    nobs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
    top = 2 * n
    commit(rew, done, nobs, top)
    ref = G.ReplayPool(pool.capacity, n, 26, 6, "cuda")
    for t, b in zip((ref.obs, ref.act, ref.rew, ref.term, ref.nobs), before):
        t.copy_(b)
    ref.write(top, before[0][top:top + n], before[1][top:top + n], (algo.scale_reward * rew.double()).float(), (done != 0).float(), nobs.float())
    for a, b in zip((pool.obs, pool.act, pool.rew, pool.term, pool.nobs), (ref.obs, ref.act, ref.rew, ref.term, ref.nobs)):
        assert torch.equal(a, b)
    assert pool.term[top:top + n].sum().item() == done.sum().item()


@pytest.mark.parametrize("batch,obs_dim,act_dim", [(1000, 26, 6), (65536, 26, 6), (4099, 26, 7), (777, 17, 6)])
def test_ddpg_gradients_match_autograd(batch, obs_dim, act_dim):
    """CassieDdpgCriticGrad and CassieDdpgActorGrad against float32 autograd on the gathered batch; indices with repeats; 4099 and 777 end in a
    tile that is not a multiple of 32.  The pool is built by rejection (ReLU condition, _margin_ok)."""
    import torch
    from cassierl_amd import ddpg as G
    pol, qf, tpol, tqf = _nets(obs_dim, act_dim, 3)
    pool, dropped = _pool_with_margin(pol, qf, obs_dim, act_dim)
    print("ReLU margin: %.2f %% of the candidate rows dropped" % (100 * dropped))
    assert dropped <= 0.03
    k = G.DdpgKernels(pol, qf, tpol, tqf)
    g = torch.Generator(device="cuda").manual_seed(5)
    idx = torch.randint(0, pool.size, (batch,), device="cuda", generator=g)
    idx[1] = idx[0]
    assert idx.unique().numel() < batch
    s, a, r, term, s2 = pool.sample(idx)
    gamma = 0.99
    # ---- critic
    with torch.no_grad():
        y = r + (1 - term) * gamma * tqf(s2, tpol(s2))
    q = qf(s, a)
    loss = ((q - y) ** 2).mean()
    gref = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(qf.parameters()))])
    part = k.critic_grad(pool, idx, gamma).clone()
    NP = gref.numel()
    assert part.shape == (k.L.CassieDdpgPartialRows(batch), NP + 2)
    tot = part.double().sum(0)
    gf = (tot[:NP] / batch).float()
    err = (gf - gref).abs().max().item()
    print("critic gradient: max error %.3g of max %.3g; loss %.8g / %.8g; mean Q %.8g / %.8g" %
          (err, gref.abs().max().item(), tot[NP].item() / batch, loss.item(), tot[NP + 1].item() / batch, q.double().mean().item()))
    assert err < 2e-4 * gref.abs().max().item()
    assert abs(tot[NP].item() / batch - loss.double().item()) < 1e-5 * abs(loss.item())
    assert abs(tot[NP + 1].item() / batch - q.double().mean().item()) < 1e-5 * abs(q.double().mean().item())
    assert torch.equal(part, k.critic_grad(pool, idx, gamma))   # fixed-order sums: the same bits twice
    # ---- actor
    qa = qf(s, pol(s))
    surr = -qa.mean()
    gref = torch.cat([x.reshape(-1) for x in torch.autograd.grad(surr, list(pol.parameters()))])
    part = k.actor_grad(pool, idx).clone()
    NP = gref.numel()
    assert part.shape == (k.L.CassieDdpgPartialRows(batch), NP + 1)
    tot = part.double().sum(0)
    gf = (tot[:NP] / batch).float()
    err = (gf - gref).abs().max().item()
    print("actor gradient: max error %.3g of max %.3g; mean Q(s, mu(s)) %.8g / %.8g" % (err, gref.abs().max().item(), tot[NP].item() / batch, qa.double().mean().item()))
    assert err < 2e-4 * gref.abs().max().item()
    assert abs(tot[NP].item() / batch - qa.double().mean().item()) < 1e-5 * abs(qa.double().mean().item())
    assert torch.equal(part, k.actor_grad(pool, idx))


@pytest.mark.parametrize("rows", [1, 64])
@pytest.mark.parametrize("which", [0, 1])
def test_ddpg_apply_matches_adam_and_the_soft_update(which, rows):
    import copy
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import trpo as T
    pol, qf, tpol, tqf = _nets(26, 6, 4)
    k = G.DdpgKernels(pol, qf, tpol, tqf)
    live, targ = (pol, tpol) if which == G.ACTOR else (qf, tqf)
    live_r, targ_r = copy.deepcopy(live), copy.deepcopy(targ)
    adam, adam_r = G.new_adam(live), G.new_adam(live_r)
    NP, ns = T.flat_params(live).numel(), 1 if which == G.ACTOR else 2
    stats = torch.zeros(ns, dtype=torch.float64, device="cuda")
    lr, tau, scale, want = 1e-3, 1e-3, 1.0 / 37, torch.zeros(ns, dtype=torch.float64, device="cuda")
    torch.manual_seed(5)
    for t in range(1, 6):
        part = torch.randn(rows, NP + ns, device="cuda") * 10.0 ** torch.randint(-4, 1, (NP + ns,), device="cuda").float()   # gradients spanning 1e-4 .. 1
        k.apply(which, part, scale, adam, lr, 0.9, 0.999, 1e-8, tau, stats)
        G._adam_on(live_r, part[:, :NP].sum(0) * scale, adam_r, lr, 0.9, 0.999, 1e-8)
        G.soft_update_(targ_r, live_r, tau)
        want += part[:, NP:].double().sum(0)
        assert adam["t"] == adam_r["t"] == t
    for a, b in ((T.flat_params(live), T.flat_params(live_r)), (adam["m"], adam_r["m"]), (adam["v"], adam_r["v"]), (T.flat_params(targ), T.flat_params(targ_r))):
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item(), ((a - b).abs().max().item(), b.abs().max().item())
    assert (stats - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_fused_update_equals_the_torch_update_on_stand_data():
    """4096 stand environments, Torque mode, 8 vector steps into the pool, then three updates of batch 4096 with fused_update True and False from
    the same state and the same indices."""
    import copy
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import trpo as T
    from cassierl_amd.trajectory import default_gait
    algo = G.make_cassie_ddpg(4096, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, replay_pool_size=4096 * 8, batch_size=4096,
                              min_pool_size=10 ** 9)
    for _ in range(8):
        assert algo.train_step() == 0
    assert algo.last_policy_step_fused and algo.pool.size == 4096 * 8 and algo.pool.top == 0
    assert torch.isfinite(algo.pool.obs).all() and torch.isfinite(algo.pool.nobs).all() and torch.isfinite(algo.pool.rew).all()
    nets = (algo.policy, algo.qf, algo.target_policy, algo.target_qf)
    state0 = [copy.deepcopy(n.state_dict()) for n in nets]
    theta0 = [T.flat_params(n).clone() for n in nets]
    idxs = [algo.sample_indices() for _ in range(3)]
    res = {}
    for fused in (True, False):
        for n, sd in zip(nets, state0):
            n.load_state_dict(sd)
        algo.adam_mu, algo.adam_q = G.new_adam(algo.policy), G.new_adam(algo.qf)
        algo.fused_update = fused
        for idx in idxs:
            algo.update(idx)
            assert algo.last_update_kind == ("ddpg_kernels" if fused else "torch")
        res[fused] = [T.flat_params(n).clone() for n in nets]
    rels = [((a - b).norm() / b.norm()).item() for a, b in zip(res[True], res[False])]
    moved = [(a - t0).norm().item() for a, t0 in zip(res[False], theta0)]
    print("fused vs torch update, relative parameter difference (actor, critic, target actor, target critic): %s; moved by %s" % (rels, moved))
    assert all(m > 0 for m in moved)
    assert all(r < 1e-5 for r in rels), rels
    algo.env.close()


def _run(cmd, timeout=600, env=None):
    p = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, capture_output=True, text=True, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-2500:])
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


def _small(batch):
    return ["--envs-per-gpu", "1024", "--batch-size", str(batch), "--pool-size", str(1024 * 8), "--min-pool-size", "2048", "--epoch-length", "6",
            "--max-path-length", "10", "--kind", "stand", "--control-mode", "Torque"]


_SMALL = _small(1024)


def test_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    """train_ddpg.py: two epochs, snapshot, one more epoch in a fresh process == three epochs uninterrupted, bit for bit (the ring wraps at 8 steps,
    paths are truncated at 10)."""
    from conftest import ROOT
    script = os.path.join(ROOT, "train_ddpg.py")
    snap, b, c = str(tmp_path / "snap.pt"), str(tmp_path / "b.npy"), str(tmp_path / "c.npy")
    _run([sys.executable, script, "--n-epochs", "2", "--snapshot", snap] + _SMALL)
    sb = _run([sys.executable, script, "--n-epochs", "1", "--load-policy", snap, "--dump-params", b] + _SMALL)
    sc = _run([sys.executable, script, "--n-epochs", "3", "--dump-params", c] + _SMALL)
    assert sb[0]["sampler_restored"] and sb[0]["pool_restored"] and sb[0]["pool_size"] == 1024 * 8
    last_b, last_c = sb[-1], sc[-1]
    assert last_b["itr"] == last_c["itr"] == 2 and last_b["updates"] == last_c["updates"] == 6 and last_c["update_kind"] == "ddpg_kernels"
    for key in ("avg_reward", "qf_loss", "policy_surr", "avg_q", "episodes"):
        assert last_b[key] == last_c[key], (key, last_b[key], last_c[key])
    tb, tc = np.load(b), np.load(c)
    assert tb.size == 2 * (2118 + 2145) and np.isfinite(tc).all()
    assert np.array_equal(tb, tc)


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_two_rank_ddpg_keeps_identical_parameters(tmp_path):
    """train_ddpg.py on two ranks with 1024 envs each (both on device 0, gloo): finite, identical parameters on both ranks."""
    from conftest import ROOT
    script = os.path.join(ROOT, "train_ddpg.py")
    out = str(tmp_path / "two.npy")
    env = dict(os.environ, CASSIE_DEVICE_MAP="0,0", CASSIE_BACKEND="gloo")
    args = _small(2048)   # the batch is counted over the two ranks
    st = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
               script, "--n-epochs", "2", "--dump-params", out] + args, timeout=900, env=env)
    assert len(st) == 2 and st[-1]["updates"] == 6 and st[-1]["env_steps"] == 2 * 1024 * 6 and st[-1]["update_kind"] == "ddpg_kernels"
    t0, t1 = np.load(out), np.load(out + ".rank1.npy")
    assert t0.size == 2 * (2118 + 2145) and np.isfinite(t0).all() and np.isfinite(t1).all()
    assert np.array_equal(t0, t1)


def test_sim_policy_rolls_out_a_ddpg_snapshot(tmp_path):
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    _run([sys.executable, os.path.join(ROOT, "train_ddpg.py"), "--envs-per-gpu", "512", "--batch-size", "512", "--pool-size", "4096", "--min-pool-size", "1024",
          "--epoch-length", "4", "--n-epochs", "2", "--kind", "stand", "--control-mode", "Torque", "--snapshot", snap])
    assert os.path.exists(snap)
    r = _run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "256", "--max-path-length", "60", "--kind", "stand", "--control-mode", "Torque"])[-1]
    assert r["itr"] == 2 and r["envs"] == 256 and r["deterministic"] and 0 < r["avg_path_length"] <= 60 and np.isfinite(r["avg_return"])
    assert np.isfinite(r["min_return"]) and np.isfinite(r["max_return"])


def test_ddpg_update_timing_batch_65536():
    """One fused update at batch 65 536 against the torch statement, alternated, median of 20 synchronised repeats after warm-up.  A guard, not the
    measurement (tools/ab_ddpg_update.py): the kernels replace dozens of launches with four, so losing to torch means a broken kernel."""
    import torch
    from cassierl_amd import ddpg as G
    pol, qf, tpol, tqf = _nets(26, 6, 9)
    pool, _ = _pool_with_margin(pol, qf, 26, 6, candidates=200000)
    k = G.DdpgKernels(pol, qf, tpol, tqf)
    idx = torch.randint(0, pool.size, (65536,), device="cuda")
    adam = {True: (G.new_adam(pol), G.new_adam(qf)), False: (G.new_adam(pol), G.new_adam(qf))}

    def fused():
        k.update(pool, idx, 0.99, 1e-3, 1e-4, 1e-3, *adam[True])

    def torch_update():
        G.ddpg_update_torch_(pol, qf, tpol, tqf, *adam[False], pool.sample(idx), 0.99, 1e-3, 1e-4, 1e-3)

    out = {}
    for name, fn in (("fused", fused), ("torch", torch_update)) * 2:   # alternated, the second round kept
        for _ in range(5):
            fn()
        ts = []
        for _ in range(20):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        out[name] = float(np.median(ts)) * 1e3
    print("DDPG update ms at batch 65536: %s" % out)
    assert out["fused"] < out["torch"]
