"""VPG's width-128 kernels (csrc/tu_pg.hip) against the torch operations they replace, and train_vpg.py on the GPU.  -m gpu only."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _policy(obs_dim, act_dim, seed, jitter=0.05):
    import torch
    from cassierl_amd import trpo as T
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(obs_dim, act_dim, (128, 128), init_std=1.0).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(jitter * torch.randn_like(p))
    return pol


@pytest.mark.parametrize("n", [5000, 65536])
@pytest.mark.parametrize("control_mode,adim", [("PD", 6), ("OSC", 7)])
def test_pg_policy_step_matches_the_torch_operations(control_mode, adim, n):
    import torch
    from cassierl_amd import trpo as T
    from cassierl_amd import vpg as V
    from cassierl_amd.vec_env import action_space
    pol = _policy(26, adim, 7)
    box = action_space(control_mode)
    amap = T.NormalizedActions(box.low, box.high, "cuda")
    algo = V.VPG(None, None, pol, T.LinearFeatureBaseline(), n, 26, amap)
    step = algo._fused_policy_step(torch.device("cuda:0"), torch.float32)
    assert step is not None
    obs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
    noise = torch.randn(n, adim, device="cuda")
    o32, mean, act = torch.empty(n, 26, device="cuda"), torch.empty(n, adim, device="cuda"), torch.empty(n, adim, device="cuda")
    step(obs, noise, o32, mean, act)
    a_ref, m_ref, _ = pol.get_actions(obs.float(), noise=noise)
    assert torch.equal(o32, obs.float())
    assert (mean - m_ref).abs().max().item() < 5e-6 * (1 + m_ref.abs().max().item())
    assert (act - a_ref).abs().max().item() < 5e-6 * (1 + a_ref.abs().max().item())
    assert (algo._env_actions - amap(act)).abs().max().item() < 1e-12
    lo, hi = torch.as_tensor(box.low, device="cuda"), torch.as_tensor(box.high, device="cuda")
    assert (algo._env_actions >= lo).all() and (algo._env_actions <= hi).all()


@pytest.mark.parametrize("n,obs_dim,act_dim", [(1000, 26, 6), (65536, 26, 6), (4099, 26, 7), (777, 17, 6)])
def test_pg_vjp_matches_autograd(n, obs_dim, act_dim):
    """J' w of the 128-128 mean network; 4099 and 777 end in a tile that is not a multiple of 32 (and in a group of fewer than four tiles)."""
    import torch
    from cassierl_amd import vpg as V
    pol = _policy(obs_dim, act_dim, 3, jitter=0.1)
    obs = torch.randn(n, obs_dim, device="cuda") * 0.7
    pk = V.PolicyGradKernels(pol, obs)
    assert pk.kind == "pg_vjp"
    w = torch.randn(n, act_dim, device="cuda") / n
    mean, _ = pol.dist_info(obs)
    g = torch.autograd.grad((mean * w).sum(), list(pol.parameters()), allow_unused=True)
    gref = torch.cat([torch.zeros_like(p).reshape(-1) if x is None else x.reshape(-1) for x, p in zip(g, pol.parameters())])
    gf = pk._pg_vjp(w)
    assert (gref - gf).abs().max().item() < 2e-4 * gref.abs().max().item()
    assert torch.equal(gf, pk._pg_vjp(w))   # fixed-order sums: the same bits twice


def test_pg_adam_matches_the_torch_adam():
    import torch
    from cassierl_amd import vpg as V
    torch.manual_seed(5)
    n = 20748
    th0 = torch.randn(n, device="cuda")
    ths, ms, vs = th0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    thf, mf, vf = th0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for t in range(1, 6):
        g = torch.randn(n, device="cuda") * 10.0 ** torch.randint(-4, 1, (n,), device="cuda").float()
        V.adam_step_(ths, g, ms, vs, t, 1e-3)
        V.fused_adam_step_(thf, g, mf, vf, t, 1e-3)
    for a, b in ((thf, ths), (mf, ms), (vf, vs)):   # relative to each tensor's scale: a few float32 ulps (contraction, division order)
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item(), ((a - b).abs().max().item(), b.abs().max().item())


def test_fused_update_equals_the_torch_update_on_one_stand_batch():
    """One batch collected on the stand env (4096 envs, horizon 4); the fused update (CassiePgVjp + CassiePgAdam) and the forced-torch update
    (autograd + torch Adam) start from the same parameters and the same batch, so env chaos cannot enter."""
    import torch
    from cassierl_amd import trpo as T
    from cassierl_amd import vpg as V
    from cassierl_amd.trajectory import default_gait
    algo = V.make_cassie_vpg(4096, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, batch_size=4096 * 4)
    d = algo.process(algo.collect())
    theta0 = T.flat_params(algo.policy).clone()
    res = {}
    for fused in (True, False):
        T.set_flat_params(algo.policy, theta0)
        algo.adam_t, algo.adam_m, algo.adam_v = 0, None, None
        algo.fused_grad = algo.fused_adam = fused
        st = algo.optimize(d)
        assert algo.last_grad_kind == ("pg_vjp" if fused else "autograd") and algo.last_adam_fused == fused
        res[fused] = (T.flat_params(algo.policy).clone(), st)
    (tf, sf), (tt, stt) = res[True], res[False]
    assert abs(sf["grad_norm"] - stt["grad_norm"]) < 1e-5 * stt["grad_norm"]
    rel = ((tf - tt).norm() / tt.norm()).item()
    print("fused vs torch update: relative parameter difference %.3g, step norms %.6g / %.6g" % (rel, sf["step_norm"], stt["step_norm"]))
    assert rel < 1e-5
    algo.env.close()


def test_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    import torch
    from cassierl_amd import trpo as T
    from cassierl_amd import vpg as V
    from cassierl_amd.trajectory import default_gait
    mk = lambda: V.make_cassie_vpg(1024, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, batch_size=1024 * 4)
    a = mk()
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ref = a.train_iteration()
    ta = T.flat_params(a.policy).clone()
    a.env.close()
    b = mk()
    _, restored = b.load(p)
    assert restored and b.adam_t == 2
    got = b.train_iteration()
    assert got["itr"] == ref["itr"] == 2
    assert got["avg_reward"] == ref["avg_reward"] and got["grad_norm"] == ref["grad_norm"]
    assert torch.equal(T.flat_params(b.policy), ta)
    b.env.close()


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_two_rank_vpg_iterations_equal_the_one_rank_run(tmp_path):
    """train_vpg.py: two ranks with 2048 envs each (both on device 0, gloo) against one rank with the same 4096 global env ids."""
    from conftest import ROOT
    script = os.path.join(ROOT, "train_vpg.py")
    common = ["--horizon", "4", "--n-itr", "2", "--kind", "stand", "--control-mode", "Torque"]
    one, two = str(tmp_path / "one.npy"), str(tmp_path / "two.npy")
    p1 = subprocess.run([sys.executable, script, "--envs-per-gpu", "4096", "--dump-params", one] + common, capture_output=True, text=True, timeout=900)
    assert p1.returncode == 0, p1.stderr[-2000:]
    env = dict(os.environ, CASSIE_DEVICE_MAP="0,0", CASSIE_BACKEND="gloo")
    p2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", str(_free_port()), script, "--envs-per-gpu", "2048", "--dump-params", two] + common,
                        capture_output=True, text=True, timeout=900, env=env)
    assert p2.returncode == 0, p2.stderr[-2000:]
    s1 = [json.loads(l) for l in p1.stdout.splitlines() if l.startswith("{")]
    s2 = [json.loads(l) for l in p2.stdout.splitlines() if l.startswith("{")]
    assert len(s1) == len(s2) == 2
    for a, b in zip(s1, s2):
        assert a["env_steps"] == b["env_steps"] == 4096 * 4 and a["gathered"] == b["gathered"] == 4096 and a["episodes"] == b["episodes"]
        assert abs(a["avg_reward"] - b["avg_reward"]) < 1e-6 and abs(a["grad_norm"] - b["grad_norm"]) < 1e-4 * a["grad_norm"]
    t1, t2 = np.load(one), np.load(two)
    assert t1.size == 26 * 128 + 128 + 128 * 128 + 128 + 6 * 128 + 6 + 6
    assert np.abs(t1 - t2).max() < 1e-4 * max(1.0, np.abs(t1).max()), np.abs(t1 - t2).max()


def test_sim_policy_rolls_out_a_vpg_snapshot(tmp_path):
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_vpg.py"), "--envs-per-gpu", "512", "--horizon", "4", "--n-itr", "2", "--kind", "stand",
                        "--control-mode", "Torque", "--snapshot", snap], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and os.path.exists(snap), p.stderr[-2000:]
    q = subprocess.run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "256", "--max-path-length", "60", "--kind", "stand",
                        "--control-mode", "Torque"], capture_output=True, text=True, timeout=900)
    assert q.returncode == 0, q.stderr[-2000:]
    r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
    assert r["itr"] == 2 and r["envs"] == 256 and 0 < r["avg_path_length"] <= 60 and np.isfinite(r["avg_return"])


def test_pg_policy_step_timing_65536_envs():
    """The fused policy step against the torch operations it replaces (convert, three GEMMs, two tanh, noise, exp, the action map), median of
    20 synchronised repeats after warm-up.  A guard against a pathological kernel, not the measurement (tools/ab_vpg_policy.py)."""
    import torch
    from cassierl_amd import trpo as T
    from cassierl_amd import vpg as V
    from cassierl_amd.vec_env import action_space
    n = 65536
    pol = _policy(26, 6, 9)
    box = action_space("PD")
    amap = T.NormalizedActions(box.low, box.high, "cuda")
    algo = V.VPG(None, None, pol, T.LinearFeatureBaseline(), n, 26, amap)
    step = algo._fused_policy_step(torch.device("cuda:0"), torch.float32)
    obs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
    noise = torch.randn(n, 6, device="cuda")
    o32, mean, act = torch.empty(n, 26, device="cuda"), torch.empty(n, 6, device="cuda"), torch.empty(n, 6, device="cuda")

    def torch_step():
        o = obs.to(torch.float32)
        a, m, _ = pol.get_actions(o, noise=noise)
        amap(a)

    out = {}
    for name, fn in (("fused", lambda: step(obs, noise, o32, mean, act)), ("torch", torch_step)) * 2:   # alternated, the second round kept
        for _ in range(5):
            fn()
        ts = []
        for _ in range(20):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        out[name] = float(np.median(ts)) * 1e3
    print("policy step ms at %d envs: %s" % (n, out))
    assert out["fused"] < 1.5 * out["torch"]
