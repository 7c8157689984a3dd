"""TRPO's width-128 kernels (csrc/tu_pg_trpo.hip) against the torch operations they replace, and train_trpo.py --hidden 128,128 on the GPU.
-m gpu only."""
import copy
import ctypes as ct
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _policy(obs_dim, act_dim, seed, jitter=0.05):
    import torch
    from cassierl_amd import trpo as T
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(obs_dim, act_dim, (128, 128), init_std=1.0).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(jitter * torch.randn_like(p))
    return pol


@pytest.mark.parametrize("n,obs_dim,act_dim", [(1000, 26, 6), (4099, 26, 7), (777, 17, 6), (65536, 26, 6)])
def test_pg_fvp_matches_the_analytic_fisher(n, obs_dim, act_dim):
    """F v of the 128-128 policy against AnalyticFisher evaluated in float64; 4099 and 777 end in a ragged tile."""
    import torch
    from cassierl_amd import trpo as T
    pol = _policy(obs_dim, act_dim, 3, jitter=0.1)
    obs = torch.randn(n, obs_dim, device="cuda") * 0.7
    F = T.PgFisher(pol, obs)
    assert F.kind == "pg_fvp"
    ref_F = T.AnalyticFisher(copy.deepcopy(pol).double(), obs.double())
    torch.manual_seed(11)
    v = torch.randn(F.NP + act_dim, device="cuda")
    got, ref = F(v), ref_F(v.double())
    err = (got.double() - ref).abs().max().item()
    assert err < 2e-4 * ref.abs().max().item(), (err, ref.abs().max().item())
    assert torch.equal(got, F(v))   # fixed-order sums: the same bits twice


@pytest.mark.parametrize("obs_dim,act_dim", [(26, 6), (17, 7)])
def test_pg_surrogate_matches_the_torch_surrogate(obs_dim, act_dim):
    import torch
    from cassierl_amd import trpo as T
    n = 5000
    pol = _policy(obs_dim, act_dim, 4)
    obs = torch.randn(n, obs_dim, device="cuda") * 0.7
    with torch.no_grad():
        old_mean, old_lstd = (x.clone() for x in pol.dist_info(obs))   # (not views of log_std, which moves below)
        act = old_mean + torch.randn_like(old_mean) * old_lstd.exp()
    adv = torch.randn(n, device="cuda")
    F = T.PgFisher(pol, obs)

    def torch_sur():
        with torch.no_grad():
            m, ls = pol.dist_info(obs)
            lr = (pol.log_likelihood(act, m, ls) - pol.log_likelihood(act, old_mean, old_lstd)).exp()
            return (-(lr * adv).mean()).item(), pol.kl(old_mean, old_lstd, m, ls).mean().item()

    loss, kl = (x.item() for x in F.surrogate(pol, act, adv, old_mean, old_lstd[0].clone()))
    # at the old weights: ratio 1 and KL 0, up to the float32 rounding of the kernel's mean against torch's (a perturbed point: ~1e-3)
    assert abs(loss + adv.mean().item()) < 1e-5 and abs(kl) < 1e-6, (loss, kl)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.02 * torch.randn_like(p))
    loss, kl = (x.item() for x in F.surrogate(pol, act, adv, old_mean, old_lstd[0].clone()))
    rl, rk = torch_sur()
    assert kl > 1e-4 and abs(kl - rk) < 1e-4 * rk, (kl, rk)
    assert abs(loss - rl) < 1e-5 * (1.0 + abs(rl)), (loss, rl)


@pytest.mark.parametrize("tol", [1e-10, 1e30])
def test_pg_cg_update_matches_the_torch_cg(tol):
    """Ten iterations at n = 20 878 (26 -> 7) against trpo.conjugate_gradient driven by the same products; tol = 1e30 exits after one."""
    import torch
    from cassierl_amd import trpo as T
    pol = _policy(26, 7, 5)
    obs = torch.randn(4096, 26, device="cuda") * 0.7
    F = T.PgFisher(pol, obs)
    torch.manual_seed(2)
    b = torch.randn(F.NP + 7, device="cuda") * 1e-2
    assert b.numel() == 20878
    reg = 1e-5
    x = F.conjugate_gradient(b, 10, reg, tol=tol)
    assert x is not None
    xr = T.conjugate_gradient(lambda v: F(v) + reg * v, b, 10, tol=tol)
    rel = ((x - xr).norm() / xr.norm()).item()
    print("CG (tol %g): relative difference %.3g" % (tol, rel))
    # one step: only the order of the two dot products differs; ten: that rounding, fed back through ten products
    assert rel < (1e-5 if tol > 1 else 1e-2), rel


def test_pg_entry_points_refuse_bad_arguments():
    import torch
    from cassierl_amd import _lib
    L = _lib.load()
    P = lambda t: ct.c_void_p(t.data_ptr())
    f = lambda k: torch.zeros(k, device="cuda")
    x, r, p, scal, apm, hls = f(21600), f(21600), f(21600), f(2), f(21600), f(7)
    cg = lambda n, ls_off, n_ls: L.CassiePgCgUpdate(n, ls_off, n_ls, P(apm), P(hls), ct.c_float(0.0), ct.c_float(1e-10), P(x), P(r), P(p), P(scal), None)
    assert cg(21505, 0, 7) == EINVAL and cg(100, 95, 7) == EINVAL and cg(0, 0, 0) == EINVAL
    D, A = 26, 6
    W1, b1, W2, b2, W3, b3 = f(128 * D), f(128), f(128 * 128 + 4), f(128), f(A * 128), f(A)
    obs, prec, work, part = f(32 * D), f(A), f(32 * A), f(20000)
    net = [P(W1), P(b1), P(W2), P(b2), P(W3), P(b3)]
    bad = [P(W1), P(b1), ct.c_void_p(W2.data_ptr() + 4), P(b2), P(W3), P(b3)]
    fvp = lambda d, th: L.CassiePgFvp(P(obs), 32, d, A, *th, *net, P(prec), ct.c_float(1.0), P(work), P(part), None)
    assert fvp(D, bad) == EINVAL and fvp(20, net) == EINVAL
    assert L.CassiePgFvp(P(obs), 32, D, A, *net, *bad, P(prec), ct.c_float(1.0), P(work), P(part), None) == EINVAL
    sur = lambda d, th: L.CassiePgSurrogate(P(obs), 32, d, A, *th, P(prec), P(prec), P(work), P(obs), P(work), P(part), None)
    assert sur(D, bad) == EINVAL and sur(20, net) == EINVAL
    torch.cuda.synchronize()


def test_sampler_at_width_128_uses_the_pg_policy_step():
    import torch
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env import action_space
    n = 5000
    box = action_space("PD")
    amap = T.NormalizedActions(box.low, box.high, "cuda")
    for hidden, entry in (((128, 128), "CassiePgPolicyStep"), ((32, 32), "CassieTrpoPolicyStep")):
        torch.manual_seed(1)
        pol = T.GaussianMLPPolicy(26, 6, hidden, init_std=1.0).cuda()
        algo = T.TRPO(None, None, pol, T.LinearFeatureBaseline(), n, 26, amap)
        step = algo._fused_policy_step(torch.device("cuda:0"), torch.float32)
        assert step is not None and algo.policy_step_entry == entry
    obs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
    noise = torch.randn(n, 6, device="cuda")
    pol = _policy(26, 6, 7)
    algo = T.TRPO(None, None, pol, T.LinearFeatureBaseline(), n, 26, amap)
    step = algo._fused_policy_step(torch.device("cuda:0"), torch.float32)
    o32, mean, act = torch.empty(n, 26, device="cuda"), torch.empty(n, 6, device="cuda"), torch.empty(n, 6, device="cuda")
    step(obs, noise, o32, mean, act)
    a_ref, m_ref, _ = pol.get_actions(obs.float(), noise=noise)
    assert (mean - m_ref).abs().max().item() < 5e-6 * (1 + m_ref.abs().max().item())
    assert (algo._env_actions - amap(act)).abs().max().item() < 1e-12


def test_fused_update_agrees_with_the_torch_update_on_one_stand_batch():
    """One batch of the stand env (4096 envs, horizon 4); the fused update (PgFisher: CassiePgFvp, CassiePgCgUpdate, CassiePgSurrogate) and
    the forced-torch one (AnalyticFisher, torch CG and line search) start from the same parameters and batch.  The two differ only in float32
    rounding (sum order of the products and dot products), which ten CG iterations on the lightly damped Fisher amplify; 1 % of the step is
    far below what any real difference (another batch, a wrong product) makes, and far above the float32 noise measured."""
    import torch
    from cassierl_amd import trpo as T
    from cassierl_amd.trajectory import default_gait
    algo = T.make_cassie_trpo(4096, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, batch_size=4096 * 4,
                              hidden_sizes=(128, 128), init_std=1.0)
    d = algo.process(algo.collect())
    theta0 = T.flat_params(algo.policy).clone()
    res = {}
    for fused in (True, False):
        T.set_flat_params(algo.policy, theta0)
        algo.fused_fisher = fused
        st = algo.optimize(d)
        assert algo.last_fisher_kind == ("pg_fvp" if fused else "analytic")
        res[fused] = (T.flat_params(algo.policy).clone(), st)
    (tf, sf), (tt, stt) = res[True], res[False]
    rel = ((tf - tt).norm() / (tt - theta0).norm()).item()
    print("fused vs torch TRPO-128 update: difference %.3g of the step; backtracks %d / %d, kl %.6g / %.6g" % (rel, sf["backtracks"], stt["backtracks"], sf["kl"], stt["kl"]))
    assert sf["backtracks"] == stt["backtracks"] and 0 <= sf["backtracks"] <= 15
    assert sf["kl"] <= algo.step_size and stt["kl"] <= algo.step_size
    assert rel < 1e-2
    algo.env.close()


@pytest.fixture(scope="module")
def wide_runs(tmp_path_factory):
    """train_trpo.py --hidden 128,128 on the stand env: 3 iterations; 2 iterations with a snapshot; the snapshot resumed for 1; 2 ranks x 1024."""
    d = tmp_path_factory.mktemp("wide")
    script = os.path.join(ROOT, "train_trpo.py")
    common = ["--horizon", "4", "--kind", "stand", "--control-mode", "Torque", "--hidden", "128,128", "--init-std", "1.0"]
    out = {}

    def run(name, args, env=None, pre=()):
        p = subprocess.run([sys.executable, *pre, script] + common + args, capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        out[name] = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]

    snap = str(d / "snap.pt")
    run("three", ["--envs-per-gpu", "2048", "--n-itr", "3", "--dump-params", str(d / "three.npy")])
    run("two", ["--envs-per-gpu", "2048", "--n-itr", "2", "--snapshot", snap, "--dump-params", str(d / "two.npy")])
    run("resumed", ["--envs-per-gpu", "2048", "--n-itr", "1", "--load-policy", snap, "--dump-params", str(d / "resumed.npy")])
    env = dict(os.environ, CASSIE_DEVICE_MAP="0,0", CASSIE_BACKEND="gloo")
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    run("ranks", ["--envs-per-gpu", "1024", "--n-itr", "2", "--dump-params", str(d / "ranks.npy")], env=env,
        pre=("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port)))
    return d, out


def test_wide_resume_equals_the_uninterrupted_run(wide_runs):
    d, out = wide_runs
    assert out["resumed"][0]["sampler_restored"] and out["resumed"][0]["itr"] == 2
    a, b = out["three"][2], out["resumed"][1]
    assert a["itr"] == b["itr"] == 2 and a["avg_reward"] == b["avg_reward"] and a["backtracks"] == b["backtracks"]
    assert np.array_equal(np.load(d / "three.npy"), np.load(d / "resumed.npy"))


def test_two_rank_wide_trpo_equals_the_one_rank_run(wide_runs):
    d, out = wide_runs
    for a, b in zip(out["two"], out["ranks"]):
        assert a["env_steps"] == b["env_steps"] == 2048 * 4 and a["gathered"] == b["gathered"] == 2048 and a["episodes"] == b["episodes"]
        assert abs(a["avg_reward"] - b["avg_reward"]) < 1e-6 and a["backtracks"] == b["backtracks"]
    t1, t2 = np.load(d / "two.npy"), np.load(d / "ranks.npy")
    assert t1.size == 26 * 128 + 128 + 128 * 128 + 128 + 6 * 128 + 6 + 6
    assert np.abs(t1 - t2).max() < 1e-4 * max(1.0, np.abs(t1).max()), np.abs(t1 - t2).max()


def test_sim_policy_rolls_out_a_wide_trpo_snapshot(wide_runs):
    d, _ = wide_runs
    q = subprocess.run([sys.executable, os.path.join(ROOT, "sim_policy.py"), str(d / "snap.pt"), "--envs", "256", "--max-path-length", "60", "--kind", "stand",
                        "--control-mode", "Torque"], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
    assert r["itr"] == 2 and r["envs"] == 256 and 0 < r["avg_path_length"] <= 60 and np.isfinite(r["avg_return"])


def test_pg_fvp_timing_524288_samples():
    """One product, fused against AnalyticFisher, median of alternated rounds.  A guard against a pathological kernel, not the measurement
    (tools/ab_trpo_wide.py)."""
    import torch
    from cassierl_amd import trpo as T
    n = 524288
    pol = _policy(26, 6, 9)
    obs = torch.randn(n, 26, device="cuda") * 0.7
    F, G = T.PgFisher(pol, obs), T.AnalyticFisher(pol, obs)
    v = torch.randn(F.NP + 6, device="cuda")
    ts = {"fused": [], "torch": []}
    for r in range(6):
        for name, fn in ((("fused", F), ("torch", G)) if r % 2 == 0 else (("torch", G), ("fused", F))):
            fn(v)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(3):
                fn(v)
            torch.cuda.synchronize(); ts[name].append((time.perf_counter() - t0) / 3)
    med = {k: float(np.median(x)) * 1e3 for k, x in ts.items()}
    print("Fisher-vector product ms at %d samples: %s" % (n, med))
    assert med["fused"] < med["torch"]
