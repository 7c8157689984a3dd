"""PPO's kernels (csrc/tu_ppo.hip) against the torch statements of cassierl_amd/ppo.py, the whole update against float64, and train_ppo.py
on the GPU.  -m gpu only.

The reference of every gradient check is FLOAT64 torch autograd of ppo_loss (policy and data cast up).  Samples whose float64 ratio lies
within 1e-4 of a clip boundary can fall on either side of it in float32; they are taken out before BOTH evaluations (at most 1 % may be)."""
import copy
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLIP = 0.2


def _policy(obs_dim, act_dim, hidden, seed, jitter=0.1):
    import torch
    from cassierl_amd import trpo as T
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(obs_dim, act_dim, hidden, init_std=1.0).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(jitter * torch.randn_like(p))
    return pol


def _clip_batch(pol, n, obs_dim):
    """Old statistics from the policy as it is, then the policy jittered by 0.05: ratios on both sides of both boundaries."""
    import torch
    obs = torch.randn(n, obs_dim, device="cuda") * 0.7
    adv = torch.randn(n, device="cuda")
    with torch.no_grad():
        old_mean, old_ls = pol.dist_info(obs)
        old_mean, old_ls = old_mean.clone(), old_ls[0].clone()
        act = old_mean + torch.randn_like(old_mean) * old_ls.exp()
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return obs, act, adv, old_mean, old_ls


def _ratio64(pol64, obs, act, adv, old_mean, old_ls):
    import torch
    from cassierl_amd import ppo as P
    with torch.no_grad():
        _, ratio, clipped = P.surrogate_terms(pol64.mean_net(obs.double()), pol64.log_std, act.double(), adv.double(), old_mean.double(), old_ls.double(), CLIP)
    return ratio, clipped


# ------------------------------------------------------------------------------------------------------------------ GAE
@pytest.mark.parametrize("T_,N", [(8, 4096), (5, 1000), (1, 77)])
@pytest.mark.parametrize("D", [26, 17])
@pytest.mark.parametrize("fitted", [False, True])
def test_gae_kernel_matches_the_torch_statement(T_, N, D, fitted):
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    torch.manual_seed(11)
    dev = torch.device("cuda:0")
    obs = torch.randn(T_, N, D, device=dev) * 3.0
    t = torch.randint(0, 300, (T_, N), device=dev)
    rew = torch.randn(T_, N, dtype=torch.float64, device=dev)
    cut = torch.rand(T_, N, device=dev) < 0.2
    base = T.LinearFeatureBaseline()
    last = None
    if fitted:
        base.fit(obs.view(-1, D), t.view(-1), torch.randn(T_ * N, dtype=torch.float64, device=dev) + obs.view(-1, D)[:, 0].double())
        last = torch.randn(N, dtype=torch.float64, device=dev)
    bk = T.BaselineKernels(dev, D)
    values = base.predict(obs.view(-1, D), t.view(-1)).view(T_, N)
    last_ref = torch.zeros(N, dtype=torch.float64, device=dev) if last is None else last
    for lam in (0.0, 0.95, 1.0):
        ret, adv, sums = bk.gae(obs, t, rew, cut, base.coeffs, last, 0.99, lam)
        ret_ref, adv_ref = P.gae_advantages(rew, cut, values, last_ref, 0.99, lam)
        e_ret, e_adv = (ret - ret_ref).abs().max().item(), (adv - adv_ref).abs().max().item()
        print("GAE T %d N %d D %d fitted %s lambda %.2f: |returns| err %.3g, |adv| err %.3g" % (T_, N, D, fitted, lam, e_ret, e_adv))
        assert e_ret <= 1e-12 * (1.0 + ret_ref.abs().max().item())
        assert e_adv <= 1e-12 * (1.0 + adv_ref.abs().max().item())
        s1, s2 = adv_ref.sum().item(), (adv_ref ** 2).sum().item()
        assert abs(sums[0].item() - s1) <= 1e-10 * abs(s1) and abs(sums[1].item() - s2) <= 1e-10 * s2
        if lam == 1.0:
            ret1, adv1, _ = bk.returns_advantages(obs, t, rew, cut, base.coeffs, last, 0.99)
            assert (ret - ret1).abs().max().item() <= 1e-12 * (1.0 + ret1.abs().max().item())
            assert (adv - adv1).abs().max().item() <= 1e-12 * (1.0 + adv1.abs().max().item())


# ------------------------------------------------------------------------------------------------------------------ clip gradient
@pytest.mark.parametrize("hidden,kind", [((32, 32), "trpo_clip"), ((128, 128), "pg_clip")])
@pytest.mark.parametrize("n,obs_dim,act_dim", [(1000, 26, 6), (65536, 26, 6), (4099, 26, 7), (777, 17, 6)])
@pytest.mark.parametrize("mode", ["rows", "subset", "repeats"])
def test_clip_grad_matches_float64_autograd(hidden, kind, n, obs_dim, act_dim, mode):
    """`rows`: idx = NULL (the first m rows of the batch, m < n); `subset`: a random subset; `repeats`: an index drawn with replacement.
    m is never a multiple of 32."""
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    ent = 0.01 if mode == "subset" else 0.0
    pol = _policy(obs_dim, act_dim, hidden, 3)
    obs, act, adv, old_mean, old_ls = _clip_batch(pol, n, obs_dim)
    pol64 = copy.deepcopy(pol).double()
    ratio, _ = _ratio64(pol64, obs, act, adv, old_mean, old_ls)
    near = ((ratio - (1.0 + CLIP)).abs() < 1e-4) | ((ratio - (1.0 - CLIP)).abs() < 1e-4)
    g = torch.Generator(device="cuda").manual_seed(5)
    if mode == "rows":      # without an index the samples are taken out of the batch itself
        keep = (~near).nonzero().squeeze(-1)
        obs, act, adv, old_mean, ratio = obs[keep].contiguous(), act[keep].contiguous(), adv[keep].contiguous(), old_mean[keep].contiguous(), ratio[keep]
        m = obs.shape[0] - 37
        m -= 1 if m % 32 == 0 else 0
        idx, taken = None, n - keep.numel()
        sel = slice(0, m)
    else:
        m0 = (n * 3) // 4 + 5
        cand = torch.randperm(n, device="cuda", generator=g)[:m0] if mode == "subset" else torch.randint(0, n, (m0,), device="cuda", generator=g)
        idx = cand[~near[cand]]
        if idx.numel() % 32 == 0:
            idx = idx[:-1]
        idx = idx.contiguous()
        m, taken, sel = idx.numel(), m0 - int((~near[cand]).sum()), idx
    print("%s n %d: m %d, %d samples within 1e-4 of a clip boundary taken out (%.3f %%)" % (mode, n, m, taken, 100.0 * taken / n))
    assert taken <= 0.01 * n and m % 32 != 0
    rows = lambda dt: [x[sel].to(dt) for x in (obs, act, adv, old_mean)]
    ref = T.flat_grad(P.ppo_loss(pol64, *rows(torch.float64), old_ls.double(), CLIP, ent), pol64)
    g32 = T.flat_grad(P.ppo_loss(pol, *rows(torch.float32), old_ls, CLIP, ent), pol).double()
    st_ref = P.minibatch_stats(pol64, *rows(torch.float64), old_ls.double(), CLIP)
    ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), obs, act, adv, old_mean, old_ls, CLIP, ent)
    assert ck.kind == kind
    got, st = ck.grad(idx, m=m)
    scale = ref.abs().max().item()
    e_k, e_t = (got.double() - ref).abs().max().item() / scale, (g32 - ref).abs().max().item() / scale
    share = st_ref[2].item() / m
    print("%s %s n %d D %d A %d: kernel %.3g, float32 torch autograd %.3g (relative to max |g_ref| of float64); clipped share %.3f"
          % (kind, mode, n, obs_dim, act_dim, e_k, e_t, share))
    assert share > 0.05
    assert e_k < 2e-4, (e_k, e_t)
    with torch.no_grad():
        sur_scale = (ratio[sel] * adv[sel].double()).abs().mean().item()
    assert abs(st[0].item() - st_ref[0].item()) / m < 2e-5 * sur_scale, (st[0].item(), st_ref[0].item())
    assert abs(st[1].item() - st_ref[1].item()) / m < 2e-5 * max(st_ref[1].item() / m, 1e-3), (st[1].item(), st_ref[1].item())
    assert st[2].item() == st_ref[2].item()
    got2, st2 = ck.grad(idx, m=m)
    assert torch.equal(got, got2) and torch.equal(st, st2)   # fixed-order sums: the same bits twice


def test_clip_grad_clamps_a_wild_index():
    """Row numbers outside [0, n) are clamped, as CassieDdpg*Grad clamps them: the gradient is that of the clamped index."""
    import torch
    from cassierl_amd import ppo as P
    pol = _policy(26, 6, (128, 128), 4)
    n = 500
    obs, act, adv, old_mean, old_ls = _clip_batch(pol, n, 26)
    ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), obs, act, adv, old_mean, old_ls, CLIP, 0.0)
    idx = torch.tensor([-7, 0, 3, n - 1, n, n + 1000, 2 ** 40, 17, 17], dtype=torch.int64, device="cuda")
    a, sa = ck.grad(idx)
    b, sb = ck.grad(idx.clamp(0, n - 1))
    assert torch.equal(a, b) and torch.equal(sa, sb) and torch.isfinite(a).all()


# ------------------------------------------------------------------------------------------------------------------ whole update
@pytest.mark.parametrize("hidden,kind", [((32, 32), "trpo_clip"), ((128, 128), "pg_clip")])
def test_fused_update_is_as_close_to_float64_as_the_torch_update(hidden, kind):
    """One stand batch (4096 envs x 4 steps), epochs = 1, 2 minibatches: the fused float32 update, the forced-torch float32 update and the torch
    float64 update from the same parameters, batch and permutation.  Required: |theta_fused - theta_64| <= 4 |theta_torch32 - theta_64|
    (the factor 4: two float32 evaluations of one expression that differ in summation order)."""
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    from cassierl_amd.trajectory import default_gait
    algo = P.make_cassie_ppo(4096, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, hidden_sizes=hidden, batch_size=4096 * 4,
                             epochs=1, minibatch_size=4096 * 2)
    d = algo.process(algo.collect())
    assert algo.last_gae_fused
    pol32 = algo.policy
    theta0 = T.flat_params(pol32).clone()
    gen0 = algo.gen_mb.get_state()
    res = {}
    for name in ("fused", "torch32", "torch64"):
        algo.adam_t, algo.adam_m, algo.adam_v = 0, None, None
        algo.gen_mb.set_state(gen0)
        algo.fused_grad = algo.fused_adam = name == "fused"
        if name == "torch64":
            algo.policy = copy.deepcopy(pol32).double()
            T.set_flat_params(algo.policy, theta0.double())
            st = algo.optimize({k: v.double() for k, v in d.items()})
        else:
            T.set_flat_params(pol32, theta0)
            st = algo.optimize(d)
        assert algo.last_grad_kind == (kind if name == "fused" else "autograd") and algo.last_adam_fused == (name == "fused")
        assert st["minibatch_steps"] == 2 and algo.adam_t == 2
        res[name] = (T.flat_params(algo.policy).double().clone(), st)
    algo.policy = pol32
    t64 = res["torch64"][0]
    e_f, e_t, step = (res["fused"][0] - t64).norm().item(), (res["torch32"][0] - t64).norm().item(), (t64 - theta0.double()).norm().item()
    print("%s update: |theta_fused - theta_64| %.4g, |theta_torch32 - theta_64| %.4g, |step_64| %.4g" % (kind, e_f, e_t, step))
    for k in ("loss_first", "loss_last", "mean_kl", "clip_frac", "grad_norm"):
        print("   %s: fused %.8g torch32 %.8g torch64 %.8g" % (k, res["fused"][1][k], res["torch32"][1][k], res["torch64"][1][k]))
    assert step > 0 and e_f <= 4.0 * e_t, (e_f, e_t)
    algo.env.close()


def test_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    from cassierl_amd.trajectory import default_gait
    mk = lambda: P.make_cassie_ppo(1024, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, batch_size=1024 * 4, epochs=2,
                                   minibatch_size=1024)
    a = mk()
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ref = a.train_iteration()
    assert a.last_grad_kind == "pg_clip" and a.last_adam_fused and a.last_gae_fused
    ta = T.flat_params(a.policy).clone()
    a.env.close()
    b = mk()
    _, restored = b.load(p)
    assert restored and b.adam_t == 16
    got = b.train_iteration()
    assert got["itr"] == ref["itr"] == 2
    for k in ("avg_reward", "grad_norm", "loss_first", "loss_last", "mean_kl", "clip_frac"):
        assert got[k] == ref[k], k
    assert torch.equal(T.flat_params(b.policy), ta)
    b.env.close()


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_two_rank_ppo_iterations_equal_the_one_rank_run(tmp_path):
    """train_ppo.py: two ranks with 2048 envs each (both on device 0, gloo) against one rank with the same 4096 global env ids; the minibatch is
    the whole batch, the only setting in which the rank count does not enter."""
    from conftest import ROOT
    script = os.path.join(ROOT, "train_ppo.py")
    common = ["--horizon", "4", "--n-itr", "2", "--kind", "stand", "--control-mode", "Torque", "--epochs", "2", "--minibatch-size", str(4096 * 4)]
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
        assert a["minibatch_steps"] == b["minibatch_steps"] == 2
        assert abs(a["avg_reward"] - b["avg_reward"]) < 1e-6 and abs(a["grad_norm"] - b["grad_norm"]) < 1e-4 * a["grad_norm"]
    t1, t2 = np.load(one), np.load(two)
    assert t1.size == 26 * 128 + 128 + 128 * 128 + 128 + 6 * 128 + 6 + 6
    assert np.abs(t1 - t2).max() < 1e-4 * max(1.0, np.abs(t1).max()), np.abs(t1 - t2).max()


def test_sim_policy_rolls_out_a_ppo_snapshot(tmp_path):
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_ppo.py"), "--envs-per-gpu", "512", "--horizon", "4", "--n-itr", "2", "--kind", "stand",
                        "--control-mode", "Torque", "--snapshot", snap], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and os.path.exists(snap), p.stderr[-2000:]
    st = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(st) == 2 and st[-1]["minibatch_steps"] == 16 and np.isfinite(st[-1]["loss_last"])
    q = subprocess.run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "256", "--max-path-length", "60", "--kind", "stand",
                        "--control-mode", "Torque"], capture_output=True, text=True, timeout=900)
    assert q.returncode == 0, q.stderr[-2000:]
    r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
    assert r["itr"] == 2 and r["envs"] == 256 and 0 < r["avg_path_length"] <= 60 and np.isfinite(r["avg_return"])


def test_ppo_update_timing_524288_samples():
    """One whole update (4 epochs x 8 minibatches of 65 536 on 65 536 x 8 samples, width 128), fused against forced-torch, alternated, medians of
    20 after warm-up.  A guard against a pathological kernel, not the measurement (tools/ab_ppo_update.py)."""
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    n, A = 65536 * 8, 6
    pol = _policy(26, A, (128, 128), 9)
    obs, act, adv, old_mean, old_ls = _clip_batch(pol, n, 26)
    d = dict(obs=obs, act=act, adv=adv, mean=old_mean, log_std=old_ls.expand(n, A))
    algo = P.PPO(None, None, pol, T.LinearFeatureBaseline(), 65536, 26, None, batch_size=n, epochs=4, minibatch_size=65536)
    theta0 = T.flat_params(pol).clone()

    def run(fused):
        T.set_flat_params(pol, theta0)
        algo.fused_grad = algo.fused_adam = fused
        torch.cuda.synchronize(); t0 = time.perf_counter()
        st = algo.optimize(d)
        torch.cuda.synchronize()
        assert st["minibatch_steps"] == 32 and algo.last_grad_kind == ("pg_clip" if fused else "autograd")
        return time.perf_counter() - t0

    out = {}
    for name, fused in (("fused", True), ("torch", False)) * 2:   # alternated, the second round kept
        for _ in range(3):
            run(fused)
        out[name] = float(np.median([run(fused) for _ in range(20)])) * 1e3
    print("PPO update ms at %d samples, 4 x 8 minibatches: %s" % (n, out))
    assert out["fused"] < 1.5 * out["torch"]
