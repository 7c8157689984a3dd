"""PPO on Cassie3d on the GPU: the 45 x 10 width-128 kernels (csrc/tu_pg3d.hip) and the baseline kernels at 45 observations
(csrc/tu_trpo_baseline.hip, tu_ppo.hip's GAE) against the torch statements, the whole update against float64, and train_ppo.py --env cassie3d
with its snapshot.  -m gpu only.  The shapes are the layout's edges (a lone lane, a second tile, a partial group of four tiles, more than one
workgroup; the ten action rows in registers 0..5; the second 32-column block of [obs | 1]), not the workload.

The reference of every gradient check is FLOAT64 torch autograd of ppo_loss, as in tests/test_gpu_ppo.py, whose construction and bounds these
tests take over."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_ppo import CLIP, _clip_batch, _policy, _ratio64

pytestmark = pytest.mark.gpu

D3, A3, HID = 45, 10, (128, 128)


# ------------------------------------------------------------------------------------------------------------------ policy step
@pytest.mark.parametrize("control_mode", ["PD", "Torque"])
@pytest.mark.parametrize("n", [1, 33, 130, 257])
def test_policy_step_matches_the_torch_operations(control_mode, n):
    """CassiePg3dPolicyStep against GaussianMLPPolicy.get_actions and NormalizedActions.  The noise is +20 / -20 / N(0, 1) by (row + column) % 3, so
    that with three rows or more every one of the ten action columns has entries clamped at BOTH bounds; a lone row (n = 1) cannot meet both
    bounds in one column: there both bounds are met across its columns.  The output buffers are 40 rows longer and pre-filled."""
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env3d import action_space
    pol = _policy(D3, A3, HID, 7)
    box = action_space(control_mode)
    amap = T.NormalizedActions(box.low, box.high, "cuda")
    algo = P.PPO(None, None, pol, T.LinearFeatureBaseline(), n, D3, amap, batch_size=n, minibatch_size=n)
    step = algo._fused_policy_step(torch.device("cuda:0"), torch.float32)
    assert step is not None and algo.policy_step_entry == "CassiePg3dPolicyStep"
    torch.manual_seed(n)
    obs = torch.randn(n, D3, dtype=torch.float64, device="cuda")
    cls = (torch.arange(n, device="cuda")[:, None] + torch.arange(A3, device="cuda")[None, :]) % 3
    noise = torch.randn(n, A3, device="cuda")
    noise[cls == 0], noise[cls == 1] = 20.0, -20.0
    pad, fill = 40, -777.0
    o32, mean, act = (torch.full((n + pad, w), fill, device="cuda") for w in (D3, A3, A3))
    env_big = torch.full((n + pad, A3), fill, dtype=torch.float64, device="cuda")
    algo._env_actions = env_big[:n]
    step(obs, noise, o32[:n], mean[:n], act[:n])
    a_ref, m_ref, _ = pol.get_actions(obs.float(), noise=noise)
    assert torch.equal(o32[:n], obs.float())
    e_m, e_a = (mean[:n] - m_ref).abs().max().item(), (act[:n] - a_ref).abs().max().item()
    e_e = (env_big[:n] - amap(act[:n])).abs().max().item()
    print("policy step %s n %d: mean err %.3g (max %.3g), action err %.3g (max %.3g), env_actions err %.3g"
          % (control_mode, n, e_m, m_ref.abs().max().item(), e_a, a_ref.abs().max().item(), e_e))
    assert e_m < 5e-6 * (1 + m_ref.abs().max().item())
    assert e_a < 5e-6 * (1 + a_ref.abs().max().item())
    assert e_e < 1e-12
    lo, hi = torch.as_tensor(box.low, device="cuda"), torch.as_tensor(box.high, device="cuda")
    env = env_big[:n]
    assert (env >= lo).all() and (env <= hi).all()
    at_lo, at_hi = env == lo, env == hi
    if n >= 3:   # per action column: some entries clamped at the low bound and some at the high bound
        assert at_lo.any(0).all() and at_hi.any(0).all(), (at_lo.sum(0).tolist(), at_hi.sum(0).tolist())
        assert (~at_lo & ~at_hi).any()
    else:
        assert at_lo.any() and at_hi.any()
    assert at_hi[cls == 0].all() and at_lo[cls == 1].all()   # every entry the noise pushes out sits on its bound
    for big in (o32, mean, act, env_big):   # rows past n: untouched
        assert (big[n:] == fill).all()


# ------------------------------------------------------------------------------------------------------------------ clip gradient
def _blocks(pol):
    """name -> index tensor into the flat parameter vector: the mean network's blocks with W1 split at column 32 (the second 32-column block of
    [obs | 1]) and W3, b3, log_std split at row 8 (the action rows in registers 4, 5 of lane half 0)."""
    import torch
    off, out = 0, {}
    for nm, p in pol.named_parameters():
        ix = torch.arange(off, off + p.numel(), device="cuda").view(p.shape)
        off += p.numel()
        if nm == "mean_net.0.weight":
            out["W1[:, :32]"], out["W1[:, 32:]"] = ix[:, :32].reshape(-1), ix[:, 32:].reshape(-1)
        elif nm in ("mean_net.4.weight", "mean_net.4.bias", "log_std"):
            short = {"mean_net.4.weight": "W3", "mean_net.4.bias": "b3", "log_std": "log_std"}[nm]
            out[short + "[:8]"], out[short + "[8:]"] = ix[:8].reshape(-1), ix[8:].reshape(-1)
        else:
            out[{"mean_net.0.bias": "b1", "mean_net.2.weight": "W2", "mean_net.2.bias": "b2"}[nm]] = ix.reshape(-1)
    return out


@pytest.mark.parametrize("n", [77, 1000, 4099])
@pytest.mark.parametrize("mode", ["rows", "subset", "repeats"])
def test_clip_grad_matches_float64_autograd(n, mode):
    """test_gpu_ppo.py's test_clip_grad_matches_float64_autograd at 45 x 10, with the 2e-4 bound applied to every parameter block on its own
    (relative to the block's own max |g_ref|): a missing or permuted block cannot hide behind a larger one."""
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    ent = 0.01 if mode == "subset" else 0.0
    pol = _policy(D3, A3, HID, 3)
    obs, act, adv, old_mean, old_ls = _clip_batch(pol, n, D3)
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
    assert ck.kind == "pg3d_clip"
    got, st = ck.grad(idx, m=m)
    scale = ref.abs().max().item()
    share = st_ref[2].item() / m
    print("pg3d_clip %s n %d: clipped share %.3f, max |g_ref| %.4g" % (mode, n, share, scale))
    assert share > 0.05
    worst = 0.0
    for name, ix in _blocks(pol).items():
        s_b = ref[ix].abs().max().item()
        e_k, e_t = (got.double()[ix] - ref[ix]).abs().max().item() / s_b, (g32[ix] - ref[ix]).abs().max().item() / s_b
        print("   %-12s kernel %.3g, float32 torch autograd %.3g (relative to the block's max |g_ref| = %.3g of the global one)" % (name, e_k, e_t, s_b / scale))
        assert e_k < 2e-4, (name, e_k, e_t)
        worst = max(worst, e_k)
    assert (got.double() - ref).abs().max().item() / scale < 2e-4
    with torch.no_grad():
        sur_scale = (ratio[sel] * adv[sel].double()).abs().mean().item()
    assert abs(st[0].item() - st_ref[0].item()) / m < 2e-5 * sur_scale, (st[0].item(), st_ref[0].item())
    assert abs(st[1].item() - st_ref[1].item()) / m < 2e-5 * max(st_ref[1].item() / m, 1e-3), (st[1].item(), st_ref[1].item())
    assert st[2].item() == st_ref[2].item()
    got2, st2 = ck.grad(idx, m=m)
    assert torch.equal(got, got2) and torch.equal(st, st2)   # fixed-order sums: the same bits twice


def test_clip_grad_clamps_a_wild_index():
    """Row numbers outside [0, n) are clamped: the gradient is that of the clamped index."""
    import torch
    from cassierl_amd import ppo as P
    pol = _policy(D3, A3, HID, 4)
    n = 500
    obs, act, adv, old_mean, old_ls = _clip_batch(pol, n, D3)
    ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), obs, act, adv, old_mean, old_ls, CLIP, 0.0)
    assert ck.kind == "pg3d_clip"
    idx = torch.tensor([-7, 0, 3, n - 1, n, n + 1000, 2 ** 40, 17, 17], dtype=torch.int64, device="cuda")
    a, sa = ck.grad(idx)
    b, sb = ck.grad(idx.clamp(0, n - 1))
    assert torch.equal(a, b) and torch.equal(sa, sb) and torch.isfinite(a).all()


# ------------------------------------------------------------------------------------------------------------------ baseline at 45
@pytest.mark.parametrize("T_,N", [(8, 4096), (5, 1000), (1, 77)])
@pytest.mark.parametrize("fitted", [False, True])
def test_gae_and_returns_match_the_torch_statements_at_45(T_, N, fitted):
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    torch.manual_seed(11)
    dev, D = torch.device("cuda:0"), D3
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
    assert bk.F == 94
    values = base.predict(obs.view(-1, D), t.view(-1)).view(T_, N)
    last_ref = torch.zeros(N, dtype=torch.float64, device=dev) if last is None else last
    if fitted:
        p = bk.predict(obs.view(-1, D), t.view(-1), base.coeffs)
        assert (p - values.view(-1)).abs().max().item() <= 1e-12 * (1.0 + values.abs().max().item())
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


def _features_dot(obs, tt, coeffs):
    from cassierl_amd import trpo as T
    return T.LinearFeatureBaseline.features(obs, tt).double() @ coeffs


def test_gram_and_ridge_solve_at_94_features():
    """The normal equations of 4099 x 3 samples on the FP64 matrix cores (21 accumulator blocks), and the LDS Cholesky (F = 94) against
    torch.linalg.solve on the same system; the all-zero matrix; a rank-deficient Gram matrix with reg = 0 against fit_normal_equations."""
    import torch
    from cassierl_amd import trpo as T
    torch.manual_seed(13)
    dev, m = torch.device("cuda:0"), 4099 * 3
    obs = torch.randn(m, D3, device=dev) * 3.0
    tt = torch.randint(0, 300, (m,), device=dev)
    y = torch.randn(m, dtype=torch.float64, device=dev)
    bk = T.BaselineKernels(dev, D3)
    A, b = bk.gram(obs, tt, y)
    Ar, br = T.gram(T.LinearFeatureBaseline.features(obs, tt).double(), y)
    assert A.shape == (94, 94) and b.shape == (94,)
    e_abs, e_rel = (A - Ar).abs().max().item() / Ar.abs().max().item(), ((A - Ar).abs() / (Ar.abs() + 1e-3 * Ar.abs().max())).max().item()
    e_b = (b - br).abs().max().item() / (br.abs().max().item() + Ar.abs().max().item() ** 0.5)
    print("Gram 94: max err %.3g of max, entry by entry %.3g, X'y %.3g" % (e_abs, e_rel, e_b))
    assert e_abs < 1e-10
    assert e_rel < 1e-9   # entry by entry: the float32 feature arithmetic is the same
    assert e_b < 1e-10
    assert torch.equal(A, A.T)
    eye = torch.eye(94, dtype=A.dtype, device=dev)
    xs = bk.ridge_solve(A, b, 1e-5)
    xr = torch.linalg.solve(A + 1e-5 * eye, b)
    res = ((A + 1e-5 * eye) @ xs - b).abs().max().item()
    pr = _features_dot(obs, tt, xr)
    e_p = (_features_dot(obs, tt, xs) - pr).abs().max().item()
    print("ridge solve 94: residual %.3g (bound %.3g), prediction err %.3g (bound %.3g)" % (res, 1e-6 * (1 + b.abs().max().item()), e_p, 1e-6 * (1 + pr.abs().max().item())))
    assert res < 1e-6 * (1 + b.abs().max().item())
    assert e_p < 1e-6 * (1 + pr.abs().max().item())
    assert torch.equal(xs, bk.ridge_solve(A, b, 1e-5))
    x0 = bk.ridge_solve(torch.zeros_like(A), b, 0.0)   # 0 x = b: no positive pivot at any regulariser 0 * 10^k -> the last attempt's vector, no hang
    torch.cuda.synchronize()
    assert x0.shape == b.shape
    # fewer samples than features, reg = 0: the factorisation of the singular matrix is what the retry rule is for
    k = 60
    Ak, bk_ = bk.gram(obs[:k].contiguous(), tt[:k].contiguous(), y[:k].contiguous())
    Ak, bk_ = Ak.clone(), bk_.clone()
    base = T.LinearFeatureBaseline(reg_coeff=0.0)
    base.fit_normal_equations(Ak.clone(), bk_.clone(), None)
    xk = bk.ridge_solve(Ak, bk_, 0.0)
    pk_ref = _features_dot(obs[:k], tt[:k], base.coeffs)
    e_k = (_features_dot(obs[:k], tt[:k], xk) - pk_ref).abs().max().item()
    print("rank-deficient Gram (%d samples, 94 features), reg 0: prediction err %.3g (bound %.3g)" % (k, e_k, 1e-6 * (1 + pk_ref.abs().max().item())))
    assert e_k < 1e-6 * (1 + pk_ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------------------ whole update
def test_fused_update_is_as_close_to_float64_as_the_torch_update():
    """One Cassie3d batch (256 envs x 4 steps), epochs = 1, 2 minibatches: the fused float32 update, the forced-torch float32 update and the torch
    float64 update from the same parameters, batch and permutation.  Required: |theta_fused - theta_64| <= 4 |theta_torch32 - theta_64|
    (the factor 4: two float32 evaluations of one expression that differ in summation order)."""
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    algo = P.make_cassie_ppo(256, env="cassie3d", batch_size=256 * 4, epochs=1, minibatch_size=256 * 2)
    assert algo.env_family == "cassie3d" and algo.obs_dim == D3 and algo.policy.log_std.numel() == A3
    d = algo.process(algo.collect())
    assert algo.last_gae_fused and algo.policy_step_entry == "CassiePg3dPolicyStep"
    assert torch.isfinite(d["adv"]).all() and torch.isfinite(algo.baseline.coeffs).all()
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
        assert algo.last_grad_kind == ("pg3d_clip" if name == "fused" else "autograd") and algo.last_adam_fused == (name == "fused")
        assert st["minibatch_steps"] == 2 and algo.adam_t == 2
        res[name] = (T.flat_params(algo.policy).double().clone(), st)
    algo.policy = pol32
    t64 = res["torch64"][0]
    e_f, e_t, step = (res["fused"][0] - t64).norm().item(), (res["torch32"][0] - t64).norm().item(), (t64 - theta0.double()).norm().item()
    print("pg3d_clip update: |theta_fused - theta_64| %.4g, |theta_torch32 - theta_64| %.4g, |step_64| %.4g" % (e_f, e_t, step))
    for k in ("loss_first", "loss_last", "mean_kl", "clip_frac", "grad_norm"):
        print("   %s: fused %.8g torch32 %.8g torch64 %.8g" % (k, res["fused"][1][k], res["torch32"][1][k], res["torch64"][1][k]))
    assert step > 0 and e_f <= 4.0 * e_t, (e_f, e_t)
    algo.env.close()


def test_fused_switches_force_the_torch_paths():
    import torch
    from cassierl_amd import ppo as P
    algo = P.make_cassie_ppo(64, env="cassie3d", control_mode="Torque", batch_size=64 * 2, epochs=1, minibatch_size=64)
    algo.fused_policy_step = algo.fused_gae = algo.fused_grad = algo.fused_adam = algo.fused_baseline = False
    st = algo.train_iteration()
    assert algo.last_grad_kind == "autograd" and not algo.last_adam_fused and not algo.last_gae_fused and not hasattr(algo, "policy_step_entry")
    assert np.isfinite(st["loss_last"]) and np.isfinite(st["avg_reward"])
    algo.env.close()


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    import torch
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    mk = lambda: P.make_cassie_ppo(256, env="cassie3d", seed=1, batch_size=256 * 4, epochs=2, minibatch_size=256)
    a = mk()
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ref = a.train_iteration()
    assert a.last_grad_kind == "pg3d_clip" and a.last_adam_fused and a.last_gae_fused
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


def test_train_ppo_on_cassie3d_and_its_snapshot(tmp_path):
    """train_ppo.py --env cassie3d for two iterations at 256 environments; sim_policy.py rolls the snapshot out; a Cassie2d PPO refuses it."""
    from conftest import ROOT
    from cassierl_amd import ppo as P
    from cassierl_amd.trajectory import default_gait
    snap = str(tmp_path / "snap.pt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_ppo.py"), "--env", "cassie3d", "--envs-per-gpu", "256", "--horizon", "4", "--n-itr", "2",
                        "--snapshot", snap], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and os.path.exists(snap), p.stderr[-2000:]
    st = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(st) == 2 and st[-1]["minibatch_steps"] == 16 and np.isfinite(st[-1]["loss_last"]) and st[-1]["env_steps"] == 256 * 4
    q = subprocess.run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "128", "--max-path-length", "30"], capture_output=True, text=True, timeout=900)
    assert q.returncode == 0, q.stderr[-2000:]
    r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
    assert r["itr"] == 2 and r["envs"] == 128 and 0 < r["avg_path_length"] <= 30 and np.isfinite(r["avg_return"])
    two = P.make_cassie_ppo(64, kind="stand", control_mode="Torque", trajectory=default_gait(), batch_size=64 * 2, minibatch_size=64)
    with pytest.raises(ValueError, match="cassie3d.*cassie2d"):
        two.load(snap)
    two.env.close()
