"""PPO's value network on the GPU: the kernels of csrc/tu_vf.hip (CassieVfPredict, CassieVfGae, CassieVfGrad) against the torch statements of
cassierl_amd/value.py at 26 and 45 observations, the whole update against float64, the switches, resume, and train_ppo.py --value mlp with its
snapshot.  -m gpu only.  The shapes are the layout's edges (a lone lane, a second tile, a partial group of four tiles, more than one workgroup,
the second trip of the group loop), not the workload.

The reference of every gradient check is FLOAT64 torch autograd of value.value_loss on a .double() copy of the network; the bounds are those of
tests/test_gpu_ppo.py for the policy's kernels of the same layout."""
import copy
import ctypes as ct
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL = -1
N_BATCH = 5000        # rows of the batch the main gradient cases index
N_BIG = 40000         # ... and the case of the second trip of the group loop (m = 32 768 + 77 rows of it)


def _vf(D, seed=4):
    import torch
    from cassierl_amd import value as VF
    torch.manual_seed(seed)
    vf = VF.MLPValueFunction(D, (128, 128)).cuda()
    with torch.no_grad():
        for p in vf.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return vf


_CASES = {}


def _case(D, n):
    """One network, batch and target per (D, n), shared by the tests and left unchanged: obs [n, D] float32, the float64 copy of the network,
    its values V_64(obs) and the targets V_64(obs) + N(0, 1) -- residuals of order one and of both signs."""
    import torch
    from cassierl_amd import value as VF
    if (D, n) not in _CASES:
        vf = _vf(D)
        g = torch.Generator(device="cuda").manual_seed(100 + D)
        obs = torch.randn(n, D, device="cuda", generator=g)
        vf64 = copy.deepcopy(vf).double()
        v64 = vf64.predict(obs.double())
        y64 = v64 + torch.randn(n, device="cuda", generator=g, dtype=torch.float64)
        theta = VF.aligned_value_params(vf)
        vk = VF.ValueKernels(vf, theta)
        assert vk.kind == "vf_grad" and theta.data_ptr() % 16 == 0
        vk.set_batch(obs, y64)
        _CASES[(D, n)] = (vf, vf64, obs, v64, y64, vk)
    return _CASES[(D, n)]


def _blocks(D):
    """(name, offset, rows, columns, column slice) of the parameter blocks the gradient is judged in."""
    H, out, o = 128, [], 0
    for name, r, c in (("W1", H, D), ("b1", H, 1), ("W2", H, H), ("b2", H, 1), ("W3", 1, H), ("b3", 1, 1)):
        if name == "W1" and D > 32:
            out += [("W1[:, :32]", o, r, c, slice(0, 32)), ("W1[:, 32:]", o, r, c, slice(32, c))]
        else:
            out.append((name, o, r, c, slice(0, c)))
        o += r * c
    return out


# ------------------------------------------------------------------------------------------------------------------ predict
@pytest.mark.parametrize("D", [26, 45])
@pytest.mark.parametrize("n", [1, 33, 130, 257])
def test_predict_matches_the_float64_forward(D, n):
    import torch
    from cassierl_amd._lib import ptr
    vf, vf64, obs, v64, _, vk = _case(D, N_BATCH)
    pad, fill = 40, -777.0
    out = torch.full((n + pad,), fill, device="cuda")
    o = obs[:n].contiguous()
    vk._call("Predict", ptr(o), n, D, *vk._net(), ptr(out))
    err, top = (out[:n].double() - v64[:n]).abs().max().item(), v64[:n].abs().max().item()
    print("predict D %d n %d: err %.3g (max |V| %.3g, bound %.3g)" % (D, n, err, top, 5e-6 * (1 + top)))
    assert err < 5e-6 * (1 + top)
    assert bool((out[n:] == fill).all())   # rows past n keep their fill
    assert torch.equal(vk.predict(o), out[:n])
    assert vk.fn["ParamCount"](D) == 128 * D + 128 + 128 * 128 + 128 + 128 + 1 and vk.fn["ParamCount"](17) == 0


# ------------------------------------------------------------------------------------------------------------------ gradient
def _index(mode, m, n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    if mode == "rows":
        return None
    if mode == "subset":
        return torch.randperm(n, device="cuda", generator=g)[:m].contiguous()
    return torch.randint(0, n, (m,), device="cuda", generator=g)   # repeats


def _check_grad(D, n, m, mode):
    import torch
    from cassierl_amd import trpo as T
    from cassierl_amd import value as VF
    vf, vf64, obs, _, y64, vk = _case(D, n)
    idx = _index(mode, m, n, 7 * m + D)
    sel = slice(0, m) if idx is None else idx
    got, st = vk.grad(idx, m=m)
    got, st = got.clone(), st.clone()
    loss64 = VF.value_loss(vf64, obs[sel].double(), y64[sel])
    ref = T.flat_grad(loss64, vf64)
    g32 = T.flat_grad(VF.value_loss(vf, obs[sel], y64[sel].float()), vf).double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    for name, o, r, c, cols in _blocks(D):
        blk = lambda g: g[o:o + r * c].view(r, c)[:, cols]
        top = blk(ref).abs().max().item()
        e_k, e_t = (blk(got.double()) - blk(ref)).abs().max().item() / top, (blk(g32) - blk(ref)).abs().max().item() / top
        print("vf_grad D %d m %d %s %s: kernel %.3g, float32 torch autograd %.3g (relative to the block's max |g_ref| %.3g)" % (D, m, mode, name, e_k, e_t, top))
        assert e_k < 2e-4, (name, e_k, e_t)
        if r == 128:   # the 32-row quarters, one per wavefront
            for q in range(4):
                rq, kq, tq = (blk(x)[32 * q:32 * q + 32] for x in (ref, got.double(), g32))
                tq_top = rq.abs().max().item()
                eq_k, eq_t = (kq - rq).abs().max().item() / tq_top, (tq - rq).abs().max().item() / tq_top
                print("      quarter %d: kernel %.3g, float32 torch autograd %.3g" % (q, eq_k, eq_t))
                assert eq_k <= max(2e-4, 4.0 * eq_t), (name, q, eq_k, eq_t)
    s_ref = loss64.item() * m
    print("   loss statistic: kernel %.9g, float64 %.9g" % (st.item(), s_ref))
    assert abs(st.item() - s_ref) / m < 2e-5 * (s_ref / m), (st.item(), s_ref)
    got2, st2 = vk.grad(idx, m=m)
    assert torch.equal(got, got2) and torch.equal(st, st2)   # fixed-order sums: the same bits twice


@pytest.mark.parametrize("D", [26, 45])
@pytest.mark.parametrize("mode", ["rows", "subset", "repeats"])
@pytest.mark.parametrize("m", [77, 1000, 4099])
def test_value_grad_matches_float64_autograd(D, m, mode):
    _check_grad(D, N_BATCH, m, mode)


@pytest.mark.parametrize("D", [26, 45])
def test_value_grad_on_the_second_trip_of_the_group_loop(D):
    """The row cap is 256 workgroups x 128 samples: m = 32 768 + 77 is the smallest kind of minibatch at which a workgroup runs a second group."""
    m = 32768 + 77
    vk = _case(D, N_BIG)[-1]
    assert vk.fn["GradRows"](m) == 256 and vk.fn["GradRows"](32768) == 256 and vk.fn["GradRows"](77) == 1 and vk.fn["GradRows"](129) == 2
    _check_grad(D, N_BIG, m, "subset")


@pytest.mark.parametrize("D", [26, 45])
def test_value_grad_clamps_a_wild_index(D):
    import torch
    vk = _case(D, N_BATCH)[-1]
    n = N_BATCH
    idx = torch.tensor([-7, 0, 3, n - 1, n, n + 1000, 2 ** 40, 17, 17], dtype=torch.int64, device="cuda")
    a, sa = vk.grad(idx)
    a, sa = a.clone(), sa.clone()
    b, sb = vk.grad(idx.clamp(0, n - 1))
    assert torch.equal(a, b) and torch.equal(sa, sb) and torch.isfinite(a).all() and torch.isfinite(sa).all()


# ------------------------------------------------------------------------------------------------------------------ GAE
@pytest.mark.parametrize("with_last", [True, False])
@pytest.mark.parametrize("T_,N", [(8, 4096), (5, 1000), (1, 77)])
def test_gae_kernel_matches_the_torch_statement(T_, N, with_last):
    import torch
    from cassierl_amd import ppo as P
    vk = _case(26, N_BATCH)[-1]
    g = torch.Generator(device="cuda").manual_seed(T_ * 1000 + N)
    rew = torch.randn(T_, N, device="cuda", generator=g, dtype=torch.float64)
    cut = torch.rand(T_, N, device="cuda", generator=g) < 0.2
    val = torch.randn(T_, N, device="cuda", generator=g)
    last = torch.randn(N, device="cuda", generator=g) if with_last else None
    ret, adv, y, sums = vk.gae(val, last, rew, cut, 0.99, 0.95)
    last64 = torch.zeros(N, device="cuda", dtype=torch.float64) if last is None else last.double()
    ret_r, adv_r = P.gae_advantages(rew, cut, val.double(), last64, 0.99, 0.95)
    y_r = adv_r + val.double()
    for name, a, b in (("returns", ret, ret_r), ("adv", adv, adv_r), ("vtarget", y, y_r)):
        err = (a - b).abs().max().item()
        print("CassieVfGae T %d N %d last %s %s: err %.3g (max %.3g)" % (T_, N, with_last, name, err, b.abs().max().item()))
        assert err <= 1e-12 * (1 + b.abs().max().item())
    s_r = torch.stack([adv_r.sum(), (adv_r * adv_r).sum()])
    print("   sums: kernel %r, float64 %r" % (sums.tolist(), s_r.tolist()))
    assert ((sums - s_r).abs() <= 1e-10 * s_r.abs()).all(), (sums, s_r)
    r2 = vk.gae(val, last, rew, cut, 0.99, 0.95)
    assert all(torch.equal(a, b) for a, b in zip((ret, adv, y, sums), r2))
    ret_t, adv_t, y_t, none = vk.gae(val, last, rew, cut, 0.99, 0.95, fused=False)   # the torch statement behind the same call
    assert none is None and torch.equal(adv_t, adv_r) and torch.equal(y_t, y_r)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_anything_is_written():
    import torch
    from cassierl_amd._lib import ptr
    D, n, m, fill = 45, 300, 200, -777.0
    vf, _, obs, _, y64, vk = _case(D, N_BATCH)
    obs, y = obs[:n].contiguous(), y64[:n].float().contiguous()
    idx = torch.arange(m, device="cuda", dtype=torch.int64)
    W = [p.value for p in vk._net()]
    rows = vk.fn["GradRows"](n)   # (the last call below runs all n rows: the buffers are sized for it)
    assert rows >= vk.fn["GradRows"](m)
    partial = torch.full((rows, vk.NP), fill, device="cuda")
    stats = torch.full((rows,), fill, device="cuda", dtype=torch.float64)
    out = torch.full((n,), fill, device="cuda")
    stream = vk._stream()
    V = ct.c_void_p

    def grad(obs_p=obs.data_ptr(), n_=n, D_=D, W_=W, idx_p=idx.data_ptr(), m_=m, y_p=y.data_ptr(), part_p=partial.data_ptr(), st_p=stats.data_ptr()):
        return vk.fn["Grad"](V(obs_p), n_, D_, *[V(w) for w in W_], V(idx_p), m_, V(y_p), ct.c_float(1.0 / m), V(part_p), V(st_p), stream)

    def predict(obs_p=obs.data_ptr(), n_=n, D_=D, W_=W, out_p=out.data_ptr()):
        return vk.fn["Predict"](V(obs_p), n_, D_, *[V(w) for w in W_], V(out_p), stream)

    bad_w = lambda k, v: W[:k] + [v] + W[k + 1:]
    cases = [grad(obs_p=None), grad(n_=0), grad(n_=-3), grad(m_=0), grad(m_=-1), grad(idx_p=None, m_=n + 1), grad(y_p=None), grad(part_p=None), grad(st_p=None),
             grad(D_=17), grad(D_=44), grad(D_=26 + 45)]
    cases += [grad(W_=bad_w(k, None)) for k in range(6)] + [grad(W_=bad_w(k, W[k] + 4)) for k in (1, 2, 3, 4)]   # null; b1 / W2 / b2 / W3 off a 16-byte boundary
    cases += [predict(obs_p=None), predict(n_=0), predict(D_=17), predict(out_p=None)] + [predict(W_=bad_w(k, None)) for k in range(6)]
    cases += [predict(W_=bad_w(k, W[k] + 4)) for k in (1, 2, 3, 4)]
    T_, N = 3, 100
    rew = torch.zeros(T_, N, device="cuda", dtype=torch.float64)
    cut = torch.zeros(T_, N, device="cuda", dtype=torch.bool)
    val = torch.zeros(T_, N, device="cuda")
    o3 = [torch.full((T_, N), fill, device="cuda", dtype=torch.float64) for _ in range(3)]
    part = torch.full((1, 2), fill, device="cuda", dtype=torch.float64)

    def gae(val_p=val.data_ptr(), rew_p=rew.data_ptr(), cut_p=cut.data_ptr(), T__=T_, N_=N, outs=tuple(x.data_ptr() for x in o3), part_p=part.data_ptr()):
        return vk.fn["Gae"](V(val_p), None, V(rew_p), V(cut_p), T__, N_, ct.c_double(0.99), ct.c_double(0.95), *[V(x) for x in outs], V(part_p), stream)

    p3 = tuple(x.data_ptr() for x in o3)
    cases += [gae(val_p=None), gae(rew_p=None), gae(cut_p=None), gae(T__=0), gae(N_=0), gae(part_p=None)] + [gae(outs=p3[:k] + (None,) + p3[k + 1:]) for k in range(3)]
    torch.cuda.synchronize()
    assert cases and all(rc == EINVAL for rc in cases), cases
    for t in [partial, stats, out, part] + o3:
        assert bool((t == fill).all())
    assert grad() == 0 and predict() == 0 and gae() == 0   # ... and the same calls with good arguments run
    torch.cuda.synchronize()
    assert torch.isfinite(partial).all() and torch.isfinite(out).all() and torch.isfinite(o3[2]).all()
    assert grad(idx_p=None, m_=n) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ whole update
def _make(family, n_envs, **kw):
    from cassierl_amd import ppo as P
    from cassierl_amd.trajectory import default_gait
    env_kw = dict(env="cassie3d") if family == "cassie3d" else dict(kind="stand", control_mode="Torque", trajectory=default_gait())
    return P.make_cassie_ppo(n_envs, seed=1, value="mlp", **env_kw, **kw)


@pytest.mark.parametrize("family", ["cassie3d", "cassie2d"])
def test_fused_update_is_as_close_to_float64_as_the_torch_update(family):
    """One batch (256 envs x 4 steps), epochs = 1, 2 minibatches: the fused float32 update, the forced-torch float32 update and the torch float64
    update from the same parameters, batch and permutation, for the policy's and the value network's vector.  Required of each:
    |theta_fused - theta_64| <= 4 |theta_torch32 - theta_64| (the factor 4: two float32 evaluations of one expression that differ in summation order)."""
    import torch
    from cassierl_amd import trpo as T
    algo = _make(family, 256, batch_size=256 * 4, epochs=1, minibatch_size=256 * 2)
    assert algo.value_kind == "mlp" and algo.obs_dim == (45 if family == "cassie3d" else 26)
    d = algo.process(algo.collect())
    assert algo.last_gae_fused and algo.last_value_kind == "vf_grad" and set(d) >= {"vtarget", "v_old"}
    assert d["vtarget"].dtype == torch.float64 and torch.isfinite(d["vtarget"]).all() and torch.isfinite(d["adv"]).all()
    pol32, vf32 = algo.policy, algo.baseline
    theta0, vtheta0 = T.flat_params(pol32).clone(), T.flat_params(vf32).clone()
    gen0 = algo.gen_mb.get_state()
    res = {}
    for name in ("fused", "torch32", "torch64"):
        algo.adam_t, algo.adam_m, algo.adam_v = 0, None, None
        algo.value_adam_t, algo.value_adam_m, algo.value_adam_v = 0, None, None
        algo.gen_mb.set_state(gen0)
        algo.fused_grad = algo.fused_adam = algo.fused_value = name == "fused"
        if name == "torch64":
            algo.policy, algo.baseline = copy.deepcopy(pol32).double(), copy.deepcopy(vf32).double()
            T.set_flat_params(algo.policy, theta0.double()); T.set_flat_params(algo.baseline, vtheta0.double())
            st = algo.optimize({k: v.double() for k, v in d.items()})
        else:
            T.set_flat_params(pol32, theta0); T.set_flat_params(vf32, vtheta0)
            st = algo.optimize(d)
        assert algo.last_value_kind == ("vf_grad" if name == "fused" else "autograd") and algo.last_adam_fused == (name == "fused")
        assert st["minibatch_steps"] == 2 and algo.adam_t == 2 and algo.value_adam_t == 2
        res[name] = (T.flat_params(algo.policy).double().clone(), T.flat_params(algo.baseline).double().clone(), st)
    algo.policy, algo.baseline = pol32, vf32
    for k in ("loss_first", "loss_last", "value_loss_first", "value_loss_last", "explained_variance"):
        print("   %s: fused %.8g torch32 %.8g torch64 %.8g" % (k, res["fused"][2][k], res["torch32"][2][k], res["torch64"][2][k]))
    for which, i, start in (("policy", 0, theta0), ("value", 1, vtheta0)):
        t64 = res["torch64"][i]
        e_f, e_t, step = (res["fused"][i] - t64).norm().item(), (res["torch32"][i] - t64).norm().item(), (t64 - start.double()).norm().item()
        print("%s %s: |theta_fused - theta_64| %.4g, |theta_torch32 - theta_64| %.4g, |step_64| %.4g" % (family, which, e_f, e_t, step))
        assert step > 0 and e_f <= 4.0 * e_t, (which, e_f, e_t)
    algo.env.close()


def test_switches_force_the_torch_paths():
    algo = _make("cassie3d", 64, batch_size=64 * 2, epochs=1, minibatch_size=64)
    st = algo.train_iteration()
    assert algo.last_value_kind == "vf_grad" and algo.last_gae_fused and np.isfinite(st["value_loss_last"])
    algo.fused_gae = False
    algo.train_iteration()
    assert algo.last_value_kind == "vf_grad" and not algo.last_gae_fused
    algo.fused_gae, algo.fused_value = True, False
    st = algo.train_iteration()
    assert algo.last_value_kind == "autograd" and not algo.last_gae_fused and algo.last_grad_kind == "pg3d_clip"
    assert np.isfinite(st["value_loss_last"]) and np.isfinite(st["explained_variance"]) and algo.value_adam_t == 3 * 2   # (two minibatches of 64 per iteration)
    algo.env.close()


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    import torch
    from cassierl_amd import trpo as T
    mk = lambda: _make("cassie3d", 128, batch_size=128 * 4, epochs=2, minibatch_size=128)
    a = mk()
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ref = a.train_iteration()
    assert a.last_grad_kind == "pg3d_clip" and a.last_value_kind == "vf_grad" and a.last_adam_fused and a.last_gae_fused
    ta, va = T.flat_params(a.policy).clone(), T.flat_params(a.baseline).clone()
    ma, wa = a.value_adam_m.clone(), a.value_adam_v.clone()
    a.env.close()
    b = mk()
    _, restored = b.load(p)
    assert restored and b.adam_t == 16 and b.value_adam_t == 16
    got = b.train_iteration()
    assert got["itr"] == ref["itr"] == 2
    for k in ("avg_reward", "grad_norm", "loss_first", "loss_last", "mean_kl", "clip_frac", "value_loss_first", "value_loss_last", "explained_variance"):
        assert got[k] == ref[k], k
    assert torch.equal(T.flat_params(b.policy), ta) and torch.equal(T.flat_params(b.baseline), va)
    assert torch.equal(b.value_adam_m, ma) and torch.equal(b.value_adam_v, wa)
    b.env.close()


def test_train_ppo_with_a_value_network_and_its_snapshot(tmp_path):
    """train_ppo.py --env cassie3d --value mlp for two iterations at 128 environments; sim_policy.py rolls the snapshot out; a linear-value run refuses it."""
    import torch
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_ppo.py"), "--env", "cassie3d", "--value", "mlp", "--envs-per-gpu", "128", "--horizon", "4",
                        "--n-itr", "2", "--snapshot", snap], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and os.path.exists(snap), p.stderr[-2000:]
    st = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(st) == 2 and st[-1]["minibatch_steps"] == 16 and np.isfinite(st[-1]["value_loss_last"]) and st[-1]["env_steps"] == 128 * 4
    ck = torch.load(snap, map_location="cpu", weights_only=True)
    assert ck["value_kind"] == "mlp" and ck["value_hidden"] == [128, 128] and ck["baseline"] is None and ck["value_adam_t"] == 32
    assert ck["value_net"].numel() == 128 * 45 + 128 + 128 * 128 + 128 + 128 + 1
    q = subprocess.run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "128", "--max-path-length", "30"], capture_output=True, text=True, timeout=900)
    assert q.returncode == 0, q.stderr[-2000:]
    r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
    assert r["itr"] == 2 and r["envs"] == 128 and 0 < r["avg_path_length"] <= 30 and np.isfinite(r["avg_return"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_ppo.py"), "--env", "cassie3d", "--value", "linear", "--envs-per-gpu", "128", "--horizon", "4",
                        "--n-itr", "1", "--load-policy", snap], capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "the snapshot's value function is 'mlp', this run's is 'linear'" in r.stderr, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]   # refused at the load: no iteration ran
