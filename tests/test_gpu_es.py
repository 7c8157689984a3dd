"""ES's kernels (csrc/tu_es.hip) against the float64 torch statements of cassierl_amd/es.py, the fused update against the torch update, resume, and
train_es.py / sim_policy.py on the GPU.  -m gpu only.

Buffer layout of every kernel case: the table is a slice out of the middle of a larger buffer whose remainder is NaN (and starts on an odd float, so
no slice is 16-byte aligned by accident); obs and env_actions are the first n rows of longer buffers with NaN / a sentinel behind them.  A read past
any end shows up in the result, a write past the end in the sentinel; neither faults.  No offset outside its range reaches a kernel (the range check
is exercised on the host: tests/test_es_cpu.py).  All inputs are drawn on the CPU."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(26, 6), (26, 7), (17, 7)]
SAT = 60.0     # the `saturated` regime of tests/test_gpu_onpolicy_edges.py: every second unit's row of W1, b1, W2, b2 times 60
PAD = 1001     # NaN floats in front of and behind the table
SENT = 777.0
# The kernel writes the action only behind the map, and the map clips every action outside [-1, 1] whatever the box is (it sends [-1, 1] onto
# [low, high]).  To compare EVERY output before the map, the accuracy launches use the unit box (low = -1, high = 1), whose map
# -1 + (act + 1) * 0.5 * 2 returns a float32 act in (-1, 1) exactly, and are repeated with the output bias b3 shifted by every integer c up to the
# largest reference action: an output whose float64 action plus c lies within 0.75 of 0 is read from the launch with that shift (every output is
# within 0.5 of an integer) and compared, unclipped, with the float64 and float32 torch statements AT THE SAME shifted parameters; c is then taken
# off all three.  The partial sums of such an output are as large with the shift as without it, and the bound keeps the scale of the unshifted
# float64 action before the map, 5e-6 (1 + max|ref|).
WINDOW = 0.75


def _check(name, got, ref64, ref32, rel, scale):
    """tests/test_gpu_offpolicy_edges.py's rule: the fixed bound rel * scale, else DESIGN.md 9h's err_kernel <= 4 err_torch32."""
    import torch
    got, ref64, ref32 = (torch.as_tensor(x).double().reshape(-1) for x in (got, ref64, ref32))
    assert torch.isfinite(got).all() and torch.isfinite(ref64).all(), name
    err_k, err_t = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    rule = "bound" if err_k < rel * scale else "4x"
    print("%s: against float64 kernel %.3g, torch float32 %.3g, of max %.3g (%s, bound %.3g)" % (name, err_k, err_t, scale, rule, rel * scale))
    assert err_k < rel * scale or err_k <= 4 * err_t, (name, err_k, err_t, scale)
    return rule


def _table(g, length):
    """(table, its buffer): `length` normal numbers in the middle of a NaN buffer, on the device."""
    import torch
    buf = torch.full((length + 2 * PAD,), float("nan"))
    buf[PAD:PAD + length] = torch.randn(length, generator=g)
    buf = buf.to(DEV)
    return buf[PAD:PAD + length], buf


def _theta(g, D, A, regime):
    """The default initialisation (Xavier-uniform, zero bias) + N(0, 0.1) jitter as the row [W1 | b1 | W2 | b2 | W3 | b3], then the regime."""
    import torch
    parts = []
    for i, (o, k) in enumerate(((32, D), (32, 32), (A, 32))):
        W = (torch.rand(o, k, generator=g) * 2 - 1) * math.sqrt(6.0 / (o + k)) + 0.1 * torch.randn(o, k, generator=g)
        b = 0.1 * torch.randn(o, generator=g)
        if regime == "saturated" and i < 2:
            W[0::2] *= SAT; b[0::2] *= SAT
        parts += [W.reshape(-1), b]
    return torch.cat(parts)


def _offsets(g, m, top):
    """m offsets in [0, top]: both ends, all four residues mod 4, two directions sharing an offset, two overlapping slices, then random ones."""
    import torch
    fixed = [top, 0, 1, 2, 3, 7, 7, 100, 100 + 1000, top - 1, top - 2]
    off = torch.cat([torch.tensor(fixed, dtype=torch.int64), torch.randint(0, top + 1, (max(0, m - len(fixed)),), generator=g)])[:m].contiguous()
    if m >= len(fixed):
        assert set((off % 4).tolist()) == {0, 1, 2, 3} and int(off.min()) == 0 and int(off.max()) == top
    return off


def _alive_cases(n):
    import torch
    ones = torch.ones(n, dtype=torch.uint8)
    one_of_a_pair = ones.clone(); one_of_a_pair[1::4] = 0; one_of_a_pair[2::4] = 0   # pairs (1, 0), (0, 1), ...
    third = ones.clone(); third[0::3] = 0
    return [("null", None), ("ones", ones), ("zeros", torch.zeros(n, dtype=torch.uint8)), ("one of a pair", one_of_a_pair), ("every third", third)]


@pytest.mark.parametrize("regime", ["default", "saturated"])
@pytest.mark.parametrize("sigma", [0.0, 0.02, 1.0])
@pytest.mark.parametrize("D,A", SHAPES)
def test_es_policy_step_matches_the_torch_statement(D, A, sigma, regime):
    import torch
    from cassierl_amd import es as E
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env import action_space
    g = torch.Generator().manual_seed(1000 * D + 10 * A + int(100 * sigma) + (7 if regime == "saturated" else 0))
    P = E.param_count(D, (32, 32), A)
    table, tbuf = _table(g, 3 * P + 1000)
    theta = _theta(g, D, A, regime).to(DEV)
    assert theta.numel() == P
    box = action_space("PD" if A == 6 else "OSC")
    real = T.NormalizedActions(box.low, box.high, DEV)
    unit = T.NormalizedActions([-1.0] * A, [1.0] * A, DEV)
    ident = lambda a: a
    mid = real.low + (real.high - real.low) / 2
    ppw = E.EsKernels(table, 2, D, A).fn["PairsPerWorkgroup"]()
    rules, widest = set(), 0
    for n in (2, 2 * ppw - 2, 2 * ppw, 2 * ppw + 2, 130, 4098):
        off = _offsets(g, n // 2, table.numel() - P).to(DEV)
        obs_buf = torch.full((n + 8, D), float("nan"), dtype=torch.float64)
        obs_buf[:n] = torch.randn(n, D, dtype=torch.float64, generator=g)
        if sigma == 0.0:
            obs_buf[1:n:2] = obs_buf[0:n:2]   # equal observations in a pair: equal bits below
        obs_buf = obs_buf.to(DEV)
        obs = obs_buf[:n]
        kw, kr = E.EsKernels(table, n, D, A, unit.low, unit.high), E.EsKernels(table, n, D, A, real.low, real.high)
        kw.set_directions(off); kr.set_directions(off)
        # the float64 and float32 torch statements before the map, every environment alive, per shift c of the output bias
        m64 = E.es_actions_torch(theta.double(), table.double(), off, sigma, obs, None, ident)
        scale = 1.0 + m64.abs().max().item()
        top_c = int(math.ceil(m64.abs().max().item()))
        shifts, ref64, ref32, sel, seen = [], [], [], [], torch.zeros_like(m64, dtype=torch.bool)
        for c in range(-top_c, top_c + 1):
            th_c = theta.clone(); th_c[P - A:] += float(c)
            r64 = E.es_actions_torch(th_c.double(), table.double(), off, sigma, obs, None, ident)
            pick = (r64.abs() <= WINDOW) & ~seen
            if not bool(pick.any()):
                continue
            seen |= pick
            shifts.append((c, th_c)); sel.append(pick); ref64.append(r64 - c)
            ref32.append(E.es_actions_torch(th_c, table, off, sigma, obs.float(), None, ident).double() - c)
        assert bool(seen.all())   # every output is read from some launch, unclipped
        widest = max(widest, len(shifts))
        for name, alive in _alive_cases(n):
            alive = None if alive is None else alive.to(DEV)
            up = torch.ones(n, dtype=torch.bool, device=DEV) if alive is None else alive.bool()
            tag = "ES policy step %s (%d, %d) sigma %g n %d alive %s" % (regime, D, A, sigma, n, name)
            env_w = torch.full((n + 8, A), SENT, dtype=torch.float64, device=DEV)
            env_r = torch.full((n + 8, A), SENT, dtype=torch.float64, device=DEV)
            env_c = torch.full((n + 8, A), SENT, dtype=torch.float64, device=DEV)
            got, want64, want32 = (torch.full_like(m64, float("nan")) for _ in range(3))
            for (c, th_c), pick, r64, r32 in zip(shifts, sel, ref64, ref32):
                kw.policy_step(obs, th_c, sigma, alive, out=env_c[:n])
                assert (env_c[:n][~up] == 0).all() and (env_c[n:] == SENT).all()
                got[pick], want64[pick], want32[pick] = env_c[:n][pick] - c, r64[pick], r32[pick]
            live = up[:, None].expand(n, A)
            if bool(live.any()):
                rules.add(_check(tag, got[live], want64[live], want32[live], 5e-6, scale))
                assert (want64[live] - m64[live]).abs().max().item() < 1e-5 * scale   # the shifted references are the unshifted action
            kw.policy_step(obs, theta, sigma, alive, out=env_w[:n])
            kr.policy_step(obs, theta, sigma, alive, out=env_r[:n])
            first = (env_w.clone(), env_r.clone())
            act = env_w[:n]
            assert (act[~up] == 0).all()
            assert (env_r[:n] - real(act)).abs().max().item() < 1e-12
            assert (env_r[:n] >= real.low).all() and (env_r[:n] <= real.high).all()
            assert torch.equal(env_r[:n][~up], mid.expand(n, A)[~up])   # a dead environment: low + (high - low) / 2 exactly
            assert (env_w[n:] == SENT).all() and (env_r[n:] == SENT).all()
            if sigma == 0.0:
                assert torch.equal(env_w[0:n:2], env_w[1:n:2]) if alive is None else torch.equal(env_w[0:n:2][up[0::2] & up[1::2]], env_w[1:n:2][up[0::2] & up[1::2]])
            kw.policy_step(obs, theta, sigma, alive, out=env_w[:n])
            kr.policy_step(obs, theta, sigma, alive, out=env_r[:n])
            assert torch.equal(env_w, first[0]) and torch.equal(env_r, first[1])
        assert torch.isnan(obs_buf[n:]).all()
    assert torch.isnan(tbuf[:PAD]).all() and torch.isnan(tbuf[-PAD:]).all()
    print("ES policy step %s (%d, %d) sigma %g: rules used %s, at most %d shifted launches per case" % (regime, D, A, sigma, sorted(rules), widest))


def test_es_policy_step_refuses_bad_arguments():
    import ctypes as ct
    import torch
    from cassierl_amd import es as E
    table = torch.randn(5000).to(DEV)
    lo, hi = torch.full((6,), -1.0, dtype=torch.float64, device=DEV), torch.full((6,), 1.0, dtype=torch.float64, device=DEV)
    ek = E.EsKernels(table, 4, 26, 6, lo, hi)
    ek.set_directions(torch.tensor([0, 5], device=DEV))
    obs, theta = torch.zeros(4, 26, dtype=torch.float64, device=DEV), torch.zeros(ek.P, device=DEV)
    P = lambda t: ct.c_void_p(t.data_ptr())
    out = torch.full((5, 6), SENT, dtype=torch.float64, device=DEV)
    good = [P(obs), 4, 26, 6, P(theta), P(table), ct.c_longlong(5000), P(ek.offsets), ct.c_float(0.1), None, P(lo), P(hi), P(out), None]
    fn = ek.fn["PolicyStep"]
    assert fn(*good) == 0
    for k, v in ((1, 3), (1, 0), (2, 20), (3, 5), (6, ct.c_longlong(ek.P - 1)), (0, None), (4, None), (5, None), (7, None), (10, None), (11, None), (12, None)):
        bad = list(good); bad[k] = v
        assert fn(*bad) == -1, k
    torch.cuda.synchronize()
    assert (out[4:] == SENT).all() and (out[:4].abs() <= 1).all()


@pytest.mark.parametrize("n_params", [1, 63, 65, 1863, 2118])
def test_es_grad_matches_the_torch_statement(n_params):
    import torch
    from cassierl_amd import es as E
    g = torch.Generator().manual_seed(n_params)
    table, tbuf = _table(g, 3 * 2118 + 1000)
    top = table.numel() - n_params
    t64 = table.double()
    for m in (1, 2, 63, 64, 65, 257, 4099, 8193):   # 8193: the cap of 128 rows, whose last row starts past m and is all zero
        ek = E.EsKernels(table, 2 * m, 26, 6)
        off = _offsets(g, m, top)
        if m >= 2:
            off[0], off[-1] = 0, top
        off = off.to(DEV)
        ek.set_directions(off, n_params=n_params)
        rows = ek.fn["GradRows"](m)
        chunk = -(-m // rows)
        assert rows >= 1 and ((rows - 1) * chunk < m or m == 8193) and (m != 8193 or (rows == 128 and 126 * chunk < m <= 127 * chunk))
        # one-hot weights: the first and the last direction and both sides of every row boundary -> exactly w_d eps_d
        hot = sorted({0, m - 1} | {d for r in range(1, rows) for d in (r * chunk - 1, r * chunk) if d < m})
        eps = E.directions(table, off[hot], n_params)
        for j, d in enumerate(hot):
            w = torch.zeros(m)
            w[d] = -1.7 if j % 2 else 0.3
            got = ek.grad(w.to(DEV))
            assert got.shape == (n_params,) and torch.equal(got, w[d].item() * eps[j]), (m, d)
        # random weights with zeros and a 1e6 spread of magnitudes
        w = torch.randn(m, generator=g) * 10.0 ** (torch.rand(m, generator=g) * 6 - 3)
        w[torch.rand(m, generator=g) < 0.2] = 0.0
        w[m - 1] = 2.5
        w = w.to(DEV)
        ref = E.es_grad_torch(t64, off, w.double(), n_params)
        got = ek.grad(w)
        assert torch.isfinite(got).all()
        err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
        print("ES grad n_params %d m %d: %d rows, error %.3g of max %.3g" % (n_params, m, rows, err, scale))
        assert err <= 2e-4 * scale
        assert torch.equal(ek.grad(w), got)   # fixed-order sums: the same bits twice
        assert ek._partial[m, n_params].shape == (rows, n_params)
        if m == 8193:
            assert (ek._partial[m, n_params][127] == 0).all() and (ek._partial[m, n_params][126] != 0).any()
    assert torch.isnan(tbuf[:PAD]).all() and torch.isnan(tbuf[-PAD:]).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_es_book_is_bit_equal_to_torch(n):
    import torch
    from cassierl_amd import es as E
    g = torch.Generator().manual_seed(n)
    ek = E.EsKernels(torch.zeros(5000, device=DEV), 2, 26, 6)
    steps = 12
    rew = torch.randn(steps, n, dtype=torch.float64, generator=g).to(DEV)
    done = (torch.rand(steps, n, generator=g) < 0.15).to(torch.uint8).to(DEV)
    fit = torch.full((n + 8,), SENT, dtype=torch.float64, device=DEV); fit[:n] = 0
    length = torch.full((n + 8,), 777, dtype=torch.int64, device=DEV); length[:n] = 0
    alive = torch.full((n + 8,), 77, dtype=torch.uint8, device=DEV); alive[:n] = 1
    fit_t, len_t, alive_t = fit[:n].clone(), length[:n].clone(), alive[:n].clone()
    for t in range(steps):
        ek.book(rew[t], done[t], alive[:n], fit[:n], length[:n])
        E.es_book_torch(rew[t], done[t], alive_t, fit_t, len_t)
        assert torch.equal(fit[:n], fit_t) and torch.equal(length[:n], len_t) and torch.equal(alive[:n], alive_t), t
    assert (fit[n:] == SENT).all() and (length[n:] == 777).all() and (alive[n:] == 77).all()
    assert 0 < int(alive_t.sum()) < n or n == 1


def _make(n, **kw):
    from cassierl_amd import es as E
    from cassierl_amd.trajectory import default_gait
    return E.make_cassie_es(n, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, max_path_length=8, table_size=1 << 22, **kw)


def test_fused_update_equals_the_torch_update_on_one_stand_rollout():
    """One fitness vector from a rollout on the stand env (1024 envs, 8 steps); the fused update (CassieEsGrad + CassiePgAdam) and the forced-torch
    update start from the same parameters and the same fitness, so env chaos cannot enter."""
    import torch
    from cassierl_amd import trpo as T
    algo = _make(1024)
    algo.draw_directions()
    roll = algo.collect()
    assert algo.last_policy_step_kind == "es_step" and algo.last_book_fused
    f = roll["fitness"]
    assert torch.isfinite(f).all() and int(roll["length"].max()) <= 8 and int(roll["length"].min()) >= 1
    theta0 = T.flat_params(algo.policy).clone()
    res = {}
    for fused in (True, False):
        T.set_flat_params(algo.policy, theta0)
        algo.adam_t, algo.adam_m, algo.adam_v = 0, None, None
        algo.fused_grad = algo.fused_adam = fused
        gn, sn = algo.update(f)
        assert algo.last_grad_kind == ("es_grad" if fused else "torch") and algo.last_adam_fused == fused
        res[fused] = (T.flat_params(algo.policy).clone(), gn.item(), sn.item())
    (tf, gf, sf), (tt, gt, st) = res[True], res[False]
    rel = ((tf - tt).norm() / tt.norm()).item()
    print("ES fused vs torch update: relative parameter difference %.3g, gradient norms %.6g / %.6g, step norms %.6g / %.6g" % (rel, gf, gt, sf, st))
    assert gt > 0 and st > 0 and abs(gf - gt) < 1e-5 * gt
    assert rel < 1e-5
    # the torch rollout (statements instead of kernels) on the same directions gives the same fitness up to the env's sensitivity: not asserted here
    algo.env.close()


def test_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    import torch
    from cassierl_amd import trpo as T
    a = _make(1024)
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    assert os.path.getsize(p) < 4 * (1 << 22)   # no table in the snapshot
    ref = a.train_iteration()
    assert a.last_policy_step_kind == "es_step" and a.last_grad_kind == "es_grad" and a.last_adam_fused and a.last_book_fused
    ta = T.flat_params(a.policy).clone()
    a.env.close()
    b = _make(1024)
    _, restored = b.load(p)
    assert restored and b.adam_t == 2
    got = b.train_iteration()
    assert b.last_policy_step_kind == "es_step" and b.last_grad_kind == "es_grad"
    assert got == ref and got["itr"] == 2
    assert torch.equal(T.flat_params(b.policy), ta)
    b.env.close()


KEYS = ["itr", "env_steps", "episodes", "avg_return", "max_return", "min_return", "avg_path_length", "grad_norm", "step_norm", "gathered"]


def test_train_es_and_sim_policy_scripts(tmp_path):
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_es.py"), "--envs-per-gpu", "512", "--n-itr", "2", "--max-path-length", "8", "--kind", "stand",
                        "--control-mode", "Torque", "--table-size", str(1 << 22), "--snapshot", snap], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and os.path.exists(snap), p.stderr[-2000:]
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 2
    for i, r in enumerate(rows):
        assert all(k in r for k in KEYS), r
        assert r["itr"] == i and r["episodes"] == r["gathered"] == 512 and 512 <= r["env_steps"] <= 512 * 8 and r["policy_step"] == "es_step" and r["grad"] == "es_grad"
        assert r["min_return"] <= r["avg_return"] <= r["max_return"] and 1 <= r["avg_path_length"] <= 8 and r["grad_norm"] > 0 and r["step_norm"] > 0
    q = subprocess.run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "256", "--max-path-length", "60", "--kind", "stand",
                        "--control-mode", "Torque"], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
    assert r["itr"] == 2 and r["envs"] == 256 and r["deterministic"] and 0 < r["avg_path_length"] <= 60 and np.isfinite(r["avg_return"])
