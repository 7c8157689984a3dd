"""ES at width 128: the policy step of csrc/tu_es_wide.hip (CassieEsWidePolicyStep) against the float64 torch statement of cassierl_amd/es.py at
hidden_sizes (128, 128), its argument checks, CassieEsGrad at the wide parameter counts, the fused update against the torch update, resume, and
train_es.py / sim_policy.py with --hidden 128,128.  -m gpu only.

The buffer layout, the shifted-bias method and the tolerance rule are tests/test_gpu_es.py's (its helpers are imported): the table is the middle of
a NaN buffer, obs and env_actions are the first n rows of longer buffers with NaN / a sentinel behind them, and every output is compared unclipped
in the launch whose shift of b3 brings it within 0.75 of 0.  The sizes n are those at which the kernel's grid changes (a lone pair, a short, a full
and a just over-full workgroup, several workgroups); the chunks a pair's slice is streamed in do not depend on n."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_es import PAD, SENT, WINDOW, _alive_cases, _check, _offsets, _table

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDE = (128, 128)
SHAPES = [(26, 6), (26, 7), (17, 7)]
SAT = 60.0   # the `saturated` regime: every second unit's row of W1, b1, W2, b2 times 60


def _theta_wide(g, D, A, regime):
    """tests/test_gpu_es.py's _theta at widths 128: Xavier-uniform + N(0, 0.1) jitter as the row [W1 | b1 | W2 | b2 | W3 | b3], then the regime."""
    import torch
    parts = []
    for i, (o, k) in enumerate(((128, D), (128, 128), (A, 128))):
        W = (torch.rand(o, k, generator=g) * 2 - 1) * math.sqrt(6.0 / (o + k)) + 0.1 * torch.randn(o, k, generator=g)
        b = 0.1 * torch.randn(o, generator=g)
        if regime == "saturated" and i < 2:
            W[0::2] *= SAT; b[0::2] *= SAT
        parts += [W.reshape(-1), b]
    return torch.cat(parts)


@pytest.mark.parametrize("regime", ["default", "saturated"])
@pytest.mark.parametrize("sigma", [0.0, 0.02, 1.0])
@pytest.mark.parametrize("D,A", SHAPES)
def test_es_wide_policy_step_matches_the_torch_statement(D, A, sigma, regime):
    """Rule per case: `bound` = inside 5e-6 (1 + max|ref64|); `4x` = err_kernel <= 4 err_torch32.  In the default regime the float32 torch statement
    sits at 0.06-0.12 of the bound (max|ref| about 4 at sigma <= 0.02, about 39 at sigma 1), so every case there must be decided by the bound."""
    import torch
    from cassierl_amd import es as E
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env import action_space
    g = torch.Generator().manual_seed(128000 + 1000 * D + 10 * A + int(100 * sigma) + (7 if regime == "saturated" else 0))
    P = E.param_count(D, WIDE, A)
    table, tbuf = _table(g, 3 * P + 1000)
    theta = _theta_wide(g, D, A, regime).to(DEV)
    assert theta.numel() == P
    box = action_space("PD" if A == 6 else "OSC")
    real = T.NormalizedActions(box.low, box.high, DEV)
    unit = T.NormalizedActions([-1.0] * A, [1.0] * A, DEV)
    ident = lambda a: a
    mid = real.low + (real.high - real.low) / 2
    ppw = E.EsKernels(table, 2, D, A, hidden=WIDE).fn["PairsPerWorkgroup"]()
    assert ppw >= 2
    rules, widest = set(), 0
    for n in (2, 2 * ppw - 2, 2 * ppw, 2 * ppw + 2, 130, 514):
        off = _offsets(g, n // 2, table.numel() - P).to(DEV)
        obs_buf = torch.full((n + 8, D), float("nan"), dtype=torch.float64)
        obs_buf[:n] = torch.randn(n, D, dtype=torch.float64, generator=g)
        if sigma == 0.0:
            obs_buf[1:n:2] = obs_buf[0:n:2]   # equal observations in a pair: equal bits below
        obs_buf = obs_buf.to(DEV)
        obs = obs_buf[:n]
        kw, kr = E.EsKernels(table, n, D, A, unit.low, unit.high, hidden=WIDE), E.EsKernels(table, n, D, A, real.low, real.high, hidden=WIDE)
        assert kw.P == P and kw.ENTRY["PolicyStep"] == "CassieEsWidePolicyStep"
        kw.set_directions(off); kr.set_directions(off)
        # the float64 and float32 torch statements before the map, every environment alive, per shift c of the output bias
        m64 = E.es_actions_torch(theta.double(), table.double(), off, sigma, obs, None, ident, WIDE)
        scale = 1.0 + m64.abs().max().item()
        top_c = int(math.ceil(m64.abs().max().item()))
        shifts, ref64, ref32, sel, seen = [], [], [], [], torch.zeros_like(m64, dtype=torch.bool)
        for c in range(-top_c, top_c + 1):
            th_c = theta.clone(); th_c[P - A:] += float(c)
            r64 = E.es_actions_torch(th_c.double(), table.double(), off, sigma, obs, None, ident, WIDE)
            pick = (r64.abs() <= WINDOW) & ~seen
            if not bool(pick.any()):
                continue
            seen |= pick
            shifts.append((c, th_c)); sel.append(pick); ref64.append(r64 - c)
            ref32.append(E.es_actions_torch(th_c, table, off, sigma, obs.float(), None, ident, WIDE).double() - c)
        assert bool(seen.all())   # every output is read from some launch, unclipped
        widest = max(widest, len(shifts))
        for name, alive in _alive_cases(n):
            alive = None if alive is None else alive.to(DEV)
            up = torch.ones(n, dtype=torch.bool, device=DEV) if alive is None else alive.bool()
            tag = "ES wide policy step %s (%d, %d) sigma %g n %d alive %s" % (regime, D, A, sigma, n, name)
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
                rule = _check(tag, got[live], want64[live], want32[live], 5e-6, scale)
                rules.add(rule)
                assert regime != "default" or rule == "bound", tag   # the reference itself is far inside the bound there
                assert (want64[live] - m64[live]).abs().max().item() < 1e-5 * scale   # the shifted references are the unshifted action
            kw.policy_step(obs, theta, sigma, alive, out=env_w[:n])
            kr.policy_step(obs, theta, sigma, alive, out=env_r[:n])
            first = (env_w.clone(), env_r.clone())
            act = env_w[:n]
            assert (act[~up] == 0).all()   # the unit box: a dead row is exactly 0
            assert (env_r[:n] - real(act)).abs().max().item() < 1e-12
            assert (env_r[:n] >= real.low).all() and (env_r[:n] <= real.high).all() and (act.abs() <= 1).all()
            assert torch.equal(env_r[:n][~up], mid.expand(n, A)[~up])   # a dead environment: low + (high - low) / 2 exactly
            assert (env_w[n:] == SENT).all() and (env_r[n:] == SENT).all()
            if sigma == 0.0:
                both = up[0::2] & up[1::2]
                assert torch.equal(env_w[0:n:2][both], env_w[1:n:2][both])
            kw.policy_step(obs, theta, sigma, alive, out=env_w[:n])
            kr.policy_step(obs, theta, sigma, alive, out=env_r[:n])
            assert torch.equal(env_w, first[0]) and torch.equal(env_r, first[1])   # two launches: equal bits
        assert torch.isnan(obs_buf[n:]).all()
    assert torch.isnan(tbuf[:PAD]).all() and torch.isnan(tbuf[-PAD:]).all()
    print("ES wide policy step %s (%d, %d) sigma %g: rules used %s, at most %d shifted launches per case" % (regime, D, A, sigma, sorted(rules), widest))


def test_es_wide_policy_step_refuses_bad_arguments():
    import ctypes as ct
    import torch
    from cassierl_amd import es as E
    table = torch.randn(45000).to(DEV)
    lo, hi = torch.full((6,), -1.0, dtype=torch.float64, device=DEV), torch.full((6,), 1.0, dtype=torch.float64, device=DEV)
    ek = E.EsKernels(table, 4, 26, 6, lo, hi, hidden=WIDE)
    assert ek.P == 20742
    ek.set_directions(torch.tensor([0, 5], device=DEV))
    obs, theta = torch.zeros(4, 26, dtype=torch.float64, device=DEV), torch.zeros(ek.P, device=DEV)
    P = lambda t: ct.c_void_p(t.data_ptr())
    out = torch.full((5, 6), SENT, dtype=torch.float64, device=DEV)
    good = [P(obs), 4, 26, 6, P(theta), P(table), ct.c_longlong(45000), P(ek.offsets), ct.c_float(0.1), None, P(lo), P(hi), P(out), None]
    fn = ek.fn["PolicyStep"]
    bads = ((1, 3), (1, 0), (2, 20), (3, 5), (6, ct.c_longlong(ek.P - 1)), (0, None), (4, None), (5, None), (7, None), (10, None), (11, None), (12, None))
    for k, v in bads:   # refused before anything has run: nothing is written
        bad = list(good); bad[k] = v
        assert fn(*bad) == -1, k
    torch.cuda.synchronize()
    assert (out == SENT).all()
    assert fn(*good) == 0
    for k, v in bads:
        bad = list(good); bad[k] = v
        assert fn(*bad) == -1, k
    torch.cuda.synchronize()
    assert (out[4:] == SENT).all() and (out[:4].abs() <= 1).all()
    with pytest.raises(ValueError):
        E.EsKernels(table, 4, 26, 6, lo, hi, hidden=(64, 64))
    with pytest.raises(ValueError):
        E.EsKernels(table[:20000], 4, 26, 6, lo, hi, hidden=WIDE)


@pytest.mark.parametrize("n_params", [19590, 20871])
def test_es_grad_at_the_wide_parameter_counts(n_params):
    """CassieEsGrad is the parent's kernel; nothing had run it at 77 - 82 workgroups per row."""
    import torch
    from cassierl_amd import es as E
    g = torch.Generator().manual_seed(n_params)
    table, tbuf = _table(g, 3 * 20871 + 1000)
    top = table.numel() - n_params
    t64 = table.double()
    for m in (1, 65, 4099):
        ek = E.EsKernels(table, 2 * m, 26, 6)
        off = _offsets(g, m, top)
        if m >= 2:
            off[0], off[-1] = 0, top
        off = off.to(DEV)
        ek.set_directions(off, n_params=n_params)
        rows = ek.fn["GradRows"](m)
        chunk = -(-m // rows)
        assert rows >= 1 and (rows - 1) * chunk < m
        # one-hot weights: the first and the last direction and both sides of every row boundary -> exactly w_d eps_d
        hot = sorted({0, m - 1} | {d for r in range(1, rows) for d in (r * chunk - 1, r * chunk) if d < m})
        eps = E.directions(table, off[hot], n_params)
        for j, d in enumerate(hot):
            w = torch.zeros(m)
            w[d] = -1.7 if j % 2 else 0.3
            got = ek.grad(w.to(DEV))
            assert got.shape == (n_params,) and torch.equal(got, w[d].item() * eps[j]), (m, d)
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
    assert torch.isnan(tbuf[:PAD]).all() and torch.isnan(tbuf[-PAD:]).all()


def _make(n, hidden=WIDE):
    from cassierl_amd import es as E
    from cassierl_amd.trajectory import default_gait
    return E.make_cassie_es(n, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, hidden_sizes=hidden, max_path_length=8, table_size=1 << 22)


def test_wide_fused_update_equals_the_torch_update_on_one_stand_rollout():
    import torch
    from cassierl_amd import trpo as T
    algo = _make(256)
    assert algo.n_params == 20742 and algo.hidden_sizes == WIDE
    algo.draw_directions()
    roll = algo.collect()
    assert algo.last_policy_step_kind == "es_wide_step" and algo.last_book_fused
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
    print("ES wide fused vs torch update: relative parameter difference %.3g, gradient norms %.6g / %.6g, step norms %.6g / %.6g" % (rel, gf, gt, sf, st))
    assert gt > 0 and st > 0 and abs(gf - gt) < 1e-5 * gt
    assert rel < 1e-5
    algo.env.close()
    narrow = _make(256, hidden=(32, 32))   # the same constructor at width 32 keeps its kernel
    narrow.draw_directions()
    narrow.collect()
    assert narrow.last_policy_step_kind == "es_step" and narrow.last_book_fused and narrow._kernels().ENTRY["PolicyStep"] == "CassieEsPolicyStep"
    narrow.env.close()


def test_wide_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    import torch
    from cassierl_amd import trpo as T
    a = _make(256)
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    assert torch.load(p, weights_only=True)["hidden_sizes"] == [128, 128] and os.path.getsize(p) < 4 * (1 << 22)   # no table in the snapshot
    ref = a.train_iteration()
    assert a.last_policy_step_kind == "es_wide_step" and a.last_grad_kind == "es_grad" and a.last_adam_fused and a.last_book_fused
    ta = T.flat_params(a.policy).clone()
    a.env.close()
    b = _make(256)
    _, restored = b.load(p)
    assert restored and b.adam_t == 2
    got = b.train_iteration()
    assert b.last_policy_step_kind == "es_wide_step" and b.last_grad_kind == "es_grad"
    assert got == ref and got["itr"] == 2
    assert torch.equal(T.flat_params(b.policy), ta)
    b.env.close()


KEYS = ["itr", "env_steps", "episodes", "avg_return", "max_return", "min_return", "avg_path_length", "grad_norm", "step_norm", "gathered"]


def test_train_es_and_sim_policy_scripts_at_width_128(tmp_path):
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_es.py"), "--hidden", "128,128", "--envs-per-gpu", "256", "--n-itr", "2", "--max-path-length", "8",
                        "--kind", "stand", "--control-mode", "Torque", "--table-size", str(1 << 22), "--snapshot", snap], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and os.path.exists(snap), p.stderr[-2000:]
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 2
    for i, r in enumerate(rows):
        assert all(k in r for k in KEYS), r
        assert r["itr"] == i and r["episodes"] == r["gathered"] == 256 and 256 <= r["env_steps"] <= 256 * 8
        assert r["policy_step"] == "es_wide_step" and r["grad"] == "es_grad"
        assert r["min_return"] <= r["avg_return"] <= r["max_return"] and 1 <= r["avg_path_length"] <= 8 and r["grad_norm"] > 0 and r["step_norm"] > 0
    q = subprocess.run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "256", "--max-path-length", "60", "--kind", "stand",
                        "--control-mode", "Torque"], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
    assert r["itr"] == 2 and r["envs"] == 256 and r["deterministic"] and 0 < r["avg_path_length"] <= 60 and np.isfinite(r["avg_return"])
