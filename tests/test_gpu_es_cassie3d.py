"""ES at Cassie3d's shape, 45 observations and 10 actions: the two policy steps of csrc/tu_es3d.hip (CassieEs3dPolicyStep, CassieEs3dWidePolicyStep)
against the float64 torch statement of cassierl_amd/es.py, the observation entries past the 32nd, the argument checks, CassieEsGrad at the two new
parameter counts, the loop on Cassie3dVecEnv (fused against torch update, resume, Torque mode), and train_es.py --env cassie3d / sim_policy.py.
-m gpu only.

The buffer layout, the shifted-bias method and the tolerance rule are tests/test_gpu_es.py's (its helpers are imported): the table is the middle of
a NaN buffer, obs and env_actions are the first n rows of longer buffers with NaN / a sentinel behind them, and every output is compared unclipped
in the launch whose shift of b3 brings it within 0.75 of 0.  The sizes n are those at which a kernel's grid changes (a lone pair, a short, a full
and a just over-full workgroup, several workgroups); how a pair's slice is staged or streamed does not depend on n."""
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
D, A = 45, 10
NARROW, WIDE = (32, 32), (128, 128)
COUNT = {NARROW: 2858, WIDE: 23690}
STEP = {NARROW: "CassieEs3dPolicyStep", WIDE: "CassieEs3dWidePolicyStep"}
KIND = {NARROW: "es3d_step", WIDE: "es3d_wide_step"}
SAT = 60.0   # the `saturated` regime: every second unit's row of W1, b1, W2, b2 times 60
IDS = ["32x32", "128x128"]


def _theta(g, hidden, regime):
    """tests/test_gpu_es.py's _theta at 45 x 10 and either width: Xavier-uniform + N(0, 0.1) jitter as the row [W1 | b1 | W2 | b2 | W3 | b3], then
    the regime."""
    import torch
    parts = []
    for i, (o, k) in enumerate(((hidden[0], D), (hidden[1], hidden[0]), (A, hidden[1]))):
        W = (torch.rand(o, k, generator=g) * 2 - 1) * math.sqrt(6.0 / (o + k)) + 0.1 * torch.randn(o, k, generator=g)
        b = 0.1 * torch.randn(o, generator=g)
        if regime == "saturated" and i < 2:
            W[0::2] *= SAT; b[0::2] *= SAT
        parts += [W.reshape(-1), b]
    return torch.cat(parts)


@pytest.mark.parametrize("regime", ["default", "saturated"])
@pytest.mark.parametrize("sigma", [0.0, 0.02, 1.0])
@pytest.mark.parametrize("hidden", [NARROW, WIDE], ids=IDS)
def test_es3d_policy_step_matches_the_torch_statement(hidden, sigma, regime):
    """Rule per case: `bound` = inside 5e-6 (1 + max|ref64|); `4x` = err_kernel <= 4 err_torch32 (tests/test_gpu_es.py's _check)."""
    import torch
    from cassierl_amd import es as E
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env3d import action_space
    g = torch.Generator().manual_seed(450000 + 1000 * hidden[0] + int(100 * sigma) + (7 if regime == "saturated" else 0))
    P = E.param_count(D, hidden, A)
    assert P == COUNT[hidden]
    table, tbuf = _table(g, 3 * P + 1000)
    theta = _theta(g, hidden, regime).to(DEV)
    assert theta.numel() == P
    box = action_space("PD")
    real = T.NormalizedActions(box.low, box.high, DEV)
    unit = T.NormalizedActions([-1.0] * A, [1.0] * A, DEV)
    ident = lambda a: a
    mid = real.low + (real.high - real.low) / 2
    ppw = E.EsKernels(table, 2, D, A, hidden=hidden).fn["PairsPerWorkgroup"]()
    assert ppw >= 2
    rules, widest = set(), 0
    for n in (2, 2 * ppw - 2, 2 * ppw, 2 * ppw + 2, 130):
        off = _offsets(g, n // 2, table.numel() - P).to(DEV)
        obs_buf = torch.full((n + 8, D), float("nan"), dtype=torch.float64)
        obs_buf[:n] = torch.randn(n, D, dtype=torch.float64, generator=g)
        if sigma == 0.0:
            obs_buf[1:n:2] = obs_buf[0:n:2]   # equal observations in a pair: equal bits below
        obs_buf = obs_buf.to(DEV)
        obs = obs_buf[:n]
        kw, kr = E.EsKernels(table, n, D, A, unit.low, unit.high, hidden=hidden), E.EsKernels(table, n, D, A, real.low, real.high, hidden=hidden)
        assert kw.P == P and kw.ENTRY["PolicyStep"] == STEP[hidden]
        kw.set_directions(off); kr.set_directions(off)
        # the float64 and float32 torch statements before the map, every environment alive, per shift c of the output bias
        m64 = E.es_actions_torch(theta.double(), table.double(), off, sigma, obs, None, ident, hidden)
        scale = 1.0 + m64.abs().max().item()
        top_c = int(math.ceil(m64.abs().max().item()))
        shifts, ref64, ref32, sel, seen = [], [], [], [], torch.zeros_like(m64, dtype=torch.bool)
        for c in range(-top_c, top_c + 1):
            th_c = theta.clone(); th_c[P - A:] += float(c)
            r64 = E.es_actions_torch(th_c.double(), table.double(), off, sigma, obs, None, ident, hidden)
            pick = (r64.abs() <= WINDOW) & ~seen
            if not bool(pick.any()):
                continue
            seen |= pick
            shifts.append((c, th_c)); sel.append(pick); ref64.append(r64 - c)
            ref32.append(E.es_actions_torch(th_c, table, off, sigma, obs.float(), None, ident, hidden).double() - c)
        assert bool(seen.all())   # every output is read from some launch, unclipped
        widest = max(widest, len(shifts))
        for name, alive in _alive_cases(n):
            alive = None if alive is None else alive.to(DEV)
            up = torch.ones(n, dtype=torch.bool, device=DEV) if alive is None else alive.bool()
            tag = "ES 45 x 10 policy step %s %s sigma %g n %d alive %s" % (regime, "x".join(map(str, hidden)), sigma, n, name)
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
                rules.add(_check(tag, got[live], want64[live], want32[live], 5e-6, scale))   # (prints the rule used)
                assert (want64[live] - m64[live]).abs().max().item() < 1e-5 * scale   # the shifted references are the unshifted action
            kw.policy_step(obs, theta, sigma, alive, out=env_w[:n])
            kr.policy_step(obs, theta, sigma, alive, out=env_r[:n])
            first = (env_w.clone(), env_r.clone())
            act = env_w[:n]
            assert (act[~up] == 0).all()   # the unit box: a dead row is exactly 0
            assert (env_r[:n] - real(act)).abs().max().item() < 1e-12
            assert (env_r[:n] >= real.low).all() and (env_r[:n] <= real.high).all() and (act.abs() <= 1).all()
            assert torch.equal(env_r[:n][~up], mid.expand(n, A)[~up])   # a dead environment: low + (high - low) / 2 exactly, Cassie3d's PD box
            assert (env_w[n:] == SENT).all() and (env_r[n:] == SENT).all()
            if sigma == 0.0:
                both = up[0::2] & up[1::2]
                assert torch.equal(env_w[0:n:2][both], env_w[1:n:2][both])
            kw.policy_step(obs, theta, sigma, alive, out=env_w[:n])
            kr.policy_step(obs, theta, sigma, alive, out=env_r[:n])
            assert torch.equal(env_w, first[0]) and torch.equal(env_r, first[1])   # two launches: equal bits
        assert torch.isnan(obs_buf[n:]).all()
    assert torch.isnan(tbuf[:PAD]).all() and torch.isnan(tbuf[-PAD:]).all()
    print("ES 45 x 10 policy step %s %r sigma %g: rules used %s, at most %d shifted launches per case" % (regime, hidden, sigma, sorted(rules), widest))


@pytest.mark.parametrize("hidden", [NARROW, WIDE], ids=IDS)
def test_observation_entries_past_the_32nd_count(hidden):
    """A lane of a half stages entries c and c + 32: changing entry 44 (and, apart, 32) of ONE environment changes that row of actions and no other."""
    import torch
    from cassierl_amd import es as E
    g = torch.Generator().manual_seed(4544 + hidden[0])
    P = COUNT[hidden]
    table = torch.randn(2 * P + 500, generator=g).to(DEV)
    theta = _theta(g, hidden, "default")
    theta[P - A * hidden[1] - A:] *= 0.05   # small outputs: nothing is clipped by the unit box
    theta = theta.to(DEV)
    lo, hi = torch.full((A,), -1.0, dtype=torch.float64, device=DEV), torch.full((A,), 1.0, dtype=torch.float64, device=DEV)
    ppw = E.EsKernels(table, 2, D, A, hidden=hidden).fn["PairsPerWorkgroup"]()
    n = 2 * ppw + 2
    ek = E.EsKernels(table, n, D, A, lo, hi, hidden=hidden)
    ek.set_directions(torch.randint(0, table.numel() - P + 1, (n // 2,), generator=g).to(DEV))
    obs = torch.randn(n, D, dtype=torch.float64, generator=g).to(DEV)
    base = ek.policy_step(obs, theta, 0.02).clone()
    assert (base.abs() < 1).all()
    for env, col in ((5, 44), (n - 2, 44), (0, 32), (3, 31)):
        o2 = obs.clone(); o2[env, col] += 0.5
        got = ek.policy_step(o2, theta, 0.02).clone()
        others = torch.ones(n, dtype=torch.bool, device=DEV); others[env] = False
        assert torch.equal(got[others], base[others]), (env, col)
        assert (got[env] != base[env]).all(), (env, col)   # (every output depends on every input through two dense layers)


@pytest.mark.parametrize("hidden", [NARROW, WIDE], ids=IDS)
def test_es3d_policy_step_refuses_bad_arguments(hidden):
    import ctypes as ct
    import torch
    from cassierl_amd import es as E
    P_ = COUNT[hidden]
    table = torch.randn(2 * P_ + 100).to(DEV)
    lo, hi = torch.full((A,), -1.0, dtype=torch.float64, device=DEV), torch.full((A,), 1.0, dtype=torch.float64, device=DEV)
    ek = E.EsKernels(table, 4, D, A, lo, hi, hidden=hidden)
    assert ek.P == P_
    ek.set_directions(torch.tensor([0, 5], device=DEV))
    obs, theta = torch.zeros(4, D, dtype=torch.float64, device=DEV), torch.zeros(ek.P, device=DEV)
    P = lambda t: ct.c_void_p(t.data_ptr())
    out = torch.full((5, A), SENT, dtype=torch.float64, device=DEV)
    good = [P(obs), 4, D, A, P(theta), P(table), ct.c_longlong(table.numel()), P(ek.offsets), ct.c_float(0.1), None, P(lo), P(hi), P(out), None]
    fn = ek.fn["PolicyStep"]

    def bads():
        for shape in ((26, 6), (45, 6), (44, 10)):
            bad = list(good); bad[2], bad[3] = shape
            yield shape, bad
        for k, v in ((1, 3), (1, 0), (1, -2), (6, ct.c_longlong(ek.P - 1)), (0, None), (4, None), (5, None), (7, None), (10, None), (11, None), (12, None)):
            bad = list(good); bad[k] = v
            yield k, bad
    for what, bad in bads():   # refused before anything has run: nothing is written
        assert fn(*bad) == -1, what
    torch.cuda.synchronize()
    assert (out == SENT).all()
    assert fn(*good) == 0
    for what, bad in bads():
        assert fn(*bad) == -1, what
    torch.cuda.synchronize()
    assert (out[4:] == SENT).all() and (out[:4].abs() <= 1).all()
    with pytest.raises(ValueError):
        E.EsKernels(table[:P_ - 1], 4, D, A, lo, hi, hidden=hidden)


@pytest.mark.parametrize("n_params", [2858, 23690])
def test_es_grad_at_the_45_by_10_parameter_counts(n_params):
    """CassieEsGrad is shape-free; the bound is tests/test_gpu_es.py's for it."""
    import torch
    from cassierl_amd import es as E
    g = torch.Generator().manual_seed(n_params)
    hidden = NARROW if n_params == COUNT[NARROW] else WIDE
    table, tbuf = _table(g, 3 * n_params + 1000)
    top = table.numel() - n_params
    t64 = table.double()
    for m in (1, 65, 257):
        ek = E.EsKernels(table, 2 * m, D, A, hidden=hidden)
        assert ek.P == n_params
        off = _offsets(g, m, top)
        if m >= 2:
            off[0], off[-1] = 0, top
        off = off.to(DEV)
        ek.set_directions(off)
        rows = ek.fn["GradRows"](m)
        chunk = -(-m // rows)
        assert rows >= 1 and (rows - 1) * chunk < m
        hot = sorted({0, m - 1} | {d for r in range(1, rows) for d in (r * chunk - 1, r * chunk) if d < m})
        eps = E.directions(table, off[hot], n_params)
        for j, d in enumerate(hot):   # one-hot weights -> exactly w_d eps_d
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
    assert torch.isnan(tbuf[:PAD]).all() and torch.isnan(tbuf[-PAD:]).all()


# ------------------------------------------------------------------------------------------------------------------ the loop on Cassie3dVecEnv
def _make(n, hidden, control_mode="PD", **kw):
    from cassierl_amd import es as E
    return E.make_cassie_es(n, env="cassie3d", control_mode=control_mode, seed=1, hidden_sizes=hidden, max_path_length=8, table_size=1 << 22, **kw)


@pytest.mark.parametrize("hidden", [NARROW, WIDE], ids=IDS)
def test_fused_update_equals_the_torch_update_on_one_cassie3d_rollout(hidden):
    """tests/test_gpu_es.py's test_fused_update_equals_the_torch_update_on_one_stand_rollout on Cassie3d: one fitness vector, both updates from the
    same parameters."""
    import torch
    from cassierl_amd import trpo as T
    algo = _make(256, hidden)
    assert algo.n_params == COUNT[hidden] and algo.obs_dim == D and algo.env_family == "cassie3d"
    algo.draw_directions()
    roll = algo.collect()
    assert algo.last_policy_step_kind == KIND[hidden] and algo.last_book_fused and algo._kernels().ENTRY["PolicyStep"] == STEP[hidden]
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
    print("ES on Cassie3d %r fused vs torch update: relative parameter difference %.3g, gradient norms %.6g / %.6g, step norms %.6g / %.6g"
          % (hidden, rel, gf, gt, sf, st))
    assert gt > 0 and st > 0 and abs(gf - gt) < 1e-5 * gt
    assert rel < 1e-5
    algo.env.close()


@pytest.mark.parametrize("hidden", [NARROW, WIDE], ids=IDS)
def test_cassie3d_resume_equals_the_uninterrupted_run(hidden, tmp_path):
    import torch
    from cassierl_amd import trpo as T
    a = _make(256, hidden)
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ck = torch.load(p, weights_only=True)
    assert ck["algo"] == "es" and ck["env_family"] == "cassie3d" and ck["env_config"] == dict(control_mode="PD", kp=[10.0] * 10, kd=[5.0] * 10)
    assert ck["hidden_sizes"] == list(hidden) and os.path.getsize(p) < 4 * (1 << 22)   # no table in the snapshot
    ref = a.train_iteration()
    assert a.last_policy_step_kind == KIND[hidden] and a.last_grad_kind == "es_grad" and a.last_adam_fused and a.last_book_fused
    ta = T.flat_params(a.policy).clone()
    a.env.close()
    b = _make(256, hidden)
    _, restored = b.load(p)
    assert restored and b.adam_t == 2
    got = b.train_iteration()
    assert b.last_policy_step_kind == KIND[hidden] and b.last_grad_kind == "es_grad"
    assert got == ref and got["itr"] == 2
    assert torch.equal(T.flat_params(b.policy), ta)
    b.env.close()
    other = _make(64, hidden, kp=20.0)
    with pytest.raises(ValueError, match="configured with"):
        other.load(p)
    other.env.close()


def test_torque_mode_takes_an_iteration():
    a = _make(64, NARROW, control_mode="Torque")
    st = a.train_iteration()
    assert a.last_policy_step_kind == "es3d_step" and a.last_book_fused and a.env_config["control_mode"] == "Torque"
    assert st["episodes"] == 64 and 64 <= st["env_steps"] <= 64 * 8 and np.isfinite(st["avg_return"]) and st["grad_norm"] > 0 and st["step_norm"] > 0
    a.env.close()


# ------------------------------------------------------------------------------------------------------------------ scripts
KEYS = ["itr", "env_steps", "episodes", "avg_return", "max_return", "min_return", "avg_path_length", "grad_norm", "step_norm", "gathered"]


@pytest.mark.parametrize("hidden", [NARROW, WIDE], ids=IDS)
def test_train_es_on_cassie3d_and_its_snapshot(hidden, tmp_path):
    """train_es.py --env cassie3d for two short iterations at 256 environments with gains of its own; sim_policy.py takes the family, the control
    mode and the gains from the snapshot (load() refuses any other configuration, so its success says they are the snapshot's)."""
    import torch
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_es.py"), "--env", "cassie3d", "--hidden", "%d,%d" % hidden, "--envs-per-gpu", "256", "--n-itr", "2",
                        "--max-path-length", "8", "--kp", "12", "--kd", "4", "--table-size", str(1 << 22), "--snapshot", snap], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and os.path.exists(snap), p.stderr[-2000:]
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 2
    for i, r in enumerate(rows):
        assert all(k in r for k in KEYS), r
        assert r["itr"] == i and r["episodes"] == r["gathered"] == 256 and 256 <= r["env_steps"] <= 256 * 8
        assert r["policy_step"] == KIND[hidden] and r["grad"] == "es_grad"
        assert r["min_return"] <= r["avg_return"] <= r["max_return"] and 1 <= r["avg_path_length"] <= 8 and r["grad_norm"] > 0 and r["step_norm"] > 0
    ck = torch.load(snap, weights_only=True)
    assert ck["env_family"] == "cassie3d" and ck["env_config"] == dict(control_mode="PD", kp=[12.0] * 10, kd=[4.0] * 10)
    q = subprocess.run([sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "128", "--max-path-length", "30"], capture_output=True, text=True,
                       timeout=600)
    assert q.returncode == 0, q.stderr[-2000:]
    r = json.loads([l for l in q.stdout.splitlines() if l.startswith("{")][-1])
    assert r["itr"] == 2 and r["envs"] == 128 and r["deterministic"] and 0 < r["avg_path_length"] <= 30 and np.isfinite(r["avg_return"])
