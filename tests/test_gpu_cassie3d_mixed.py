"""Cassie3d on the HIP path with DIFFERENT robots in one wavefront.  -m gpu only.

The lane-per-leg kernel (cassie3d_leg_core.h, cassie3d_leg.hip) runs 16 robots per wavefront (32 with CASSIE3D_LEG=64) and masks its
control flow per lane under wavefront-wide any() tests: the sweeping mask of the Gauss-Seidel loop, nlim > j, ncon > p, live, overflow.
tests/test_gpu_cassie3d.py compares batches of identical copies with the oracle and mixed batches with themselves; here the mixed pool of
tests/cassie3d_pool.py (standing, flying, dropped and lying robots, robots over a leg's slot budget or crossing the row capacity inside a
step, robots with joint-limit rows; interleaved) is
  A. compared robot by robot with each robot's own oracle, teacher-forced, in every kernel configuration,
  B. run in many placements (orders, prefixes that leave the last wavefront partly filled, 17 copies of one robot), which must all give
     every robot the same 80-double record, bit for bit, as the natural order,
  C. checked for complete clocks and for hand-overs that did happen.
tests/test_leg3d_mixed_cpu.py runs the same pool on the CPU build of the same source."""
import json
import os

import numpy as np
import pytest

import cassie3d_pool as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CONFIGS = {"leg16": {}, "leg32": {"CASSIE3D_LEG": "64"}, "wave": {"CASSIE3D_LEG": "0"}, "pair": {"CASSIE3D_PAIR": "1"}}
SWITCHES = ("CASSIE3D_LEG", "CASSIE3D_PAIR", "CASSIE3D_SEGMENTS")
N_SUB, STEPS = 10, 3
# test B: the leg configurations with the step in segments (the default) and in one launch, the wavefront-per-robot tiers as they are
B_CASES = [("leg16", None), ("leg16", "0"), ("leg32", None), ("leg32", "0"), ("wave", None)]
B_IDS = ["%s%s" % (c, "" if s is None else "-segments" + s) for c, s in B_CASES]


@pytest.fixture(scope="module")
def V3():
    from cassierl_amd import vec_env3d
    return vec_env3d


@pytest.fixture(scope="module")
def pool(oracle_mod):
    with open(os.path.join(ROOT, "tests", "golden", "model3d_kat.json")) as f:
        kat = json.load(f)
    oracle_mod.build3d()
    return P.make_pool(oracle_mod, kat, 0)


@pytest.fixture(scope="module")
def trajectory(pool):
    """computed once: it does not depend on the kernel"""
    return P.teacher_trajectory(pool)


@pytest.fixture(scope="module")
def natural_runs():
    """placement (a) per case of B, computed once and shared by B and C"""
    return {}


def make_env(V3, monkeypatch, n, config, segments=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    if segments is not None:
        monkeypatch.setenv("CASSIE3D_SEGMENTS", segments)
    return V3.Cassie3dVec(n)   # (the switches are read here)


def run(V3, monkeypatch, pool, idx, config, segments):
    """STEPS steps of N_SUB substeps through env.step of the robots idx under their own torques: the records after each step, the counters"""
    import torch
    env = make_env(V3, monkeypatch, len(idx), config, segments)
    env.set_state_host(pool.recs[idx])
    u = torch.as_tensor(np.ascontiguousarray(pool.torques[idx]), device="cuda")
    out = []
    for _ in range(STEPS):
        env.step(u, N_SUB)
        env.synchronize()
        out.append(env.get_state_host())
    c = env.counters()
    env.close()
    return out, c


def natural(V3, monkeypatch, pool, natural_runs, config, segments):
    key = (config, segments)
    if key not in natural_runs:
        natural_runs[key] = run(V3, monkeypatch, pool, np.arange(len(pool)), config, segments)
    return natural_runs[key]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_robot_of_a_mixed_batch_matches_its_own_oracle(V3, pool, trajectory, monkeypatch, config):
    """A. 30 teacher-forced substeps of the whole pool in one batch: every substep starts every robot from its own oracle's state and warm
    start, and every robot is compared with its own oracle -- tolerances of tests/test_gpu_cassie3d.py by the ORACLE's row count (up to 32
    rows: |dq| < 1e-9, |dv| / (1 + max |v|) < 1e-7; above: 1e-7 for both).  The row count in the record is the oracle's, nothing overflowed,
    and the leg configurations handed some substeps down and kept others."""
    tr = trajectory
    env = make_env(V3, monkeypatch, len(pool), config)
    env.reset_counters()
    worst, wq, wv = {}, 0.0, 0.0
    for t in range(len(tr.u)):
        env.set_state_host(tr.recs[t])
        env.step_host(tr.u[t], 1)
        s = env.get_state_host()
        dq, dv = P.errors(s, tr, t)
        bq, bv = P.bounds(tr.nefc[t])
        for k in range(len(pool)):
            w = worst.setdefault(pool.labels[k], [0.0, 0.0])
            w[0], w[1] = max(w[0], dq[k]), max(w[1], dv[k])
        assert np.isfinite(s).all(), (t, np.flatnonzero(~np.isfinite(s).all(axis=1)))
        bad = (dq >= bq) | (dv >= bv) | (s[:, 73] != tr.nefc[t]) | (s[:, 74] != 0.0)
        assert not bad.any(), (config, t, [(k, pool.labels[k], dq[k], dv[k], s[k, 73], tr.nefc[t, k], s[k, 74]) for k in np.flatnonzero(bad)])
        wq, wv = max(wq, dq.max()), max(wv, dv.max())
    c = env.counters()
    env.close()
    for lab, w in sorted(worst.items()):
        print("cassie3d[%s] mixed batch, %-8s worst |dq| %.2e  |dv|/(1+|v|) %.2e" % (config, lab, w[0], w[1]))
    print("cassie3d[%s] mixed batch, all kinds: worst |dq| %.3e  |dv|/(1+|v|) %.3e; counters %s" % (config, wq, wv, c))
    assert c["substeps"] == len(pool) * len(tr.u)
    if config.startswith("leg"):
        assert 0 < c["leg_handover_substeps"] < c["substeps"], c
    assert c["general_kernel_substeps"] > 0 and c["capped_substeps"] == 0, c


def same(ref, got, idx, what):
    for step, (s0, s1) in enumerate(zip(ref, got)):
        assert np.isfinite(s1).all(), (what, step)
        for i, k in enumerate(idx):
            if not np.array_equal(s1[i], s0[k]):
                d = np.flatnonzero(s1[i] != s0[k])
                raise AssertionError("%s: step %d, position %d = pool robot %d differs from the natural order in slots %s by up to %.3e" %
                                     (what, step, i, k, d[:8].tolist() + (["..."] if len(d) > 8 else []), np.abs(s1[i][d] - s0[k][d]).max()))


@pytest.mark.parametrize("config,segments", B_CASES, ids=B_IDS)
def test_results_do_not_depend_on_the_placement_in_the_batch(V3, pool, natural_runs, monkeypatch, config, segments):
    """B, placements (b) to (f): 3 steps of 10 substeps through env.step under fixed per-robot torques; every robot's whole record (state,
    warm start, ctrl, clock, niter, nefc, overflow) after each step equals, bit for bit, its record in the natural order -- sorted by kind
    (wavefronts as uniform as the pool allows), permuted, reversed, rotated so that a lying robot is robot 0 (idle and gone lanes alias
    record 0), that rotation with 47 robots, and prefixes that leave the last wavefront partly filled."""
    ref, _ = natural(V3, monkeypatch, pool, natural_runs, config, segments)
    assert pool.labels[P.placements(pool)["lying_first"][0]] == "lying"
    for name, idx in P.placements(pool).items():
        if name == "natural":
            continue
        got, _ = run(V3, monkeypatch, pool, idx, config, segments)
        same(ref, got, idx, "%s %s" % (B_IDS[B_CASES.index((config, segments))], name))


@pytest.mark.parametrize("config,segments", B_CASES, ids=B_IDS)
def test_seventeen_copies_of_a_robot_give_its_record_in_the_mixed_batch(V3, pool, natural_runs, monkeypatch, config, segments):
    """B, placement (g): for every robot k a batch of 17 copies (one full wavefront of 16 robots and one robot in the next): all 17
    records equal robot k's record in the natural order -- which ties the mixed result to the uniform regime that the oracle tests of
    tests/test_gpu_cassie3d.py pin."""
    ref, _ = natural(V3, monkeypatch, pool, natural_runs, config, segments)
    for k in range(len(pool)):
        idx = np.full(17, k)
        got, _ = run(V3, monkeypatch, pool, idx, config, segments)
        same(ref, got, idx, "%s 17 copies of robot %d (%s)" % (B_IDS[B_CASES.index((config, segments))], k, pool.labels[k]))


def test_sixteen_and_thirty_two_robots_per_wavefront_agree(V3, pool, natural_runs, monkeypatch):
    """leg16 against leg32 on the natural order: within the cross-kernel bound of tests/test_gpu_cassie3d.py (atol 1e-8 on q and v)."""
    a, _ = natural(V3, monkeypatch, pool, natural_runs, "leg16", None)
    b, _ = natural(V3, monkeypatch, pool, natural_runs, "leg32", None)
    print("cassie3d leg16 against leg32, natural order, %d steps: bit-equal records: %s; worst |difference| in q, v: %.3e" %
          (STEPS, all(np.array_equal(x, y) for x, y in zip(a, b)), max(np.abs(x[:, :41] - y[:, :41]).max() for x, y in zip(a, b))))
    for x, y in zip(a, b):
        np.testing.assert_allclose(y[:, :41], x[:, :41], rtol=0, atol=1e-8)


@pytest.mark.parametrize("config", ["leg16", "leg32", "wave"])
def test_clocks_and_counters_of_the_mixed_batch(V3, pool, natural_runs, monkeypatch, config):
    """C. after the natural-order run of B: every substep of every robot was done exactly once, robots did reach the general kernel, none
    the row cap; the leg configurations handed robots down and kept others."""
    s, c = natural(V3, monkeypatch, pool, natural_runs, config, None)
    print("cassie3d[%s] mixed batch, %d steps of %d substeps: counters %s" % (config, STEPS, N_SUB, c))
    assert np.abs(s[-1][:, 71] - STEPS * N_SUB * P.DT).max() < 1e-12
    assert (s[-1][:, 74] == 0.0).all()
    assert c["substeps"] == len(pool) * STEPS * N_SUB
    assert c["general_kernel_substeps"] > 0 and c["capped_substeps"] == 0, c
    if config.startswith("leg"):
        assert 0 < c["leg_handover_substeps"] < c["substeps"], c
