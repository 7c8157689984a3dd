"""The Cassie3d environment layer on the CPU: the PD mode of the lane-per-leg physics source (cassie3d_leg_core.h, Core3::env_step<true>)
under the lane emulation, and the environment arithmetic (cassie3d_env.h), both compiled by this test with g++ into a temporary directory
from the harnesses under tests/host/ and checked against the oracle (tests/cassie3d_env_ref.py).  The CPU twin of
tests/test_gpu_cassie3d_env.py: a failure there with this file green points at the device build or the launch code.  The CPU build has the
first tier only, so a robot over the row capacity of a leg (pending > 0) is checked to be left untouched and counted out; the GPU test
checks every robot."""
import ctypes as ct
import json
import os
import subprocess

import numpy as np
import pytest

import cassie3d_env_ref as R
import cassie3d_pool as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp, ip = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int)


@pytest.fixture(scope="module")
def pool(oracle_mod):
    with open(os.path.join(ROOT, "tests", "golden", "model3d_kat.json")) as f:
        return P.make_pool(oracle_mod, json.load(f), 0)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cassie3d_env_host"))
    pd = R.gxx(os.path.join(d, "libleg3d_pd_host.so"), "leg3d_pd_host.cpp", "-O2", "-fPIC", "-shared", "-DLEG_HOST_FAST", "-DLEG_HOST_LANES=4")
    env = R.gxx(os.path.join(d, "libcassie3d_env_host.so"), "cassie3d_env_host.cpp", "-O2", "-fPIC", "-shared")
    return dict(dir=d, pd=ct.CDLL(pd), env=ct.CDLL(env))


def pd_step(built, recs, targets, n_sub, kp=R.KP, kd=R.KD):
    s = np.ascontiguousarray(recs, dtype=np.float64).copy()
    n = len(s)
    t = np.ascontiguousarray(targets, dtype=np.float64)
    g = np.concatenate([kp, kd])
    pend, nrows = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    built["pd"].leg3d_pd_host_step(s.ctypes.data_as(dp), t.ctypes.data_as(dp), g.ctypes.data_as(dp), n, n_sub, pend.ctypes.data_as(ip),
                                   nrows.ctypes.data_as(ip))
    return s, pend, nrows


def env_finish(built, recs, actions):
    recs, actions = np.ascontiguousarray(recs, dtype=np.float64), np.ascontiguousarray(actions, dtype=np.float64)
    n = len(recs)
    obs, rew, done, guard = np.full((n, R.NOBS), 7.0), np.full(n, 7.0), np.full(n, 7.0), np.full(n, 7.0)
    built["env"].env3d_host_finish(recs.ctypes.data_as(dp), actions.ctypes.data_as(dp), n, obs.ctypes.data_as(dp), rew.ctypes.data_as(dp),
                                   done.ctypes.data_as(dp), guard.ctypes.data_as(dp))
    return obs, rew, done != 0, guard != 0


def test_pd_teacher_forced_matches_the_oracle(pool, built):
    """30 substeps, every one restarted from the oracle's state: the PD substep of the core against Oracle3D.step_torque(kp (t - q) - kd v)
    with the command computed from the oracle's own state, bounds of cassie3d_pool.bounds()."""
    targets = R.pd_targets(pool)
    tr = R.pd_teacher_trajectory(pool, targets)
    kept = np.zeros(len(pool), dtype=int)
    worst = [0.0, 0.0]
    for t in range(len(tr.u)):
        s, pend, nrows = pd_step(built, tr.recs[t], targets, 1)
        keep = pend == 0
        kept += keep
        assert np.isfinite(s).all()
        assert np.array_equal(s[~keep, :61], tr.recs[t][~keep, :61])     # over the capacity: left untouched for the next tier
        assert np.array_equal(nrows[keep], tr.nefc[t][keep])
        assert np.allclose(s[keep, 61:71], tr.u[t][keep], rtol=0, atol=1e-12)   # E3_CTRL: the command applied, pre-clamp
        dq, dv = P.errors(s, tr, t)
        bq, bv = P.bounds(tr.nefc[t])
        worst = [max(worst[0], dq[keep].max()), max(worst[1], dv[keep].max())]
        bad = keep & ((dq >= bq) | (dv >= bv))
        assert not bad.any(), (t, [(k, pool.labels[k], dq[k], dv[k], tr.nefc[t, k]) for k in np.flatnonzero(bad)])
    print("PD teacher-forced, CPU build: worst |dq| %.2e |dv|/(1+|v|) %.2e, robot-substeps kept %d of %d" % (worst[0], worst[1], kept.sum(), kept.size * len(tr.u)))
    assert (np.abs(tr.u) > P.CTRL).any() and (np.abs(tr.u) < P.CTRL).any()    # the clamp is exercised, and not everywhere
    assert kept.sum() > kept.size * len(tr.u) // 2


def test_pd_ten_substeps_in_one_call_apply_the_law_every_substep(pool, built):
    """Ten substeps in ONE call against ten oracle substeps with the command recomputed every substep (1e-5 relative, the free-run
    tolerance).  The oracle with the FIRST substep's command held is more than 1e-3 away in q on every robot counted, so a torque held
    over the call fails this test; a robot whose commands saturate with one sign throughout cannot tell and is left out."""
    targets = R.pd_targets(pool)
    ten = R.TenSubsteps(pool, targets)
    counted = ~ten.saturated
    print("held-command gap in q: min %.2e max %.2e; saturated throughout: %d of %d; actuator-substeps saturated %.2f" %
          (ten.held_gap[counted].min(), ten.held_gap[counted].max(), ten.saturated.sum(), len(pool), ten.saturated_frac.mean()))
    assert ten.saturated.sum() <= len(pool) // 4
    assert (ten.held_gap[counted] > 1e-3).all(), ten.held_gap
    s, pend, _ = pd_step(built, pool.recs, targets, 10)
    done = counted & (pend == 0)
    err = ten.rel_errors(s)
    print("PD, ten substeps in one call, CPU build: worst relative error %.2e over %d robots" % (err[done].max(), done.sum()))
    assert done.sum() >= len(pool) // 2
    assert (err[done] < 1e-5).all(), [(k, pool.labels[k], err[k]) for k in np.flatnonzero(done & (err >= 1e-5))]
    # per-actuator gains reach the right actuator: another gain on ONE actuator moves that hinge and matches the oracle run with it
    kp = R.KP.copy()
    kp[7] = 40.0
    k = pool.labels.index("air")
    o = pool.oracle_mod.Oracle3D()
    R.start(o, pool.recs[k])
    for _ in range(10):
        q, v = o.state()
        o.step_torque(R.pd_command(q, v, targets[k], kp=kp))
    q1, v1 = o.state()
    s2, pend2, _ = pd_step(built, pool.recs[k:k + 1], targets[k:k + 1], 10, kp=kp)
    assert pend2[0] == 0 and np.abs(s2[0, :21] - q1).max() < 1e-9 and np.abs(s2[0, :21] - s[k, :21]).max() > 1e-6


@pytest.fixture(scope="module")
def env_cases(pool):
    """pool states with the action rows of the PD targets, plus the same robots moved to heights around the done threshold"""
    recs = np.concatenate([pool.recs, pool.recs[:12]])
    recs[len(pool):, 2] = [0.4, 0.49, 0.499, 0.5 - 2e-6, 0.5 + 2e-6, 0.501, 0.51, 0.6, 0.9, 1.0, 0.3, 0.7]
    actions = np.concatenate([R.pd_targets(pool), pool.torques[:12]])
    return recs, actions


def test_env_arithmetic_matches_numpy_and_the_oracles_sites(pool, built, env_cases):
    recs, actions = env_cases
    o = pool.oracle_mod.Oracle3D()
    ref_obs, ref_rew, ref_done = R.reference(o, recs, actions)
    assert (np.abs(recs[:, 2] - 0.5) >= 1e-6).all() and ref_done.any() and not ref_done.all()
    obs, rew, done, guard = env_finish(built, recs, actions)
    assert not guard.any()
    assert np.array_equal(obs[:, R.COPIED], ref_obs[:, R.COPIED])          # copied from the record: exactly
    print("env arithmetic, CPU build: worst |d obs| %.2e |d reward| %.2e" % (np.abs(obs - ref_obs).max(), np.abs(rew - ref_rew).max()))
    assert np.abs(obs - ref_obs).max() <= 1e-11 and np.abs(rew - ref_rew).max() <= 1e-11
    assert np.array_equal(done, ref_done)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 1e11, -1e11])
def test_failure_guard_fires_on_a_single_bad_slot(pool, built, value):
    k = pool.labels.index("air")
    act = R.pd_targets(pool)[k:k + 1]
    for slot in (0, 2, 3, 7, 20, 21, 24, 27, 40):      # qpos and qvel: base position, quaternion, first and last hinge, rates
        rec = pool.recs[k:k + 1].copy()
        rec[0, slot] = value
        obs, rew, done, guard = env_finish(built, rec, act)
        assert guard[0] and done[0] and rew[0] == 0.0 and not obs.any(), (slot, value)
    for slot in (41, 60, 61, 70, 71, 75):              # warm start, ctrl, time, pad: not part of the guard
        rec = pool.recs[k:k + 1].copy()
        rec[0, slot] = value
        _, _, done, guard = env_finish(built, rec, act)
        assert not guard[0] and not done[0], (slot, value)
    rec = pool.recs[k:k + 1].copy()
    rec[0, 21] = 1e10                                   # the bound itself is inside
    assert not env_finish(built, rec, act)[3][0]


def test_env_arithmetic_under_address_and_undefined_sanitizers(pool, built, env_cases, tmp_path):
    """The same harness with its own main, instrumented (the sanitizer runtimes linked into the program itself), run as a program on a
    file of inputs (good states and guarded ones): clean exit and the library build's results."""
    exe = R.gxx(os.path.join(built["dir"], "cassie3d_env_host_san"), "cassie3d_env_host.cpp", "-O1", "-g", "-fsanitize=address,undefined",
                "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DENV3D_HOST_MAIN")
    recs, actions = (a.copy() for a in env_cases)
    recs[1, 5], recs[3, 30], recs[5, 0], recs[7, 22] = np.nan, np.inf, -1e11, -np.inf
    n = len(recs)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([[float(n)], recs.ravel(), actions.ravel()]).tofile(inp)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    got = np.fromfile(out)
    assert got.size == n * (R.NOBS + 3)
    obs, rew, done, guard = env_finish(built, recs, actions)
    assert np.array_equal(got[:n * R.NOBS].reshape(n, R.NOBS), obs) and np.array_equal(got[n * R.NOBS:n * R.NOBS + n], rew)
    assert np.array_equal(got[-2 * n:-n] != 0, done) and np.array_equal(got[-n:] != 0, guard)
    assert guard.sum() == 4 and guard[[1, 3, 5, 7]].all()
    # a truncated input is refused, not read past
    np.concatenate([[float(n)], recs.ravel()]).tofile(inp)
    assert subprocess.run([exe, inp, out], capture_output=True, text=True).returncode == 2
