"""The Cassie3d environment layer on the HIP path.  -m gpu only.

PD mode inside the physics tiers (the law applied at every substep, in the lane-per-leg kernel and in the wavefront-per-robot kernels that
finish a robot handed over mid-step), the finish kernel (observation, reward, done, failure guard, auto-reset from the reset record), the
masked reset and the error paths of include/cassie3d_vec.h -- on the mixed pool of tests/cassie3d_pool.py at batch sizes 1 (a lone robot),
17 (a partial wavefront), 48 (three wavefronts) and 257 (a block boundary of the finish kernel; pool robots repeated), against the oracle
and numpy (tests/cassie3d_env_ref.py).  tests/test_cassie3d_env_cpu.py checks the same sources on the CPU.  No test here feeds a NaN to the
GPU: the guard test uses a finite, too large velocity."""
import ctypes as ct
import json
import os

import numpy as np
import pytest

import cassie3d_env_ref as R
import cassie3d_pool as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = [1, 17, 48, 257]
# first tier: one lane per leg with 16 robots per wavefront, the same with 32 (CASSIE3D_LEG=64), the wavefront-per-robot kernels alone
TIERS = {"leg": {"CASSIE3D_LEG": "1"}, "leg32": {"CASSIE3D_LEG": "64"}, "wave": {"CASSIE3D_LEG": "0"}}
SWITCHES = ("CASSIE3D_LEG", "CASSIE3D_PAIR", "CASSIE3D_SEGMENTS")
EINVAL = -1


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
def targets(pool):
    return R.pd_targets(pool)


@pytest.fixture(scope="module")
def trajectory(pool, targets):
    """computed once: it does not depend on the kernel"""
    return R.pd_teacher_trajectory(pool, targets)


@pytest.fixture(scope="module")
def ten(pool, targets):
    return R.TenSubsteps(pool, targets)


def switches(monkeypatch, tier="leg", segments=None, pair=False):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in TIERS[tier].items():
        monkeypatch.setenv(k, v)
    if segments is not None:
        monkeypatch.setenv("CASSIE3D_SEGMENTS", segments)
    if pair:
        monkeypatch.setenv("CASSIE3D_PAIR", "1")


def make_env(V3, monkeypatch, n, tier="leg", segments=None, **kw):
    switches(monkeypatch, tier, segments)
    return V3.Cassie3dVecEnv(n, **kw)   # (the switches are read here)


def robots(n):
    return np.arange(n) % P.K


@pytest.fixture(scope="module")
def reset_record(V3):
    """what Cassie3dVecReset leaves on a fresh handle"""
    env = V3.Cassie3dVec(1)
    env.synchronize()
    rec = env.get_state_host()[0]
    env.close()
    return rec


# ------------------------------------------------------------------------------------------------ PD against the oracle
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tier", list(TIERS))
def test_pd_teacher_forced_matches_the_oracle(V3, pool, targets, trajectory, monkeypatch, tier, n):
    """30 PD substeps, each restarted from the oracle's state, every robot against Oracle3D.step_torque(kp (t - q) - kd v) with the command
    from the oracle's own state: cassie3d_pool.bounds() by the oracle's row count."""
    tr, idx = trajectory, robots(n)
    env = make_env(V3, monkeypatch, n, tier)
    wq = wv = 0.0
    for t in range(len(tr.u)):
        env.set_state_host(tr.recs[t][idx])
        env.substep_pd_host(targets[idx], 1)
        s = env.get_state_host()
        assert np.isfinite(s).all()
        dq = np.abs(s[:, :21] - tr.q1[t][idx]).max(axis=1)
        dv = np.abs(s[:, 21:41] - tr.v1[t][idx]).max(axis=1) / (1.0 + np.abs(tr.v1[t][idx]).max(axis=1))
        bq, bv = P.bounds(tr.nefc[t][idx])
        wq, wv = max(wq, dq.max()), max(wv, dv.max())
        bad = (dq >= bq) | (dv >= bv)
        assert not bad.any(), (t, [(i, pool.labels[idx[i]], dq[i], dv[i], tr.nefc[t, idx[i]]) for i in np.flatnonzero(bad)])
        assert np.array_equal(s[:, 73], tr.nefc[t][idx])
        assert np.abs(s[:, 61:71] - tr.u[t][idx]).max() < 1e-9        # E3_CTRL: the last command applied, whichever tier applied it
    print("PD teacher-forced, %s n=%d: worst |dq| %.2e |dv|/(1+|v|) %.2e" % (tier, n, wq, wv))
    env.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tier", list(TIERS))
def test_pd_ten_substeps_in_one_call_apply_the_law_every_substep(V3, pool, targets, ten, monkeypatch, tier, n):
    """Ten substeps in one call against ten oracle substeps with the command recomputed every substep: 1e-5 relative.  The oracle with the
    first substep's command held is more than 1e-3 away in q on every robot counted, so a held torque -- in the first tier or in a tier
    that finishes a robot handed over mid-step -- fails."""
    idx = robots(n)
    counted = ~ten.saturated
    assert ten.saturated.sum() <= P.K // 4 and (ten.held_gap[counted] > 1e-3).all()
    env = make_env(V3, monkeypatch, n, tier)
    env.set_state_host(pool.recs[idx])
    env.reset_counters()
    env.substep_pd_host(targets[idx], 10)
    s = env.get_state_host()
    c = env.counters()
    env.close()
    eq = np.abs(s[:, :21] - ten.q_pd[idx]).max(axis=1) / (1.0 + np.abs(ten.q_pd[idx]).max(axis=1))
    ev = np.abs(s[:, 21:41] - ten.v_pd[idx]).max(axis=1) / (1.0 + np.abs(ten.v_pd[idx]).max(axis=1))
    err = np.maximum(eq, ev)
    print("PD ten substeps, %s n=%d: worst relative error %.2e; hand-over substeps %d" % (tier, n, err[counted[idx]].max(), c["leg_handover_substeps"]))
    assert (err[counted[idx]] < 1e-5).all(), [(i, pool.labels[idx[i]], err[i]) for i in np.flatnonzero(err >= 1e-5)]
    if tier != "wave" and n >= 17:
        assert 0 < c["leg_handover_substeps"] < 10 * n      # robots finished by the lower tiers, some of them part-way through the step


@pytest.mark.parametrize("n", [48, 257])
def test_pd_step_in_segments_and_in_one_launch_agree_bit_for_bit(V3, pool, targets, monkeypatch, n):
    idx = robots(n)
    out = []
    for seg in ("0", "1"):
        env = make_env(V3, monkeypatch, n, "leg", seg)
        env.set_state_host(pool.recs[idx])
        env.substep_pd_host(targets[idx], 10)
        out.append(env.get_state_host())
        env.close()
    assert np.array_equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------ one EnvStep
def env_step_pair(V3, monkeypatch, pool, idx, mode, actions):
    """two handles from the same records, auto_reset 0 and 1: (obs, reward, done, records) of the first, (obs, reward, done, terminal_obs,
    records) of the second"""
    res = []
    for auto in (False, True):
        env = make_env(V3, monkeypatch, len(idx), control_mode=mode, auto_reset=auto)
        env.set_state_host(pool.recs[idx])
        r = env.step_host(actions, terminal_obs=auto)
        res.append(r + (env.get_state_host(), env.counters()))
        env.close()
    return res


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", ["PD", "Torque"])
def test_env_step_outputs_and_auto_reset(V3, pool, targets, reset_record, monkeypatch, mode, n):
    idx = robots(n)
    actions = (targets if mode == "PD" else pool.torques)[idx]
    (obs, rew, done, rec, c0), (obs1, rew1, done1, tobs1, rec1, c1) = env_step_pair(V3, monkeypatch, pool, idx, mode, actions)
    o = pool.oracle_mod.Oracle3D()
    assert np.isfinite(rec).all() and (np.abs(rec[:, 2] - 0.5) >= 1e-6).all()
    ref_obs, ref_rew, ref_done = R.reference(o, rec, actions)
    print("EnvStep %s n=%d: worst |d obs| %.2e |d reward| %.2e, done %d" % (mode, n, np.abs(obs - ref_obs).max(), np.abs(rew - ref_rew).max(), done.sum()))
    assert np.array_equal(obs[:, R.COPIED], ref_obs[:, R.COPIED])
    assert np.abs(obs - ref_obs).max() <= 1e-11 and np.abs(rew - ref_rew).max() <= 1e-11
    assert np.array_equal(done, ref_done)
    lab = np.array(pool.labels)[idx]
    assert done[np.isin(lab, ["lying", "low"])].all() and not done[np.isin(lab, ["stand", "air"])].any()
    if n >= 17:
        assert done[:16].any() and not done[:16].all()           # both kinds side by side in one wavefront
    # the second handle: same step, then the reset
    assert np.array_equal(done1, done) and np.array_equal(rew1, rew) and np.array_equal(tobs1, obs)
    assert np.array_equal(rec1[~done], rec[~done])
    assert np.array_equal(rec1[done], np.broadcast_to(reset_record, rec1[done].shape))
    assert np.array_equal(obs1[~done], obs[~done])
    if done.any():
        reset_obs = R.observation(o, reset_record)
        assert np.abs(obs1[done] - reset_obs).max() <= 1e-11 and np.array_equal(obs1[done][:, R.COPIED], np.broadcast_to(reset_obs[R.COPIED], (done.sum(), 39)))
    assert (c0["done"], c0["guard"]) == (done.sum(), 0) and (c1["done"], c1["guard"]) == (done.sum(), 0)
    if mode == "PD":
        # the physics of the step is the PD substeps of the contract, not a torque held over the step
        env = make_env(V3, monkeypatch, n)
        env.set_state_host(pool.recs[idx])
        env.substep_pd_host(actions, 10)
        assert np.array_equal(env.get_state_host(), rec)
        env.close()


def test_masked_reset_leaves_the_others_untouched(V3, pool, reset_record, monkeypatch):
    n = 257
    idx = robots(n)
    env = make_env(V3, monkeypatch, n)
    env.set_state_host(pool.recs[idx])
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    obs = env.reset_host(mask)
    rec = env.get_state_host()
    m = mask.astype(bool)
    assert np.array_equal(rec[~m], pool.recs[idx][~m])
    assert np.array_equal(rec[m], np.broadcast_to(reset_record, rec[m].shape))
    o = pool.oracle_mod.Oracle3D()
    ref = np.array([R.observation(o, r) for r in rec])
    assert np.array_equal(obs[:, R.COPIED], ref[:, R.COPIED]) and np.abs(obs - ref).max() <= 1e-11
    obs = env.reset_host()                                       # no mask: everyone
    assert np.array_equal(env.get_state_host(), np.broadcast_to(reset_record, rec.shape))
    assert np.abs(obs - R.observation(o, reset_record)).max() <= 1e-11
    env.close()


def test_failure_guard_on_a_finite_runaway_velocity(V3, pool, targets, reset_record, monkeypatch):
    """A flying robot with qvel[0] = 1e11 (finite): done, reward 0, the reset observation, counted once; its neighbours as without it."""
    n = P.K
    idx = robots(n)
    k = pool.labels.index("air")
    res = []
    for wild in (False, True):
        recs = pool.recs[idx].copy()
        if wild:
            recs[k, 21] = 1e11
        env = make_env(V3, monkeypatch, n, auto_reset=True)
        env.set_state_host(recs)
        obs, rew, done, tobs = env.step_host(targets[idx], terminal_obs=True)
        res.append((obs, rew, done, tobs, env.get_state_host(), env.counters()))
        env.close()
    (obs0, rew0, done0, tobs0, rec0, c0), (obs, rew, done, tobs, rec, c) = res
    assert not done0[k] and done[k] and rew[k] == 0.0 and not tobs[k].any()
    o = pool.oracle_mod.Oracle3D()
    assert np.abs(obs[k] - R.observation(o, reset_record)).max() <= 1e-11 and np.array_equal(rec[k], reset_record)
    assert (c0["done"], c0["guard"]) == (done0.sum(), 0) and (c["done"], c["guard"]) == (done0.sum() + 1, 1)
    others = np.arange(n) != k
    for a, b in ((obs0, obs), (rew0, rew), (done0, done), (tobs0, tobs), (rec0, rec)):
        assert np.array_equal(a[others], b[others])


# ------------------------------------------------------------------------------------------------ placement
@pytest.fixture(scope="module")
def natural_step():
    return {}


def placed_step(V3, monkeypatch, pool, targets, idx):
    env = make_env(V3, monkeypatch, len(idx), auto_reset=True)
    env.set_state_host(pool.recs[idx])
    out = env.step_host(targets[idx], terminal_obs=True) + (env.get_state_host(),)
    env.close()
    return out


@pytest.mark.parametrize("name", ["by_kind", "permuted", "reversed", "lying_first", "lying_first_47"] + ["prefix_%d" % m for m in (1, 15, 16, 17, 31, 32, 33, 47)])
def test_env_step_outputs_do_not_depend_on_the_placement(V3, pool, targets, natural_step, monkeypatch, name):
    if "nat" not in natural_step:
        natural_step["nat"] = placed_step(V3, monkeypatch, pool, targets, np.arange(P.K))
    idx = P.placements(pool)[name]
    for ref, got in zip(natural_step["nat"], placed_step(V3, monkeypatch, pool, targets, idx)):
        assert np.array_equal(got, ref[idx]), name


# ------------------------------------------------------------------------------------------------ errors
def test_error_paths(V3, monkeypatch):
    import torch
    from cassierl_amd import _lib
    switches(monkeypatch)
    env = V3.Cassie3dVec(3)
    L = env.L
    a = torch.zeros((3, 10), dtype=torch.float64, device="cuda")
    obs = torch.zeros((3, 45), dtype=torch.float64, device="cuda")
    rew = torch.zeros(3, dtype=torch.float64, device="cuda")
    done = torch.zeros(3, dtype=torch.uint8, device="cuda")
    step = lambda: L.Cassie3dVecEnvStep(env.h, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None)
    assert step() == EINVAL and b"Configure" in L.Cassie3dVecLastError(env.h)

    def cfg(mode=1, n_sub=10, auto=1, kp=10.0, kd=5.0):
        c = _lib.Cassie3dEnvConfig(mode, n_sub, auto)
        c.kp[:], c.kd[:] = [kp] * 10, [kd] * 10
        return L.Cassie3dVecEnvConfigure(env.h, ct.byref(c))
    assert cfg(mode=2) == EINVAL and cfg(mode=-1) == EINVAL
    assert cfg(n_sub=0) == EINVAL and cfg(n_sub=-3) == EINVAL
    assert cfg(kp=-1.0) == EINVAL and cfg(kd=-0.5) == EINVAL and cfg(auto=2) == EINVAL
    assert step() == EINVAL                                       # a refused configuration configures nothing
    assert L.Cassie3dVecEnvConfigure(env.h, None) == EINVAL
    assert cfg() == 0 and step() == 0
    env.synchronize()
    assert cfg() == EINVAL                                        # after the first EnvStep
    env.close()
    with pytest.raises(ValueError):
        V3.Cassie3dVecEnv(2, n_substeps=0)
    # the two-environments-per-wavefront cross-check kernel has no PD mode
    switches(monkeypatch, pair=True)
    monkeypatch.delenv("CASSIE3D_LEG", raising=False)
    with pytest.raises(ValueError, match="CASSIE3D_PAIR"):
        V3.Cassie3dVecEnv(2, control_mode="PD")
    env = V3.Cassie3dVecEnv(2, control_mode="Torque")
    assert env.L.Cassie3dVecSubstepPd(env.h, a.data_ptr(), 1) == EINVAL
    env.close()
