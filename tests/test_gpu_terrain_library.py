"""N4 at scale: a LIBRARY of height fields with a field id per environment (CassieVecSetTerrainLibrary / CassieVecSetTerrainIds).
The invariant: an environment on field k computes, bit for bit, what it computes in a batch with CassieVecSetHeightField(field k) --
in every kernel tier, through auto-reset and hand-over -- and matches the oracle on that field.  -m gpu only."""
import glob
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, state_vec
from cassierl_amd import terrain as T

pytestmark = pytest.mark.gpu

TQ = np.array([12.0, 12.0, 0.9] * 2)
PD_LO, PD_HI = np.radians([-50, -164, -140] * 2), np.radians([80, -37, -30] * 2)


def _relief(amp=0.015, wavelength=1.5, phase=0.0, ncol=2001):
    xs = np.linspace(-10.0, 10.0, ncol)
    return np.tile(amp * (1.0 - np.cos(2.0 * np.pi * xs / wavelength + phase)), (64, 1))


@pytest.fixture(scope="module")
def fields():
    """K = 4 fields of different shapes: the ramp, the ramp reversed, the 3 cm rolling relief, the golden PNG shifted below the spawn."""
    ramp = T.ramp(nrow=64, ncol=2001, size_x=10.0, slope=0.1, x0=0.5)
    gray = np.load(os.path.join(GOLDEN, "terrain_png.npz"))["gray"].astype(np.float64)
    png = T.clear_spawn(T.hfield_from_gray(gray, (10, 10, 0.2, 0.001)))
    return [ramp, np.ascontiguousarray(ramp[:, ::-1]), _relief(), png]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _wave_flags():
    from cassierl_amd.vec_env import WAVE_PER_ENV
    return WAVE_PER_ENV


def _library_vs_single_fields(make, fields, mode, n=256, steps=20, seed=7, pre=120):
    """One batch on the library (mixed ids) against one batch per field, same initial states and actions, auto-reset on.  The initial
    states are those of `pre` Env.steps on the library (robots under random torques are falling by then: the compared steps see resets)."""
    import torch
    from cassierl_amd import rollout as R
    from cassierl_amd.vec_env import action_space
    k = len(fields)
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.arange(n) % k).astype(np.int32)
    lib = make(n, kind="stand", control_mode=mode, n_substeps=10, auto_reset=True)
    lib.set_terrain_library(fields, (10.0, 10.0))
    lib.set_terrain_ids(torch.from_numpy(ids).cuda())
    assert np.array_equal(lib.terrain_ids().cpu().numpy(), ids)
    lout = lib.alloc()
    lib.reset(lout)
    box = action_space(mode)
    env_ids = torch.arange(n, device="cuda")

    def act(t):
        return R.random_actions(seed, env_ids, t, box.low, box.high) if mode == "PD" else R.random_actions(seed, env_ids, t, -TQ, TQ)
    for t in range(pre):
        lib.step(act(t), lout)
    s0 = lib.get_full_state_host()
    refs = []
    for f in fields:
        e = make(n, kind="stand", control_mode=mode, n_substeps=10, auto_reset=True)
        e.set_heightfield(f, 10.0, 10.0)
        e.set_full_state_host(s0)
        refs.append((e, e.alloc()))
    dones = 0
    for t in range(pre, pre + steps):
        a = act(t)
        lib.step(a, lout)
        for e, out in refs:
            e.step(a, out)
        torch.cuda.synchronize()
        s = lib.get_full_state_host()
        for j, (e, out) in enumerate(refs):
            m = ids == j
            sr = e.get_full_state_host()
            assert np.array_equal(bits(s[m]), bits(sr[m])), (t, j)
            for key in ("obs", "reward", "done"):
                x, y = lout[key].cpu().numpy()[m], out[key].cpu().numpy()[m]
                assert np.array_equal(bits(x) if key != "done" else x, bits(y) if key != "done" else y), (t, j, key)
        dones += int(lout["done"].sum())
    assert np.isfinite(lib.get_full_state_host()).all()
    for e, _ in refs:
        e.close()
    lib.close()
    return dones


@pytest.mark.parametrize("mode", ["PD", "Torque"])
def test_library_bit_identical_to_single_fields_per_tier(vec_tier, fields, mode):
    """256 environments on four fields (mixed ids), 20 Env.steps with auto-reset: every environment's state, observation, reward and
    done equal, bit for bit, a batch that holds only its field -- for each first tier (four per wavefront, two lanes, 64 per wavefront)."""
    dones = _library_vs_single_fields(vec_tier, fields, mode)
    if mode == "Torque":
        assert dones > 0   # random torques topple robots: the auto-reset path ran on the library too


@pytest.mark.parametrize("mode", ["PD", "Torque"])
def test_library_bit_identical_to_single_fields_wave_per_env(fields, mode):
    from cassierl_amd.vec_env import CassieVecEnv

    def make(*a, **k):
        return CassieVecEnv(*a, flags=_wave_flags(), **k)
    _library_vs_single_fields(make, fields, mode)


def _tier_flags(t):
    from cassierl_amd.vec_env import WAVE_PER_ENV, LEG_TIER_ON, DUO_TIER_ON, DUO_TIER_OFF
    return {False: 0, True: WAVE_PER_ENV, "leg": LEG_TIER_ON | DUO_TIER_OFF, "duo": LEG_TIER_ON | DUO_TIER_ON}[t]


@pytest.mark.parametrize("tier", [False, True, "leg", "duo"])
@pytest.mark.parametrize("mode", ["Torque", "PD"])
def test_library_teacher_forced_against_the_oracle(oracle_mod, fields, mode, tier):
    """Eight robots over the four fields, one oracle per robot holding that robot's field; 150 teacher-forced substeps (tolerance of
    test_gpu_terrain.py::test_ramp_teacher_forced_substeps)."""
    from cassierl_amd.vec_env import CassieVecEnv
    place = [(0, 1.0, 0.05), (0, -1.0, 0.0), (1, -1.0, 0.05), (1, 1.0, 0.0), (2, 0.0, 0.012), (2, 0.75, 0.03), (3, 0.0, 0.0), (3, 1.7, None)]
    os_, ids = [], []
    for k, dx, dz in place:
        hm = fields[k]
        if dz is None:
            dz = T.height_at(hm, 10, 10, dx, 0.0) - T.height_at(hm, 10, 10, 0.0, 0.0) + 0.03
        o = oracle_mod.Oracle()
        o.set_hfield(hm, 10.0, 10.0)
        q, v = o.state()
        q[0] += dx; q[1] += dz
        o.set_state_raw(q, v, np.zeros(13))
        os_.append(o)
        ids.append(k)
    import torch
    n = len(os_)
    env = CassieVecEnv(n, kind="stand", control_mode=mode, n_substeps=1, auto_reset=False, flags=_tier_flags(tier))
    env.set_terrain_library(fields, (10.0, 10.0))
    env.set_terrain_ids(torch.tensor(ids, dtype=torch.int32, device="cuda"))
    rng = np.random.default_rng(21)
    worst, contacts = 0.0, 0
    for t in range(150):
        if t % 10 == 0:
            a = rng.uniform(-1, 1, (n, 6)) * TQ if mode == "Torque" else rng.uniform(PD_LO, PD_HI, (n, 6))
        env.set_full_state_host(np.array([state_vec(*o.state(), o.warmstart()) for o in os_]))
        env.substep_host(mode, a, 1)
        sg = env.get_full_state_host()
        for i, o in enumerate(os_):
            (o.step_torque if mode == "Torque" else o.step_pd)(a[i])
            q1, v1 = o.state()
            worst = max(worst, np.abs(sg[i, :13] - q1).max(), np.abs(sg[i, 13:26] - v1).max() / (1 + np.abs(v1).max()))
            contacts += o.ncon > 0
    assert worst < 1e-9, worst
    assert contacts > 300
    env.close()


def test_reassignment_under_a_mask_and_range_errors(fields):
    """Ids changed under a mask between Env.steps give the bits of a fresh single-field run from the same state; an out-of-range id
    raises and leaves the assignment untouched (unselected entries are not checked)."""
    import torch
    from cassierl_amd import rollout as R
    from cassierl_amd.vec_env import CassieVecEnv, action_space
    n, k = 128, len(fields)
    ids = torch.arange(n, dtype=torch.int32, device="cuda") % k
    lib = CassieVecEnv(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True)
    lib.set_terrain_library(fields)
    assert int(lib.terrain_ids().abs().sum()) == 0           # a new library puts everybody on field 0
    lib.set_terrain_ids(ids)
    out = lib.alloc()
    lib.reset(out)
    box = action_space("PD")
    env_ids = torch.arange(n, device="cuda")
    for t in range(3):
        lib.step(R.random_actions(3, env_ids, t, box.low, box.high), out)
    mask = (env_ids % 3 == 0)
    new = ((ids + 1) % k).to(torch.int32)
    lib.set_terrain_ids(new, mask=mask)
    want = torch.where(mask, new, ids)
    assert torch.equal(lib.terrain_ids(), want)
    # out of range (too large, negative) under the mask: refused, nothing changes
    for badv in (k, -1):
        bad = want.clone()
        bad[5] = badv
        with pytest.raises(RuntimeError):
            lib.set_terrain_ids(bad, mask=torch.ones(n, dtype=torch.bool, device="cuda"))
        assert torch.equal(lib.terrain_ids(), want)
    # an out-of-range value where the mask does not select is never read
    bad = want.clone()
    bad[1] = k + 7
    sel = torch.zeros(n, dtype=torch.bool, device="cuda"); sel[0] = True
    lib.set_terrain_ids(bad, mask=sel)
    assert torch.equal(lib.terrain_ids(), want)
    with pytest.raises(ValueError):
        lib.set_terrain_ids(want.to(torch.int64))
    s = lib.get_full_state_host()
    wn = want.cpu().numpy()
    refs = []
    for f in fields:
        e = CassieVecEnv(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True)
        e.set_heightfield(f)
        e.set_full_state_host(s)
        refs.append((e, e.alloc()))
    for t in range(3, 8):
        a = R.random_actions(3, env_ids, t, box.low, box.high)
        lib.step(a, out)
        for e, o in refs:
            e.step(a, o)
    sl = lib.get_full_state_host()
    for j, (e, o) in enumerate(refs):
        m = wn == j
        assert np.array_equal(bits(sl[m]), bits(e.get_full_state_host()[m])), j
        assert np.array_equal(bits(out["obs"].cpu().numpy()[m]), bits(o["obs"].cpu().numpy()[m])), j
        e.close()
    # back to the flat floor and to a library of one
    lib.set_terrain_library([])
    assert int(lib.terrain_ids().abs().sum()) == 0
    with pytest.raises(RuntimeError):
        lib.set_terrain_ids(want)
    lib.close()


def test_sixteen_fields_at_size_split_between_the_first_tier_kernels():
    """98 304 robots (the size rule splits them: whole rounds in the 64-environments kernel, the rest in the two-lanes kernel) on 16
    reliefs, random PD, 25 Env.steps with auto-reset: everything finite, and sampled environments of both halves bit-identical to
    batches that hold only their field."""
    import torch
    from cassierl_amd import rollout as R
    from cassierl_amd.vec_env import CassieVecEnv, action_space
    n, k = 98304, 16
    fl = [T.clear_spawn(_relief(amp=0.004 + 0.0008 * j, wavelength=0.8 + 0.1 * j, phase=0.4 * j)) for j in range(k)]
    env_ids = torch.arange(n, device="cuda")
    ids = T.assign_terrains(5, env_ids, k).cuda()
    lib = CassieVecEnv(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True)
    nd = lib.tier_info()["duo_envs"]
    assert 0 < nd < n, nd
    lib.set_terrain_library(fl)
    lib.set_terrain_ids(ids)
    out = lib.alloc()
    lib.reset(out)
    s0 = lib.get_full_state_host()
    box = action_space("PD")
    acts = [R.random_actions(9, env_ids, t, box.low, box.high) for t in range(25)]
    for a in acts:
        lib.step(a, out)
        assert np.isfinite(out["obs"].cpu().numpy()).all()
    s = lib.get_full_state_host()
    assert np.isfinite(s).all()
    assert lib.counters()["nonfinite_resets"] == 0
    idn = ids.cpu().numpy()
    rng = np.random.default_rng(0)
    sample = np.concatenate([rng.choice(nd, 48, replace=False), nd + rng.choice(n - nd, 48, replace=False)])
    for j in sorted(set(idn[sample].tolist()))[:4]:
        e = CassieVecEnv(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True)
        assert e.tier_info()["duo_envs"] == nd
        e.set_heightfield(fl[j])
        e.set_full_state_host(s0)
        eo = e.alloc()
        for a in acts:
            e.step(a, eo)
        m = sample[idn[sample] == j]
        assert len(m)
        assert np.array_equal(bits(s[m]), bits(e.get_full_state_host()[m])), j
        e.close()
    lib.close()


def test_trpo_on_a_terrain_library_snapshot_resume(tmp_path):
    """Two TRPO iterations on a three-field library: a snapshot after the first and a resumed second iteration reproduce the
    uninterrupted run; a job on other ground refuses the snapshot."""
    import torch
    from cassierl_amd.trajectory import default_gait
    from cassierl_amd.trpo import make_cassie_trpo, flat_params
    tdir = tmp_path / "terrains"
    tdir.mkdir()
    for i in range(3):
        shutil.copy(sorted(glob.glob(os.path.join(GOLDEN, "*.png")))[0], str(tdir / ("t%d.png" % i)))
    spec = T.terrain_spec(str(tdir), 3, 0.05, 4)
    n = 512

    def job(sp):
        return make_cassie_trpo(n, kind="stand", control_mode="PD", trajectory=default_gait(), seed=1, batch_size=n * 4, terrain=sp)
    a = job(spec)
    ids = a.env.terrain_ids()
    assert torch.equal(ids.cpu(), T.assign_terrains(4, torch.arange(n), 3))
    snap = str(tmp_path / "snap.pt")
    st1 = a.train_iteration()
    a.save(snap)
    st2 = a.train_iteration()
    theta = flat_params(a.policy).clone()
    a.env.close()
    b = job(spec)
    _, restored = b.load(snap)
    assert restored
    st2b = b.train_iteration()
    assert torch.equal(flat_params(b.policy), theta)
    for key in ("avg_reward", "avg_return", "episodes", "kl", "loss_before", "loss_after"):
        if key in st2:
            assert np.array_equal(st2[key], st2b[key], equal_nan=True), key   # (avg_return is nan while no path has ended)
    assert np.isfinite(st1["avg_reward"])
    b.env.close()
    other = job(dict(spec, elevation=0.06))
    with pytest.raises(ValueError):
        other.load(snap)
    other.env.close()
    flat = job(None)
    with pytest.raises(ValueError):
        flat.load(snap)
    flat.env.close()
