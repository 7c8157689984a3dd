"""The direct path of the 64-environments-per-wavefront Env.step (cassierl_amd/csrc/cassie_duo_core.h, env_step2: when group B's set-up ends in its
six-row tail and group A is not in the eight-row format, B's rows go from the set-up's registers straight into the joint sweep, without the round trip
through the workspace) on the CPU, through oracle/leg_host as tests/test_duo_host.py does: the 64-env form against the two-lanes form, BIT FOR BIT --
state records, observation, reward, done flag, hand-over counts.

The emulation's lane count decides the group size (G = lanes / 2 environments per group, one call group = G environments of group A and the next G of
group B); the batch sizes and the odd environments' indices of tests/test_gpu_duo_direct_rows.py (group size 32) are scaled to it.  The emulated
workspace starts as NaN in every call, so a read of a row slot of group B that nobody wrote (the stand-alone block or widen_rows taken where B's rows
were never stored) shows as a difference.  One regime per branch of a pass:

  (a) direct path in every substep and in the reset pass: walk/PD, auto-reset, random targets; B with one environment, a full call group, two
  (b) B absent: the stand-alone block with idle rows for B (A alone; and a last call group with A alone behind full ones)
  (c) A eight-row (one environment of A with a knee past its joint limit), B six-row: B stores its rows and is widened
  (d) B eight-row, A six-row: rows_general, A widened
  (e) both eight-row
  (f) reset pass with one group only: stand/PD, auto-reset, one environment's pelvis below the termination height -- of group A (stand-alone block,
      idle B), of group B (direct path with idle rows for A).  The pelvis is lowered by 0.5 m (record word 1 and its snapshot copy, word 40) AND
      pitched by 1.5 rad (word 2 and its copy, word 41): lowered alone, the feet start half a metre under the floor, the environment is over eight
      rows per leg in its first substep and leaves the tier (pending = 10) -- a lower tier would reset it and this kernel's reset pass would not run.
      Pitched, the legs lie level above the floor, the environment stays in the tier for the ten substeps and is reset by it.
  (h) the height-field instantiation: (a) and (c) on the relief of tests/test_gpu_step_io.py.  The emulation's height-field entry takes no reference
      gait, so (a) runs the stand env there, and one environment of B starts below the termination height so that the reset pass (on terrain: with its
      own outputs call) is part of it.
"""
import numpy as np
import pytest

from conftest import state_vec
from leg_host import LegHostEnv, lib

PD_LO, PD_HI = np.radians([-50, -164, -140] * 2), np.radians([80, -37, -30] * 2)
KEEP = np.r_[0:39, 65:88]   # a handed-over environment: everything but the setState snapshot (tests/test_duo_host.py says why)


def _g():
    return lib().leg_host_lanes() // 2


def _odd(group):
    """The odd environment of a group of the first call group: what environment 5 (group A) / 40 (group B) is at group size 32."""
    g = _g()
    return (g if group else 0) + min(5 if group == 0 else 8, g - 1)


def _same(a, b, what):
    assert np.array_equal(a, b, equal_nan=True), (what, np.argwhere(np.asarray(a) != np.asarray(b))[:5])


def _relief(e):
    xs = np.linspace(-10.0, 10.0, 2001)
    e.set_heightfield(np.tile(0.015 * (1.0 - np.cos(2.0 * np.pi * xs / 1.5)), (64, 1)), 10.0, 10.0)


def _start(oracle_mod, n, hf=False):
    o = oracle_mod.Oracle()
    q, v = o.state()
    s0 = np.tile(state_vec(q, v, np.zeros(13) if hf else o.warmstart(), qstate=q), (n, 1))
    if hf:
        s0[:, 0] += np.linspace(-3.0, 3.0, n)
        s0[:, 1] += 0.03
        s0[:, 39:41] = s0[:, 0:2]
    return s0


def _sink(s0, e):
    """Environment e below the stand env's termination height (0.5 m) with nothing under the floor: regime (f) of the module's docstring."""
    s0[e, 1] -= 0.5; s0[e, 40] -= 0.5
    s0[e, 2] += 1.5; s0[e, 41] += 1.5


def _rollout(pair, duo, s0, actions):
    """Both forms from s0 through `actions` (one array per step); every output compared after every step.  Returns the done flags per step."""
    for e in (pair, duo):
        e.set_full_state_host(s0)
    dones = []
    for t, a in enumerate(actions):
        rp, rd = pair.step_host(a), duo.step_host(a)
        dones.append(rd[2].copy())
        _same(pair.pending, duo.pending, (t, "pending"))
        stay = pair.pending == 0
        for x, y, w in zip(rp, rd, ("obs", "reward", "done")):
            _same(x[stay], y[stay], (t, w))
        sp, sd = pair.get_full_state_host(), duo.get_full_state_host()
        _same(sp[stay], sd[stay], (t, "state"))
        _same(sp[~stay][:, KEEP], sd[~stay][:, KEEP], (t, "state of the handed-over environments, snapshot aside"))
        assert pair.nonfinite == duo.nonfinite, t
        if (~stay).any():   # on the GPU the lower tiers finish them; here: back to the start
            sp[~stay] = s0[~stay]
            pair.set_full_state_host(sp); duo.set_full_state_host(sp)
    return dones


def _pair_and_duo(n, **kw):
    return LegHostEnv(n, **kw), LegHostEnv(n, duo=True, **kw)


# (a) n = G + 1, 2 G, 4 G;  (b) n = G - 1 (if any), G, 2 G + 1, 3 G
@pytest.mark.parametrize("size", ["a:G+1", "a:2G", "a:4G", "b:G-1", "b:G", "b:2G+1", "b:3G"])
def test_walk_pd_with_resets(oracle_mod, traj, size):
    g = _g()
    n = {"a:G+1": g + 1, "a:2G": 2 * g, "a:4G": 4 * g, "b:G-1": max(1, g - 1), "b:G": g, "b:2G+1": 2 * g + 1, "b:3G": 3 * g}[size]
    rng = np.random.default_rng(11)
    pair, duo = _pair_and_duo(n, kind="walk", control_mode="PD", n_substeps=10, auto_reset=True)
    for e in (pair, duo):
        e.set_trajectory(traj["time"], traj["qpos"])
    dones = _rollout(pair, duo, _start(oracle_mod, n), [rng.uniform(PD_LO, PD_HI, (n, 6)) for _ in range(3)])
    assert sum(int(d.sum()) for d in dones) >= 2 * n, "the bench's regime: the environments terminate and reset on every step"


# (c), (d), (e): one substep, and 10 substeps
@pytest.mark.parametrize("nsub", [1, 10])
@pytest.mark.parametrize("regime", ["c", "d", "e"])
def test_eight_row_groups(oracle_mod, regime, nsub):
    n = 4 * _g()
    pair, duo = _pair_and_duo(n, kind="stand", control_mode="Torque", n_substeps=nsub, auto_reset=False)
    s0 = _start(oracle_mod, n)
    for e in {"c": [_odd(0)], "d": [_odd(1)], "e": [_odd(0), _odd(1)]}[regime]:
        s0[e, 6] += 1.5; s0[e, 39 + 6] += 1.5
    _rollout(pair, duo, s0, [np.zeros((n, 6)) for _ in range(3)])


# (f)
@pytest.mark.parametrize("group", [0, 1])
def test_reset_pass_with_one_group(oracle_mod, group):
    n = 2 * _g()
    rng = np.random.default_rng(13)
    pair, duo = _pair_and_duo(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True)
    s0 = _start(oracle_mod, n)
    e = _odd(group)
    _sink(s0, e)
    dones = _rollout(pair, duo, s0, [rng.uniform(PD_LO, PD_HI, (n, 6)) for _ in range(3)])
    assert dones[0].tolist() == [i == e for i in range(n)]
    assert (pair.pending == 0).all(), "the odd environment is reset by this tier"


# (h)
def test_height_field_direct_and_reset(oracle_mod):
    n = 2 * _g()
    rng = np.random.default_rng(17)
    pair, duo = _pair_and_duo(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True)
    for e in (pair, duo):
        _relief(e)
    s0 = _start(oracle_mod, n, hf=True)
    e = _odd(1)
    _sink(s0, e)
    dones = _rollout(pair, duo, s0, [rng.uniform(PD_LO, PD_HI, (n, 6)) for _ in range(3)])
    assert dones[0][e]


@pytest.mark.parametrize("nsub", [1, 10])
def test_height_field_eight_row_a(oracle_mod, nsub):
    n = 4 * _g()
    pair, duo = _pair_and_duo(n, kind="stand", control_mode="Torque", n_substeps=nsub, auto_reset=False)
    for e in (pair, duo):
        _relief(e)
    s0 = _start(oracle_mod, n, hf=True)
    e = _odd(0)
    s0[e, 6] += 1.5; s0[e, 39 + 6] += 1.5
    _rollout(pair, duo, s0, [np.zeros((n, 6)) for _ in range(3)])
