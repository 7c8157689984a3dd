"""The direct path of the 64-environments-per-wavefront Env.step (cassierl_amd/csrc/cassie_duo_core.h, env_step2): when group B's set-up ends in its
six-row tail and group A is not in the eight-row format, B's rows go from the set-up's registers straight into the joint sweep instead of through the
workspace.  The 64-env kernel (LEG_TIER_ON | DUO_TIER_ON) against the two-lanes kernel (LEG_TIER_ON | DUO_TIER_OFF), each forced as the first tier,
BIT FOR BIT: the 88-double records, observation, reward, done flag, terminal observation after every step, and the counters.  One regime per branch
of a pass (environments 0..31 of a wavefront are its group A, 32..63 its group B):

  (a) direct path in every substep and in the reset pass: walk/PD with resets; n = 33 (B holds one environment), 64, 128
  (b) B absent: n = 31, 32; n = 65, 96 (the last wavefront has group A only: the stand-alone block with idle rows for B)
  (c) A eight-row, B six-row (B stores its rows and is widened): stand/Torque, zero torque, no reset, the left knee of environment 5 past its limit
  (d) B eight-row, A six-row: the same with environment 40         (e) both: environments 5 and 40
  (f) reset pass with one group only: stand/PD with resets, n = 64, one environment below the termination height -- environment 5 (the reset pass runs A
      alone: stand-alone block, idle B) or 40 (B alone: direct path, idle rows for A)
  (g) paths changing from substep to substep: stand/Torque, random torques, no reset
  (h) the height-field kernel: (a) at n = 64 and (c) on the relief of tests/test_gpu_step_io.py
  (i) commands from the record (env_step_duo_kernel<2>, one substep per launch): the OSC controller in the loop
  (j) the workspace claim table: a slot is re-used by a later wavefront that no longer writes B's rows

(f): the pelvis is lowered by 0.5 m (record word 1 and its snapshot copy, word 40) AND pitched by 1.5 rad (word 2 and its copy, word 41).  Lowered alone,
the feet start half a metre under the floor, the environment is over eight rows per leg in its first substep and leaves the tier: a lower tier resets it
and this kernel's reset pass never runs (seen on the CPU emulation: pending = 10; tests/test_duo_direct_rows_host.py).  Pitched, the legs lie level
above the floor, the environment stays in the tier (cleanup_substeps == 0 is asserted) and this kernel resets it.

That (c) - (f) reach the branch they name was confirmed once, when the path was written, from the hand-over workspace after ONE launch
(CassieVecEnv.debug_workspace_host, as tools/dbg_duo_ws.py reads it): group B's row slots behind its six force slots hold what the launch found there
where B took the direct path, six-row data where it stored its rows, the eight-row block where it was widened or went eight-row itself.  For (f) the
done flag of exactly the odd environment together with cleanup_substeps == 0 says that this kernel's reset pass ran for that group alone.
-m gpu only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PD_LO, PD_HI = np.radians([-50, -164, -140] * 2), np.radians([80, -37, -30] * 2)
TQ = np.array([12.0, 12.0, 0.9] * 2)
OSC_LO, OSC_HI = np.array([-2.0, -2.0, -2.0, 0.0, -2.0, 0.0, -2.0]), np.full(7, 2.0)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, np.argwhere(a != b)[:6].tolist())


def _relief(env):
    xs = np.linspace(-10.0, 10.0, 2001)
    env.set_heightfield(np.tile(0.015 * (1.0 - np.cos(2.0 * np.pi * xs / 1.5)), (64, 1)), 10.0, 10.0)


def _knee(envs):
    def f(s):
        for e in envs:
            s[e, 6] += 1.5; s[e, 39 + 6] += 1.5   # (the recipe of tools/dbg_duo_limit.py)
    return f


def _sink(e):
    def f(s):
        s[e, 1] -= 0.5; s[e, 40] -= 0.5
        s[e, 2] += 1.5; s[e, 41] += 1.5
    return f


def _rollout(env, traj, steps, lo, hi, seed=11, hf=False, edit=None):
    """`steps` Env.steps of random actions (lo is None: zero torque); after every step the outputs and the records."""
    import torch
    from cassierl_amd import rollout as R
    n = env.n_envs
    ids = torch.arange(n, device="cuda:0")
    if env.kind == "walk":
        env.set_trajectory(traj["time"], traj["qpos"])
    if hf:
        _relief(env)
    bufs = env.alloc()
    tobs = torch.zeros((n, 26), dtype=torch.float64, device="cuda:0")
    env.reset(bufs)
    s = env.get_full_state_host()
    if hf:
        s[:, 0] += np.linspace(-3.0, 3.0, n)
        s[:, 1] += 0.03
    if edit is not None:
        edit(s)
    env.set_full_state_host(s)
    rows = []
    for t in range(steps):
        a = torch.zeros((n, 6), dtype=torch.float64, device="cuda:0") if lo is None else R.random_actions(seed, ids, t, lo, hi)
        o, r, d = env.step(a, bufs, terminal_obs=tobs)
        env.synchronize()
        rows.append(dict(obs=o.cpu().numpy().copy(), reward=r.cpu().numpy().copy(), done=d.cpu().numpy().copy(), tobs=tobs.cpu().numpy().copy(),
                         state=env.get_full_state_host()))
    return rows, env.counters()


def _compare(n, traj, steps=3, lo=PD_LO, hi=PD_HI, table=None, **kw):
    """Both kernels through the same rollout; everything bit for bit.  Returns the 64-env kernel's rows and counters."""
    from cassierl_amd import vec_env as V
    roll = {k: kw.pop(k) for k in ("seed", "hf", "edit") if k in kw}
    pair = V.CassieVecEnv(n, flags=V.LEG_TIER_ON | V.DUO_TIER_OFF, **kw)
    duo = V.CassieVecEnv(n, flags=V.LEG_TIER_ON | V.DUO_TIER_ON, **kw)
    info = duo.tier_info()
    assert pair.tier_info()["first_tier"] == "leg" and info["first_tier"] == "duo"
    if table is not None:
        assert info["duo_table_slots"] == table
    (ra, ca), (rb, cb) = _rollout(pair, traj, steps, lo, hi, **roll), _rollout(duo, traj, steps, lo, hi, **roll)
    for t, (a, b) in enumerate(zip(ra, rb)):
        for k in a:
            _same(a[k], b[k], (t, k))
    assert ca["nonfinite_resets"] == cb["nonfinite_resets"]
    assert ca["cleanup_substeps"] == cb["cleanup_substeps"]
    pair.close(); duo.close()
    return rb, cb


WALK = dict(kind="walk", control_mode="PD", n_substeps=10, auto_reset=True)


@pytest.mark.parametrize("n", [33, 64, 128, 31, 32, 65, 96])
def test_walk_pd_with_resets(n, traj):
    """(a): 33, 64, 128;  (b): 31, 32, 65, 96"""
    rows, c = _compare(n, traj, **WALK)
    assert sum(int(r["done"].sum()) for r in rows) >= 2 * n, "the bench's regime: the environments terminate and reset on every step"
    assert c["cleanup_substeps"] == 0


@pytest.mark.parametrize("nsub", [1, 10])
@pytest.mark.parametrize("regime", ["c", "d", "e"])
def test_eight_row_groups(regime, nsub, traj):
    _compare(128, traj, lo=None, edit=_knee({"c": [5], "d": [40], "e": [5, 40]}[regime]), kind="stand", control_mode="Torque", n_substeps=nsub, auto_reset=False)


@pytest.mark.parametrize("odd", [5, 40])
def test_reset_pass_with_one_group(odd, traj):
    """(f)"""
    rows, c = _compare(64, traj, edit=_sink(odd), kind="stand", control_mode="PD", n_substeps=10, auto_reset=True)
    assert rows[0]["done"].astype(bool).tolist() == [e == odd for e in range(64)]
    assert c["cleanup_substeps"] == 0, "the odd environment is reset by this tier"


def test_paths_changing_between_substeps(traj):
    """(g)"""
    _compare(128, traj, steps=6, lo=-TQ, hi=TQ, kind="stand", control_mode="Torque", n_substeps=10, auto_reset=False)


def test_height_field_walk_pd_with_resets(traj):
    """(h), regime (a)"""
    _compare(64, traj, hf=True, **WALK)


@pytest.mark.parametrize("nsub", [1, 10])
def test_height_field_eight_row_a(nsub, traj):
    """(h), regime (c)"""
    _compare(128, traj, lo=None, hf=True, edit=_knee([5]), kind="stand", control_mode="Torque", n_substeps=nsub, auto_reset=False)


def test_commands_from_the_record(traj):
    """(i)"""
    _compare(64, traj, steps=2, lo=OSC_LO, hi=OSC_HI, seed=4, kind="stand", control_mode="OSC", n_substeps=10, auto_reset=True)


def test_workspace_claim_table(traj, monkeypatch):
    """(j)"""
    monkeypatch.setenv("CASSIE2D_DUO_TABLE", "64")
    monkeypatch.setenv("CASSIE2D_DUO_FLAT_HINT", "1")
    _compare(4096 + 45, traj, steps=2, table=64, **WALK)
