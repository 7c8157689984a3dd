"""The reset of a terminated environment inside the fused Env.step of the 64-environments-per-wavefront kernel (cassie_duo_core.h: ONE outputs
section -- the call after the last substep stores the reset observation itself, the reset pass ends at its finish) against the two-lanes-per-environment
kernel, which keeps the generic form (reset pass, then a second outputs call): observations, rewards, done flags and state records BIT-IDENTICAL
where every environment resets, where a few lanes of a wavefront reset, with each quirk flag, with the motor commands taken from the record, with a
failure-guard reset, and on terrain (where the 64-environments kernel keeps the generic form too).  -m gpu only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PD_LO, PD_HI = np.radians([-50, -164, -140] * 2), np.radians([80, -37, -30] * 2)
JAC_LO, JAC_HI = np.array([-40.0, 50.0, -15.0] * 2), np.array([40.0, 250.0, 15.0] * 2)


def _envs(n, **kw):
    from cassierl_amd.vec_env import CassieVecEnv, LEG_TIER_ON, DUO_TIER_ON, DUO_TIER_OFF
    flags = kw.pop("flags", 0)
    pair = CassieVecEnv(n, flags=flags | LEG_TIER_ON | DUO_TIER_OFF, **kw)
    duo = CassieVecEnv(n, flags=flags | LEG_TIER_ON | DUO_TIER_ON, **kw)
    assert pair.tier_info()["first_tier"] == "leg" and duo.tier_info()["first_tier"] == "duo"
    return pair, duo


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), (what, np.argwhere(a != b)[:6].tolist())


def _rollout(env, traj, steps, lo, hi, seed, prepare=None, tobs=False):
    """`steps` Env.steps under random actions; every step's observation, reward, done (and terminal observation), the records and counters."""
    import torch
    from cassierl_amd import rollout as R
    n = env.n_envs
    ids = torch.arange(n, device="cuda:0")
    env.set_trajectory(traj["time"], traj["qpos"])
    bufs = env.alloc()
    env.reset(bufs)
    if prepare is not None:
        prepare(env, bufs)
    term = torch.zeros((n, 26), dtype=torch.float64, device="cuda:0") if tobs else None
    rows = []
    for t in range(steps):
        o, r, d = env.step(R.random_actions(seed, ids, t, lo, hi), bufs, terminal_obs=term)
        rows.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy(), term.cpu().numpy().copy() if tobs else np.zeros(0)))
    return rows, env.get_full_state_host(), env.counters()


def _compare(outs, resets_wanted=True):
    (ra, sa, ca), (rb, sb, cb) = outs
    n_done = 0
    for t, (a, b) in enumerate(zip(ra, rb)):
        _same(a[0], b[0], (t, "obs")); _same(a[1], b[1], (t, "reward")); _same(a[2], b[2], (t, "done")); _same(a[3], b[3], (t, "terminal obs"))
        n_done += int(b[2].sum())
    _same(sa, sb, "state records")
    assert ca["nonfinite_resets"] == cb["nonfinite_resets"] and ca["cleanup_substeps"] == cb["cleanup_substeps"]
    if resets_wanted:
        assert n_done > 0, "the run must include resets"
    return n_done


@pytest.mark.parametrize("n", [8, 37, 129])
def test_every_environment_resets(n, traj):
    """(a) walk env, PD, random targets: every environment terminates on every step.  8: group B empty; 37: group B partly filled; 129: a second
    workgroup's wavefront with one lane pair."""
    pair, duo = _envs(n, kind="walk", control_mode="PD", n_substeps=10, auto_reset=True)
    outs = [_rollout(e, traj, 20, PD_LO, PD_HI, 1, tobs=True) for e in (pair, duo)]
    assert _compare(outs) >= 19 * n
    pair.close(); duo.close()


def test_a_few_lanes_of_a_wavefront_reset(traj):
    """(b) stand env, PD: robots hold the pose they are sent to, so nobody terminates on its own for the first steps; a chosen subset is put below
    z = 0.5 through the masked reset-to-states call and terminates on the next step: one environment of group A only (3), one of group B only (40),
    both of a lane pair's environments (10 and 42: lanes 20/21 serve both), all of group A of the second wavefront (64..95).  The wavefront runs the
    reset pass for those lanes while the others stay live; everybody is compared."""
    import torch
    n = 96
    low = [3, 40, 10, 42] + list(range(64, 96))

    def prepare(env, bufs):
        q, v = env.get_state()
        q, v = q.clone(), v.clone()
        mask = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        mask[low] = 1
        q[low, 1] = 0.45
        env.reset_to(q, v, bufs, mask=mask)

    pair, duo = _envs(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True)
    hold = np.array([0.68111815, -1.40730357, -1.77611107] * 2)   # targets at the reset pose's hip / knee / toe: a gentle PD hold
    outs = [_rollout(e, traj, 20, hold - 0.02, hold + 0.02, 2, prepare=prepare, tobs=True) for e in (pair, duo)]
    _compare(outs)
    first_done = outs[1][0][0][2].astype(bool)
    assert first_done[low].all(), "the lowered robots terminate on the first step"
    assert not first_done.all() and first_done[:64].sum() < 64, "a wavefront must reset some lanes while others stay live"
    pair.close(); duo.close()


@pytest.mark.parametrize("flag", ["FIX_STALE_KIN", "FIX_STALE_QSTATE"])
def test_each_quirk_flag_on_its_own(flag, traj):
    """(c) as (a) with one flag set: FIX_STALE_KIN makes the reset observation the operational-space state of the reset pose itself (the branch that
    does not re-use the step's values); FIX_STALE_QSTATE changes the walk reward, i.e. who terminates."""
    from cassierl_amd import vec_env as V
    pair, duo = _envs(96, kind="walk", control_mode="PD", n_substeps=10, auto_reset=True, flags=getattr(V, flag))
    outs = [_rollout(e, traj, 20, PD_LO, PD_HI, 3, tobs=True) for e in (pair, duo)]
    _compare(outs)
    pair.close(); duo.close()


def test_motor_commands_from_the_record(traj):
    """(d) Jacobian control: the controller kernel writes the motor commands into the record and the kernel runs in MODE 2, one substep per launch; the
    reset pass reads the same record for its stale commands."""
    pair, duo = _envs(96, kind="walk", control_mode="Jacobian", n_substeps=10, auto_reset=True)
    outs = [_rollout(e, traj, 10, JAC_LO, JAC_HI, 4, tobs=True) for e in (pair, duo)]
    _compare(outs)
    pair.close(); duo.close()


@pytest.mark.parametrize("flag", [None, "FIX_STALE_KIN"])
def test_the_failure_guard_lane(flag, traj):
    """(e) one environment's record holds a non-finite velocity (environment 40: group B of the first wavefront): outputs zeroed, the environment
    reset, its reset observation the reset pose's own -- and nonfinite_resets == 1 in both handles.  Also with FIX_STALE_KIN, where every
    resetting lane, the poisoned one among them, takes the reset pose's own values."""
    from cassierl_amd import vec_env as V
    flag = getattr(V, flag) if flag else 0

    def prepare(env, bufs):
        s = env.get_full_state_host()
        s[40, 13 + 9] = np.inf
        env.set_full_state_host(s)

    pair, duo = _envs(70, kind="walk", control_mode="PD", n_substeps=10, auto_reset=True, flags=flag)
    outs = [_rollout(e, traj, 20, PD_LO, PD_HI, 5, prepare=prepare, tobs=True) for e in (pair, duo)]
    _compare(outs)
    assert outs[0][2]["nonfinite_resets"] == outs[1][2]["nonfinite_resets"] == 1
    first = outs[1][0][0]
    assert first[2][40] and first[1][40] == 0.0 and np.isfinite(first[0]).all() and (first[3][40] == 0.0).all()
    assert np.isfinite(outs[1][1]).all()
    pair.close(); duo.close()


def test_terrain_batch_keeps_the_generic_path(traj):
    """(f) a one-field terrain library: the height-field kernels keep the reset pass with its own outputs call; still equal to the two-lanes kernel."""
    import torch
    n = 70
    xs = np.linspace(-10.0, 10.0, 2001)
    relief = np.tile(0.015 * (1.0 - np.cos(2.0 * np.pi * xs / 1.5)), (64, 1))

    def prepare(env, bufs):
        env.set_terrain_library([relief], (10.0, 10.0))
        env.set_terrain_ids(torch.zeros(n, dtype=torch.int32, device="cuda:0"))
        s = env.get_full_state_host()
        s[:, 0] += np.linspace(-3.0, 3.0, n)
        s[:, 1] += 0.03
        env.set_full_state_host(s)

    pair, duo = _envs(n, kind="walk", control_mode="PD", n_substeps=10, auto_reset=True)
    outs = [_rollout(e, traj, 20, PD_LO, PD_HI, 6, prepare=prepare, tobs=True) for e in (pair, duo)]
    _compare(outs)
    pair.close(); duo.close()
