"""step_outputs (cassie_leg_core.h) writes the observation row ONCE: in the 64-environments-per-wavefront form (one outputs section) the row holds the
reset observation on the lanes that reset and the step's observation on the other live lanes, where the code before it stored the step's row and
then the reset row over it.  The bytes must be the same.  On the CPU lane emulation (oracle/leg_host), stand env / PD with a gentle hold so that
nobody terminates on its own, each environment given a role: `done` (pelvis at z = 0.45, pitched by a quarter turn so that no foot is near the floor: it
falls freely, terminates and resets without leaving the tier), `live` (keeps standing), `bad` (a
NaN velocity: failure guard, outputs zeroed, reset pose's own observation).  Batches of 1, 2 and 5 environments, the roles rotated so that a batch of
one sees each of them.  Compared with (a) the two-lanes form, which keeps the two stores, and (b) tests/golden/step_outputs_single_write.npz, the
same runs recorded from the emulation of the source before the single write (observation, reward, done, records of every step)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, state_vec
from leg_host import LegHostEnv

ROLES = ("done", "live", "bad")
HOLD = np.array([0.68111815, -1.40730357, -1.77611107] * 2)   # PD targets at the reset pose's hip / knee / toe
STEPS = 4


def run(oracle_mod, n, shift, duo, flags=0):
    """STEPS Env.steps; the roles are applied before the first and again before the third step (by then everybody stands in the reset pose or near it)."""
    env = LegHostEnv(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True, duo=duo, flags=flags)
    o = oracle_mod.Oracle()
    q, v = o.state()
    env.set_full_state_host(np.tile(state_vec(q, v, o.warmstart(), qstate=q), (n, 1)))
    rng = np.random.default_rng(100 * n + shift)
    rows = []
    for t in range(STEPS):
        if t % 2 == 0:
            s = env.get_full_state_host()
            for e in range(n):
                role = ROLES[(e + shift + t // 2) % 3]
                if role == "done":
                    s[e, 1], s[e, 2] = 0.45, np.pi / 2
                elif role == "bad":
                    s[e, 13 + 9] = np.nan
            env.set_full_state_host(s)
        obs, rew, done = env.step_host(HOLD + rng.uniform(-0.02, 0.02, (n, 6)))
        rows.append((obs, rew, done.astype(np.uint8), env.get_full_state_host()))
    return [np.stack([r[k] for r in rows]) for k in range(4)], env.nonfinite


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_single_write_of_the_observation_row_keeps_the_bytes(oracle_mod, n, shift):
    golden = np.load(os.path.join(GOLDEN, "step_outputs_single_write.npz"))
    (pair, bad_pair), (duo, bad_duo) = run(oracle_mod, n, shift, False), run(oracle_mod, n, shift, True)
    roles0 = [ROLES[(e + shift) % 3] for e in range(n)]
    for k, what in enumerate(("obs", "reward", "done", "records")):
        assert np.array_equal(pair[k], duo[k], equal_nan=True), ("two-lanes form against the single write", what)
        assert np.array_equal(duo[k], golden["n%d_s%d_%s" % (n, shift, what)], equal_nan=True), ("the bytes before the single write", what)
    assert bad_pair == bad_duo == sum(ROLES[(e + shift + h) % 3] == "bad" for e in range(n) for h in range(STEPS // 2))
    # the scenario is what it says: who terminates on the first step, and what the row then holds
    done0, obs0 = duo[2][0].astype(bool), duo[0][0]
    assert list(done0) == [r != "live" for r in roles0]
    assert np.isfinite(duo[0]).all() and (obs0[:, 17:] == 0.0).all()
    for e, r in enumerate(roles0):
        if r == "done":
            assert obs0[e, 0] < 0.6, "a reset lane keeps the operational-space values of the last setState (the lowered body)"
        if r == "bad":
            assert obs0[e, 0] > 0.9, "a failure-guard lane takes the reset pose's own operational-space state"


@pytest.mark.parametrize("n", [2, 5])
def test_single_write_with_fix_stale_kin(oracle_mod, n):
    """FLAG_FIX_STALE_KIN: every resetting lane takes the reset pose's own values (the `own` branch for all of them)."""
    golden = np.load(os.path.join(GOLDEN, "step_outputs_single_write.npz"))
    (pair, _), (duo, _) = run(oracle_mod, n, 0, False, flags=1), run(oracle_mod, n, 0, True, flags=1)
    for k, what in enumerate(("obs", "reward", "done", "records")):
        assert np.array_equal(pair[k], duo[k], equal_nan=True), what
        assert np.array_equal(duo[k], golden["n%d_kin_%s" % (n, what)], equal_nan=True), what
