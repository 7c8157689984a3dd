"""The input and output sections of the 64-environments-per-wavefront Env.step (cassie_kernels_duo.hip: the batch arrays are addressed through one
descriptor per array and a 32-bit lane offset; cassie_leg_core.h / cassie_duo_core.h: the records are loaded in one batch, the observation row is
written once, the stores go out mask by mask) against the two-lanes-per-environment kernel, each forced as the first tier: observation, terminal
observation, reward, done flag and the full 88-double records BIT-IDENTICAL over three steps, at batch sizes around every edge of the lane layout
(1: one lane pair; 31 / 32 / 33: group B empty, group A full, group B with one pair; 63 / 64 / 65: a full wavefront and one pair of the next; 129:
a second workgroup).  Every output array is a window into a larger allocation filled with a sentinel: the rows before and beyond the batch must
come back untouched.  -m gpu only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PD_LO, PD_HI = np.radians([-50, -164, -140] * 2), np.radians([80, -37, -30] * 2)
TQ = np.array([12.0, 12.0, 0.9] * 2)
SIZES = [1, 31, 32, 33, 63, 64, 65, 129]
PAD = 3            # sentinel rows on either side of every output array (3 reward rows = 24 bytes: the window is only 8-byte aligned)
SENTINEL = -7.25   # no output takes this value (0xA5 for the done bytes)
STEPS = 3

# name -> (kind, mode, auto_reset, terminal-obs buffer, flag name, special)
CASES = {
    "walk_pd_reset_tobs": ("walk", "PD", True, True, None, None),
    "walk_pd_reset": ("walk", "PD", True, False, None, None),
    "walk_pd_noreset_tobs": ("walk", "PD", False, True, None, None),
    "walk_torque_reset_tobs": ("walk", "Torque", True, True, None, None),
    "stand_pd_reset_tobs": ("stand", "PD", True, True, None, None),
    "stand_torque_noreset": ("stand", "Torque", False, False, None, None),
    "stand_torque_bare_substeps": ("stand", "Torque", False, False, None, "bare"),
    "walk_pd_fix_stale_kin": ("walk", "PD", True, True, "FIX_STALE_KIN", None),
    "walk_pd_poisoned": ("walk", "PD", True, True, None, "nan"),
    "walk_pd_height_field": ("walk", "PD", True, True, None, "hf"),
}


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (what, np.argwhere(a != b)[:6].tolist())


class _Windows:
    """obs / terminal obs / reward / done of n environments as windows [PAD, PAD + n) of sentinel-filled allocations."""

    def __init__(self, n, tobs):
        import torch
        self.n = n
        self.full = dict(obs=torch.full((n + 2 * PAD, 26), SENTINEL, dtype=torch.float64, device="cuda:0"),
                         reward=torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda:0"),
                         done=torch.full((n + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda:0"))
        if tobs:
            self.full["tobs"] = torch.full((n + 2 * PAD, 26), SENTINEL, dtype=torch.float64, device="cuda:0")
        self.win = {k: v[PAD:PAD + n] for k, v in self.full.items()}

    def read(self):
        """The windows as host arrays, after checking that nothing outside them was written."""
        out = {}
        for k, v in self.full.items():
            h = v.cpu().numpy()
            edge = np.concatenate([h[:PAD], h[PAD + self.n:]])
            assert (edge == (0xA5 if k == "done" else SENTINEL)).all(), "%s: a row outside the batch was written" % k
            out[k] = h[PAD:PAD + self.n].copy()
        return out


def _run(env, case, traj):
    import torch
    from cassierl_amd import rollout as R
    kind, mode, auto_reset, tobs, flag, special = CASES[case]
    n = env.n_envs
    ids = torch.arange(n, device="cuda:0")
    lo, hi = (-TQ, TQ) if mode == "Torque" else (PD_LO, PD_HI)
    if kind == "walk":
        env.set_trajectory(traj["time"], traj["qpos"])
    if special == "hf":
        xs = np.linspace(-10.0, 10.0, 2001)
        env.set_heightfield(np.tile(0.015 * (1.0 - np.cos(2.0 * np.pi * xs / 1.5)), (64, 1)), 10.0, 10.0)
    w = _Windows(n, tobs)
    env.reset(w.win)
    s = env.get_full_state_host()
    if special == "hf":
        s[:, 0] += np.linspace(-3.0, 3.0, n)
        s[:, 1] += 0.03
    if special == "nan":
        s[min(n - 1, 40), 13 + 9] = np.nan   # (40: group B of the first wavefront; smaller batches: their last environment)
    env.set_full_state_host(s)
    rows = []
    for t in range(STEPS):
        a = R.random_actions(11, ids, t, lo, hi)
        if special == "bare":
            env.substep_host(mode, a.cpu().numpy(), 4)   # physics only: no observation arrays in the launch
        else:
            env.step(a, w.win, terminal_obs=w.win.get("tobs"))
            env.synchronize()
        rows.append((w.read(), env.get_full_state_host()))
    return rows, env.counters()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_step_io_is_bit_identical_and_stays_in_range(case, n, traj):
    from cassierl_amd import vec_env as V
    kind, mode, auto_reset, tobs, flag, special = CASES[case]
    flags = getattr(V, flag) if flag else 0
    kw = dict(kind=kind, control_mode=mode, n_substeps=10, auto_reset=auto_reset)
    pair = V.CassieVecEnv(n, flags=flags | V.LEG_TIER_ON | V.DUO_TIER_OFF, **kw)
    duo = V.CassieVecEnv(n, flags=flags | V.LEG_TIER_ON | V.DUO_TIER_ON, **kw)
    assert pair.tier_info()["first_tier"] == "leg" and duo.tier_info()["first_tier"] == "duo"
    (ra, ca), (rb, cb) = _run(pair, case, traj), _run(duo, case, traj)
    for t, ((wa, sa), (wb, sb)) in enumerate(zip(ra, rb)):
        for k in wa:
            _same(wa[k], wb[k], (t, k))
        _same(sa, sb, (t, "state records"))
    assert ca["nonfinite_resets"] == cb["nonfinite_resets"] == (1 if special == "nan" else 0)
    assert ca["cleanup_substeps"] == cb["cleanup_substeps"]
    if special == "nan":
        k = min(n - 1, 40)
        first = rb[0][0]
        assert first["done"][k] and first["reward"][k] == 0.0 and (first["tobs"][k] == 0.0).all() and np.isfinite(first["obs"]).all()
    if case == "walk_pd_reset_tobs":
        assert sum(int(w["done"].sum()) for w, _ in rb) >= (STEPS - 1) * n, "the bench's regime: the environments terminate and reset on every step"
    pair.close(); duo.close()
