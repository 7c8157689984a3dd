"""A mixed pool of Cassie3d robots for the tests that put DIFFERENT robots into one wavefront (tests/test_gpu_cassie3d_mixed.py on the
GPU, tests/test_leg3d_mixed_cpu.py on the CPU build of the same source).  The lane-per-leg kernel (cassie3d_leg_core.h) runs 16 or 32 robots
per wavefront and masks nearly all of its control flow per lane under wavefront-wide any() tests (sweeping, nlim > j, ncon > p, live,
overflow); a batch of identical copies never makes two lanes disagree.  This pool does: standing, flying, dropped, lying robots, robots
over a leg's slot budget, robots that cross the row capacity inside a step, and robots with joint-limit rows -- interleaved, so that every
run of 16 consecutive robots holds several kinds.

Everything is drawn on the CPU from a seed and selected with the ORACLE alone (row types, row counts, free runs), so the pool -- and
what coverage() says about it -- is the same wherever the tests run."""
import numpy as np

from cassierl_amd import vec_env3d

CTRL = vec_env3d.CTRL_RANGE
DT = 0.0005
K = 48
# the slot budget of one leg in the lane-per-leg kernel (cassie3d_leg_core.h: NSLOT3, R3_N, C3_N): nlim * 18 + ncon * 52 <= 160
NSLOT3, R3_N, C3_N = 160, 18, 52
# limited hinges of cassie3d_stiff.xml: dofs 6..11 (left) and 13..18 (right), qpos address = dof + 1; ranges as in
# test_row_cap_beyond_64_rows_matches_the_capped_oracle
LIM_DOF = [6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18]
LIM_RNG = np.radians([[-15, 22.5], [-22.5, 22.5], [-50, 80], [-164, -37], [50, 170], [-140, -30]] * 2)
OVERSHOOT = 0.02
SIDE = [np.cos(np.pi / 4), np.sin(np.pi / 4), 0.0, 0.0]   # rolled 90 degrees: lying on its side


class Pool:
    """recs [K][80] state records (oracle warm start), labels [K] kind of each robot, q / v the states, torques [K][10] one fixed torque
    per robot (placement tests, coverage's free run)."""

    def __init__(self, oracle_mod, q, v, recs, labels, torques):
        self.oracle_mod, self.q, self.v, self.recs, self.labels, self.torques = oracle_mod, q, v, recs, labels, torques

    def __len__(self):
        return len(self.labels)


def rows(o):
    """(nlim[2], ncon[2], nefc) of the oracle's current state: limit rows and contacts per leg as the lane-per-leg kernel books them
    (the pelvis sphere rides on the left lane)."""
    J, _, _, _, typ = o.efc()
    nlim, ncon = [0, 0], [0, 0]
    for i in np.flatnonzero(typ == 1):
        nlim[int(np.flatnonzero(J[i])[0] >= 13)] += 1
    for i in np.flatnonzero(typ == 2)[::3]:
        ncon[int(np.abs(J[i:i + 3, 13:20]).max() > 0.0)] += 1
    return nlim, ncon, o.nefc


def fits(nlim, ncon):
    return all(nl * R3_N + nc * C3_N <= NSLOT3 for nl, nc in zip(nlim, ncon))


def perturbed(rng, kat, spread, height):
    """the pose perturbation of random_state (tests/test_gpu_cassie3d.py)"""
    q = np.array(kat["qpos_init"])
    q[:2] += rng.uniform(-0.5, 0.5, 2)
    q[2] = height
    quat = np.array([1.0, 0, 0, 0]) + rng.uniform(-spread, spread, 4)
    q[3:7] = quat / np.linalg.norm(quat)
    q[7:] += rng.uniform(-spread, spread, 14)
    return q, rng.uniform(-1.0, 1.0, 20)


def at_limits(q, ks, rng):
    """push the limited hinges ks (indices into LIM_DOF) OVERSHOOT beyond a random end of their range"""
    q = q.copy()
    for k in ks:
        q[LIM_DOF[k] + 1] = LIM_RNG[k, 1] + OVERSHOOT if rng.integers(2) else LIM_RNG[k, 0] - OVERSHOOT
    return q


def lower_until(o, q, v, ok, z0, z1, dz=0.002):
    """the first height from z0 down to z1 at which ok(rows) holds; at z0, if there is none"""
    q = q.copy()
    for z in np.arange(z0, z1, -dz):
        q[2] = z
        o.reset(q, v)
        if ok(*rows(o)):
            return q
    q[2] = z0
    return q


def make_pool(oracle_mod, kat, seed=0):
    rng = np.random.default_rng(seed)
    o = oracle_mod.Oracle3D()
    q0 = np.array(kat["qpos_init"])

    def draw(make, ok, tries=400):
        for _ in range(tries):
            q, v = make()
            o.reset(q, v)
            if ok(*rows(o)):
                return q, v
        raise AssertionError("no state of the wanted kind in %d draws" % tries)

    def standing():
        return q0.copy(), rng.uniform(-0.05, 0.05, 20)

    def lying():
        q = q0.copy()
        q[:2] += rng.uniform(-0.5, 0.5, 2)
        q[2] = 0.12
        q[3:7] = SIDE
        return q, rng.uniform(-0.05, 0.05, 20)

    def limits_in_air(ks):
        def make():
            q = q0.copy()
            q[2] = 1.3
            return at_limits(q, ks, rng), rng.uniform(-0.2, 0.2, 20)
        return make

    def limits_on_ground(ks, leg):
        # the standing pose with hinges of one leg at their limits, lowered until that leg's foot is on the floor
        def make():
            v = rng.uniform(-0.05, 0.05, 20)
            q = at_limits(q0, ks, rng)
            return lower_until(o, q, v, lambda nl, nc, n: 1 <= nc[leg] <= 2 and fits(nl, nc), q0[2] + 0.1, q0[2] - 0.3), v
        return make

    def side_drop(speed, u, z0, z1, start_ok, later_ok):
        # the side-lying drop of test_many_contacts_hand_over_to_the_general_kernel, lower and faster: the highest start at which the
        # rows satisfy start_ok at substep 0 and later_ok before substep 10 (free run of the oracle under the robot's torque)
        q = q0.copy()
        q[3:7] = SIDE
        v = np.zeros(20)
        v[2] = -speed
        for z in np.arange(z0, z1, -0.0005):
            q[2] = z
            o.reset(q, v)
            if not start_ok(*rows(o)):
                continue
            for _ in range(9):
                o.step_torque(u)
                if later_ok(*rows(o)):
                    return q, v
        raise AssertionError("no side-lying drop of the wanted kind at speed %g" % speed)

    kinds = dict(
        stand=lambda: draw(standing, lambda nl, nc, n: n == 18),
        air=lambda: draw(lambda: perturbed(rng, kat, 0.25, rng.uniform(1.2, 1.5)), lambda nl, nc, n: n == 6),
        low=lambda: draw(lambda: perturbed(rng, kat, rng.choice([0.05, 0.25]), 0.25), lambda nl, nc, n: n > 6),
        lying=lambda: draw(lying, lambda nl, nc, n: n > 32),
        budget=lambda: draw(lambda: perturbed(rng, kat, 0.25, rng.uniform(0.2, 0.45)), lambda nl, nc, n: 21 <= n <= 32 and not fits(nl, nc)),
        lim1=lambda: draw(limits_in_air([rng.integers(12)]), lambda nl, nc, n: n == 7),
        limboth=lambda: draw(limits_in_air([rng.integers(6), 6 + rng.integers(6)]), lambda nl, nc, n: n == 8 and nl == [1, 1]),
        lim3=lambda: draw(limits_in_air(6 * rng.integers(2) + rng.choice(6, 3, replace=False)), lambda nl, nc, n: n == 9 and max(nl) == 3),
        lim6=lambda: draw(limits_in_air(6 * rng.integers(2) + np.arange(6)), lambda nl, nc, n: n == 12 and max(nl) == 6),
        lim12=lambda: draw(limits_in_air(np.arange(12)), lambda nl, nc, n: n == 18 and nl == [6, 6]),
    )

    def limcon():
        leg = int(rng.integers(2))
        ks = 6 * leg + rng.choice(5, int(rng.integers(1, 4)), replace=False)   # hinges 0..4: the toe joint is limfoot's
        return limits_on_ground(ks, leg)()

    def limfoot():
        leg = int(rng.integers(2))
        return limits_on_ground([6 * leg + 5], leg)()

    kinds["limcon"] = lambda: draw(limcon, lambda nl, nc, n: max(nl) >= 1 and sum(nc) > 0, tries=40)
    kinds["limfoot"] = lambda: draw(limfoot, lambda nl, nc, n: sum(nl) == 1 and sum(nc) > 0, tries=40)
    # cross32: at most 32 rows at substep 0 (over the leg kernel's slots: the 32-row kernel starts it), more than 32 before substep 10;
    # legcross: inside the leg kernel's slots at substep 0, over them -- but never over 32 rows -- before substep 10.  Two kinds, because
    # no side-lying drop does both in one step: the last height that fits a leg's slots (2 contacts, 0.175) is 23 mm above the first with
    # more than 32 rows (0.152), and the contacts stop a robot dropped at up to 16 m/s before it gets there (the oracle, 9 substeps)
    kinds["cross32"] = lambda u, speeds=[1.0, 2.0]: side_drop(speeds.pop(0), u, 0.17, 0.15, lambda nl, nc, n: n <= 32, lambda nl, nc, n: n > 32)
    kinds["legcross"] = lambda u, speeds=[6.0, 8.0]: side_drop(speeds.pop(0), u, 0.20, 0.17, lambda nl, nc, n: fits(nl, nc),
                                                                lambda nl, nc, n: not fits(nl, nc) and n <= 32)

    lim = ["lim1", "limcon", "lim3", "limfoot", "lim6", "limboth", "limcon", "lim12", "lim3", "limcon", "lim6", "limfoot",
           "lim1", "limcon", "lim12", "limboth", "limfoot", "limcon"]
    other = ["stand", "low", "budget", "cross32", "stand", "legcross", "budget", "stand", "low", "budget", "cross32", "low",
             "stand", "budget", "low", "legcross", "budget", "low"]
    # every aligned block of 16: six robots with limits, two in the air, two lying, six others -- no two neighbours of one kind
    block = ["lim", "air", "lying", "other", "lim", "other", "lim", "other", "lim", "air", "lying", "other", "lim", "other", "lim", "other"]
    labels = []
    for i in range(K):
        what = block[i % 16]
        labels.append(lim.pop(0) if what == "lim" else other.pop(0) if what == "other" else what)
    torques = rng.uniform(-0.5, 0.5, (K, 10)) * CTRL
    qs, vs, recs = [], [], []
    for k, lab in enumerate(labels):
        q, v = kinds[lab](torques[k]) if lab in ("cross32", "legcross") else kinds[lab]()
        o.reset(q, v)
        qs.append(q), vs.append(v), recs.append(vec_env3d.state_record(q, v, o.warmstart()))
    return Pool(oracle_mod, np.array(qs), np.array(vs), np.array(recs), labels, torques)


def coverage(pool):
    """What the pool holds, from the oracle alone: row types and counts of every start state and a 10-substep free run under the
    robot's torque."""
    o = pool.oracle_mod.Oracle3D()
    c = dict(rows6=0, rows18=0, limits=0, limits3=0, limits_and_contacts=0, over32=0, rows21_32=0, cross32=0, blocks=[])
    per = []
    for k in range(len(pool)):
        o.reset(pool.q[k], pool.v[k])
        nl, nc, n = rows(o)
        c["rows6"] += n == 6
        c["rows18"] += n == 18
        c["limits"] += sum(nl) > 0
        c["limits3"] += max(nl) >= 3
        c["limits_and_contacts"] += sum(nl) > 0 and sum(nc) > 0
        c["over32"] += n > 32
        c["rows21_32"] += 21 <= n <= 32
        crossed = False
        for _ in range(9):
            o.step_torque(pool.torques[k])
            crossed |= o.nefc > 32
        c["cross32"] += n <= 32 and crossed
        per.append((sum(nl) > 0, n > 32, n == 6))
    for b in range(0, len(pool), 16):
        blk = per[b:b + 16]
        c["blocks"].append(tuple(any(p[i] for p in blk) for i in range(3)))
    return {k: (int(v) if k != "blocks" else v) for k, v in c.items()}


def placements(pool, seed=1):
    """Named placements of test B: index arrays into the pool (robot at position i = pool robot idx[i])."""
    n = len(pool)
    nat = np.arange(n)
    first_lying = pool.labels.index("lying")
    rot = np.roll(nat, -first_lying)
    out = {"natural": nat,
           "by_kind": np.array(sorted(range(n), key=lambda i: (pool.labels[i], i))),
           "permuted": np.random.default_rng(seed).permutation(n),
           "reversed": nat[::-1].copy(),
           "lying_first": rot,
           "lying_first_47": rot[:47]}
    for m in (1, 15, 16, 17, 31, 32, 33, 47):
        out["prefix_%d" % m] = nat[:m]
    return out


class Trajectory:
    """Teacher forcing: per substep t the start records [T][K][80] (state + warm start of the robot's OWN oracle), the torques [T][K][10],
    the oracle's next state q1 [T][K][21], v1 [T][K][20] and its row count nefc [T][K] in that substep."""

    def __init__(self, recs, u, q1, v1, nefc):
        self.recs, self.u, self.q1, self.v1, self.nefc = recs, u, q1, v1, nefc


def teacher_trajectory(pool, substeps=30, redraw=10, seed=2):
    """One oracle per pool robot, `substeps` substeps under random torques within +-CTRL (a new draw every `redraw` substeps).  The
    trajectory does not depend on the kernel under test: every substep of the kernel restarts from the oracle's state."""
    rng = np.random.default_rng(seed)
    n = len(pool)
    os_ = [pool.oracle_mod.Oracle3D() for _ in range(n)]
    for k, o in enumerate(os_):
        o.reset(pool.q[k], pool.v[k])
    tr = Trajectory(np.zeros((substeps, n, 80)), np.zeros((substeps, n, 10)), np.zeros((substeps, n, 21)), np.zeros((substeps, n, 20)),
                    np.zeros((substeps, n), dtype=int))
    for t in range(substeps):
        if t % redraw == 0:
            u = rng.uniform(-1, 1, (n, 10)) * CTRL
        tr.u[t] = u
        for k, o in enumerate(os_):
            q, v = o.state()
            tr.recs[t, k] = vec_env3d.state_record(q, v, o.warmstart())
            o.step_torque(u[k])
            tr.q1[t, k], tr.v1[t, k] = o.state()
            tr.nefc[t, k] = o.nefc
    return tr


def errors(s, tr, t):
    """per robot: |dq| and |dv| / (1 + max |v|) of the records s [K][80] after substep t against the oracle"""
    dq = np.abs(s[:, :21] - tr.q1[t]).max(axis=1)
    dv = np.abs(s[:, 21:41] - tr.v1[t]).max(axis=1) / (1.0 + np.abs(tr.v1[t]).max(axis=1))
    return dq, dv


def bounds(nefc):
    """the tolerances of tests/test_gpu_cassie3d.py by the ORACLE's row count: up to 32 rows (teacher-forced test: 1e-9 in q, 1e-7 in v),
    above (the general kernel, test_many_contacts...: 1e-7 for both); the pool has no robot in the row-cap regime (> 64 rows)"""
    big = np.asarray(nefc) > 32
    return np.where(big, 1e-7, 1e-9), np.where(big, 1e-7, 1e-7)
