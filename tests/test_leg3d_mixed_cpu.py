"""The mixed pool of tests/cassie3d_pool.py on the CPU build of the lane-per-leg Cassie3d kernel source (oracle/leg3d_host.py: 4 emulated lanes
= 2 robots per "wavefront"): the CPU twin of tests/test_gpu_cassie3d_mixed.py.  It pins what the pool holds (coverage, from the oracle alone),
that the SOURCE matches every robot's own oracle in a mixed batch, and that its results do not depend on the placement of a robot in
the batch -- so that a failure of the GPU tests points at the device build or the launch and hand-over code.  Two robots per emulated
wavefront are too few for this test to stand in for the GPU one."""
import json
import os

import numpy as np
import pytest

import cassie3d_pool as P
from leg3d_host import Leg3dHostVec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SUB, STEPS = 10, 3


@pytest.fixture(scope="module")
def pool(oracle_mod):
    with open(os.path.join(ROOT, "tests", "golden", "model3d_kat.json")) as f:
        kat = json.load(f)
    return P.make_pool(oracle_mod, kat, 0)


def run(pool, idx):
    """STEPS steps of N_SUB substeps of the robots idx under their own torques: per step (records, pending, niter)"""
    env = Leg3dHostVec(len(idx))
    env.set_state_host(pool.recs[idx])
    out = []
    for _ in range(STEPS):
        env.step_host(pool.torques[idx], N_SUB)
        out.append((env.get_state_host(), env.pending.copy(), env.niter.copy()))
    return out


@pytest.fixture(scope="module")
def natural(pool):
    return run(pool, np.arange(len(pool)))


def test_pool_coverage(pool):
    """What the mixed tests rely on, counted with the oracle alone."""
    c = P.coverage(pool)
    print("cassie3d pool coverage:", c)
    assert len(pool) == P.K == 48
    assert c["rows6"] >= 2 and c["rows18"] >= 2
    assert c["limits"] >= 8 and c["limits3"] >= 3 and c["limits_and_contacts"] >= 2
    assert c["over32"] >= 4 and c["rows21_32"] >= 2 and c["cross32"] >= 1
    # natural order: every aligned block of 16 holds a robot with limits, one with more than 32 rows and a 6-row one
    assert len(c["blocks"]) == 3 and all(all(b) for b in c["blocks"]), c["blocks"]
    # interleaved: no two neighbours of one kind, several kinds in every run of 16 consecutive robots
    assert all(a != b for a, b in zip(pool.labels, pool.labels[1:]))
    assert all(len(set(pool.labels[i:i + 16])) >= 8 for i in range(len(pool) - 15))


def test_make_pool_is_deterministic(pool, oracle_mod):
    with open(os.path.join(ROOT, "tests", "golden", "model3d_kat.json")) as f:
        again = P.make_pool(oracle_mod, json.load(f), 0)
    assert again.labels == pool.labels and np.array_equal(again.recs, pool.recs) and np.array_equal(again.torques, pool.torques)


def test_every_robot_of_the_mixed_batch_matches_its_own_oracle(pool):
    """Test A of the GPU suite for the robots the CPU build keeps (pending == 0): 30 teacher-forced substeps, each robot against its
    own oracle with the bounds of tests/test_gpu_cassie3d.py by the oracle's row count."""
    tr = P.teacher_trajectory(pool)
    env = Leg3dHostVec(len(pool))
    worst, kept = {}, np.zeros(len(pool), dtype=int)
    for t in range(len(tr.u)):
        env.set_state_host(tr.recs[t])
        env.step_host(tr.u[t], 1)
        s = env.get_state_host()
        keep = env.pending == 0
        kept += keep
        assert np.isfinite(s).all()
        assert np.array_equal(s[~keep, :61], tr.recs[t][~keep, :61])   # the state and warm start of a robot over the capacity are left untouched
        assert np.array_equal(env.nrows[keep], tr.nefc[t][keep])
        dq, dv = P.errors(s, tr, t)
        bq, bv = P.bounds(tr.nefc[t])
        for k in np.flatnonzero(keep):
            w = worst.setdefault(pool.labels[k], [0.0, 0.0])
            w[0], w[1] = max(w[0], dq[k]), max(w[1], dv[k])
        bad = keep & ((dq >= bq) | (dv >= bv))
        assert not bad.any(), (t, [(k, pool.labels[k], dq[k], dv[k], tr.nefc[t, k]) for k in np.flatnonzero(bad)])
    for lab, w in sorted(worst.items()):
        print("leg3d host, mixed batch, %-8s worst |dq| %.2e  |dv|/(1+|v|) %.2e" % (lab, w[0], w[1]))
    lim = np.array([lab.startswith("lim") for lab in pool.labels])
    assert (kept[lim] == len(tr.u)).all()                        # limit rows stay in the packed tier
    assert 0 < kept.sum() < kept.size * len(tr.u)


def test_hand_overs_of_the_mixed_batch(natural, pool):
    """On a 10-substep step some robot leaves the capacity part-way, robots over the budget leave at once, robots with limit rows stay."""
    _, pending, niter = natural[0]
    lab = np.array(pool.labels)
    assert ((pending > 0) & (pending < N_SUB)).any(), pending
    assert (pending[lab == "budget"] == N_SUB).all() and (pending[lab == "lying"] == N_SUB).all()
    assert (pending[[l.startswith("lim") for l in lab]] == 0).all()
    assert len(np.unique(niter[pending == 0])) > 3                # sweep counts differ between lanes: the sweeping mask diverges


def same(ref, got, idx, what):
    for step, ((s0, p0, n0), (s1, p1, n1)) in enumerate(zip(ref, got)):
        for i, k in enumerate(idx):
            assert np.array_equal(s1[i], s0[k]) and p1[i] == p0[k] and n1[i] == n0[k], (what, step, i, k)


@pytest.mark.parametrize("name", ["permuted"] + ["prefix_%d" % m for m in (1, 15, 16, 17, 31, 32, 33, 47)])
def test_results_do_not_depend_on_the_placement(natural, pool, name):
    """Placements (c) and (f) of the GPU test, bit for bit: records, pending and niter after each of 3 steps of 10 substeps."""
    idx = P.placements(pool)[name]
    same(natural, run(pool, idx), idx, name)


def test_seventeen_copies_of_a_robot_give_its_result_in_the_mixed_batch(natural, pool):
    """Placement (g): for every robot k a batch of 17 copies; all equal to robot k's result in the natural order."""
    for k in range(len(pool)):
        idx = np.full(17, k)
        same(natural, run(pool, idx), idx, "copies of %d" % k)
