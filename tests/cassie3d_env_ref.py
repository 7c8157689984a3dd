"""Reference side of the Cassie3d environment-layer tests (tests/test_cassie3d_env_cpu.py on the CPU build of the sources,
tests/test_gpu_cassie3d_env.py on the GPU): the PD law and the observation / reward / done definition of include/cassie3d_vec.h restated in
numpy on top of the ORACLE alone (Oracle3D.step_torque, Oracle3D.site_pos), and the g++ builds of the harnesses under tests/host/.
Nothing here depends on the code under test."""
import os
import subprocess

import numpy as np

import cassie3d_pool as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
NOBS = 45
ACT_DOF = np.array([6, 7, 8, 9, 11, 13, 14, 15, 16, 18])   # c3_act_dof: abduction, yaw, hip, knee, toe per leg; the hinge angle is qpos[dof + 1]
KP, KD = np.full(10, 10.0), np.full(10, 5.0)               # the defaults of the contract
FOOT_SITES = (2, 3, 4, 5)                                   # left_contact_front / rear, right_contact_front / rear (cassie3d_stiff.xml)


def pd_command(q, v, target, kp=KP, kd=KD):
    """kp (target - q) - kd v of the ten actuators, pre-clamp, from the state (q, v)"""
    return kp * (target - q[ACT_DOF + 1]) - kd * v[ACT_DOF]


def start(oracle, rec):
    """the oracle at the state AND warm start of the record: where the solver stops at its iteration limit the step depends on the
    warm start, and the one in a pool record depends on what the pool's oracle solved before (Oracle3D.reset keeps its last one)"""
    oracle.set_state_raw(rec[:21], rec[21:41], rec[41:61])


def pd_targets(pool, seed=5):
    """the robot's actuated angles + U(-0.2, 0.2)"""
    rng = np.random.default_rng(seed)
    return pool.q[:, ACT_DOF + 1] + rng.uniform(-0.2, 0.2, (len(pool), 10))


def pd_teacher_trajectory(pool, targets, substeps=30):
    """cassie3d_pool.teacher_trajectory with the torque of every substep computed by the PD law from the ORACLE's own state at the start
    of that substep (tr.u holds those commands)."""
    n = len(pool)
    os_ = [pool.oracle_mod.Oracle3D() for _ in range(n)]
    for k, o in enumerate(os_):
        start(o, pool.recs[k])
    tr = P.Trajectory(np.zeros((substeps, n, 80)), np.zeros((substeps, n, 10)), np.zeros((substeps, n, 21)), np.zeros((substeps, n, 20)),
                      np.zeros((substeps, n), dtype=int))
    for t in range(substeps):
        for k, o in enumerate(os_):
            q, v = o.state()
            tr.recs[t, k] = P.vec_env3d.state_record(q, v, o.warmstart())
            tr.u[t, k] = pd_command(q, v, targets[k])
            o.step_torque(tr.u[t, k])
            tr.q1[t, k], tr.v1[t, k] = o.state()
            tr.nefc[t, k] = o.nefc
    return tr


class TenSubsteps:
    """Ten oracle substeps from the pool states towards `targets`: q_pd, v_pd with the PD command of EVERY substep, q_held with the first
    substep's command held for all ten; saturated[k]: every command of robot k was beyond its actuator's range at every substep with one
    sign (the clamp then makes the two runs the same run, so the robot cannot tell a held torque from the law)."""

    def __init__(self, pool, targets, n_sub=10):
        n = len(pool)
        self.q_pd, self.v_pd, self.q_held = np.zeros((n, 21)), np.zeros((n, 20)), np.zeros((n, 21))
        self.saturated = np.zeros(n, dtype=bool)
        self.saturated_frac = np.zeros(n)
        o = pool.oracle_mod.Oracle3D()
        for k in range(n):
            start(o, pool.recs[k])
            side = []
            for _ in range(n_sub):
                q, v = o.state()
                u = pd_command(q, v, targets[k])
                side.append(np.sign(u) * (np.abs(u) >= P.CTRL))
                o.step_torque(u)
            self.q_pd[k], self.v_pd[k] = o.state()
            side = np.array(side)
            self.saturated[k] = bool(np.all(side != 0) and np.all(side == side[0]))
            self.saturated_frac[k] = np.mean(side != 0)
            start(o, pool.recs[k])
            u0 = pd_command(pool.q[k], pool.v[k], targets[k])
            for _ in range(n_sub):
                o.step_torque(u0)
            self.q_held[k] = o.state()[0]
        self.held_gap = np.abs(self.q_held - self.q_pd).max(axis=1)

    def rel_errors(self, s):
        """the north-star measure of tests/test_gpu_cassie3d.py for the records s [n][80] against the per-substep run"""
        eq = np.abs(s[:, :21] - self.q_pd).max(axis=1) / (1.0 + np.abs(self.q_pd).max(axis=1))
        ev = np.abs(s[:, 21:41] - self.v_pd).max(axis=1) / (1.0 + np.abs(self.v_pd).max(axis=1))
        return np.maximum(eq, ev)


def feet_rel(oracle, q):
    """[2][3]: mean of a leg's two contact sites minus the pelvis position, world axes, from the oracle's site positions"""
    s = [np.asarray(oracle.site_pos(q, i), dtype=np.float64) for i in FOOT_SITES]
    return np.array([0.5 * (s[0] + s[1]) - q[:3], 0.5 * (s[2] + s[3]) - q[:3]])


def observation(oracle, rec):
    q, v = rec[:21], rec[21:41]
    return np.concatenate([q[2:3], q[3:7], q[7:21], v[0:3], v[3:6], v[6:20], feet_rel(oracle, q).ravel()])


def reward(obs, action):
    fx, fy = 0.5 * (obs[39] + obs[42]), 0.5 * (obs[40] + obs[43])
    return 1.0 - 2.0 * (0.9 - obs[0]) ** 2 - 2.0 * fx ** 2 - 2.0 * fy ** 2 - 0.001 * float(np.dot(action, action))


def reference(oracle, recs, actions):
    """(obs [n][45], reward [n], done [n]) of finite records by the contract"""
    obs = np.array([observation(oracle, r) for r in recs])
    rew = np.array([reward(o, a) for o, a in zip(obs, actions)])
    return obs, rew, recs[:, 2] < 0.5


COPIED = np.r_[0:39]   # observation entries copied from the record (everything but the feet)


def gxx(out, src, *flags):
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-ffp-contract=off", "-Wno-psabi"] + list(flags) + ["-o", out, os.path.join(HOST, src)]
    subprocess.check_call(cmd)
    return out
