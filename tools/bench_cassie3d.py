#!/usr/bin/env python3
"""Throughput of BASELINE.json configs[4] (not the bench line, not a test): 16 384 Cassie3d envs, torque mode,
actions ~ U(-ctrlrange, +ctrlrange) redrawn every env-step (counter-based RNG), 10 substeps per env-step.
Every `--episode` env-steps all environments are put back on the standing pose (there is no reference Cassie3d
environment, hence no reference termination rule).
--env: the environment layer instead (Cassie3dVecEnv: PD targets ~ U(joint ranges) or torques, observation / reward / done and auto-reset
inside the step); the same number of torque-mode Cassie3dVecStep calls is timed beside it on a second handle."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import rollout as R  # noqa: E402
from cassierl_amd.vec_env3d import Cassie3dVec, Cassie3dVecEnv, CTRL_RANGE  # noqa: E402


def bench_env(a):
    """Env.step of the environment layer, timed with HIP events on its stream, beside the bare torque-mode physics step"""
    env = Cassie3dVecEnv(a.envs, control_mode=a.mode, n_substeps=10, auto_reset=True)
    env.use_torch_stream()
    box = env.action_space
    ids = torch.arange(a.envs, device="cuda")
    acts = [R.random_actions(1, ids, t, box.low, box.high) for t in range(8)]
    out = env.alloc()
    env.reset(out)
    for t in range(5):
        env.step(acts[t % 8], out)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for t in range(a.steps):
        env.step(acts[t % 8], out)
    ev[1].record()
    torch.cuda.synchronize()
    ms_env = ev[0].elapsed_time(ev[1]) / a.steps
    cnt = env.counters()
    finite = bool(torch.isfinite(out["obs"]).all() and torch.isfinite(out["reward"]).all())
    env.close()
    phys = Cassie3dVec(a.envs)
    tq = [R.random_actions(1, ids, t, -CTRL_RANGE, CTRL_RANGE) for t in range(8)]
    for t in range(5):
        phys.step(tq[t % 8], 10)
    phys.reset()
    ms_phys = 0.0
    for t0 in range(0, a.steps, a.episode):
        for t in range(min(a.episode, a.steps - t0)):
            ms_phys += phys.time_steps(tq[(t0 + t) % 8], 10, 1)
        phys.reset()
    ms_phys /= a.steps
    phys.close()
    print(json.dumps(dict(config="Cassie3d environment layer, %s mode, auto-reset" % a.mode, n_envs=a.envs, steps=a.steps, ms_per_env_step=ms_env,
                          env_steps_per_s=a.envs / (ms_env * 1e-3), ms_per_torque_physics_step=ms_phys, done_per_step=cnt["done"] / (a.steps + 5.0),
                          guard=cnt["guard"], leg_handover_frac=cnt["leg_handover_frac"], finite=finite)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--episode", type=int, default=40)
    ap.add_argument("--cpu-baseline", action="store_true", help="also time oracle/liboracle3d.so on the host cores (OpenMP over envs)")
    ap.add_argument("--env", action="store_true", help="time Cassie3dVecEnv.step (observation, reward, done, auto-reset) instead")
    ap.add_argument("--mode", default="PD", choices=["PD", "Torque"], help="control mode of --env")
    a = ap.parse_args()
    if a.env:
        return bench_env(a)
    env = Cassie3dVec(a.envs)
    ids = torch.arange(a.envs, device="cuda")
    acts = [R.random_actions(1, ids, t, -CTRL_RANGE, CTRL_RANGE) for t in range(8)]
    for t in range(5):
        env.step(acts[t % 8], 10)
    env.reset()
    env.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tot_ms = 0.0
    for t0 in range(0, a.steps, a.episode):
        k = min(a.episode, a.steps - t0)
        for t in range(k):  # timed with HIP events on the library's own stream
            tot_ms += env.time_steps(acts[(t0 + t) % 8], 10, 1)
        env.reset()
    s = env.get_state_host()
    cnt = env.counters()
    out = dict(leg_handover_frac=cnt.get("leg_handover_frac"), general_frac=cnt.get("general_frac"), config="configs[4]: Cassie3d torque-mode random rollout", n_envs=a.envs, steps=a.steps, ms_per_step=tot_ms / a.steps,
               env_steps_per_s=a.envs * a.steps / (tot_ms * 1e-3), physics_substeps_per_s=10 * a.envs * a.steps / (tot_ms * 1e-3),
               overflowed_envs=int((s[:, 74] != 0).sum()), finite=bool(np.isfinite(s).all()))
    if a.cpu_baseline:
        import ctypes as ct
        import time
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle_py as O
        cores = len(os.sched_getaffinity(0))
        n_cpu, steps_cpu = 4 * cores, 3
        os_ = [O.Oracle3D() for _ in range(n_cpu)]
        arr = (ct.c_void_p * n_cpu)(*[o.h for o in os_])
        u = np.ascontiguousarray(acts[0][:n_cpu].cpu().numpy())
        L = O.lib3d()
        L.orc_batch_step_torque(arr, n_cpu, u.ctypes.data_as(O.dp), 10, cores)  # warm-up
        t0 = time.perf_counter()
        for t in range(steps_cpu):
            u = np.ascontiguousarray(acts[(t + 1) % 8][:n_cpu].cpu().numpy())
            L.orc_batch_step_torque(arr, n_cpu, u.ctypes.data_as(O.dp), 10, cores)
        dt = time.perf_counter() - t0
        out["cpu_baseline"] = dict(value=n_cpu * steps_cpu / dt, unit="env-steps/s", cores=cores, kind="port",
                                   sample="%d envs x %d env-steps (10 substeps each) in %.1f s, OpenMP over envs" % (n_cpu, steps_cpu, dt))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
