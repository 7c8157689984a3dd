#!/usr/bin/env python3
"""A/B of the terrain library (not a test): the stand env with random PD targets (bench.py's terrain_stand_pd_random workload) on
  single  one 3 cm rolling relief under everybody (CassieVecSetHeightField: a library of one)
  mod16   16 reliefs, environment i on field i % 16
  rand16  16 reliefs, ids drawn by terrain.assign_terrains
timed with HIP events around `--steps` Env.steps after `--warmup`, the configurations alternated over `--rounds` rounds so that clock
drift hits every one alike.  One JSON line per measurement, then one summary line (median per configuration, ratio to single).
usage: python tools/ab_terrain_library.py [--envs 65536] [--rounds 3] [--warmup 60] [--steps 40]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reliefs(k):
    xs = np.linspace(-10.0, 10.0, 2001)
    base = [np.tile(0.015 * (1.0 - np.cos(2.0 * np.pi * xs / 1.5)), (64, 1))]   # bench.py's relief is field 0
    for j in range(1, k):
        amp, wl, ph = 0.010 + 0.0004 * j, 1.0 + 0.06 * j, 0.35 * j
        base.append(np.tile(amp * (1.0 - np.cos(2.0 * np.pi * xs / wl + ph)), (64, 1)))
    return base


def measure(cfg, n, warmup, steps, fields):
    import torch
    from cassierl_amd import rollout as R
    from cassierl_amd import terrain as T
    from cassierl_amd.vec_env import CassieVecEnv, action_space
    env = CassieVecEnv(n, kind="stand", control_mode="PD", n_substeps=10, auto_reset=True, device=0)
    env.use_torch_stream()
    ids = torch.arange(n, device="cuda")
    if cfg == "single":
        env.set_heightfield(fields[0], 10.0, 10.0)
    else:
        env.set_terrain_library(fields, (10.0, 10.0))
        tid = (ids % len(fields)).to(torch.int32) if cfg == "mod16" else T.assign_terrains(3, ids, len(fields)).cuda()
        env.set_terrain_ids(tid)
    box = action_space("PD")
    out = env.alloc()
    env.reset(out)
    for t in range(warmup):
        env.step(R.random_actions(2, ids, t, box.low, box.high), out)
    acts = [R.random_actions(2, ids, warmup + t, box.low, box.high) for t in range(steps)]
    env.reset_counters()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for t in range(steps):
        env.step(acts[t], out)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / steps
    c = env.counters()
    q, v = env.get_state_host()
    row = dict(config=cfg, envs=n, steps=steps, warmup=warmup, ms_per_step=ms, env_steps_per_s=n / ms * 1e3, cleanup_frac=c["cleanup_frac"],
               k1_frac=c["k1_frac"], nonfinite_resets=c["nonfinite_resets"], finite=bool(np.isfinite(q).all() and np.isfinite(v).all()),
               first_tier=env.tier_info()["first_tier"])
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--configs", default="single,mod16,rand16")
    args = ap.parse_args()
    fields = reliefs(16)
    cfgs = args.configs.split(",")
    rows = []
    for r in range(args.rounds):
        for cfg in (cfgs if r % 2 == 0 else cfgs[::-1]):
            row = measure(cfg, args.envs, args.warmup, args.steps, fields)
            row["round"] = r
            print(json.dumps(row), flush=True)
            rows.append(row)
    med = {c: float(np.median([x["env_steps_per_s"] for x in rows if x["config"] == c])) for c in cfgs}
    spread = {c: [float(min(x["env_steps_per_s"] for x in rows if x["config"] == c)), float(max(x["env_steps_per_s"] for x in rows if x["config"] == c))]
              for c in cfgs}
    summary = dict(summary=True, envs=args.envs, median_env_steps_per_s=med, min_max=spread)
    if "single" in med:
        summary["ratio_to_single"] = {c: med[c] / med["single"] for c in cfgs}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
