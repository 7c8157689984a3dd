#!/usr/bin/env python3
"""A/B of the HOST side of two builds of the extension (not a test): the kernels of both are the same objects, so what can differ is launch
overhead.  For each library on the command line, in the order given (alternate them: A B A B ...), one fresh process each for
  headline  -- `bench.py --gpus 1` (65 536 walk / PD envs; ms per Env.step by the host clock around the timed region), and
  configs2  -- bench.py's configs[2] row (65 536 stand envs, OSC: ten controller + physics launches per Env.step, where launch overhead counts tenfold).
One JSON line per run goes to the output file, then per library and workload the median, minimum and maximum of its runs.
usage: python tools/ab_cabi_host.py OUT.jsonl libA.so libB.so libA.so libB.so ..."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS2 = r'''
import json, sys
sys.path.insert(0, %r)
import numpy as np, torch
import bench
from cassierl_amd import rollout as R
from cassierl_amd.trajectory import default_gait
g, n = default_gait(), 65536
ids = torch.arange(n, device="cuda:0")
lo, hi = np.array([-2.0, -2.0, -2.0, 0.0, -2.0, 0.0, -2.0]), np.full(7, 2.0)
row = bench.run_env_workload("configs[2]_stand_osc_in_loop", n, "stand", "OSC", 0, dict(time=g.time, qpos=g.qpos), 20, 30,
                             lambda t: R.random_actions(4, ids, t, lo, hi), "")
print("ROW " + json.dumps(dict(ms_per_step=row["ms_per_step"], finite=row["finite"], qp_mean=row["qp_iterations_per_substep"]["mean"])))
''' % ROOT


def run(cmd, lib, tag):
    p = subprocess.run(cmd, env=dict(os.environ, CASSIE2D_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=240, cwd=ROOT)
    if p.returncode != 0:
        sys.exit("%s with %s failed (%d): %s" % (tag, lib, p.returncode, p.stderr[-1500:]))
    return p.stdout


out_path, libs = sys.argv[1], sys.argv[2:]
rows = []
with open(out_path, "w") as out:
    for k, lib in enumerate(libs):
        line = json.loads([l for l in run([sys.executable, "bench.py", "--gpus", "1", "--steps", "150", "--warmup", "50"], lib, "headline").splitlines() if l.startswith("{")][-1])
        rows.append(dict(run=k, lib=lib, workload="headline", ms_per_step=line["ms_per_step"], returns_checksum=line["returns_checksum"],
                         first_tier=line["config"]["first_tier"], duo_workspace_MB=line["config"]["duo_workspace_MB"]))
        r2 = json.loads([l for l in run([sys.executable, "-c", CONFIGS2], lib, "configs2").splitlines() if l.startswith("ROW ")][-1][4:])
        rows.append(dict(run=k, lib=lib, workload="configs2", **r2))
        for r in rows[-2:]:
            out.write(json.dumps(r) + "\n")
            out.flush()
            print(json.dumps(r), flush=True)
    for w in ("headline", "configs2"):
        for lib in dict.fromkeys(libs):
            m = [r["ms_per_step"] for r in rows if r["workload"] == w and r["lib"] == lib]
            s = dict(summary=w, lib=lib, runs=len(m), median=float(np.median(m)), min=min(m), max=max(m))
            out.write(json.dumps(s) + "\n")
            print(json.dumps(s), flush=True)
