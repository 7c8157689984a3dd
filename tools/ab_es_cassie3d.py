#!/usr/bin/env python3
"""A/B of ES at the Cassie3d shape, 45 observations and 10 actions (csrc/tu_es3d.hip; not a test).
  1. the policy step of a population of 16 384 environments, every one alive, at both widths: CassieEs3dPolicyStep / CassieEs3dWidePolicyStep
     against es.es_actions_torch on the same table, offsets and observations, alternated in one process; each round a warm-up, then `reps`
     synchronised repeats per side: median, minimum and maximum.  The torch statement materialises the [n, P] weight matrix (1.5 GB in float32
     at width 128, and as much again for eps), so at width 128 it runs over 4 chunks of 4096 environments; the chunking is part of its time.
  2. train_es.py --env cassie3d --timing at 16 384 environments, episodes of at most 16 steps, both widths, each in a child process: rollout and
     update seconds of the iterations after the first.
One JSON line per round, width and side, then one per training iteration.
usage: python tools/ab_es_cassie3d.py [rounds] [reps] > profiles/es_cassie3d_ab.jsonl"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import es as E  # noqa: E402
from cassierl_amd.policy import NormalizedActions  # noqa: E402
from cassierl_amd.vec_env3d import action_space  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
D, A, n, sigma = 45, 10, 16384, 0.02


def timed_us(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts) * 1e6
    return dict(median_us=float(np.median(ts)), min_us=float(ts.min()), max_us=float(ts.max()))


torch.manual_seed(1)
table = E.make_table(1 << 24, 1, "cuda")
box = action_space("PD")
amap = NormalizedActions(box.low, box.high, "cuda")
obs = torch.randn(n, D, dtype=torch.float64, device="cuda")
for hidden, chunk in (((32, 32), n), ((128, 128), 4096)):
    P = E.param_count(D, hidden, A)
    theta = 0.1 * torch.randn(P, device="cuda")
    off = torch.randint(0, table.numel() - P + 1, (n // 2,), device="cuda")
    ek = E.EsKernels(table, n, D, A, amap.low, amap.high, hidden=hidden)
    ek.set_directions(off)

    def fused():
        return ek.policy_step(obs, theta, sigma)

    def statement():
        return torch.cat([E.es_actions_torch(theta, table, off[i // 2:(i + chunk) // 2], sigma, obs[i:i + chunk], None, amap, hidden) for i in range(0, n, chunk)])
    err = (fused() - statement()).abs().max().item()
    sides = [("fused", fused), ("torch", statement)]
    for r in range(rounds):
        for side, fn in (sides if r % 2 == 0 else sides[::-1]):
            print(json.dumps(dict(what="policy step", hidden=list(hidden), envs=n, n_params=P, round=r, side=side, entry=ek.ENTRY["PolicyStep"], reps=reps,
                                  torch_chunk_envs=chunk, max_abs_difference_of_the_sides=err, **timed_us(fn))), flush=True)
    del ek, theta, off
    torch.cuda.empty_cache()
del table, obs
torch.cuda.empty_cache()
for hidden in ("32,32", "128,128"):
    cmd = [sys.executable, os.path.join(ROOT, "train_es.py"), "--env", "cassie3d", "--timing", "--hidden", hidden, "--envs-per-gpu", str(n), "--max-path-length", "16",
           "--n-itr", "4"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.exit("train_es.py failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    st = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    for s in st[1:]:
        print(json.dumps(dict(what="train_es.py --env cassie3d --timing", hidden=hidden, envs=n, max_path_length=16, itr=s["itr"], env_steps=s["env_steps"],
                              policy_step=s["policy_step"], grad=s["grad"], seconds_rollout=s["seconds_rollout"], seconds_update=s["seconds_update"],
                              env_steps_per_s=s["env_steps_per_s"])), flush=True)
