#!/usr/bin/env python3
"""A/B of one DDPG update (csrc/tu_ddpg.hip: critic gradient, apply, actor gradient, apply -- four launches) against the torch statement it
replaces (ddpg.ddpg_update_torch_: gather, four forward passes, two backward passes, two Adam steps, two soft updates), alternated in one
process at batch 32, 4096 and 65 536 on a pool of 1 048 576 rows.  Each round: warm-up, then the median of `reps` synchronised repeats per side
(the synchronisations are around the timed update only).  One JSON line per round, batch and side.
usage: python tools/ab_ddpg_update.py [rounds] [reps] > profiles/ddpg_update_ab.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import ddpg as G  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def med_us(fn):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


torch.manual_seed(1)
D, A, rows = 26, 6, 1 << 20
nets = [G.DeterministicMLPPolicy(D, A).cuda(), G.ContinuousMLPQFunction(D, A).cuda(), G.DeterministicMLPPolicy(D, A).cuda(), G.ContinuousMLPQFunction(D, A).cuda()]
pool = G.ReplayPool(rows, 1, D, A, "cuda")
pool.obs.normal_(0, 0.7); pool.nobs.normal_(0, 0.7); pool.act.uniform_(-1, 1); pool.rew.normal_(0, 0.01)
pool.term.copy_((torch.rand(rows, device="cuda") < 0.01).float())
pool.size = rows
k = G.DdpgKernels(*nets)
adam = {s: (G.new_adam(nets[0]), G.new_adam(nets[1])) for s in ("fused", "torch")}
for r in range(rounds):
    for batch in (32, 4096, 65536):
        idx = torch.randint(0, rows, (batch,), device="cuda")
        sides = [("fused", lambda: k.update(pool, idx, 0.99, 1e-3, 1e-4, 1e-3, *adam["fused"])),
                 ("torch", lambda: G.ddpg_update_torch_(*nets, *adam["torch"], pool.sample(idx), 0.99, 1e-3, 1e-4, 1e-3))]
        for side, fn in (sides if r % 2 == 0 else sides[::-1]):
            print(json.dumps(dict(round=r, batch=batch, side=side, median_us=med_us(fn))), flush=True)
