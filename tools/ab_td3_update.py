#!/usr/bin/env python3
"""A/B of one TD3 update (csrc/tu_td3.hip: both critics' gradient, both critics' apply -- two launches; a delayed update adds DDPG's actor gradient
and apply) against the torch statement it replaces (td3.td3_update_torch_), alternated in one process at batch 32, 4096 and 65 536 on a pool of
1 048 576 rows, for an update that leaves the actor alone and for a delayed one.  Each round: warm-up, then the median of `reps` synchronised
repeats per side (the synchronisations are around the timed update only).  One JSON line per round, batch, kind of update and side; run
tools/ab_ddpg_update.py in the same session for DDPG's figure.
usage: python tools/ab_td3_update.py [rounds] [reps] > profiles/td3_update_ab.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import ddpg as G  # noqa: E402
from cassierl_amd import td3 as D3  # noqa: E402

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
nets = [c(D, A).cuda() for c in (G.DeterministicMLPPolicy, G.ContinuousMLPQFunction, G.ContinuousMLPQFunction) * 2]   # actor, qf1, qf2 and their targets
pool = G.ReplayPool(rows, 1, D, A, "cuda")
pool.obs.normal_(0, 0.7); pool.nobs.normal_(0, 0.7); pool.act.uniform_(-1, 1); pool.rew.normal_(0, 0.01)
pool.term.copy_((torch.rand(rows, device="cuda") < 0.01).float())
pool.size = rows
k = D3.Td3Kernels(*nets)
adam = {s: [G.new_adam(n) for n in nets[:3]] for s in ("fused", "torch")}
for r in range(rounds):
    for batch in (32, 4096, 65536):
        idx = torch.randint(0, rows, (batch,), device="cuda")
        eps2 = torch.randn(batch, A, device="cuda")
        for with_actor in (False, True):
            sides = [("fused", lambda: k.update(pool, idx, eps2, with_actor, 0.2, 0.5, 0.99, 3e-4, 3e-4, 5e-3, *adam["fused"])),
                     ("torch", lambda: D3.td3_update_torch_(*nets, *adam["torch"], pool.sample(idx), eps2, 1 if with_actor else 0, 2, 0.2, 0.5, 0.99, 3e-4, 3e-4, 5e-3))]
            for side, fn in (sides if r % 2 == 0 else sides[::-1]):
                print(json.dumps(dict(round=r, batch=batch, delayed=with_actor, side=side, median_us=med_us(fn))), flush=True)
