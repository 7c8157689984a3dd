#!/usr/bin/env python3
"""A/B of the ES kernels (csrc/tu_es.hip) against the torch statements they replace (cassierl_amd/es.py), alternated in one process:
  step  the policy step of a population of 65 536 environments, every one alive (CassieEsPolicyStep vs es_actions_torch: the [n, P] weight
        matrix, three bmm, two tanh, the action map)
  grad  the weighted sum of the 32 768 directions (CassieEsGrad + the row sum vs es_grad_torch)
Each round: warm-up, then the median of `reps` repeats per side; a repeat is `batch` calls enqueued back to back between two synchronisations, divided
by `batch`, so that the launch and synchronisation overhead of a 0.07 ms kernel is not part of the figure (`batch` = 1 gives the cost of one
synchronised call).  Both kernels are bound by the table read, P floats per direction (277 MB at 65 536 environments and P = 2118):
`table_gb_per_s` is that figure over the time -- the table is 64 MB and lives in the Infinity Cache,
so this is not an HBM rate.  One JSON line per round and side.  With the hidden sizes 128,128 the policy is the 128 x 128 one (P = 20 742,
2.72 GB of table reads per step at 65 536 environments), the fused step is CassieEsWidePolicyStep (csrc/tu_es_wide.hip) and the torch side is
es_actions_torch(..., hidden_sizes=(128, 128)), whose [n, P] temporaries are 5.4 GB each at 65 536 environments.
usage: python tools/ab_es_policy.py [rounds] [reps] [envs] [batch] [hidden] > profiles/es_policy_ab.jsonl
       python tools/ab_es_policy.py 3 20 65536 20 128,128 > profiles/es_wide_policy_ab.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import es as E  # noqa: E402
from cassierl_amd import trpo as T  # noqa: E402
from cassierl_amd.vec_env import action_space  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 20
hidden = tuple(int(x) for x in sys.argv[5].split(",")) if len(sys.argv) > 5 else (32, 32)
D, A, SIGMA = 26, 6, 0.02


def med_ms(fn):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(batch):
            fn()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) / batch)
    return float(np.median(ts)) * 1e3


torch.manual_seed(1)
dev = torch.device("cuda:0")
pol = T.GaussianMLPPolicy(D, A, hidden, init_std=1.0).to(dev)
theta = T.flat_params(pol.mean_net).contiguous()
box = action_space("PD")
amap = T.NormalizedActions(box.low, box.high, dev)
table = E.make_table(1 << 24, 7, dev)
ek = E.EsKernels(table, n, D, A, amap.low, amap.high, hidden=hidden)
g = torch.Generator().manual_seed(3)
offsets = torch.randint(0, table.numel() - ek.P + 1, (n // 2,), generator=g).to(dev)
ek.set_directions(offsets)
obs = torch.randn(n, D, dtype=torch.float64, generator=g).to(dev)
alive = torch.ones(n, dtype=torch.uint8, device=dev)
w = torch.randn(n // 2, generator=g).to(dev)
table_bytes = 4.0 * ek.P * (n // 2)

cases = [("step", "fused", lambda: ek.policy_step(obs, theta, SIGMA, alive)),
         ("step", "torch", lambda: E.es_actions_torch(theta, table, offsets, SIGMA, obs, alive, amap, hidden)),
         ("grad", "fused", lambda: ek.grad(w)),
         ("grad", "torch", lambda: E.es_grad_torch(table, offsets, w, ek.P))]
for r in range(rounds):
    for what, side, fn in (cases if r % 2 == 0 else cases[::-1]):
        ms = med_ms(fn)
        print(json.dumps(dict(round=r, what=what, side=side, hidden=list(hidden), envs=n, directions=n // 2, n_params=ek.P, calls_per_sync=batch, median_ms=ms, table_mb=table_bytes / 1e6,
                              table_gb_per_s=table_bytes / (ms * 1e-3) / 1e9)), flush=True)
