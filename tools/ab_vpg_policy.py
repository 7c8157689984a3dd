#!/usr/bin/env python3
"""A/B of the width-128 policy kernels (csrc/tu_pg.hip) against the torch operations they replace, alternated in one process:
  step  the sampler's policy step at 65 536 envs (CassiePgPolicyStep vs convert, 3 GEMMs, 2 tanh, noise, exp, the action map)
  vjp   the policy gradient's J' w at 524 288 samples (CassiePgVjp + the row sum vs autograd through the mean network)
Each round: warm-up, then the median of `reps` synchronised repeats per side.  Share of peak: the multiply-adds the layer shapes need
(2 FLOP each; the forward pass is 26*128 + 128*128 + 6*128 = 20 480 per sample, the VJP forward + backward + weight gradients 3x that)
over the time, against the 157.3 TFLOP/s FP32 peak of the MI355X.  One JSON line per round and side.
usage: python tools/ab_vpg_policy.py [rounds] [reps] > profiles/vpg_ab.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import trpo as T  # noqa: E402
from cassierl_amd import vpg as V  # noqa: E402
from cassierl_amd.vec_env import action_space  # noqa: E402

PEAK = 157.3e12
MAC = 26 * 128 + 128 * 128 + 6 * 128
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20


def med_ms(fn):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


torch.manual_seed(1)
pol = T.GaussianMLPPolicy(26, 6, (128, 128), init_std=1.0).cuda()
box = action_space("PD")
amap = T.NormalizedActions(box.low, box.high, "cuda")
n = 65536
algo = V.VPG(None, None, pol, T.LinearFeatureBaseline(), n, 26, amap)
step = algo._fused_policy_step(torch.device("cuda:0"), torch.float32)
obs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
noise = torch.randn(n, 6, device="cuda")
o32, mean, act = torch.empty(n, 26, device="cuda"), torch.empty(n, 6, device="cuda"), torch.empty(n, 6, device="cuda")


def torch_step():
    a, _, _ = pol.get_actions(obs.to(torch.float32), noise=noise)
    amap(a)


N = 524288
obs_b = torch.randn(N, 26, device="cuda")
w = torch.randn(N, 6, device="cuda") / N
pk = V.PolicyGradKernels(pol, obs_b)
assert pk.kind == "pg_vjp"


def autograd_vjp():
    m, _ = pol.dist_info(obs_b)
    torch.autograd.grad((m * w).sum(), list(pol.parameters()), allow_unused=True)


cases = [("step", "fused", lambda: step(obs, noise, o32, mean, act), 2 * MAC * n), ("step", "torch", torch_step, 2 * MAC * n),
         ("vjp", "fused", lambda: pk._pg_vjp(w), 6 * MAC * N), ("vjp", "torch", autograd_vjp, 6 * MAC * N)]
for r in range(rounds):
    for what, side, fn, flop in (cases if r % 2 == 0 else cases[::-1]):
        ms = med_ms(fn)
        print(json.dumps(dict(round=r, what=what, side=side, samples=n if what == "step" else N, median_ms=ms, gflop=flop / 1e9,
                              share_of_fp32_peak=flop / (ms * 1e-3) / PEAK)), flush=True)
