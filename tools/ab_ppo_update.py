#!/usr/bin/env python3
"""A/B of one PPO update (ppo.PPO.optimize: per minibatch the clip-gradient launch of csrc/tu_ppo.hip, the row sum and CassiePgAdam) against the
forced-torch update (autograd of ppo.ppo_loss + torch Adam), alternated in one process on 65 536 x 8 = 524 288 samples, 4 epochs, both policy
widths, minibatch 65 536 (8 per epoch) and 524 288 (the batch).  Each round: warm-up, then the median of `reps` synchronised repeats per side
(the synchronisations are around the timed update only).  The last lines time the clip-gradient launch alone, with and without an index, beside
the VJP launch of the same width on the same rows.  One JSON line per measurement.
usage: python tools/ab_ppo_update.py [rounds] [reps] > profiles/ppo_update_ab.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import ppo as P  # noqa: E402
from cassierl_amd import trpo as T  # noqa: E402
from cassierl_amd import vpg as V  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N, D, A = 65536 * 8, 26, 6


def med_us(fn, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def case(hidden):
    torch.manual_seed(1)
    pol = T.GaussianMLPPolicy(D, A, hidden, init_std=1.0).cuda()
    obs = torch.randn(N, D, device="cuda") * 0.7
    adv = torch.randn(N, device="cuda")
    with torch.no_grad():
        old_mean, old_ls = pol.dist_info(obs)
        old_mean, old_ls = old_mean.clone(), old_ls[0].clone()
        act = old_mean + torch.randn_like(old_mean) * old_ls.exp()
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return pol, dict(obs=obs, act=act, adv=adv, mean=old_mean, log_std=old_ls.expand(N, A))


for hidden in ((32, 32), (128, 128)):
    pol, d = case(hidden)
    theta0 = T.flat_params(pol).clone()
    for mb in (65536, N):
        algo = P.PPO(None, None, pol, T.LinearFeatureBaseline(), 65536, D, None, batch_size=N, epochs=4, minibatch_size=mb)

        def update(fused):
            T.set_flat_params(pol, theta0)
            algo.fused_grad = algo.fused_adam = fused
            algo.optimize(d)

        for r in range(rounds):
            sides = [("fused", lambda: update(True)), ("torch", lambda: update(False))]
            for side, fn in (sides if r % 2 == 0 else sides[::-1]):
                print(json.dumps(dict(what="update", hidden=hidden[0], samples=N, epochs=4, minibatch=mb, round=r, side=side, median_us=med_us(fn))), flush=True)
    # the launch alone: clip gradient (rows 0 .. m - 1, and through a permutation) beside the VJP of the same width on m rows
    T.set_flat_params(pol, theta0)
    ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), d["obs"], d["act"], d["adv"], d["mean"], d["log_std"], 0.2, 0.0)
    for m in (65536, N):
        idx = torch.randperm(N, device="cuda")[:m].contiguous()
        pk = V.PolicyGradKernels(pol, d["obs"][:m].contiguous())
        w = torch.randn(m, A, device="cuda") / m
        vjp = (lambda: pk._vjp(w)) if pk._vjp is not None else None
        for what, fn in (("clip_grad_rows", lambda: ck.grad(None, m=m)), ("clip_grad_idx", lambda: ck.grad(idx)), ("vjp", vjp)):
            if fn is not None:   # (each includes its row sum; the VJP reads its cotangent from memory)
                print(json.dumps(dict(what=what, kind=ck.kind, hidden=hidden[0], rows=m, median_us=med_us(fn, warm=5))), flush=True)
