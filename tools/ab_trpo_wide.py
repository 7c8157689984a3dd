#!/usr/bin/env python3
"""A/B of TRPO's width-128 kernels (csrc/tu_pg_trpo.hip) against the torch operations they replace, alternated in one process:
  fvp        one Fisher-vector product at 524 288 samples (PgFisher: CassiePgFvp + the row sum, vs AnalyticFisher)
  surrogate  the line search's loss and mean KL at 524 288 samples (CassiePgSurrogate vs the torch forward and formulas)
  cg         ten CG iterations with their products (PgFisher.conjugate_gradient vs trpo.conjugate_gradient over AnalyticFisher)
  update     a whole TRPO update (optimize) on one stand batch of 65 536 envs x horizon 8 (fused_fisher True vs False)
Each round: warm-up, then the median of `reps` synchronised repeats per side; odd rounds run the sides in the other order.  Share of
peak: the multiply-adds a product needs by count (forward 26*128 + 128*128 + 32*128 with the output layer padded to 32 rows, tangent
and reverse twice the unpadded layer sizes each; the VJP's second forward pass not counted) times 2 FLOP, over the time, against the 157.3 TFLOP/s FP32 peak of the MI355X.
usage: python tools/ab_trpo_wide.py [rounds] [reps] > profiles/trpo_wide_ab.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import trpo as T  # noqa: E402
from cassierl_amd.trajectory import default_gait  # noqa: E402

PEAK = 157.3e12
LAYERS = 26 * 128 + 128 * 128 + 6 * 128
MAC_FVP = (26 * 128 + 128 * 128 + 32 * 128) + 2 * LAYERS + 2 * LAYERS   # forward (padded), tangent, reverse (G2 / G1 and the weight gradients)
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10


def med_ms(fn, r=None):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(r or reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


N = 524288
torch.manual_seed(1)
pol = T.GaussianMLPPolicy(26, 6, (128, 128), init_std=1.0).cuda()
obs = torch.randn(N, 26, device="cuda") * 0.7
with torch.no_grad():
    old_mean, old_lstd = pol.dist_info(obs)
    act = (old_mean + torch.randn_like(old_mean) * old_lstd.exp()).contiguous()
adv = torch.randn(N, device="cuda")
F, G = T.PgFisher(pol, obs), T.AnalyticFisher(pol, obs)
v = torch.randn(F.NP + 6, device="cuda")
b = torch.randn(F.NP + 6, device="cuda") * 1e-2
old_ls = old_lstd[0].clone()


def torch_sur():
    with torch.no_grad():
        m, ls = pol.dist_info(obs)
        lr = (pol.log_likelihood(act, m, ls) - pol.log_likelihood(act, old_mean, old_lstd)).exp()
        return -(lr * adv).mean(), pol.kl(old_mean, old_lstd, m, ls).mean()


algo = T.make_cassie_trpo(65536, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, batch_size=65536 * 8, hidden_sizes=(128, 128),
                          init_std=1.0)
d = algo.process(algo.collect())
theta0 = T.flat_params(algo.policy).clone()


def update(fused):
    def fn():
        T.set_flat_params(algo.policy, theta0)
        algo.fused_fisher = fused
        algo.optimize(d)
        assert algo.last_fisher_kind == ("pg_fvp" if fused else "analytic")
    return fn


cases = [("fvp", "fused", lambda: F(v), 2 * MAC_FVP * N), ("fvp", "torch", lambda: G(v), 2 * MAC_FVP * N),
         ("surrogate", "fused", lambda: F.surrogate(pol, act, adv, old_mean, old_ls), 2 * (26 * 128 + 128 * 128 + 32 * 128) * N),
         ("surrogate", "torch", torch_sur, 2 * (26 * 128 + 128 * 128 + 32 * 128) * N),
         ("cg", "fused", lambda: F.conjugate_gradient(b, 10, 1e-5), 10 * 2 * MAC_FVP * N),
         ("cg", "torch", lambda: T.conjugate_gradient(lambda p: G(p) + 1e-5 * p, b, 10), 10 * 2 * MAC_FVP * N),
         ("update", "fused", update(True), None), ("update", "torch", update(False), None)]
for r in range(rounds):
    for what, side, fn, flop in (cases if r % 2 == 0 else cases[::-1]):
        ms = med_ms(fn, 3 if what == "update" else None)
        rec = dict(round=r, what=what, side=side, samples=d["obs"].shape[0] if what == "update" else N, median_ms=ms)
        if flop:
            rec.update(gflop=flop / 1e9, share_of_fp32_peak=flop / (ms * 1e-3) / PEAK)
        print(json.dumps(rec), flush=True)
algo.env.close()
