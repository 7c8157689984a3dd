#!/usr/bin/env python3
"""A/B of SAC at the Cassie3d shape, 45 observations and 10 actions (csrc/tu_sac3d.hip, whose kernels are csrc/sac_kernels.h's at <45, 10>; not a test).
  1. one update, the five launches against sac.sac_update_torch_, alternated in one process at batch 4096 and 65 536 on a pool of 1 048 576
     rows, as tools/ab_sac_update.py does for 26 x 6: each round warm-up, then the median of `reps` synchronised repeats per side;
  2. train_sac.py --env cassie3d --timing at 16 384 environments, batch 16 384, with and without --torch-update, each in a child process: the
     seconds of the second epoch of 8 vector steps (the first fills the pool and warms up).
One JSON line per round, batch and side, then one per training run.  With --update-only part 2 is left out (an A/B of two builds of the library,
CASSIE2D_LIB, times part 1 in alternated processes).
usage: python tools/ab_sac_cassie3d.py [rounds] [reps] [--update-only] > profiles/sac_cassie3d_ab.jsonl"""
import copy
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import ddpg as G  # noqa: E402
from cassierl_amd import sac as S  # noqa: E402

update_only = "--update-only" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--update-only"]
rounds = int(argv[0]) if len(argv) > 0 else 3
reps = int(argv[1]) if len(argv) > 1 else 20


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
D, A, rows = 45, 10, 1 << 20
pool = G.ReplayPool(rows, 1, D, A, "cuda")
pool.obs.normal_(0, 0.7); pool.nobs.normal_(0, 0.7); pool.act.uniform_(-1, 1); pool.rew.normal_(0, 0.01)
pool.term.copy_((torch.rand(rows, device="cuda") < 0.01).float())
pool.size = rows
first = [S.SquashedGaussianMLPPolicy(D, A).cuda()] + [G.ContinuousMLPQFunction(D, A).cuda() for _ in range(4)]   # actor, qf1, qf2, their targets
SIDES = ("fused", "torch")
nets = {s: [copy.deepcopy(m) for m in first] for s in SIDES}   # each side steps its own copy of the same networks, log_alpha and Adam states
la = {s: torch.zeros(1, device="cuda") for s in SIDES}
k = S.SacKernels(*nets["fused"], la["fused"])
assert k.is3d
adam = {s: (G.new_adam(nets[s][0]), G.new_adam(nets[s][1]), G.new_adam(nets[s][2]), S.new_alpha_adam(la[s])) for s in SIDES}
for r in range(rounds):
    for batch in (4096, 65536):
        idx = torch.randint(0, rows, (batch,), device="cuda")
        noise = torch.randn(2, batch, A, device="cuda")
        sides = [("fused", lambda: k.update(pool, idx, noise[0], noise[1], 0.99, 3e-4, 3e-4, 3e-4, 5e-3, -float(A), *adam["fused"])),
                 ("torch", lambda: S.sac_update_torch_(*nets["torch"], la["torch"], *adam["torch"], pool.sample(idx), noise[0], noise[1], 0.99, 3e-4, 3e-4, 3e-4, 5e-3,
                                                      -float(A)))]
        for side, fn in (sides if r % 2 == 0 else sides[::-1]):
            print(json.dumps(dict(what="update", round=r, batch=batch, side=side, median_us=med_us(fn))), flush=True)
if update_only:
    sys.exit(0)
del pool, nets, k
torch.cuda.empty_cache()
n = 16384
for extra in ([], ["--torch-update"]):
    cmd = [sys.executable, os.path.join(ROOT, "train_sac.py"), "--env", "cassie3d", "--timing", "--envs-per-gpu", str(n), "--batch-size", str(n), "--pool-size", str(n * 16),
           "--min-pool-size", str(n), "--epoch-length", "8", "--n-epochs", "3"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit("train_sac.py failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    st = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    for s in st[1:]:
        print(json.dumps(dict(what="train_sac.py --env cassie3d --timing", envs=n, batch=n, epoch_length=8, torch_update=bool(extra), itr=s["itr"], updates=s["updates"],
                              update_kind=s["update_kind"], seconds_epoch=s["seconds_epoch"], env_steps_per_s=s["env_steps_per_s"])), flush=True)
