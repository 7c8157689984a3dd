#!/usr/bin/env python3
"""A/B of the fused value path of PPO (csrc/tu_vf.hip: CassieVfGrad + CassiePgAdam per minibatch step) against the torch value path it replaces
(autograd of value.value_loss + torch Adam), in the manner of tools/ab_ppo_cassie3d.py: 16 384 envs x 8 steps = 131 072 samples, 4 epochs x 4
minibatches of 32 768, the policy on its fused kernels on every side.
  update       ppo.PPO.optimize with value="mlp": fused_value on, fused_value off, and beside them the linear-baseline update (no value step at all),
               alternated in one process; per side the median AND the range of `reps` synchronised repeats -- the condition is that the ranges of
               the fused and the torch value path do not touch.  At the Cassie3d shape (45 x 10) and once at the Cassie2d shape (26 x 6);
  vf_*         CassieVfPredict on the batch and CassieVfGrad on a minibatch alone (with its row sum), with and without an index;
  train_ppo    `train_ppo.py --env cassie3d --value mlp --timing` at 16 384 envs x 8 steps in a child process: rollout / update seconds.
One JSON line per measurement.
usage: python tools/ab_ppo_value.py [rounds] [reps] > profiles/ppo_value_ab.jsonl"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import ppo as P  # noqa: E402
from cassierl_amd import trpo as T  # noqa: E402
from cassierl_amd import value as VF  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ENVS, STEPS, HID = 16384, 8, (128, 128)
N, MB = ENVS * STEPS, ENVS * STEPS // 4


def out(**kw):
    print(json.dumps(kw), flush=True)


def timed_us(fn, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return [t * 1e6 for t in ts]


def case(D, A, n, seed=1, jitter=0.05):
    """A policy and a value network off their initial values, and a batch with the likelihood ratios spread around 1 and value residuals of order one."""
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(D, A, HID, init_std=1.0).cuda()
    vf = VF.MLPValueFunction(D, HID).cuda()
    with torch.no_grad():
        for p in list(pol.parameters()) + list(vf.parameters()):
            p.add_(0.1 * torch.randn_like(p))
    obs = torch.randn(n, D, device="cuda") * 0.7
    adv = torch.randn(n, device="cuda")
    with torch.no_grad():
        old_mean, old_ls = pol.dist_info(obs)
        old_mean, old_ls = old_mean.clone(), old_ls[0].clone()
        act = old_mean + torch.randn_like(old_mean) * old_ls.exp()
        for p in pol.parameters():
            p.add_(jitter * torch.randn_like(p))
        v_old = vf(obs)
    y = v_old.double() + torch.randn(n, device="cuda", dtype=torch.float64)
    return pol, vf, dict(obs=obs, act=act, adv=adv, mean=old_mean, log_std=old_ls.expand(n, A), v_old=v_old, vtarget=y)


def ab_update(D, A, family):
    from cassierl_amd.vec_env3d import action_space
    pol, vf, d = case(D, A, N)
    theta0, vtheta0 = T.flat_params(pol).clone(), T.flat_params(vf).clone()
    box = action_space("PD")
    amap = T.NormalizedActions(box.low[:A], box.high[:A], "cuda")   # (optimize never maps an action: the bounds only have to be there)
    kw = dict(batch_size=N, epochs=4, minibatch_size=MB)
    mlp = P.PPO(None, None, pol, vf, ENVS, D, amap, **kw)
    lin = P.PPO(None, None, pol, T.LinearFeatureBaseline(), ENVS, D, amap, **kw)
    d_lin = {k: v for k, v in d.items() if k not in ("v_old", "vtarget")}

    def update(side):
        T.set_flat_params(pol, theta0); T.set_flat_params(vf, vtheta0)
        if side == "linear":
            lin.optimize(d_lin)
            return
        mlp.fused_value = side == "fused_value"
        mlp.optimize(d)
        assert mlp.last_value_kind == ("vf_grad" if side == "fused_value" else "autograd") and mlp.last_grad_kind in ("pg_clip", "pg3d_clip")

    all_us = {"fused_value": [], "torch_value": [], "linear": []}
    for r in range(rounds):
        order = list(all_us) if r % 2 == 0 else list(all_us)[::-1]
        for side in order:
            us = timed_us(lambda: update(side))
            all_us[side] += us
            out(what="update", family=family, obs_dim=D, act_dim=A, samples=N, epochs=4, minibatch=MB, round=r, side=side, median_us=float(np.median(us)),
                min_us=float(min(us)), max_us=float(max(us)), reps=len(us))
    f, t, l = (all_us[k] for k in ("fused_value", "torch_value", "linear"))
    out(what="update_ratio", family=family, fused_value_us=float(np.median(f)), fused_value_range_us=[float(min(f)), float(max(f))], torch_value_us=float(np.median(t)),
        torch_value_range_us=[float(min(t)), float(max(t))], linear_us=float(np.median(l)), ranges_apart=bool(max(f) < min(t)),
        torch_over_fused=float(np.median(t) / np.median(f)),
        value_step_torch_over_fused=float((np.median(t) - np.median(l)) / max(np.median(f) - np.median(l), 1e-9)))
    return vf, d


vf, d = ab_update(45, 10, "cassie3d")

# ---- the launches alone, at the Cassie3d shape
vk = VF.ValueKernels(vf, VF.aligned_value_params(vf))
assert vk.kind == "vf_grad"
vk.set_batch(d["obs"], d["vtarget"])
out(what="vf_predict", rows=N, median_us=float(np.median(timed_us(lambda: vk.predict(d["obs"]), warm=5))))
for m in (MB, N):
    idx = torch.randperm(N, device="cuda")[:m].contiguous()
    for what, fn in (("vf_grad_rows", lambda: vk.grad(None, m=m)), ("vf_grad_idx", lambda: vk.grad(idx))):
        out(what=what, rows=m, median_us=float(np.median(timed_us(fn, warm=5))))
del vk, vf, d

ab_update(26, 6, "cassie2d")

# ---- the trainer (a child process: its own environment and networks)
for extra, side in ((["--value", "mlp"], "mlp fused"), (["--value", "mlp", "--torch-update"], "mlp torch"), ([], "linear fused")):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_ppo.py"), "--env", "cassie3d", "--envs-per-gpu", str(ENVS), "--horizon", str(STEPS), "--n-itr", "6",
                        "--timing"] + extra, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        out(what="train_ppo", side=side, error=p.stderr[-500:])
        continue
    st = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][2:]   # (the first iterations carry the first-call costs)
    out(what="train_ppo --env cassie3d --timing", side=side, envs=ENVS, horizon=STEPS, iterations=len(st), seconds_rollout=float(np.median([s["seconds_rollout"] for s in st])),
        seconds_update=float(np.median([s["seconds_update"] for s in st])), env_steps_per_s=float(np.median([s["env_steps_per_s"] for s in st])))
