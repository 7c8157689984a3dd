#!/usr/bin/env python3
"""A/B of PPO's fused path at the Cassie3d shape (45 observations, 10 actions, 128 x 128: csrc/tu_pg3d.hip, CassiePgAdam) against the torch path it
replaces, in the manner of tools/ab_ppo_update.py: 16 384 envs x 8 steps = 131 072 samples, 4 epochs x 4 minibatches of 32 768.
  update       ppo.PPO.optimize, fused against forced-torch (autograd of ppo_loss + torch Adam), alternated in one process;
  policy_step  CassiePg3dPolicyStep against the torch operations of TRPO.collect (float32 view, get_actions, NormalizedActions) at 16 384 envs;
  clip_grad_*  the clip-gradient launch alone (with its row sum), with and without an index;
  block_error  the kernel's error per parameter block against float64 autograd on 4099 samples (the tolerance of the tests is 2e-4), with
               float32 torch autograd's next to it;
  train_ppo    `train_ppo.py --env cassie3d --timing` at 16 384 envs x 8 steps in a child process: rollout / update seconds and env-steps/s.
Each timing: warm-up, then the median of `reps` synchronised repeats per side.  One JSON line per measurement.
usage: python tools/ab_ppo_cassie3d.py [rounds] [reps] > profiles/ppo_cassie3d_ab.jsonl"""
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
from cassierl_amd import ppo as P  # noqa: E402
from cassierl_amd import trpo as T  # noqa: E402
from cassierl_amd.vec_env3d import action_space  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ENVS, STEPS, D, A, HID = 16384, 8, 45, 10, (128, 128)
N, MB = ENVS * STEPS, ENVS * STEPS // 4


def out(**kw):
    print(json.dumps(kw), flush=True)


def med_us(fn, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def case(n, seed=1, jitter=0.05):
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(D, A, HID, init_std=1.0).cuda()
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.1 * torch.randn_like(p))
    obs = torch.randn(n, D, device="cuda") * 0.7
    adv = torch.randn(n, device="cuda")
    with torch.no_grad():
        old_mean, old_ls = pol.dist_info(obs)
        old_mean, old_ls = old_mean.clone(), old_ls[0].clone()
        act = old_mean + torch.randn_like(old_mean) * old_ls.exp()
        for p in pol.parameters():
            p.add_(jitter * torch.randn_like(p))
    return pol, dict(obs=obs, act=act, adv=adv, mean=old_mean, log_std=old_ls.expand(n, A))


# ---- the update
pol, d = case(N)
theta0 = T.flat_params(pol).clone()
amap = T.NormalizedActions(action_space("PD").low, action_space("PD").high, "cuda")
algo = P.PPO(None, None, pol, T.LinearFeatureBaseline(), ENVS, D, amap, batch_size=N, epochs=4, minibatch_size=MB)


def update(fused):
    T.set_flat_params(pol, theta0)
    algo.fused_grad = algo.fused_adam = fused
    algo.optimize(d)
    assert algo.last_grad_kind == ("pg3d_clip" if fused else "autograd")


med = {"fused": [], "torch": []}
for r in range(rounds):
    sides = [("fused", lambda: update(True)), ("torch", lambda: update(False))]
    for side, fn in (sides if r % 2 == 0 else sides[::-1]):
        us = med_us(fn)
        med[side].append(us)
        out(what="update", samples=N, epochs=4, minibatch=MB, round=r, side=side, median_us=us)
out(what="update_ratio", fused_us=float(np.median(med["fused"])), torch_us=float(np.median(med["torch"])),
    torch_over_fused=float(np.median(med["torch"]) / np.median(med["fused"])))

# ---- the policy step
T.set_flat_params(pol, theta0)
step = algo._fused_policy_step(torch.device("cuda:0"), torch.float32)
assert step is not None and algo.policy_step_entry == "CassiePg3dPolicyStep"
obs64 = torch.randn(ENVS, D, dtype=torch.float64, device="cuda")
noise = torch.randn(ENVS, A, device="cuda")
o32, mean, act = torch.empty(ENVS, D, device="cuda"), torch.empty(ENVS, A, device="cuda"), torch.empty(ENVS, A, device="cuda")


def torch_step():
    with torch.no_grad():
        o = obs64.to(torch.float32)
        a, m, _ = pol.get_actions(o, noise=noise)
        return amap(a)


med = {"fused": [], "torch": []}
for r in range(rounds):
    sides = [("fused", lambda: step(obs64, noise, o32, mean, act)), ("torch", torch_step)]
    for side, fn in (sides if r % 2 == 0 else sides[::-1]):
        us = med_us(fn, warm=5)
        med[side].append(us)
        out(what="policy_step", envs=ENVS, round=r, side=side, median_us=us)
out(what="policy_step_ratio", fused_us=float(np.median(med["fused"])), torch_us=float(np.median(med["torch"])),
    torch_over_fused=float(np.median(med["torch"]) / np.median(med["fused"])))

# ---- the launch alone
ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), d["obs"], d["act"], d["adv"], d["mean"], d["log_std"], 0.2, 0.0)
for m in (MB, N):
    idx = torch.randperm(N, device="cuda")[:m].contiguous()
    for what, fn in (("clip_grad_rows", lambda: ck.grad(None, m=m)), ("clip_grad_idx", lambda: ck.grad(idx))):
        out(what=what, kind=ck.kind, rows=m, median_us=med_us(fn, warm=5))

# ---- the error per parameter block against float64 autograd
n = 4099
pol, b = case(n, seed=3)
pol64 = copy.deepcopy(pol).double()
old_ls = b["log_std"][0].clone()
rows = lambda dt: [b[k].to(dt) for k in ("obs", "act", "adv", "mean")]
ref = T.flat_grad(P.ppo_loss(pol64, *rows(torch.float64), old_ls.double(), 0.2, 0.0), pol64)
g32 = T.flat_grad(P.ppo_loss(pol, *rows(torch.float32), old_ls, 0.2, 0.0), pol).double()
ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), b["obs"], b["act"], b["adv"], b["mean"], b["log_std"], 0.2, 0.0)
got = ck.grad()[0].double()
off = 0
for nm, p in pol.named_parameters():
    ix = torch.arange(off, off + p.numel(), device="cuda").view(p.shape)
    off += p.numel()
    parts = {nm: ix}
    if nm == "mean_net.0.weight":
        parts = {"W1[:, :32]": ix[:, :32], "W1[:, 32:]": ix[:, 32:]}
    elif nm in ("mean_net.4.weight", "mean_net.4.bias", "log_std"):
        parts = {nm + "[:8]": ix[:8], nm + "[8:]": ix[8:]}
    for name, i in parts.items():
        i = i.reshape(-1)
        s = ref[i].abs().max().item()
        out(what="block_error", kind=ck.kind, samples=n, block=name, tolerance=2e-4, kernel=(got[i] - ref[i]).abs().max().item() / s,
            torch32=(g32[i] - ref[i]).abs().max().item() / s, block_max_over_global_max=s / ref.abs().max().item())

# ---- the trainer (a child process: its own environment and policy)
del algo, ck
for extra, side in (([], "fused"), (["--torch-update"], "torch")):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "train_ppo.py"), "--env", "cassie3d", "--envs-per-gpu", str(ENVS), "--horizon", str(STEPS), "--n-itr", "6",
                        "--timing"] + extra, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        out(what="train_ppo", side=side, error=p.stderr[-500:])
        continue
    st = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][2:]   # (the first iterations carry the first-call costs)
    out(what="train_ppo --env cassie3d --timing", side=side, envs=ENVS, horizon=STEPS, iterations=len(st), seconds_rollout=float(np.median([s["seconds_rollout"] for s in st])),
        seconds_update=float(np.median([s["seconds_update"] for s in st])), env_steps_per_s=float(np.median([s["env_steps_per_s"] for s in st])))
