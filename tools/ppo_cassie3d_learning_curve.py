#!/usr/bin/env python3
"""Learning-curve record for PPO on Cassie3d (not a test, not a criterion): make_cassie_ppo(env="cassie3d") from the standing reset, PD mode,
default gains, one JSON line per iteration: average per-step reward, finished episodes and their average return, mean path age, loss, KL, clip
fraction, wall-clock.  The reward is csrc/cassie3d_env.h's: 1 - 2 (0.9 - z)^2 - 2 fx^2 - 2 fy^2 - 0.001 |action|^2, done at z < 0.5.
usage: python tools/ppo_cassie3d_learning_curve.py [iterations] [envs] [horizon] > profiles/ppo_cassie3d_learning_curve.jsonl"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cassierl_amd.ppo import make_cassie_ppo  # noqa: E402

n_itr = int(sys.argv[1]) if len(sys.argv) > 1 else 50
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
horizon = int(sys.argv[3]) if len(sys.argv) > 3 else 16
algo = make_cassie_ppo(n, env="cassie3d", control_mode="PD", device=0, seed=1, batch_size=n * horizon)
print(json.dumps(dict(run="ppo cassie3d", envs=n, horizon_env_steps=horizon, samples_per_iteration=n * horizon, control_mode="PD", kp=10.0, kd=5.0,
                      hyper="45-128-128-10 tanh Gaussian MLP, init_std 1.0, linear feature baseline, Adam lr 3e-4, clip 0.2, GAE 0.95, 4 epochs x 4 minibatches, "
                            "gamma 0.99, path <= 1000")), flush=True)
t0 = time.perf_counter()
for it in range(n_itr):
    st = algo.train_iteration()
    print(json.dumps(dict(itr=st["itr"], avg_reward=st["avg_reward"], episodes=st["episodes"], avg_return=st["avg_return"], loss_first=st["loss_first"],
                          mean_kl=st["mean_kl"], clip_frac=st["clip_frac"], grad_norm=st["grad_norm"], grad_kind=algo.last_grad_kind,
                          mean_path_age_steps=float(algo.path_t.double().mean().item()), seconds=time.perf_counter() - t0)), flush=True)
algo.env.close()
