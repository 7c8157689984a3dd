#!/usr/bin/env python3
"""Learning-curve evidence for VPG (not a test): train_vpg.py-style runs on the device environment, one JSON line per (every k-th)
iteration: average per-step reward, episodes, average return, mean path age, gradient / step norms, wall-clock.
  stand   cassie_stand2d reward, torque mode;  walk   the env vpg_cassie.py trains (Cassie2dEnv, PD control, reference semantics)
usage: python tools/vpg_learning_curve.py [stand|walk] [iterations] [envs] [every] [horizon]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cassierl_amd.trajectory import default_gait  # noqa: E402
from cassierl_amd.vpg import make_cassie_vpg  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "stand"
n_itr = int(sys.argv[2]) if len(sys.argv) > 2 else 300
n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
every = int(sys.argv[4]) if len(sys.argv) > 4 else 10
horizon = int(sys.argv[5]) if len(sys.argv) > 5 else 16
kw = dict(stand=dict(kind="stand", control_mode="Torque"), walk=dict(kind="walk", control_mode="PD"))[which]
algo = make_cassie_vpg(n, device=0, trajectory=default_gait(), seed=1, batch_size=n * horizon, **kw)
print(json.dumps(dict(run=which, envs=n, horizon_env_steps=horizon, samples_per_iteration=n * horizon,
                      hyper="vpg_cassie.py: 26-128-128-A tanh Gaussian MLP, init_std 1.0, linear feature baseline, Lasagne Adam lr 1e-3, gamma 0.99, path <= 1000")), flush=True)
t0 = time.perf_counter()
for it in range(n_itr):
    st = algo.train_iteration()
    if it % every == 0 or it == n_itr - 1:
        print(json.dumps(dict(itr=st["itr"], avg_reward=st["avg_reward"], episodes=st["episodes"], avg_return=st["avg_return"], grad_norm=st["grad_norm"],
                              step_norm=st["step_norm"], mean_path_age_steps=float(algo.path_t.double().mean().item()), seconds=time.perf_counter() - t0)), flush=True)
algo.env.close()
