#!/usr/bin/env python3
"""Learning-curve evidence for DDPG (not a test): train_ddpg.py-style runs on the device environment, one JSON line per (every k-th) epoch:
average per-step reward, episodes, average return, critic loss, mean Q, the policy's surrogate, wall-clock.
  stand   cassie_stand2d reward, torque mode;  walk   the env ddpg_cassie.py trains (Cassie2dEnv, PD control, reference semantics)
usage: python tools/ddpg_learning_curve.py [stand|walk] [epochs] [envs] [every] [epoch_length] [batch]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cassierl_amd.ddpg import make_cassie_ddpg  # noqa: E402
from cassierl_amd.trajectory import default_gait  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "stand"
n_epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 300
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
every = int(sys.argv[4]) if len(sys.argv) > 4 else 10
epoch_length = int(sys.argv[5]) if len(sys.argv) > 5 else 20
batch = int(sys.argv[6]) if len(sys.argv) > 6 else n
kw = dict(stand=dict(kind="stand", control_mode="Torque"), walk=dict(kind="walk", control_mode="PD"))[which]
algo = make_cassie_ddpg(n, device=0, trajectory=default_gait(), seed=1, batch_size=batch, epoch_length=epoch_length, **kw)
print(json.dumps(dict(run=which, envs=n, epoch_length=epoch_length, batch_size=batch, pool_rows=algo.pool.capacity,
                      hyper="ddpg_cassie.py: 32 x 32 ReLU actor and critic, OU(0.15, 0.3), gamma 0.99, scale_reward 0.01, Lasagne Adam 1e-3 / 1e-4, tau 1e-3, "
                            "path <= 100, min_pool_size 10000, one update per vector step")), flush=True)
t0 = time.perf_counter()
for ep in range(n_epochs):
    st = algo.train_iteration()
    if ep % every == 0 or ep == n_epochs - 1:
        print(json.dumps(dict(epoch=st["itr"], avg_reward=st["avg_reward"], episodes=st["episodes"], avg_return=st["avg_return"], qf_loss=st["qf_loss"],
                              avg_q=st["avg_q"], policy_surr=st["policy_surr"], updates=st["updates"], pool_size=st["pool_size"],
                              seconds=time.perf_counter() - t0)), flush=True)
algo.env.close()
