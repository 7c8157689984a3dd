#!/usr/bin/env python3
"""Learning-curve evidence for SAC (not a test): train_sac.py-style runs on the device stand environment, one JSON line per (every k-th) epoch:
average per-step reward, episodes, average return, the critics' losses, mean Q, the actor's loss, mean log pi, alpha, wall-clock.
  torque   cassie_stand2d reward, torque mode;  pd   the same reward under PD control
usage: python tools/sac_learning_curve.py [torque|pd] [epochs] [envs] [every] [epoch_length] [batch] > profiles/sac_learning_curve_<mode>.jsonl"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cassierl_amd.sac import make_cassie_sac  # noqa: E402
from cassierl_amd.trajectory import default_gait  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "torque"
n_epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 300
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
every = int(sys.argv[4]) if len(sys.argv) > 4 else 10
epoch_length = int(sys.argv[5]) if len(sys.argv) > 5 else 20
batch = int(sys.argv[6]) if len(sys.argv) > 6 else n
kw = dict(torque=dict(kind="stand", control_mode="Torque"), pd=dict(kind="stand", control_mode="PD"))[which]
algo = make_cassie_sac(n, device=0, trajectory=default_gait(), seed=1, batch_size=batch, epoch_length=epoch_length, **kw)
print(json.dumps(dict(run="stand_" + which, envs=n, epoch_length=epoch_length, batch_size=batch, pool_rows=algo.pool.capacity,
                      hyper="sac.py defaults: 32 x 32 ReLU actor and twin critics, gamma 0.99, scale_reward 1, Lasagne Adam 3e-4 x 3, tau 5e-3, alpha from 1 "
                            "towards target entropy -A, path <= 100, min_pool_size 10000, one update per vector step")), flush=True)
t0 = time.perf_counter()
for ep in range(n_epochs):
    st = algo.train_iteration()
    if ep % every == 0 or ep == n_epochs - 1:
        print(json.dumps(dict(epoch=st["itr"], avg_reward=st["avg_reward"], episodes=st["episodes"], avg_return=st["avg_return"], qf1_loss=st["qf1_loss"],
                              qf2_loss=st["qf2_loss"], avg_q=st["avg_q"], policy_loss=st["policy_loss"], avg_log_pi=st["avg_log_pi"], alpha=st["alpha"],
                              updates=st["updates"], pool_size=st["pool_size"], seconds=time.perf_counter() - t0)), flush=True)
algo.env.close()
