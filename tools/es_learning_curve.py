#!/usr/bin/env python3
"""Learning-curve evidence for ES (not a test): train_es.py-style runs on the device environment, one JSON line per (every k-th) iteration:
average / best / worst return of the perturbed population, average path length, live env-steps, gradient / step norms, wall-clock.
  stand   cassie_stand2d reward, torque mode;  walk   Cassie2dEnv, PD control, reference semantics
usage: python tools/es_learning_curve.py [stand|walk] [iterations] [envs] [every] [max_path_length]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cassierl_amd.es import make_cassie_es  # noqa: E402
from cassierl_amd.trajectory import default_gait  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "stand"
n_itr = int(sys.argv[2]) if len(sys.argv) > 2 else 100
n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
every = int(sys.argv[4]) if len(sys.argv) > 4 else 10
max_path_length = int(sys.argv[5]) if len(sys.argv) > 5 else 1000
kw = dict(stand=dict(kind="stand", control_mode="Torque"), walk=dict(kind="walk", control_mode="PD"))[which]
algo = make_cassie_es(n, device=0, trajectory=default_gait(), seed=1, max_path_length=max_path_length, **kw)
print(json.dumps(dict(run=which, envs=n, directions=n // 2, max_path_length=max_path_length,
                      hyper="26-32-32-A tanh mean network, sigma %g, Adam lr %g, l2 %g, %s, table 2^24" % (algo.sigma, algo.learning_rate, algo.l2_coeff,
                                                                                                        algo.fitness_shaping))), flush=True)
t0 = time.perf_counter()
for it in range(n_itr):
    st = algo.train_iteration()
    if it % every == 0 or it == n_itr - 1:
        print(json.dumps(dict(itr=st["itr"], avg_return=st["avg_return"], max_return=st["max_return"], min_return=st["min_return"],
                              avg_path_length=st["avg_path_length"], env_steps=st["env_steps"], grad_norm=st["grad_norm"], step_norm=st["step_norm"],
                              policy_step=algo.last_policy_step_kind, grad=algo.last_grad_kind, seconds=time.perf_counter() - t0)), flush=True)
algo.env.close()
