#!/usr/bin/env python3
"""Learning-curve record for ES on Cassie3d (not a test, not a criterion): make_cassie_es(env="cassie3d") from the standing reset, PD mode, default
gains, 4096 environments (2048 antithetic directions), episodes of at most 300 steps, 50 iterations, the 32 x 32 policy, OpenAI's defaults
(sigma 0.02, Adam 0.01, l2 0.005, centered ranks).  One JSON line per iteration: mean / max / min fitness of the population (the PERTURBED
policies), mean episode length, gradient and step norms, what ran, wall-clock.  The reward is csrc/cassie3d_env.h's:
1 - 2 (0.9 - z)^2 - 2 fx^2 - 2 fy^2 - 0.001 |action|^2, done at z < 0.5; an episode of 300 steps can earn at most 300.
usage: python tools/es_cassie3d_learning_curve.py [iterations] [envs] [max_path_length] [hidden] > profiles/es_cassie3d_learning_curve.jsonl"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cassierl_amd.es import make_cassie_es  # noqa: E402

n_itr = int(sys.argv[1]) if len(sys.argv) > 1 else 50
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
horizon = int(sys.argv[3]) if len(sys.argv) > 3 else 300
hidden = tuple(int(x) for x in sys.argv[4].split(",")) if len(sys.argv) > 4 else (32, 32)
algo = make_cassie_es(n, env="cassie3d", control_mode="PD", kp=10.0, kd=5.0, device=0, seed=1, hidden_sizes=hidden, max_path_length=horizon)
print(json.dumps(dict(run="es cassie3d", envs=n, directions=n // 2, max_path_length=horizon, control_mode="PD", kp=10.0, kd=5.0, n_params=algo.n_params,
                      hyper="45-%d-%d-10 tanh mean network, sigma %g, Adam %g, l2 %g, %s, table %d" % (hidden + (algo.sigma, algo.learning_rate, algo.l2_coeff,
                                                                                                    algo.fitness_shaping, algo.table_size)))), flush=True)
t0 = time.perf_counter()
for it in range(n_itr):
    st = algo.train_iteration()
    print(json.dumps(dict(itr=st["itr"], avg_return=st["avg_return"], max_return=st["max_return"], min_return=st["min_return"], avg_path_length=st["avg_path_length"],
                          env_steps=st["env_steps"], grad_norm=st["grad_norm"], step_norm=st["step_norm"], policy_step=algo.last_policy_step_kind,
                          grad=algo.last_grad_kind, book_fused=algo.last_book_fused, seconds=time.perf_counter() - t0)), flush=True)
algo.env.close()
