#!/usr/bin/env python3
"""Learning-curve record for SAC on Cassie3d (not a test, not a criterion): make_cassie_sac(env="cassie3d") from the standing reset, PD mode,
default gains, the environment samples of tools/ppo_cassie3d_learning_curve.py's record (4096 envs x 16 steps x 50 = 3 276 800), one JSON line
per epoch of 16 vector steps: average per-step reward, finished episodes and their average return, mean path age, the losses, log pi, the
temperature, wall-clock.  The reward is csrc/cassie3d_env.h's: 1 - 2 (0.9 - z)^2 - 2 fx^2 - 2 fy^2 - 0.001 |action|^2, done at z < 0.5.
usage: python tools/sac_cassie3d_learning_curve.py [epochs] [envs] [epoch_length] > profiles/sac_cassie3d_learning_curve.jsonl"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cassierl_amd.sac import make_cassie_sac  # noqa: E402

n_epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 50
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 16
algo = make_cassie_sac(n, env="cassie3d", control_mode="PD", kp=10.0, kd=5.0, device=0, seed=1, batch_size=n, updates_per_step=1, min_pool_size=4 * n,
                       epoch_length=steps, max_path_length=1000)
print(json.dumps(dict(run="sac cassie3d", envs=n, epoch_env_steps=steps, samples_per_epoch=n * steps, control_mode="PD", kp=10.0, kd=5.0,
                      hyper="45-32-32-20 squashed Gaussian actor, two 55-32-32-1 critics (ReLU), batch %d, 1 update per vector step after %d rows, the three "
                            "learning rates 3e-4, tau 0.005, gamma 0.99, init_alpha 1, target entropy -10, pool %d rows, path <= 1000" % (n, 4 * n, algo.pool.capacity))),
      flush=True)
t0 = time.perf_counter()
for it in range(n_epochs):
    st = algo.train_iteration()
    print(json.dumps(dict(itr=st["itr"], avg_reward=st["avg_reward"], episodes=st["episodes"], avg_return=st["avg_return"], updates=st["updates"],
                          qf_loss=st["qf_loss"], avg_q=st["avg_q"], policy_loss=st["policy_loss"], avg_log_pi=st["avg_log_pi"], alpha=st["alpha"],
                          update_kind=st["update_kind"], policy_step_fused=algo.last_policy_step_fused,
                          mean_path_age_steps=float(algo.path_t.double().mean().item()), seconds=time.perf_counter() - t0)), flush=True)
algo.env.close()
