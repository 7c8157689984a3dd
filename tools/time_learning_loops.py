#!/usr/bin/env python3
"""Host-side speed of five learning loops in the tree given as argv[1] (its cassierl_amd is imported; CASSIE2D_LIB selects the library; not a test):
one JSON line per loop, `value` = the median over the timed iterations of this process (TRPO: env-steps/s; the others: ms per train_iteration).
tools/ab_learning_layer.py runs it in two trees alternately."""
import json
import statistics
import sys
import time

sys.path.insert(0, sys.argv[1])
import torch  # noqa: E402
from cassierl_amd.trajectory import default_gait  # noqa: E402


def timed(algo, warm, reps):
    for _ in range(warm):
        algo.train_iteration()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        algo.train_iteration()
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    algo.env.close()
    return statistics.median(ts)


def emit(loop, value, unit):
    print(json.dumps(dict(loop=loop, value=value, unit=unit)), flush=True)


N, H = 65536, 8
from cassierl_amd.trpo import make_cassie_trpo  # noqa: E402
s = timed(make_cassie_trpo(N, kind="walk", control_mode="PD", trajectory=default_gait(), batch_size=N * H), 3, 15)
emit("TRPO outer loop 65536 walk/PD x 8", N * H / s, "env-steps/s")
from cassierl_amd.vpg import make_cassie_vpg  # noqa: E402
emit("VPG train_iteration 65536 x 8", 1e3 * timed(make_cassie_vpg(N, kind="walk", control_mode="PD", trajectory=default_gait(), batch_size=N * H), 3, 15), "ms")
from cassierl_amd.ppo import make_cassie_ppo  # noqa: E402
emit("PPO train_iteration 65536 x 8, 4 epochs x 8 minibatches",
     1e3 * timed(make_cassie_ppo(N, kind="walk", control_mode="PD", trajectory=default_gait(), batch_size=N * H, epochs=4, minibatch_size=N * H // 8), 3, 15), "ms")
from cassierl_amd.es import make_cassie_es  # noqa: E402
emit("ES train_iteration 4096 envs", 1e3 * timed(make_cassie_es(4096, kind="walk", control_mode="PD", trajectory=default_gait()), 3, 15), "ms")
from cassierl_amd.ddpg import make_cassie_ddpg  # noqa: E402
emit("DDPG epoch: 4096 envs, 32 steps, batch 4096, pool 1048576",
     1e3 * timed(make_cassie_ddpg(4096, kind="walk", control_mode="PD", trajectory=default_gait(), batch_size=4096, replay_pool_size=1 << 20,
                                  min_pool_size=4096, epoch_length=32), 2, 10), "ms")
