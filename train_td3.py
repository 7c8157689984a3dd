#!/usr/bin/env python3
"""TD3 (cassierl_amd/td3.py) on the batched MI355X environment; train_sac.py's flags and schedule, so that the two can be compared line for
line, and it runs under torchrun as train_sac.py does
(`python -m torch.distributed.run --nproc-per-node 8 train_td3.py --envs-per-gpu 65536 --batch-size 524288`).

Defaults: 32 x 32 networks, batch 256, both learning rates 3e-4, tau 0.005, discount 0.99, scale_reward 1, target-policy noise 0.2 clipped at 0.5,
the actor and the targets move on every second update, exploration noise 0.1; max_path_length 100, epoch_length 1000, min_pool_size 10000 and the
pool of 1 000 000 transitions are DDPG's.  With N environments one vector step stores N transitions and is followed by --updates-per-step updates
of --batch-size rows (summed over ranks).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs-per-gpu", type=int, default=4096)
    ap.add_argument("--batch-size", type=int, default=256, help="rows per update, over all ranks")
    ap.add_argument("--updates-per-step", type=int, default=1, help="updates after every vector step (rllab's n_updates_per_sample)")
    ap.add_argument("--pool-size", type=int, default=0, help="rows of each rank's replay pool, a multiple of --envs-per-gpu (default: 1 000 000 rounded up to one); "
                    "a row is 4 (2 D + A + 2) bytes = 240 B for the 26-wide observation and 6 actions, so 1 000 000 rows are 240 MB and hold "
                    "16 vector steps of 65 536 environments")
    ap.add_argument("--min-pool-size", type=int, default=10000, help="transitions (over all ranks) before the first update")
    ap.add_argument("--epoch-length", type=int, default=1000, help="vector steps per epoch (one log line, one read-back)")
    ap.add_argument("--n-epochs", type=int, default=10)
    ap.add_argument("--max-path-length", type=int, default=100)
    ap.add_argument("--scale-reward", type=float, default=1.0)
    ap.add_argument("--qf-learning-rate", type=float, default=3e-4)
    ap.add_argument("--policy-learning-rate", type=float, default=3e-4)
    ap.add_argument("--policy-noise", type=float, default=0.2, help="standard deviation of the noise added to the target actor's action")
    ap.add_argument("--noise-clip", type=float, default=0.5, help="that noise is clipped to +- this")
    ap.add_argument("--policy-delay", type=int, default=2, help="the actor and the three targets move on every policy-delay-th update")
    ap.add_argument("--exploration-sigma", type=float, default=0.1, help="standard deviation of the exploration noise added to mu(s)")
    ap.add_argument("--kind", default="walk", choices=["walk", "stand"])
    ap.add_argument("--control-mode", default="PD", choices=["PD", "Torque", "OSC"])
    ap.add_argument("--snapshot", default="")
    ap.add_argument("--snapshot-pool", type=int, default=1, help="0: the snapshot omits the replay pool (it can be gigabytes); a run loaded from it restarts with an empty pool")
    ap.add_argument("--load-policy", default="")
    ap.add_argument("--timing", action="store_true", help="report the seconds of an epoch between two synchronisations")
    ap.add_argument("--torch-update", action="store_true", help="run the torch statements instead of the HIP kernels (A/B)")
    ap.add_argument("--terrain-dir", default="", help="folder of terrain PNGs (model/terrains/ of the reference): robots on a terrain library")
    ap.add_argument("--num-terrains", type=int, default=1, help="K fields drawn (with replacement) from --terrain-dir")
    ap.add_argument("--terrain-elevation", type=float, default=1.0, help="height of a white pixel in metres (the <hfield> size_z)")
    ap.add_argument("--terrain-seed", type=int, default=1, help="seed of the file draw and of the per-environment field ids")
    ap.add_argument("--dump-params", default="", help="after the last epoch rank 0 writes the flat actor, qf1, qf2, target actor, target_qf1, target_qf2 parameters, in this order, to this .npy file, rank r > 0 to <file>.rank<r>.npy")
    args = ap.parse_args()
    import torch
    from cassierl_amd import rollout as R
    from cassierl_amd.td3 import make_cassie_td3
    from cassierl_amd.trajectory import default_gait
    rank, local_rank, world = R.init_distributed()
    dev = R.local_device(local_rank) if world > 1 else 0   # CASSIE_DEVICE_MAP (test hook): several ranks on one GPU
    torch.cuda.set_device(dev)
    from cassierl_amd.terrain import terrain_spec
    terrain = terrain_spec(args.terrain_dir, args.num_terrains, args.terrain_elevation, args.terrain_seed) if args.terrain_dir else None
    algo = make_cassie_td3(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, trajectory=default_gait(), seed=1, terrain=terrain,
                           replay_pool_size=args.pool_size or None, batch_size=args.batch_size, updates_per_step=args.updates_per_step,
                           min_pool_size=args.min_pool_size, epoch_length=args.epoch_length, max_path_length=args.max_path_length,
                           scale_reward=args.scale_reward, qf_learning_rate=args.qf_learning_rate, policy_learning_rate=args.policy_learning_rate,
                           policy_noise=args.policy_noise, noise_clip=args.noise_clip, policy_delay=args.policy_delay, exploration_sigma=args.exploration_sigma,
                           snapshot_pool=bool(args.snapshot_pool))
    algo.timing = args.timing
    if args.torch_update:
        algo.fused_update = algo.fused_policy_step = False
    if args.load_policy:
        _, restored = algo.load(args.load_policy)
        if rank == 0:
            print(json.dumps(dict(loaded=args.load_policy, itr=algo.itr, sampler_restored=restored, pool_restored=algo.pool_restored, pool_size=algo.pool.size)))
    for _ in range(args.n_epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = algo.train_iteration()
        torch.cuda.synchronize()
        st["seconds"] = time.perf_counter() - t0
        st["env_steps_per_s"] = st["env_steps"] / st["seconds"]
        if rank == 0:
            print(json.dumps(st), flush=True)
        if args.snapshot:
            algo.save(args.snapshot)  # snapshot_mode="last"
    if args.dump_params:   # rank r > 0 writes <file>.rank<r>.npy: the ranks must hold the same numbers
        from cassierl_amd.trpo import flat_params
        np.save(args.dump_params if rank == 0 else "%s.rank%d.npy" % (args.dump_params, rank), torch.cat([flat_params(m) for m in (algo.policy, algo.qf1, algo.qf2, algo.target_policy, algo.target_qf1, algo.target_qf2)]).double().cpu().numpy())
    if R.dist.is_initialized():
        R.dist.barrier()
        R.dist.destroy_process_group()


if __name__ == "__main__":
    main()
