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
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cassierl_amd import train_cli as cli  # noqa: E402


def parser():
    ap = cli.add_common_flags(argparse.ArgumentParser(), timing="report the seconds of an epoch between two synchronisations",
                              dump_params="after the last epoch rank 0 writes the flat actor, qf1, qf2, target actor, target_qf1, target_qf2 parameters, in this order, to this .npy file, rank r > 0 to <file>.rank<r>.npy")
    cli.add_pool_flags(ap, batch_size=256, batch_help="rows per update, over all ranks", scale_reward=1.0, qf_learning_rate=3e-4, policy_learning_rate=3e-4)
    ap.add_argument("--policy-noise", type=float, default=0.2, help="standard deviation of the noise added to the target actor's action")
    ap.add_argument("--noise-clip", type=float, default=0.5, help="that noise is clipped to +- this")
    ap.add_argument("--policy-delay", type=int, default=2, help="the actor and the three targets move on every policy-delay-th update")
    ap.add_argument("--exploration-sigma", type=float, default=0.1, help="standard deviation of the exploration noise added to mu(s)")
    return ap


def main():
    args = parser().parse_args()
    rank, world, dev, terrain = cli.setup(args)
    from cassierl_amd.td3 import make_cassie_td3
    from cassierl_amd.trajectory import default_gait
    algo = make_cassie_td3(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, trajectory=default_gait(), seed=1, terrain=terrain,
                           policy_noise=args.policy_noise, noise_clip=args.noise_clip, policy_delay=args.policy_delay, exploration_sigma=args.exploration_sigma,
                           **cli.pool_kwargs(args))
    if args.torch_update:
        algo.fused_update = algo.fused_policy_step = False
    cli.train(algo, args, args.n_epochs, rank, loaded=cli.pool_loaded,
              dump=cli.pool_dump("policy", "qf1", "qf2", "target_policy", "target_qf1", "target_qf2"))


if __name__ == "__main__":
    main()
