#!/usr/bin/env python3
"""Counterpart of rllab/envs/ddpg_cassie.py on the batched MI355X environment; runs under torchrun exactly as train_trpo.py and train_vpg.py do
(`python -m torch.distributed.run --nproc-per-node 8 train_ddpg.py --envs-per-gpu 65536 --batch-size 524288`).

Hyper-parameters are those of ddpg_cassie.py:30-45 (32 x 32 networks, batch 32, max_path_length 100, epoch_length 1000, min_pool_size 10000,
discount 0.99, scale_reward 0.01, learning rates 1e-3 / 1e-4) and of rllab's DDPG (pool of 1 000 000 transitions, tau 0.001, one update per step).
With --envs-per-gpu 1 these run rllab's loop.  With N environments one vector step stores N transitions and is followed by --updates-per-step
updates of --batch-size rows (summed over ranks): at large N set both, e.g. `--batch-size 65536 --updates-per-step 1`; no scaling rule is applied.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cassierl_amd import train_cli as cli  # noqa: E402


def parser():
    ap = cli.add_common_flags(argparse.ArgumentParser(), timing="report the seconds of an epoch between two synchronisations",
                              dump_params="after the last epoch rank 0 writes the flat actor, critic and target parameters to this .npy file, rank r > 0 to <file>.rank<r>.npy")
    return cli.add_pool_flags(ap, batch_size=32, batch_help="rows per update, over all ranks (ddpg_cassie.py: 32)", scale_reward=0.01, qf_learning_rate=1e-3,
                              policy_learning_rate=1e-4)


def main():
    args = parser().parse_args()
    rank, world, dev, terrain = cli.setup(args)
    from cassierl_amd.ddpg import make_cassie_ddpg
    from cassierl_amd.trajectory import default_gait
    algo = make_cassie_ddpg(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, trajectory=default_gait(), seed=1, terrain=terrain,
                            **cli.pool_kwargs(args))
    if args.torch_update:
        algo.fused_update = algo.fused_policy_step = False
    cli.train(algo, args, args.n_epochs, rank, loaded=cli.pool_loaded, dump=cli.pool_dump("policy", "qf", "target_policy", "target_qf"))


if __name__ == "__main__":
    main()
