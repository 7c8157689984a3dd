#!/usr/bin/env python3
"""Counterpart of rllab/envs/trpo_cassie.py on the batched MI355X environment (BASELINE.json config 4 when launched with
`python -m torch.distributed.run --nproc-per-node 8 train_trpo.py --envs-per-gpu 65536`).

Hyper-parameters are those of trpo_cassie.py:21-42 (MLP 32x32, init_std 2.0, discount 0.99, step_size 0.005,
max_path_length 1000); batch_size defaults to one Env.step of every environment per iteration times --horizon.
--hidden 128,128 (with --init-std 1.0: vpg_cassie.py's policy) trains the wide policy on its own kernels (csrc/tu_pg_trpo.hip).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cassierl_amd import train_cli as cli  # noqa: E402


def parser():
    ap = cli.add_common_flags(argparse.ArgumentParser())
    ap.add_argument("--horizon", type=int, default=4, help="Env.steps per environment per iteration")
    ap.add_argument("--n-itr", type=int, default=10)
    ap.add_argument("--hidden", default="32,32", help="hidden layer widths of the Gaussian MLP policy (32,32 and 128,128 run on HIP kernels)")
    ap.add_argument("--init-std", type=float, default=2.0)
    return ap


def main():
    args = parser().parse_args()
    rank, world, dev, terrain = cli.setup(args)
    from cassierl_amd.trajectory import default_gait
    from cassierl_amd.trpo import make_cassie_trpo
    hidden = tuple(int(x) for x in args.hidden.split(","))
    algo = make_cassie_trpo(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev,
                            trajectory=default_gait(), seed=1, batch_size=args.envs_per_gpu * world * args.horizon, terrain=terrain,
                            hidden_sizes=hidden, init_std=args.init_std)
    cli.train(algo, args, args.n_itr, rank)


if __name__ == "__main__":
    main()
