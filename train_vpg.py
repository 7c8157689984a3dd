#!/usr/bin/env python3
"""Counterpart of rllab/envs/vpg_cassie.py on the batched MI355X environment; runs under torchrun exactly as train_trpo.py does
(`python -m torch.distributed.run --nproc-per-node 8 train_vpg.py --envs-per-gpu 65536`).

Hyper-parameters are those of vpg_cassie.py:15-48 (MLP 128x128, init_std 1.0, discount 0.99, max_path_length 1000) and of rllab's VPG
(one full-batch Lasagne Adam step per iteration, learning rate 1e-3); batch_size is one Env.step of every environment times --horizon.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cassierl_amd import train_cli as cli  # noqa: E402


def parser():
    ap = argparse.ArgumentParser(epilog="vpg_cassie.py also passes step_size=0.005 and use_gpu=True: rllab's VPG never reads them "
                                 "(BatchPolopt's **kwargs swallows both), so they have no counterpart here.")
    cli.add_common_flags(ap)
    ap.add_argument("--horizon", type=int, default=4, help="Env.steps per environment per iteration")
    ap.add_argument("--n-itr", type=int, default=10)
    ap.add_argument("--hidden", default="128,128", help="hidden layer widths of the Gaussian MLP policy")
    ap.add_argument("--init-std", type=float, default=1.0)
    ap.add_argument("--learning-rate", type=float, default=1e-3, help="Adam step size (rllab's FirstOrderOptimizer default)")
    ap.add_argument("--log-kl", action="store_true", help="also log mean_kl / max_kl / loss_after (one more forward pass over the batch)")
    return ap


def main():
    args = parser().parse_args()
    rank, world, dev, terrain = cli.setup(args)
    from cassierl_amd.trajectory import default_gait
    from cassierl_amd.vpg import make_cassie_vpg
    hidden = tuple(int(x) for x in args.hidden.split(","))
    algo = make_cassie_vpg(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, trajectory=default_gait(), seed=1,
                           hidden_sizes=hidden, init_std=args.init_std, learning_rate=args.learning_rate, log_kl=args.log_kl,
                           batch_size=args.envs_per_gpu * world * args.horizon, terrain=terrain)
    cli.train(algo, args, args.n_itr, rank)


if __name__ == "__main__":
    main()
