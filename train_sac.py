#!/usr/bin/env python3
"""Soft Actor-Critic (cassierl_amd/sac.py) on the batched MI355X environment; train_ddpg.py's flags and schedule, so that the two can be compared
line for line, and it runs under torchrun as train_ddpg.py does
(`python -m torch.distributed.run --nproc-per-node 8 train_sac.py --envs-per-gpu 65536 --batch-size 524288`).

Defaults: 32 x 32 networks, batch 256, the three learning rates 3e-4, tau 0.005, discount 0.99, scale_reward 1, alpha starts at 1 and is learned
towards the target entropy -A; max_path_length 100, epoch_length 1000, min_pool_size 10000 and the pool of 1 000 000 transitions are DDPG's.
With N environments one vector step stores N transitions and is followed by --updates-per-step updates of --batch-size rows (summed over ranks).
--env cassie3d runs the same schedule on Cassie3dVecEnv (45 observations, 10 actions, --control-mode PD or Torque, --kp / --kd): a pool row is then
408 B, the default pool 408 MB per rank.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cassierl_amd import train_cli as cli  # noqa: E402


def parser():
    ap = cli.add_common_flags(argparse.ArgumentParser(), timing="report the seconds of an epoch between two synchronisations",
                              dump_params="after the last epoch rank 0 writes the flat actor, qf1, qf2, target_qf1, target_qf2 parameters and log_alpha, in this order, to this .npy file, rank r > 0 to <file>.rank<r>.npy")
    cli.add_pool_flags(ap, batch_size=256, batch_help="rows per update, over all ranks", scale_reward=1.0, qf_learning_rate=3e-4, policy_learning_rate=3e-4)
    ap.add_argument("--env", default="cassie2d", choices=["cassie2d", "cassie3d"], help="cassie3d: the 3-D robot from its standing reset (45 observations, 10 actions)")
    ap.add_argument("--kp", type=float, default=10.0, help="--env cassie3d, PD mode: proportional gain of the ten actuated hinges")
    ap.add_argument("--kd", type=float, default=5.0, help="--env cassie3d, PD mode: damping gain")
    ap.add_argument("--alpha-lr", type=float, default=3e-4, help="learning rate of log_alpha")
    ap.add_argument("--init-alpha", type=float, default=1.0)
    ap.add_argument("--fixed-alpha", type=float, default=None, help="hold the temperature at this value (no temperature step)")
    ap.add_argument("--target-entropy", type=float, default=None, help="default: minus the number of actions")
    return ap


def main():
    args = parser().parse_args()
    rank, world, dev, terrain = cli.setup(args)
    from cassierl_amd.sac import make_cassie_sac
    from cassierl_amd.trajectory import default_gait
    env_kw = dict(trajectory=default_gait()) if args.env == "cassie2d" else dict(env="cassie3d", kp=args.kp, kd=args.kd)
    algo = make_cassie_sac(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, seed=1, terrain=terrain, **env_kw,
                           alpha_learning_rate=args.alpha_lr, init_alpha=args.init_alpha, fixed_alpha=args.fixed_alpha, target_entropy=args.target_entropy,
                           **cli.pool_kwargs(args))
    if args.torch_update:
        algo.fused_update = algo.fused_policy_step = False
    cli.train(algo, args, args.n_epochs, rank, loaded=cli.pool_loaded,
              dump=cli.pool_dump("policy", "qf1", "qf2", "target_qf1", "target_qf2", tail=("log_alpha",)))


if __name__ == "__main__":
    main()
