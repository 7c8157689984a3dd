#!/usr/bin/env python3
"""PPO (clipped surrogate, GAE(lambda), epochs of minibatch Adam steps: cassierl_amd/ppo.py) on the batched MI355X environment; runs under
torchrun exactly as train_vpg.py does (`python -m torch.distributed.run --nproc-per-node 8 train_ppo.py --envs-per-gpu 65536`).

The policy and the environment are train_vpg.py's (MLP 128x128, init_std 1.0, discount 0.99, max_path_length 1000); batch_size is one Env.step of
every environment times --horizon, --minibatch-size counts samples over all ranks (default: a quarter of the batch).
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
    ap.add_argument("--env", default="cassie2d", choices=["cassie2d", "cassie3d"], help="cassie3d: the 3-D robot from its standing reset (45 observations, 10 actions)")
    ap.add_argument("--kp", type=float, default=10.0, help="--env cassie3d, PD mode: proportional gain of the ten actuated hinges")
    ap.add_argument("--kd", type=float, default=5.0, help="--env cassie3d, PD mode: damping gain")
    ap.add_argument("--hidden", default="128,128", help="hidden layer widths of the Gaussian MLP policy")
    ap.add_argument("--init-std", type=float, default=1.0)
    ap.add_argument("--learning-rate", type=float, default=3e-4, help="Adam step size")
    ap.add_argument("--clip-range", type=float, default=0.2)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--epochs", type=int, default=4, help="passes over each rollout")
    ap.add_argument("--minibatch-size", type=int, default=0, help="samples per Adam step over all ranks (0: a quarter of the batch)")
    ap.add_argument("--entropy-coeff", type=float, default=0.0)
    ap.add_argument("--value", default="linear", choices=["linear", "mlp"], help="the value function: rllab's LinearFeatureBaseline, or a learned tanh MLP (cassierl_amd/value.py)")
    ap.add_argument("--value-hidden", default="128,128", help="--value mlp: hidden layer widths of the value network")
    ap.add_argument("--value-learning-rate", type=float, default=1e-3, help="--value mlp: Adam step size of the value network")
    ap.add_argument("--torch-update", action="store_true", help="force the torch statements (autograd, torch Adam, torch GAE, the value network's too) instead of the kernels: A/B")
    return ap


def main():
    args = parser().parse_args()
    rank, world, dev, terrain = cli.setup(args)
    from cassierl_amd.ppo import make_cassie_ppo
    from cassierl_amd.trajectory import default_gait
    hidden = tuple(int(x) for x in args.hidden.split(","))
    # the environment: Cassie2d with its gait, or Cassie3d with its gains (which has neither gait nor kind: make_cassie_algo refuses them)
    env_kw = dict(trajectory=default_gait()) if args.env == "cassie2d" else dict(env="cassie3d", kp=args.kp, kd=args.kd)
    algo = make_cassie_ppo(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, seed=1,
                           hidden_sizes=hidden, init_std=args.init_std, learning_rate=args.learning_rate, clip_range=args.clip_range,
                           gae_lambda=args.gae_lambda, epochs=args.epochs, minibatch_size=args.minibatch_size or None, entropy_coeff=args.entropy_coeff,
                           batch_size=args.envs_per_gpu * world * args.horizon, terrain=terrain, value=args.value,
                           value_hidden=tuple(int(x) for x in args.value_hidden.split(",")), value_learning_rate=args.value_learning_rate, **env_kw)
    if args.torch_update:
        algo.fused_grad = algo.fused_adam = algo.fused_gae = algo.fused_value = False
    cli.train(algo, args, args.n_itr, rank)


if __name__ == "__main__":
    main()
