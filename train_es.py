#!/usr/bin/env python3
"""Evolution strategy (cassierl_amd/es.py) on the batched MI355X environment; runs under torchrun exactly as train_vpg.py does
(`python -m torch.distributed.run --nproc-per-node 8 train_es.py --envs-per-gpu 65536`).

Every environment runs its own perturbed copy of the policy (--hidden: 32,32 or 128,128 on the kernels) for one episode (two environments per direction, antithetic); an iteration
is one rollout of up to --max-path-length steps and one Adam step on the weighted sum of the directions.  Defaults are OpenAI's.
--env cassie3d runs the same loop on Cassie3dVecEnv (45 observations, 10 actions, --control-mode PD or Torque, --kp / --kd), both widths on the kernels.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cassierl_amd import train_cli as cli  # noqa: E402


def parser():
    ap = cli.add_common_flags(argparse.ArgumentParser(), envs_per_gpu="population per rank (even: two environments per direction)",
                              terrain_seed="seed of the file draw and of the per-pair field ids")
    ap.add_argument("--n-itr", type=int, default=10)
    ap.add_argument("--env", default="cassie2d", choices=["cassie2d", "cassie3d"], help="cassie3d: the 3-D robot from its standing reset (45 observations, 10 actions)")
    ap.add_argument("--kp", type=float, default=10.0, help="--env cassie3d, PD mode: proportional gain of the ten actuated hinges")
    ap.add_argument("--kd", type=float, default=5.0, help="--env cassie3d, PD mode: damping gain")
    ap.add_argument("--hidden", default="32,32", help="hidden layer widths of the policy (32,32 and 128,128 run on the kernels, any other on the torch statements)")
    ap.add_argument("--sigma", type=float, default=0.02, help="standard deviation of the parameter perturbations")
    ap.add_argument("--learning-rate", type=float, default=0.01, help="Adam step size")
    ap.add_argument("--l2-coeff", type=float, default=0.005, help="weight decay added to the descent direction")
    ap.add_argument("--max-path-length", type=int, default=1000, help="longest episode of an iteration")
    ap.add_argument("--table-size", type=int, default=1 << 24, help="entries of the shared noise table (float32)")
    ap.add_argument("--fitness-shaping", default="centered_rank", choices=["centered_rank", "zscore"])
    ap.add_argument("--torch-update", action="store_true", help="gradient and Adam step as torch statements (the rollout keeps its kernels)")
    return ap


def main():
    args = parser().parse_args()
    rank, world, dev, terrain = cli.setup(args)
    from cassierl_amd.es import make_cassie_es
    from cassierl_amd.trajectory import default_gait
    hidden = tuple(int(x) for x in args.hidden.split(","))
    env_kw = dict(trajectory=default_gait()) if args.env == "cassie2d" else dict(env="cassie3d", kp=args.kp, kd=args.kd)
    algo = make_cassie_es(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, seed=1, hidden_sizes=hidden, **env_kw,
                          terrain=terrain, sigma=args.sigma, learning_rate=args.learning_rate, l2_coeff=args.l2_coeff, max_path_length=args.max_path_length,
                          table_size=args.table_size, fitness_shaping=args.fitness_shaping)
    if args.torch_update:
        algo.fused_grad = algo.fused_adam = False
    cli.train(algo, args, args.n_itr, rank, line=lambda algo, st: st.update(policy_step=algo.last_policy_step_kind, grad=algo.last_grad_kind))


if __name__ == "__main__":
    main()
