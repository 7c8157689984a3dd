#!/usr/bin/env python3
"""PPO (clipped surrogate, GAE(lambda), epochs of minibatch Adam steps: cassierl_amd/ppo.py) on the batched MI355X environment; runs under
torchrun exactly as train_vpg.py does (`python -m torch.distributed.run --nproc-per-node 8 train_ppo.py --envs-per-gpu 65536`).

The policy and the environment are train_vpg.py's (MLP 128x128, init_std 1.0, discount 0.99, max_path_length 1000); batch_size is one Env.step of
every environment times --horizon, --minibatch-size counts samples over all ranks (default: a quarter of the batch).
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
    ap.add_argument("--horizon", type=int, default=4, help="Env.steps per environment per iteration")
    ap.add_argument("--n-itr", type=int, default=10)
    ap.add_argument("--env", default="cassie2d", choices=["cassie2d", "cassie3d"], help="cassie3d: the 3-D robot from its standing reset (45 observations, 10 actions)")
    ap.add_argument("--kind", default="walk", choices=["walk", "stand"])
    ap.add_argument("--control-mode", default="PD", choices=["PD", "Torque", "OSC"])
    ap.add_argument("--kp", type=float, default=10.0, help="--env cassie3d, PD mode: proportional gain of the ten actuated hinges")
    ap.add_argument("--kd", type=float, default=5.0, help="--env cassie3d, PD mode: damping gain")
    ap.add_argument("--snapshot", default="")
    ap.add_argument("--load-policy", default="")
    ap.add_argument("--timing", action="store_true", help="report rollout / update seconds separately (adds synchronisations)")
    ap.add_argument("--terrain-dir", default="", help="folder of terrain PNGs (model/terrains/ of the reference): robots on a terrain library")
    ap.add_argument("--num-terrains", type=int, default=1, help="K fields drawn (with replacement) from --terrain-dir")
    ap.add_argument("--terrain-elevation", type=float, default=1.0, help="height of a white pixel in metres (the <hfield> size_z)")
    ap.add_argument("--terrain-seed", type=int, default=1, help="seed of the file draw and of the per-environment field ids")
    ap.add_argument("--dump-params", default="", help="rank 0 writes the flat policy parameters (.npy) after the last iteration")
    ap.add_argument("--hidden", default="128,128", help="hidden layer widths of the Gaussian MLP policy")
    ap.add_argument("--init-std", type=float, default=1.0)
    ap.add_argument("--learning-rate", type=float, default=3e-4, help="Adam step size")
    ap.add_argument("--clip-range", type=float, default=0.2)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--epochs", type=int, default=4, help="passes over each rollout")
    ap.add_argument("--minibatch-size", type=int, default=0, help="samples per Adam step over all ranks (0: a quarter of the batch)")
    ap.add_argument("--entropy-coeff", type=float, default=0.0)
    ap.add_argument("--torch-update", action="store_true", help="force the torch statements (autograd, torch Adam, torch GAE) instead of the kernels: A/B")
    args = ap.parse_args()
    import torch
    from cassierl_amd import rollout as R
    from cassierl_amd.trajectory import default_gait
    from cassierl_amd.ppo import make_cassie_ppo
    rank, local_rank, world = R.init_distributed()
    dev = R.local_device(local_rank) if world > 1 else 0   # CASSIE_DEVICE_MAP (test hook): several ranks on one GPU
    torch.cuda.set_device(dev)
    from cassierl_amd.terrain import terrain_spec
    terrain = terrain_spec(args.terrain_dir, args.num_terrains, args.terrain_elevation, args.terrain_seed) if args.terrain_dir else None
    hidden = tuple(int(x) for x in args.hidden.split(","))
    # the environment: Cassie2d with its gait, or Cassie3d with its gains (which has neither gait nor kind: make_cassie_algo refuses them)
    env_kw = dict(trajectory=default_gait()) if args.env == "cassie2d" else dict(env="cassie3d", kp=args.kp, kd=args.kd)
    algo = make_cassie_ppo(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, seed=1,
                           hidden_sizes=hidden, init_std=args.init_std, learning_rate=args.learning_rate, clip_range=args.clip_range,
                           gae_lambda=args.gae_lambda, epochs=args.epochs, minibatch_size=args.minibatch_size or None, entropy_coeff=args.entropy_coeff,
                           batch_size=args.envs_per_gpu * world * args.horizon, terrain=terrain, **env_kw)
    algo.timing = args.timing
    if args.torch_update:
        algo.fused_grad = algo.fused_adam = algo.fused_gae = False
    if args.load_policy:
        _, restored = algo.load(args.load_policy)
        if rank == 0:
            print(json.dumps(dict(loaded=args.load_policy, itr=algo.itr, sampler_restored=restored)))
    for _ in range(args.n_itr):
        t0 = time.perf_counter()
        st = algo.train_iteration()
        torch.cuda.synchronize()
        st["seconds"] = time.perf_counter() - t0
        st["env_steps_per_s"] = st["env_steps"] / st["seconds"]
        if rank == 0:
            print(json.dumps(st))
        if args.snapshot:
            algo.save(args.snapshot)  # snapshot_mode="last"
    if args.dump_params and rank == 0:
        from cassierl_amd.trpo import flat_params
        np.save(args.dump_params, flat_params(algo.policy).double().cpu().numpy())
    if R.dist.is_initialized():
        R.dist.barrier()
        R.dist.destroy_process_group()


if __name__ == "__main__":
    main()
