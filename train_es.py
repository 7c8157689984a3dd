#!/usr/bin/env python3
"""Evolution strategy (cassierl_amd/es.py) on the batched MI355X environment; runs under torchrun exactly as train_vpg.py does
(`python -m torch.distributed.run --nproc-per-node 8 train_es.py --envs-per-gpu 65536`).

Every environment runs its own perturbed copy of the policy (--hidden: 32,32 or 128,128 on the kernels) for one episode (two environments per direction, antithetic); an iteration
is one rollout of up to --max-path-length steps and one Adam step on the weighted sum of the directions.  Defaults are OpenAI's.
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
    ap.add_argument("--envs-per-gpu", type=int, default=4096, help="population per rank (even: two environments per direction)")
    ap.add_argument("--n-itr", type=int, default=10)
    ap.add_argument("--kind", default="walk", choices=["walk", "stand"])
    ap.add_argument("--control-mode", default="PD", choices=["PD", "Torque", "OSC"])
    ap.add_argument("--snapshot", default="")
    ap.add_argument("--load-policy", default="")
    ap.add_argument("--timing", action="store_true", help="report rollout / update seconds separately (adds synchronisations)")
    ap.add_argument("--terrain-dir", default="", help="folder of terrain PNGs (model/terrains/ of the reference): robots on a terrain library")
    ap.add_argument("--num-terrains", type=int, default=1, help="K fields drawn (with replacement) from --terrain-dir")
    ap.add_argument("--terrain-elevation", type=float, default=1.0, help="height of a white pixel in metres (the <hfield> size_z)")
    ap.add_argument("--terrain-seed", type=int, default=1, help="seed of the file draw and of the per-pair field ids")
    ap.add_argument("--dump-params", default="", help="rank 0 writes the flat policy parameters (.npy) after the last iteration")
    ap.add_argument("--hidden", default="32,32", help="hidden layer widths of the policy (32,32 and 128,128 run on the kernels, any other on the torch statements)")
    ap.add_argument("--sigma", type=float, default=0.02, help="standard deviation of the parameter perturbations")
    ap.add_argument("--learning-rate", type=float, default=0.01, help="Adam step size")
    ap.add_argument("--l2-coeff", type=float, default=0.005, help="weight decay added to the descent direction")
    ap.add_argument("--max-path-length", type=int, default=1000, help="longest episode of an iteration")
    ap.add_argument("--table-size", type=int, default=1 << 24, help="entries of the shared noise table (float32)")
    ap.add_argument("--fitness-shaping", default="centered_rank", choices=["centered_rank", "zscore"])
    ap.add_argument("--torch-update", action="store_true", help="gradient and Adam step as torch statements (the rollout keeps its kernels)")
    args = ap.parse_args()
    import torch
    from cassierl_amd import rollout as R
    from cassierl_amd.es import make_cassie_es
    from cassierl_amd.trajectory import default_gait
    rank, local_rank, world = R.init_distributed()
    dev = R.local_device(local_rank) if world > 1 else 0   # CASSIE_DEVICE_MAP (test hook): several ranks on one GPU
    torch.cuda.set_device(dev)
    from cassierl_amd.terrain import terrain_spec
    terrain = terrain_spec(args.terrain_dir, args.num_terrains, args.terrain_elevation, args.terrain_seed) if args.terrain_dir else None
    hidden = tuple(int(x) for x in args.hidden.split(","))
    algo = make_cassie_es(args.envs_per_gpu, kind=args.kind, control_mode=args.control_mode, device=dev, trajectory=default_gait(), seed=1, hidden_sizes=hidden,
                          terrain=terrain, sigma=args.sigma, learning_rate=args.learning_rate, l2_coeff=args.l2_coeff, max_path_length=args.max_path_length,
                          table_size=args.table_size, fitness_shaping=args.fitness_shaping)
    algo.timing = args.timing
    if args.torch_update:
        algo.fused_grad = algo.fused_adam = False
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
        st.update(policy_step=algo.last_policy_step_kind, grad=algo.last_grad_kind)
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
