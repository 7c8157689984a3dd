#!/usr/bin/env python3
"""Counterpart of rllab/envs/sim_policy.py:19-31 on the batched MI355X environment: load a snapshot written by train_trpo.py,
train_vpg.py, train_ddpg.py, train_sac.py, train_td3.py or train_es.py (`--snapshot`, snapshot_mode="last"; a VPG snapshot carries its policy's hidden sizes, a DDPG or TD3 snapshot is rolled out with mu(s), a SAC snapshot with tanh of the Gaussian's mean or sample, an ES snapshot with the unperturbed mean on an even number of envs) and roll the policy out -- no training.  The reference animates ONE env through rllab's
`rollout(env, policy, max_path_length, animated=True)`; here N resident envs run the same loop in parallel (there is no
viewer: GUI is out of scope) and the script prints what the reference's loop would let one read off the screen: path
lengths and returns.

    python sim_policy.py snapshot.pt --envs 1024 --max-path-length 1000 [--kind stand --control-mode Torque] [--deterministic]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file", help="snapshot written by --snapshot of train_trpo.py, train_vpg.py, train_ppo.py, train_ddpg.py, train_sac.py, train_td3.py or train_es.py")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--max-path-length", type=int, default=1000)   # sim_policy.py:14 default
    ap.add_argument("--kind", default="walk", choices=["walk", "stand"])
    ap.add_argument("--control-mode", default="PD", choices=["PD", "Torque", "OSC"])
    ap.add_argument("--deterministic", action="store_true", help="act with the policy mean (no exploration noise)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--terrain-dir", default="", help="folder of terrain PNGs (model/terrains/ of the reference): robots on a terrain library")
    ap.add_argument("--num-terrains", type=int, default=1, help="K fields drawn (with replacement) from --terrain-dir")
    ap.add_argument("--terrain-elevation", type=float, default=1.0, help="height of a white pixel in metres (the <hfield> size_z)")
    ap.add_argument("--terrain-seed", type=int, default=1, help="seed of the file draw and of the per-environment field ids")
    args = ap.parse_args()
    import torch
    from cassierl_amd import rollout as R
    from cassierl_amd.trajectory import default_gait
    from cassierl_amd.trpo import make_cassie_trpo
    from cassierl_amd.terrain import terrain_spec
    terrain = terrain_spec(args.terrain_dir, args.num_terrains, args.terrain_elevation, args.terrain_seed) if args.terrain_dir else None
    ck = torch.load(args.file, map_location="cpu", weights_only=True)
    if ck.get("algo") == "vpg":   # a train_vpg.py snapshot: the policy's shape comes from it
        from cassierl_amd.vpg import make_cassie_vpg
        algo = make_cassie_vpg(args.envs, kind=args.kind, control_mode=args.control_mode, device=0, trajectory=default_gait(), seed=args.seed,
                               terrain=terrain, hidden_sizes=tuple(ck.get("hidden_sizes", (32, 32))))
    elif ck.get("algo") == "ppo":   # a train_ppo.py snapshot: the policy's shape comes from it; only the policy is loaded, so the batch shape is free
        from cassierl_amd.ppo import make_cassie_ppo
        if ck.get("env_family", "cassie2d") == "cassie3d":   # written by train_ppo.py --env cassie3d: the control mode and gains are the snapshot's
            cfg = ck["env_config"]
            env_kw = dict(env="cassie3d", control_mode=cfg["control_mode"], kp=cfg["kp"], kd=cfg["kd"])
        else:
            env_kw = dict(kind=args.kind, control_mode=args.control_mode, trajectory=default_gait(), terrain=terrain)
        algo = make_cassie_ppo(args.envs, device=0, seed=args.seed, hidden_sizes=tuple(ck.get("hidden_sizes", (128, 128))), batch_size=args.envs,
                               minibatch_size=args.envs, value=ck.get("value_kind", "linear"), value_hidden=tuple(ck.get("value_hidden", (128, 128))), **env_kw)
    elif ck.get("algo") == "es":   # a train_es.py snapshot: the unperturbed parameters, rolled out with the mean (the noise table is the snapshot's)
        from cassierl_amd.es import make_cassie_es
        if args.envs % 2:
            ap.error("an ES snapshot needs an even --envs (two environments per direction), got %d" % args.envs)
        if ck.get("env_family", "cassie2d") == "cassie3d":   # written by train_es.py --env cassie3d: the control mode and gains are the snapshot's
            cfg = ck["env_config"]
            env_kw = dict(env="cassie3d", control_mode=cfg["control_mode"], kp=cfg["kp"], kd=cfg["kd"])
        else:
            env_kw = dict(kind=args.kind, control_mode=args.control_mode, trajectory=default_gait(), terrain=terrain)
        algo = make_cassie_es(args.envs, device=0, seed=args.seed, **env_kw,
                              hidden_sizes=tuple(ck.get("hidden_sizes", (32, 32))), table_size=ck["table_size"], table_seed=ck["table_seed"])
        args.deterministic = True
    elif ck.get("algo") == "ddpg":   # a train_ddpg.py snapshot: the deterministic actor mu(s); only the policy is loaded, so the smallest pool will do
        from cassierl_amd.ddpg import make_cassie_ddpg
        algo = make_cassie_ddpg(args.envs, kind=args.kind, control_mode=args.control_mode, device=0, trajectory=default_gait(), seed=args.seed,
                                terrain=terrain, replay_pool_size=args.envs)
        args.deterministic = True
    elif ck.get("algo") == "td3":   # a train_td3.py snapshot: the deterministic actor mu(s), as for DDPG
        from cassierl_amd.td3 import make_cassie_td3
        algo = make_cassie_td3(args.envs, kind=args.kind, control_mode=args.control_mode, device=0, trajectory=default_gait(), seed=args.seed,
                               terrain=terrain, replay_pool_size=args.envs)
        args.deterministic = True
    elif ck.get("algo") == "sac":   # a train_sac.py snapshot: the squashed Gaussian; only the actor is loaded, so the smallest pool will do
        from cassierl_amd.sac import make_cassie_sac
        if ck.get("env_family", "cassie2d") == "cassie3d":   # written by train_sac.py --env cassie3d: the control mode and gains are the snapshot's
            cfg = ck["env_config"]
            env_kw = dict(env="cassie3d", control_mode=cfg["control_mode"], kp=cfg["kp"], kd=cfg["kd"])
        else:
            env_kw = dict(kind=args.kind, control_mode=args.control_mode, trajectory=default_gait(), terrain=terrain)
        algo = make_cassie_sac(args.envs, device=0, seed=args.seed, replay_pool_size=args.envs, **env_kw)
    else:   # a train_trpo.py snapshot: 32 x 32 unless it records other hidden sizes
        algo = make_cassie_trpo(args.envs, kind=args.kind, control_mode=args.control_mode, device=0, trajectory=default_gait(), seed=args.seed,
                                terrain=terrain, hidden_sizes=tuple(ck.get("hidden_sizes", (32, 32))))
    squashed = ck.get("algo") == "sac"   # the action is tanh of the Gaussian's mean (--deterministic) or sample
    del ck
    _, _ = algo.load(args.file, restore_sampler=False)   # policy + baseline only: every path starts from env.reset()
    pol, n = algo.policy, args.envs
    dt = next(pol.parameters()).dtype
    obs = algo.env_reset().clone()
    alive = torch.ones(n, dtype=torch.bool, device=obs.device)
    ret = torch.zeros(n, dtype=torch.float64, device=obs.device)
    length = torch.zeros(n, dtype=torch.int64, device=obs.device)
    with torch.no_grad():
        for t in range(args.max_path_length):     # rllab.sampler.utils.rollout: until done or max_path_length
            mean, log_std = (pol(obs.to(dt)), None) if args.deterministic and not hasattr(pol, "dist_info") else pol.dist_info(obs.to(dt))
            a = mean if args.deterministic else mean + R.counter_normal(args.seed, algo.env_ids, t, mean.shape[1]).to(dt) * log_std.exp()
            if squashed:
                a = torch.tanh(a)
            obs, rew, done = algo.env_step(algo.act_map(a))
            ret += torch.where(alive, rew, torch.zeros_like(rew))
            length += alive.to(torch.int64)
            alive &= ~done.bool()
            obs = obs.clone()
            if t % 50 == 49 and not bool(alive.any()):
                break
    print(json.dumps(dict(snapshot=args.file, itr=algo.itr, envs=n, max_path_length=args.max_path_length, deterministic=args.deterministic,
                          avg_return=float(ret.mean()), min_return=float(ret.min()), max_return=float(ret.max()),
                          avg_path_length=float(length.double().mean()), paths_reaching_max_length=int(alive.sum()))))
    algo.env.close()


if __name__ == "__main__":
    main()
