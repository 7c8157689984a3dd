"""What the seven train_*.py scripts share: the common flags, the set-up of a rank, the timed iteration loop with its JSON lines and snapshots, the
parameter dump and the teardown.  A script keeps its docstring, its own flags, its make_cassie_* call and what only it prints or dumps.  Nothing
here imports torch before a script has parsed its arguments (--help and parser() stay cheap)."""
import json
import time

HELP = dict(
    envs_per_gpu=None,
    timing="report rollout / update seconds separately (adds synchronisations)",
    terrain_seed="seed of the file draw and of the per-environment field ids",
    dump_params="rank 0 writes the flat policy parameters (.npy) after the last iteration")


def add_common_flags(ap, **help_of):
    """The flags every script has.  help_of: a script's own wording of a help string of HELP, by destination."""
    h = dict(HELP, **help_of)
    assert set(h) == set(HELP), sorted(set(h) - set(HELP))
    ap.add_argument("--envs-per-gpu", type=int, default=4096, help=h["envs_per_gpu"])
    ap.add_argument("--kind", default="walk", choices=["walk", "stand"])
    ap.add_argument("--control-mode", default="PD", choices=["PD", "Torque", "OSC"])
    ap.add_argument("--snapshot", default="")
    ap.add_argument("--load-policy", default="")
    ap.add_argument("--timing", action="store_true", help=h["timing"])
    ap.add_argument("--terrain-dir", default="", help="folder of terrain PNGs (model/terrains/ of the reference): robots on a terrain library")
    ap.add_argument("--num-terrains", type=int, default=1, help="K fields drawn (with replacement) from --terrain-dir")
    ap.add_argument("--terrain-elevation", type=float, default=1.0, help="height of a white pixel in metres (the <hfield> size_z)")
    ap.add_argument("--terrain-seed", type=int, default=1, help=h["terrain_seed"])
    ap.add_argument("--dump-params", default="", help=h["dump_params"])
    return ap


def add_pool_flags(ap, batch_size, batch_help, scale_reward, qf_learning_rate, policy_learning_rate):
    """The schedule and pool flags of train_ddpg.py, train_sac.py and train_td3.py; the arguments are the defaults in which they differ."""
    ap.add_argument("--batch-size", type=int, default=batch_size, help=batch_help)
    ap.add_argument("--updates-per-step", type=int, default=1, help="updates after every vector step (rllab's n_updates_per_sample)")
    ap.add_argument("--pool-size", type=int, default=0, help="rows of each rank's replay pool, a multiple of --envs-per-gpu (default: 1 000 000 rounded up to one); "
                    "a row is 4 (2 D + A + 2) bytes = 240 B for the 26-wide observation and 6 actions, so 1 000 000 rows are 240 MB and hold "
                    "16 vector steps of 65 536 environments")
    ap.add_argument("--min-pool-size", type=int, default=10000, help="transitions (over all ranks) before the first update")
    ap.add_argument("--epoch-length", type=int, default=1000, help="vector steps per epoch (one log line, one read-back)")
    ap.add_argument("--n-epochs", type=int, default=10)
    ap.add_argument("--max-path-length", type=int, default=100)
    ap.add_argument("--scale-reward", type=float, default=scale_reward)
    ap.add_argument("--qf-learning-rate", type=float, default=qf_learning_rate)
    ap.add_argument("--policy-learning-rate", type=float, default=policy_learning_rate)
    ap.add_argument("--snapshot-pool", type=int, default=1, help="0: the snapshot omits the replay pool (it can be gigabytes); a run loaded from it restarts with an empty pool")
    ap.add_argument("--torch-update", action="store_true", help="run the torch statements instead of the HIP kernels (A/B)")
    return ap


def pool_kwargs(args):
    """The keyword arguments of make_cassie_ddpg / _sac / _td3 that add_pool_flags and the common flags give."""
    return dict(replay_pool_size=args.pool_size or None, batch_size=args.batch_size, updates_per_step=args.updates_per_step, min_pool_size=args.min_pool_size,
                epoch_length=args.epoch_length, max_path_length=args.max_path_length, scale_reward=args.scale_reward, qf_learning_rate=args.qf_learning_rate,
                policy_learning_rate=args.policy_learning_rate, snapshot_pool=bool(args.snapshot_pool))


def setup(args):
    """Process group, device and terrain spec of this rank: (rank, world, device index, terrain spec or None)."""
    import torch
    from . import rollout as R
    from .terrain import terrain_spec
    rank, local_rank, world = R.init_distributed()
    dev = R.local_device(local_rank) if world > 1 else 0   # CASSIE_DEVICE_MAP (test hook): several ranks on one GPU
    torch.cuda.set_device(dev)
    terrain = terrain_spec(args.terrain_dir, args.num_terrains, args.terrain_elevation, args.terrain_seed) if args.terrain_dir else None
    return rank, world, dev, terrain


def pool_loaded(algo):
    """The off-policy scripts' entries of the load line."""
    return dict(pool_restored=algo.pool_restored, pool_size=algo.pool.size)


def pool_dump(*names, tail=()):
    """dump of the off-policy scripts: every rank writes the flat parameters of the networks `names` (then the tensors named by `tail`), rank
    r > 0 to <file>.rank<r>.npy -- the ranks must hold the same numbers."""
    def dump(algo, path, rank):
        import numpy as np
        import torch
        from .policy import flat_params
        flat = torch.cat([flat_params(getattr(algo, n)) for n in names] + [getattr(algo, n) for n in tail])
        np.save(path if rank == 0 else "%s.rank%d.npy" % (path, rank), flat.double().cpu().numpy())
    return dump


def policy_dump(algo, path, rank):
    """The default dump: rank 0 writes the flat policy parameters."""
    if rank == 0:
        import numpy as np
        from .policy import flat_params
        np.save(path, flat_params(algo.policy).double().cpu().numpy())


def train(algo, args, n_iterations, rank, loaded=None, line=None, dump=policy_dump):
    """--load-policy, n_iterations timed train_iteration()s -- rank 0 prints each one's dict as a JSON line with `seconds` (between two
    synchronisations) and `env_steps_per_s`, every rank writes --snapshot after each --, --dump-params, and the process group's teardown.
    loaded(algo) -> a script's entries of the load line; line(algo, st): adds a script's entries to an iteration's dict; dump(algo, path, rank)."""
    import torch
    import torch.distributed as dist
    algo.timing = args.timing
    if args.load_policy:
        _, restored = algo.load(args.load_policy)
        if rank == 0:
            print(json.dumps(dict(loaded=args.load_policy, itr=algo.itr, sampler_restored=restored, **(loaded(algo) if loaded else {}))))
    for _ in range(n_iterations):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = algo.train_iteration()
        torch.cuda.synchronize()
        st["seconds"] = time.perf_counter() - t0
        st["env_steps_per_s"] = st["env_steps"] / st["seconds"]
        if line is not None:
            line(algo, st)
        if rank == 0:
            print(json.dumps(st), flush=True)
        if args.snapshot:
            algo.save(args.snapshot)  # snapshot_mode="last"
    if args.dump_params:
        dump(algo, args.dump_params, rank)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
