"""The learning layer's cut (cassierl_amd/comm.py, policy.py, baseline.py, adam.py, fisher.py, sampler.py, trpo.py, train_cli.py): who may import
what from trpo.py, the collective timer that bench.py installs as `trpo.COMM`, and the snapshot's top-level keys of all seven algorithms.  The span
names and the key lists were recorded on the commit before the cut, when trpo.py held all of it."""
import ast
import glob
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cassierl_amd import ddpg as G
from cassierl_amd import es as E
from cassierl_amd import ppo as P
from cassierl_amd import sac as S
from cassierl_amd import td3 as D3
from cassierl_amd import trpo as T
from cassierl_amd import vpg as V
from test_trpo_cpu import ToyVecEnv, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---- import direction
def _trpo_names(path):
    """What the file takes from cassierl_amd.trpo: (names imported from it, attributes read through a name the module is bound to)."""
    tree = ast.parse(open(path).read(), path)
    imported, aliases = set(), set()
    for n in ast.walk(tree):
        if isinstance(n, ast.ImportFrom) and (n.module or "") in ("trpo", "cassierl_amd.trpo"):   # from .trpo import X / from cassierl_amd.trpo import X
            imported |= {a.name for a in n.names}
        elif isinstance(n, ast.ImportFrom) and (n.module or "") in ("", "cassierl_amd"):          # from . import trpo / from cassierl_amd import trpo as T
            aliases |= {a.asname or a.name for a in n.names if a.name == "trpo"}
        elif isinstance(n, ast.Import):
            aliases |= {a.asname or a.name for a in n.names if a.name == "cassierl_amd.trpo"}
    attrs = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id in aliases}
    return imported, attrs


def _reexported():
    """The names of trpo.py's trailing re-export: every module-level `from .<module> import ...` behind the last definition."""
    tree = ast.parse(open(os.path.join(ROOT, "cassierl_amd", "trpo.py")).read())
    last_def = max(i for i, n in enumerate(tree.body) if isinstance(n, (ast.FunctionDef, ast.ClassDef)))
    tail = tree.body[last_def + 1:]
    assert tail and all(isinstance(n, ast.ImportFrom) and n.level == 1 for n in tail), "trpo.py ends with its re-exports and nothing else"
    return {a.asname or a.name for n in tail for a in n.names}


def test_only_the_algorithm_is_imported_from_trpo():
    files = sorted(glob.glob(os.path.join(ROOT, "cassierl_amd", "*.py")) + glob.glob(os.path.join(ROOT, "train_*.py"))) + [os.path.join(ROOT, "sim_policy.py")]
    assert len(files) > 20
    for path in files:
        imported, attrs = _trpo_names(path)
        assert imported <= {"TRPO", "make_cassie_trpo"}, (path, imported)
        assert attrs <= {"COMM"}, (path, attrs)   # (the timer slot, looked up at call time: comm.py, sampler.py)


def test_the_reexports_of_trpo_are_the_names_its_users_reach_through_it():
    used = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) + [os.path.join(ROOT, "bench.py")]:
        imported, attrs = _trpo_names(path)
        used |= imported | attrs
    # the family tests reach these through getattr(T, name) / `mod.Kernels`, which the parse above cannot see
    used |= {"_MEAN_ORDER", "_two_layer_tanh", "closed_form_grad", "adam_step_", "fused_adam_step_", "FlatAdam", "hidden_sizes_of", "make_cassie_algo",
             "add_to_log_std_slot_", "Kernels", "available"}
    own = {"TRPO", "make_cassie_trpo", "COMM"}
    re = _reexported()
    assert not re & own
    assert re - used == set(), "re-exported but reached by nothing under tests/, tools/ or bench.py"
    bound = {a.asname or a.name for n in ast.parse(open(os.path.join(ROOT, "cassierl_amd", "trpo.py")).read()).body if isinstance(n, ast.ImportFrom) for a in n.names}
    assert used - own - bound == set(), "reached through trpo but not there"   # (what TRPO imports for itself needs no re-export)
    for name in used:
        assert hasattr(T, name), name


# ---- the timer through trpo.COMM
TRPO_SPANS = {"advantage_all_reduce", "baseline_all_reduce", "gradient_all_reduce", "fvp_all_reduce", "line_search_all_reduce", "stats_all_reduce",
              "returns_all_gather"}
PPO_SPANS = {"advantage_all_reduce", "baseline_all_reduce", "gradient_all_reduce", "stats_all_reduce", "returns_all_gather"}


def _on_policy(cls, n=16, **kw):
    env = ToyVecEnv(n, 0)
    torch.manual_seed(0)
    pol = T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=F64)
    return cls(env.step, env.reset, pol, T.LinearFeatureBaseline(), n, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"), seed=1, **kw)


def _timer_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for name, cls, kw in (("trpo", T.TRPO, dict(batch_size=64)), ("ppo", P.PPO, dict(batch_size=64, epochs=2, minibatch_size=16))):
        algo = _on_policy(cls, **kw)
        T.COMM = T.CommTimer()   # bench.py's statements around its timed TRPO iterations
        algo.train_iteration()
        out[name] = T.COMM.summary()
        T.COMM = None
    algo.train_iteration()
    out["off"] = T.COMM
    if rank == 0:
        q.put(out)
    dist.destroy_process_group()


def test_a_timer_set_as_trpo_comm_sees_every_collective():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_timer_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=180)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    print({k: (sorted(v) if v else v) for k, v in out.items()})
    for name, spans in (("trpo", TRPO_SPANS), ("ppo", PPO_SPANS)):
        assert set(out[name]) == spans, name
        assert all(v["calls"] > 0 and v["total_ms"] >= 0.0 for v in out[name].values()), name
    assert out["trpo"]["returns_all_gather"]["calls"] == 1 and out["trpo"]["baseline_all_reduce"]["calls"] == 2
    assert out["ppo"]["gradient_all_reduce"]["calls"] == 2 * 4   # epochs x minibatches (a rank's 32 samples in minibatches of 16 / 2 ranks = 8)
    assert out["off"] is None


# ---- the snapshot's top-level keys
COMMON = {"n_envs_global", "policy", "baseline", "itr", "extra", "noise_step", "noise_seed", "gen_state", "obs", "path_t", "path_ret", "steps_to_trunc",
          "env_state", "terrain", "env_family", "env_config", "hidden_sizes"}
ADAM = {"adam_t", "adam_m", "adam_v"}
POOL = {"algo", "idx_gen_state", "n_updates", "pool"}
SNAPSHOT_KEYS = {
    "trpo": COMMON,
    "vpg": COMMON | ADAM | {"algo", "learning_rate"},
    "ppo": COMMON | ADAM | {"algo", "learning_rate", "clip_range", "gae_lambda", "epochs", "minibatch_size", "entropy_coeff", "gen_mb_state"},
    "es": COMMON | ADAM | {"algo", "sigma", "learning_rate", "l2_coeff", "fitness_shaping", "max_path_length", "table_seed", "table_size", "gen_off_state"},
    "ddpg": COMMON | POOL | {"qf", "target_policy", "target_qf", "adam_mu", "adam_q", "ou_state"},
    "sac": COMMON | POOL | {"qf1", "qf2", "target_qf1", "target_qf2", "log_alpha", "adam_pi", "adam_q1", "adam_q2", "adam_alpha"},
    "td3": COMMON | POOL | {"qf1", "qf2", "target_policy", "target_qf1", "target_qf2", "adam_mu", "adam_q1", "adam_q2", "noise_gen_state"},
}


def _off_policy(name):
    env = ToyVecEnv(4, 0)
    torch.manual_seed(0)
    qf = lambda: G.ContinuousMLPQFunction(4, 2, dtype=F64)
    cls, nets = {"ddpg": (G.DDPG, lambda: (G.DeterministicMLPPolicy(4, 2, dtype=F64), qf())),
                 "sac": (S.SAC, lambda: (S.SquashedGaussianMLPPolicy(4, 2, dtype=F64), qf(), qf())),
                 "td3": (D3.TD3, lambda: (G.DeterministicMLPPolicy(4, 2, dtype=F64), qf(), qf()))}[name]
    return cls(env.step, env.reset, *nets(), 4, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"), batch_size=4, epoch_length=3, min_pool_size=4,
               replay_pool_size=8, seed=1)


def _algo(name):
    if name in ("ddpg", "sac", "td3"):
        return _off_policy(name)
    cls, kw = {"trpo": (T.TRPO, dict(batch_size=32)), "vpg": (V.VPG, dict(batch_size=32)), "ppo": (P.PPO, dict(batch_size=32, epochs=2, minibatch_size=8)),
               "es": (E.ES, dict(max_path_length=20, table_size=1 << 14))}[name]
    return _on_policy(cls, **kw)


@pytest.mark.parametrize("name", sorted(SNAPSHOT_KEYS))
def test_snapshot_keys_are_those_of_the_commit_before_the_cut(name, tmp_path):
    algo = _algo(name)
    algo.train_iteration()
    path = str(tmp_path / "snap.pt")
    algo.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    print(name, sorted(ck))
    assert set(ck) == SNAPSHOT_KEYS[name]
    assert ("algo" in ck) == (name != "trpo") and ck.get("algo", "trpo") == name
    assert (ck["baseline"] is None) == (name in ("es", "ddpg", "sac", "td3"))   # ES never fits its baseline; the pool's algorithms have none
    other = _algo(name)
    _, restored = other.load(path)
    assert other.itr == 1 and not restored   # (the toy environment has no state record: policy, optimiser and iteration only)
    for k, v in algo.policy.state_dict().items():
        assert torch.equal(other.policy.state_dict()[k], v), k
