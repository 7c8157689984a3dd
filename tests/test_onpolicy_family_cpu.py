"""The on-policy family's shape (cassierl_amd/sampler.py, trpo.py, vpg.py, ppo.py, es.py): the shared helpers defined once, one kernel-call base, process /
save / load / the Adam step / hidden_sizes in one class each, and what each algorithm writes into a snapshot and reports per iteration -- the
key lists are the ones the four modules had when each carried its own copy."""
import pytest
import torch

from cassierl_amd import _lib
from cassierl_amd import es as E
from cassierl_amd import offpolicy as O
from cassierl_amd import ppo as P
from cassierl_amd import sampler as SM
from cassierl_amd import trpo as T
from cassierl_amd import vpg as V
from test_trpo_cpu import ToyVecEnv

F64 = torch.float64
ALGOS = {"trpo": T.TRPO, "vpg": V.VPG, "ppo": P.PPO, "es": E.ES}
ADAM = {"adam_t", "adam_m", "adam_v"}

SNAPSHOT_KEYS = {
    "trpo": {"hidden_sizes"},
    "vpg": {"algo", "hidden_sizes", "learning_rate"} | ADAM,
    "ppo": {"algo", "hidden_sizes", "learning_rate", "clip_range", "gae_lambda", "epochs", "minibatch_size", "entropy_coeff", "gen_mb_state"} | ADAM,
    "es": {"algo", "hidden_sizes", "sigma", "learning_rate", "l2_coeff", "fitness_shaping", "max_path_length", "table_seed", "table_size", "gen_off_state"} | ADAM,
}
_TAIL = ["itr", "env_steps", "episodes", "avg_return", "avg_reward", "gathered"]
REPORT_KEYS = {
    "trpo": ["loss_before", "loss_after", "kl", "backtracks"] + _TAIL,
    "vpg": ["grad_norm", "step_norm"] + _TAIL,
    "ppo": ["loss_first", "loss_last", "mean_kl", "clip_frac", "grad_norm", "minibatch_steps"] + _TAIL,
    "es": ["itr", "env_steps", "episodes", "avg_return", "max_return", "min_return", "avg_path_length", "grad_norm", "step_norm", "gathered"],
}


def _toy(name, hidden=(32, 32), **kw):
    env = ToyVecEnv(16, 0)
    torch.manual_seed(0)
    pol = T.GaussianMLPPolicy(4, 2, hidden, init_std=1.0, dtype=F64)
    own = {"trpo": dict(batch_size=32), "vpg": dict(batch_size=32), "ppo": dict(batch_size=32, epochs=2, minibatch_size=8),
           "es": dict(max_path_length=20, table_size=1 << 14)}[name]
    return ALGOS[name](env.step, env.reset, pol, T.LinearFeatureBaseline(), 16, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"), seed=1, **own, **kw)


def test_shared_helpers_are_defined_once():
    for name in ("_MEAN_ORDER", "_two_layer_tanh", "closed_form_grad", "adam_step_", "fused_adam_step_", "FlatAdam", "hidden_sizes_of", "make_cassie_algo"):
        assert getattr(V, name) is getattr(T, name), name
    for name in ("_MEAN_ORDER", "_two_layer_tanh", "add_to_log_std_slot_", "FlatAdam", "make_cassie_algo"):
        assert getattr(P, name) is getattr(T, name), name
    for name in ("_two_layer_tanh", "FlatAdam", "make_cassie_algo"):
        assert getattr(E, name) is getattr(T, name), name
    assert O.adam_step_ is T.adam_step_ and O.make_cassie_algo is T.make_cassie_algo
    for mod in (T, P, E, O):
        assert mod.Kernels is _lib.Kernels and mod.available is _lib.available


def test_the_kernel_call_families_derive_from_the_one_base():
    for cls in (T.BaselineKernels, T.FusedFisher, T.PgFisher, P.ClipGradKernels, E.EsKernels, O.PoolKernels):
        assert issubclass(cls, _lib.Kernels), cls
        for method in ("_call", "_stream"):
            assert method not in cls.__dict__, (cls, method)
    assert issubclass(T.PgFisher, T.FusedFisher) and set(T.PgFisher.ENTRY) == set(T.FusedFisher.ENTRY)
    assert T.PgFisher.ENTRY["Vjp"] == "CassiePgVjp" and T.FusedFisher.ENTRY["Vjp"] == "CassieTrpoVjp"
    assert _lib.Kernels.STREAM_LAST and E.EsKernels.STREAM_LAST and not O.PoolKernels.STREAM_LAST
    exported = set(_lib.EXPORTS)
    for cls in (T.BaselineKernels, T.FusedFisher, T.PgFisher, E.EsKernels):
        assert set(cls.ENTRY.values()) <= exported, cls


def test_a_call_goes_through_fn_and_a_failure_names_the_symbol():
    k = _lib.Kernels.__new__(_lib.Kernels)
    k.ENTRY, k.STREAM_LAST, seen = {"Step": "CassieSomething"}, False, []
    k.fn = {"Step": lambda *a: seen.append(a) or 0}
    k._call("Step", 1, 2)
    assert seen == [(1, 2)]
    k.fn["Step"] = lambda *a: -3   # looked up at call time: a wrapped entry is what runs
    with pytest.raises(RuntimeError, match=r"CassieSomething failed \(-3\)"):
        k._call("Step")
    t = torch.zeros(3)
    assert _lib.ptr(None) is None and _lib.ptr(t).value == t.data_ptr()
    assert _lib.available("no_such_symbol_in_the_library") is False


@pytest.mark.parametrize("name", ["vpg", "ppo", "es"])
def test_shared_methods_live_in_one_class_alone(name):
    """Each shared method has one owner: Sampler (what all seven algorithms share), OnPolicy (TRPO, VPG, PPO: the batch and the baseline) or
    FlatAdam; TRPO owns its own update and nobody derives from it."""
    cls = ALGOS[name]
    base = SM.Sampler if name == "es" else SM.OnPolicy   # ES rolls whole episodes out itself: it is on Sampler's snapshot and gather alone
    assert issubclass(cls, base) and issubclass(cls, T.FlatAdam) and issubclass(SM.OnPolicy, SM.Sampler) and issubclass(T.TRPO, SM.OnPolicy)
    assert not issubclass(cls, T.TRPO) and (name != "es" or not issubclass(cls, SM.OnPolicy))
    for method in ("save", "load", "hidden_sizes", "_fused_sampler_step"):
        assert method not in cls.__dict__ and method not in SM.OnPolicy.__dict__ and method not in T.TRPO.__dict__ and method in SM.Sampler.__dict__, method
    for method in ("process", "_baseline_kernels", "_fused_policy_step"):
        assert method not in cls.__dict__ and method not in SM.Sampler.__dict__ and method not in T.TRPO.__dict__ and method in SM.OnPolicy.__dict__, method
        assert hasattr(cls, method) == (name != "es"), method
    assert "optimize" in T.TRPO.__dict__ and "optimize" not in SM.OnPolicy.__dict__ and not hasattr(SM.Sampler, "optimize")
    assert getattr(cls, "optimize", None) is not T.TRPO.optimize   # (the natural gradient, CG and line search: TRPO's alone)
    for method in ("adam_step", "_adam_snapshot", "_adam_load"):
        assert method not in cls.__dict__ and method in T.FlatAdam.__dict__, method
        assert all(method not in c.__dict__ for c in (T.TRPO, SM.OnPolicy, SM.Sampler)), method
    assert "process" not in O.OffPolicy.__dict__ and "save" not in O.OffPolicy.__dict__ and "hidden_sizes" not in O.OffPolicy.__dict__


@pytest.mark.parametrize("name", sorted(ALGOS))
def test_snapshot_fields_and_report_keys_are_the_algorithms_own(name):
    algo = _toy(name)
    assert algo.hidden_sizes == (32, 32)
    out = algo.train_iteration()
    assert list(out) == REPORT_KEYS[name]
    assert out["itr"] == 0 and algo.itr == 1
    fields = algo._snapshot_fields()
    assert set(fields) == SNAPSHOT_KEYS[name]
    assert fields.get("algo") == (None if name == "trpo" else name) and fields["hidden_sizes"] == [32, 32]
    if name != "trpo":
        assert fields["adam_t"] == algo.adam_t >= 1 and torch.equal(fields["adam_m"], algo.adam_m) and algo.last_adam_fused is False
        algo.adam_t, algo.adam_m = 7, None   # plain attributes: readable and writable
        assert algo._snapshot_fields()["adam_t"] == 7 and algo._snapshot_fields()["adam_m"] is None


def test_who_loads_whose_snapshot(tmp_path):
    """A plain TRPO run continues a VPG or an ES snapshot of the same policy shape; VPG, PPO and ES take back only their own; nobody on this
    side takes a ddpg snapshot."""
    paths = {}
    for name in sorted(ALGOS):
        a = _toy(name)
        a.train_iteration()
        paths[name] = str(tmp_path / (name + ".pt"))
        a.save(paths[name])
    for theirs in ("vpg", "es", "ppo", "trpo"):
        t = _toy("trpo")
        t.load(paths[theirs], restore_sampler=False)
        assert t.itr == 1
    with pytest.raises(ValueError, match="VPG.load: the snapshot was written by trpo, this run is vpg"):
        _toy("vpg").load(paths["trpo"])
    with pytest.raises(ValueError, match="PPO.load: the snapshot was written by vpg, this run is ppo"):
        _toy("ppo").load(paths["vpg"])
    with pytest.raises(ValueError, match="ES.load: the snapshot was written by ppo, this run is es"):
        _toy("es").load(paths["ppo"])
    ck = torch.load(paths["trpo"], weights_only=True)
    ck["algo"] = "ddpg"
    torch.save(ck, paths["trpo"])
    with pytest.raises(ValueError, match="TRPO.load: the snapshot was written by ddpg, this run is trpo"):
        _toy("trpo").load(paths["trpo"])
    with pytest.raises(ValueError, match=r"TRPO.load: the snapshot's policy has hidden sizes \(32, 32\), this run's has \(16, 16\)"):
        _toy("trpo", hidden=(16, 16)).load(paths["vpg"])
    v = _toy("vpg")
    v.load(paths["vpg"], restore_sampler=False)
    assert v.adam_t == 1 and v.adam_m is not None and v.adam_m.dtype == F64
