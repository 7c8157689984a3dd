"""The off-policy family's shape (cassierl_amd/offpolicy.py): one base class, the shared helpers defined once, and what each algorithm writes
into a snapshot and reports per epoch -- the key lists are the ones ddpg.py, sac.py and td3.py had when each carried its own copy."""
import pytest
import torch

from cassierl_amd import ddpg as G
from cassierl_amd import offpolicy as O
from cassierl_amd import sac as S
from cassierl_amd import sampler as SM
from cassierl_amd import td3 as D3
from cassierl_amd import trpo as T
from test_trpo_cpu import ToyVecEnv

F64 = torch.float64
ALGOS = {"ddpg": G.DDPG, "sac": S.SAC, "td3": D3.TD3}

SNAPSHOT_KEYS = {
    "ddpg": {"algo", "hidden_sizes", "qf", "target_policy", "target_qf", "adam_mu", "adam_q", "ou_state", "idx_gen_state", "n_updates", "pool"},
    "sac": {"algo", "hidden_sizes", "qf1", "qf2", "target_qf1", "target_qf2", "log_alpha", "adam_pi", "adam_q1", "adam_q2", "adam_alpha", "idx_gen_state",
            "n_updates", "pool"},
    "td3": {"algo", "hidden_sizes", "qf1", "qf2", "target_policy", "target_qf1", "target_qf2", "adam_mu", "adam_q1", "adam_q2", "idx_gen_state",
            "noise_gen_state", "n_updates", "pool"},
}
REPORT_KEYS = {
    "ddpg": ["itr", "env_steps", "updates", "pool_size", "avg_reward", "episodes", "avg_return", "qf_loss", "avg_q", "policy_surr", "update_kind"],
    "sac": ["itr", "env_steps", "updates", "pool_size", "avg_reward", "episodes", "avg_return", "qf_loss", "avg_q", "qf1_loss", "qf2_loss", "policy_loss",
            "avg_log_pi", "avg_min_q", "alpha", "update_kind"],
    "td3": ["itr", "env_steps", "updates", "actor_updates", "pool_size", "avg_reward", "episodes", "avg_return", "qf1_loss", "qf2_loss", "avg_q1", "avg_q2",
            "policy_surr", "update_kind"],
}


def _toy(name):
    env = ToyVecEnv(4, 0)
    torch.manual_seed(0)
    qf = lambda: G.ContinuousMLPQFunction(4, 2, dtype=F64)
    nets = {"ddpg": lambda: (G.DeterministicMLPPolicy(4, 2, dtype=F64), qf()), "sac": lambda: (S.SquashedGaussianMLPPolicy(4, 2, dtype=F64), qf(), qf()),
            "td3": lambda: (G.DeterministicMLPPolicy(4, 2, dtype=F64), qf(), qf())}[name]()
    return ALGOS[name](env.step, env.reset, *nets, 4, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"), batch_size=4, epoch_length=3, min_pool_size=4,
                       replay_pool_size=8, seed=1)


def test_the_three_algorithms_derive_from_the_base_and_not_from_each_other():
    for cls in ALGOS.values():
        assert issubclass(cls, O.OffPolicy) and issubclass(cls, SM.Sampler)
        assert not issubclass(cls, T.TRPO) and not issubclass(cls, SM.OnPolicy)
    assert issubclass(T.TRPO, SM.Sampler) and not issubclass(O.OffPolicy, T.TRPO)
    for method in ("optimize", "collect", "process", "_baseline_kernels", "_advantages"):   # what only an on-policy algorithm can run
        assert not hasattr(O.OffPolicy, method), method
    for method in ("save", "_book_step", "_reset_truncated", "_fused_sampler_step", "_gather_returns", "_check_env_family"):   # the sampler state and the snapshot
        assert method in SM.Sampler.__dict__ and method not in O.OffPolicy.__dict__, method
    assert not issubclass(S.SAC, G.DDPG) and not issubclass(D3.TD3, G.DDPG)
    for cls in (G.DdpgKernels, S.SacKernels, D3.Td3Kernels):
        assert issubclass(cls, O.PoolKernels)


def test_shared_helpers_are_defined_once():
    for name in ("ReplayPool", "new_adam", "soft_update_", "_ptrs", "_adam_on", "default_pool_size", "broadcast_initial_networks"):
        assert getattr(G, name) is getattr(O, name), name
    assert not hasattr(O, "_NoBaseline") and not hasattr(G, "_NoBaseline")   # (stood in for a baseline while OffPolicy derived from TRPO)
    for mod in (S, D3):
        for name in ("new_adam", "soft_update_", "_ptrs", "broadcast_initial_networks"):
            assert getattr(mod, name) is getattr(O, name), (mod.__name__, name)


@pytest.mark.parametrize("name", sorted(ALGOS))
def test_shared_methods_live_in_the_base_alone(name):
    for method in ("_fused_step", "train_iteration", "load", "_load_fields", "_snapshot_fields", "train_step", "env_step_into_pool", "_update_kernels"):
        assert method not in ALGOS[name].__dict__, method
        assert method in O.OffPolicy.__dict__, method


@pytest.mark.parametrize("name", sorted(ALGOS))
def test_snapshot_fields_are_the_algorithms_own(name):
    algo = _toy(name)
    fields = algo._snapshot_fields()
    assert set(fields) == SNAPSHOT_KEYS[name]
    assert fields["algo"] == name and fields["pool"]["capacity"] == 8


@pytest.mark.parametrize("name", sorted(ALGOS))
def test_epoch_report_keys_and_their_order(name):
    algo = _toy(name)
    out = algo.train_iteration()
    assert list(out) == REPORT_KEYS[name]
    assert out["updates"] == 3 and out["update_kind"] == "torch" and out["itr"] == 0 and algo.itr == 1
