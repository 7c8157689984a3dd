"""TRPO with the 128x128 policy on CPU: the factory and CLI options, the Fisher-object choice, learning on the toy env, and the hidden sizes
that TRPO snapshots record and check."""
import inspect
import os
import sys

import pytest
import torch

from cassierl_amd import trpo as T
from test_trpo_cpu import ToyVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train_trpo_parser():
    sys.path.insert(0, ROOT)
    import train_trpo
    return train_trpo.parser()


def test_make_cassie_trpo_takes_the_policy_shape_with_trpo_cassie_defaults():
    sig = inspect.signature(T.make_cassie_trpo).parameters
    assert sig["hidden_sizes"].default == (32, 32) and sig["init_std"].default == 2.0


def test_train_trpo_parser_accepts_hidden_and_init_std():
    ap = _train_trpo_parser()
    d = ap.parse_args([])
    assert d.hidden == "32,32" and d.init_std == 2.0
    a = ap.parse_args(["--hidden", "128,128", "--init-std", "1.0"])
    assert tuple(int(x) for x in a.hidden.split(",")) == (128, 128) and a.init_std == 1.0


def _toy_trpo(n=64, seed=1, hidden=(128, 128), env=None, **kw):
    env = env or ToyVecEnv(n, seed)
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(4, 2, hidden, init_std=1.0, dtype=torch.float64)
    algo = T.TRPO(env.step, env.reset, pol, T.LinearFeatureBaseline(), n, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"),
                  batch_size=n * 40, max_path_length=1000, discount=0.99, step_size=0.01, seed=seed, **kw)
    return algo


def test_wide_trpo_picks_the_analytic_fisher_on_cpu_and_improves_reward_on_toy_env():
    algo = _toy_trpo(n=128, seed=3)
    first = algo.train_iteration()["avg_reward"]
    assert algo.last_fisher_kind == "analytic"
    for _ in range(25):
        st = algo.train_iteration()
    last = st["avg_reward"]
    assert st["kl"] <= 0.01 + 1e-9 and algo.last_fisher_kind == "analytic"
    assert last > first + 0.05, (first, last)
    algo.analytic_fisher = False
    algo.train_iteration()
    assert algo.last_fisher_kind == "autograd"


def test_snapshot_records_hidden_sizes_and_load_refuses_other_ones(tmp_path):
    a = _toy_trpo(n=16)
    a.train_iteration()
    p = str(tmp_path / "wide.pt")
    a.save(p)
    ck = torch.load(p, weights_only=True)
    assert ck["hidden_sizes"] == [128, 128] and "algo" not in ck
    b = _toy_trpo(n=16, seed=4)
    b.load(p)
    assert b.itr == 1 and torch.equal(T.flat_params(a.policy), T.flat_params(b.policy))
    narrow = _toy_trpo(n=16, hidden=(32, 32))
    before = T.flat_params(narrow.policy).clone()
    with pytest.raises(ValueError, match=r"\(128, 128\).*\(32, 32\)"):
        narrow.load(p)
    assert torch.equal(T.flat_params(narrow.policy), before)


def test_snapshot_without_hidden_sizes_is_a_32x32_run(tmp_path):
    a = _toy_trpo(n=16, hidden=(32, 32))
    a.train_iteration()
    p = str(tmp_path / "old.pt")
    a.save(p)
    ck = torch.load(p, weights_only=True)
    assert ck.pop("hidden_sizes") == [32, 32]
    torch.save(ck, p)   # what a snapshot of an earlier version holds
    b = _toy_trpo(n=16, seed=5, hidden=(32, 32))
    b.load(p)
    assert torch.equal(T.flat_params(a.policy), T.flat_params(b.policy))
    with pytest.raises(ValueError, match=r"\(32, 32\).*\(128, 128\)"):
        _toy_trpo(n=16).load(p)
