"""ES on Cassie3d, the parts that need no GPU: the builder's refusals (raised before any device is touched), the CassieEs3d* exports and their
parameter counts, which entries the kernel-call layer picks at 45 x 10, the environment family in snapshots, and the torch statement at 45 x 10
against a loop over the environments' own weights w_i."""
import ctypes as ct
import os
import re

import pytest
import torch

from cassierl_amd import es as E
from cassierl_amd import trpo as T
from conftest import ROOT
from test_es_cpu import FixedTargetEnv

D, A = 45, 10
NARROW, WIDE = (32, 32), (128, 128)
PD = dict(control_mode="PD", kp=[10.0] * 10, kd=[5.0] * 10)
NAMES = {NARROW: ["CassieEs3dParamCount", "CassieEs3dPairsPerWorkgroup", "CassieEs3dPolicyStep"],
         WIDE: ["CassieEs3dWideParamCount", "CassieEs3dWidePairsPerWorkgroup", "CassieEs3dWidePolicyStep"]}
COUNT = {NARROW: 2858, WIDE: 23690}


# ---------------------------------------------------------------------------------------------------------------------- the builder
@pytest.mark.parametrize("kw,match", [(dict(terrain=dict(seed=1, files=["a.png"])), "terrain"), (dict(trajectory=object()), "gait"), (dict(kind="stand"), "kind"),
                                      (dict(control_mode="OSC"), "OSC")])
def test_builder_refuses_what_cassie3d_does_not_have(kw, match):
    """Device 123456 does not exist, and nothing gets as far as asking for it."""
    assert E.ES.CASSIE3D
    with pytest.raises(ValueError, match=match):
        E.make_cassie_es(64, env="cassie3d", device=123456, **kw)


def test_builder_refuses_an_unknown_family():
    assert E.ES.CASSIE3D
    with pytest.raises(ValueError, match="cassie2d.*cassie3d"):
        E.make_cassie_es(64, env="cassie4d", device=123456)


# ---------------------------------------------------------------------------------------------------------------------- the library
def test_the_library_exports_the_six_entry_points_and_counts_parameters():
    from cassierl_amd import _lib
    from cassierl_amd import build as B
    L = ct.CDLL(B.build())
    hdr = open(os.path.join(ROOT, "include", "cassie_trpo.h")).read()
    assert "tu_es3d" in B.UNITS and os.path.exists(os.path.join(B.CSRC, "tu_es3d.hip"))
    for hidden, names in NAMES.items():
        for s in names:
            assert hasattr(L, s), "missing export " + s
            assert s in _lib.EXPORTS and re.search(r"^int %s\(" % s, hdr, flags=re.M), s
        count, ppw = getattr(L, names[0]), getattr(L, names[1])   # host only: no device is touched
        assert count(D, A) == COUNT[hidden] == E.param_count(D, hidden, A)
        assert [count(*s) for s in ((45, 6), (44, 10), (26, 10), (26, 6))] == [0, 0, 0, 0]
        assert ppw() >= 2
    assert L.CassieEsParamCount(D, A) == 0 and L.CassieEsWideParamCount(D, A) == 0   # the shape lives behind the new symbols only


# ---------------------------------------------------------------------------------------------------------------------- entry selection
@pytest.mark.parametrize("hidden", [NARROW, WIDE])
def test_the_kernel_call_layer_selects_the_45_by_10_symbols(hidden):
    names = NAMES[hidden]
    entry = E.EsKernels.entry_for(hidden, (D, A))
    assert entry == {"ParamCount": names[0], "PairsPerWorkgroup": names[1], "PolicyStep": names[2], "Book": "CassieEsBook", "GradRows": "CassieEsGradRows",
                     "Grad": "CassieEsGrad"}
    for shape in (None, (26, 6), (45, 6), (44, 10)):   # any other shape: the units of the 2-D robot, whose ParamCount then says 0
        assert not any("3d" in v for v in E.EsKernels.entry_for(hidden, shape).values())
    with pytest.raises(ValueError, match="hidden"):
        E.EsKernels.entry_for((64, 64), (D, A))
    table = torch.randn(60000)
    ek = E.EsKernels(table, 8, D, A, hidden=hidden)
    assert ek.P == COUNT[hidden] and ek.hidden == hidden and ek.ENTRY == entry
    assert ek.step_kind == ("es3d_step" if hidden == NARROW else "es3d_wide_step")
    assert E.EsKernels(table, 8, 26, 6, hidden=hidden).step_kind == ("es_step" if hidden == NARROW else "es_wide_step")
    ek.fn["PolicyStep"] = ek.fn["Grad"] = ek.fn["Book"] = lambda *a: pytest.fail("a kernel was launched")
    top = 60000 - ek.P
    ek.set_directions(torch.tensor([0, top, 5, 5], dtype=torch.int64))
    with pytest.raises(ValueError, match="offsets must lie in"):
        ek.set_directions(torch.tensor([0, top + 1, 5, 5]))
    if hidden == WIDE:
        with pytest.raises(ValueError, match="offsets must lie in"):
            ek.set_directions(torch.tensor([0, 60000 - COUNT[NARROW], 5, 5]))   # fits the 32-wide row, not the 128-wide one
    for args in ((table, 8, 45, 6), (table, 8, 44, 10), (table, 8, 26, 10), (table[:COUNT[hidden] - 1], 8, D, A), (table, 7, D, A)):
        with pytest.raises(ValueError):
            E.EsKernels(*args, hidden=hidden)


# ---------------------------------------------------------------------------------------------------------------------- snapshots
class Toy45Env(FixedTargetEnv):
    """The fixed-target point masses seen through 45 observations (the first four are the toy's) and driven by the first of 10 actions."""

    def _obs(self):
        o = super()._obs()
        return torch.cat([o, torch.zeros(self.n, D - o.shape[1], dtype=o.dtype)], dim=1)


def _toy_es3d(seed, family=None, config=None):
    env = Toy45Env(32, seed)
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(D, A, NARROW, init_std=1.0, dtype=torch.float64)
    algo = E.ES(env.step, env.reset, pol, T.LinearFeatureBaseline(), 32, D, T.NormalizedActions([-1] * A, [1] * A, "cpu"), max_path_length=20, seed=seed,
                sigma=0.05, learning_rate=0.02, table_size=1 << 16)
    algo.env = env
    if family is not None:
        algo.env_family, algo.env_config = family, config
    return algo


def _trained(tmp_path, name, family=None, config=None):
    a = _toy_es3d(2, family, config)
    a.train_iteration()
    p = str(tmp_path / name)
    a.save(p)
    return a, p


def _everything(a):
    return [T.flat_params(a.policy).clone(), a.adam_m.clone(), a.adam_v.clone()]


def test_snapshot_records_the_family_and_refuses_the_other_one(tmp_path):
    assert E.ES.CASSIE3D
    a3, p3 = _trained(tmp_path, "c3.pt", "cassie3d", PD)
    assert a3.n_params == COUNT[NARROW] and a3._kernels() is None and a3.last_policy_step_kind == "torch"
    ck = torch.load(p3, weights_only=True)
    assert ck["algo"] == "es" and ck["env_family"] == "cassie3d" and ck["env_config"] == PD and ck["hidden_sizes"] == [32, 32]
    a2, p2 = _trained(tmp_path, "c2.pt")
    ck = torch.load(p2, weights_only=True)
    assert ck["env_family"] == "cassie2d" and ck["env_config"] is None
    a2.train_iteration()   # a2 is now past its snapshot: a restored policy would show
    before = T.flat_params(a2.policy).clone()
    with pytest.raises(ValueError, match="cassie3d.*cassie2d"):
        a2.load(p3)
    assert torch.equal(T.flat_params(a2.policy), before)
    before = T.flat_params(a3.policy).clone()
    with pytest.raises(ValueError, match="cassie2d.*cassie3d"):
        a3.load(p2)
    assert torch.equal(T.flat_params(a3.policy), before)
    ref = a3.train_iteration()
    b3 = _toy_es3d(7, "cassie3d", dict(PD))
    _, restored = b3.load(p3)
    assert restored and b3.adam_t == 1
    assert b3.train_iteration() == ref and all(torch.equal(x, y) for x, y in zip(_everything(a3), _everything(b3)))
    for other in (dict(PD, control_mode="Torque"), dict(PD, kp=[20.0] * 10)):
        b3.env_config = other
        with pytest.raises(ValueError, match="configured"):
            b3.load(p3)


# ---------------------------------------------------------------------------------------------------------------------- the torch statement at 45 x 10
@pytest.mark.parametrize("hidden", [NARROW, WIDE])
def test_the_torch_statement_at_45_by_10_is_a_network_per_environment(hidden):
    g = torch.Generator().manual_seed(45 + hidden[0])
    n, sigma, (h1, h2) = 6, 0.3, hidden
    P = E.param_count(D, hidden, A)
    theta = 0.2 * torch.randn(P, dtype=torch.float64, generator=g)
    table = torch.randn(2 * P + 50, generator=g)
    offsets = torch.tensor([0, P + 50, 7], dtype=torch.int64)
    obs = torch.randn(n, D, dtype=torch.float64, generator=g)
    alive = torch.tensor([1, 0, 1, 1, 0, 0], dtype=torch.uint8)
    low, high = -torch.rand(A, dtype=torch.float64, generator=g) - 0.5, torch.rand(A, dtype=torch.float64, generator=g) + 0.5
    got = E.es_actions_torch(theta, table, offsets, sigma, obs, alive, T.NormalizedActions(low, high, "cpu"), hidden)
    assert got.shape == (n, A)
    for i in range(n):
        o = int(offsets[i >> 1])
        w = theta + (sigma if i % 2 == 0 else -sigma) * table[o:o + P].double()
        W1, b1, W2, b2, W3, b3 = torch.split(w, [h1 * D, h1, h2 * h1, h2, A * h2, A])
        mean = W3.view(A, h2) @ torch.tanh(W2.view(h2, h1) @ torch.tanh(W1.view(h1, D) @ obs[i] + b1) + b2) + b3
        if not alive[i]:
            mean = torch.zeros(A, dtype=torch.float64)
            assert torch.equal(got[i], low + (high - low) / 2)
        ref = torch.minimum(torch.maximum(low + (mean + 1.0) * 0.5 * (high - low), low), high)
        assert (got[i] - ref).abs().max().item() < 1e-12
