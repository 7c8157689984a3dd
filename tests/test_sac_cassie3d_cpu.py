"""SAC on Cassie3d, the parts that need no GPU: the builder's refusals (raised before any device is touched), which shapes the kernels cover, the
environment family in snapshots, the torch statement of the update at 45 x 10, and the library's CassieSac3d* exports (csrc/tu_sac3d.hip, a unit of its own on the shape-generic kernels of csrc/sac_kernels.h)."""
import ctypes as ct

import pytest
import torch

from cassierl_amd import ddpg as G
from cassierl_amd import sac as S
from cassierl_amd import td3 as D3
from cassierl_amd import trpo as T
from test_sac_cpu import _snap_sac

D, A = 45, 10
PD = dict(control_mode="PD", kp=[10.0] * 10, kd=[5.0] * 10)
ENTRIES = ["CassieSac3dParamCount", "CassieSac3dPolicyStep", "CassieSac3dCriticGrad", "CassieSac3dActorGrad", "CassieSac3dCriticApply", "CassieSac3dActorApply"]


# ---------------------------------------------------------------------------------------------------------------------- the builder
@pytest.mark.parametrize("kw,match", [(dict(terrain=dict(seed=1, files=["a.png"])), "terrain"), (dict(trajectory=object()), "gait"), (dict(kind="stand"), "kind"),
                                      (dict(control_mode="OSC"), "OSC")])
def test_builder_refuses_what_cassie3d_does_not_have(kw, match):
    """Device 123456 does not exist, and nothing gets as far as asking for it."""
    with pytest.raises(ValueError, match=match):
        S.make_cassie_sac(64, env="cassie3d", device=123456, **kw)


def test_builder_refuses_an_unknown_family_and_the_other_pool_algorithms():
    with pytest.raises(ValueError, match="cassie2d.*cassie3d"):
        S.make_cassie_sac(64, env="cassie4d", device=123456)
    assert S.SAC.CASSIE3D and not G.DDPG.CASSIE3D and not D3.TD3.CASSIE3D
    with pytest.raises(ValueError, match="DDPG.*cassie3d.*SAC"):
        G.make_cassie_ddpg(64, env="cassie3d", device=123456)
    with pytest.raises(ValueError, match="TD3.*cassie3d.*SAC"):
        D3.make_cassie_td3(64, env="cassie3d", device=123456)


# ---------------------------------------------------------------------------------------------------------------------- shapes
def _on_device(monkeypatch):
    """kernels_cover asks for float32 CUDA parameters; without a device the question about the SHAPE is put with that answer given."""
    real = torch.Tensor.is_cuda
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return real


def _nets(d, a, hidden=(32, 32)):
    return S.SquashedGaussianMLPPolicy(d, a, hidden), G.ContinuousMLPQFunction(d, a, hidden), G.ContinuousMLPQFunction(d, a, hidden)


def test_kernels_cover_45_by_10_and_nothing_near_it(monkeypatch):
    assert not S.kernels_cover(*_nets(D, A))   # CPU tensors: the torch statements
    _on_device(monkeypatch)
    assert S.kernels_cover(*_nets(D, A)) and S.kernels_cover(*_nets(26, 6)) and S.kernels_cover(*_nets(17, 7))
    assert not S.kernels_cover(*_nets(45, 6)) and not S.kernels_cover(*_nets(44, 10)) and not S.kernels_cover(*_nets(26, 10))
    assert not S.kernels_cover(*_nets(D, A, (64, 64))) and not S.kernels_cover(*_nets(D, A, (128, 128)))
    pol, q1, _ = _nets(D, A)
    assert not S.kernels_cover(pol, q1, G.ContinuousMLPQFunction(26, 6))
    assert S.SAC.STEP_ENTRY == {26: "CassieSacPolicyStep", 45: "CassieSac3dPolicyStep"} and 45 not in G.DDPG.STEP_ENTRY and 45 not in D3.TD3.STEP_ENTRY


# ---------------------------------------------------------------------------------------------------------------------- snapshots
def _trained(tmp_path, name, family=None, config=None):
    a = _snap_sac(2)
    if family is not None:
        a.env_family, a.env_config = family, config
    a.env.g = torch.Generator().manual_seed(2); a.env.reset(); a.obs = None
    a.train_iteration()
    p = str(tmp_path / name)
    a.save(p)
    return a, p


def _everything(a):
    return [T.flat_params(n).clone() for n in (a.policy, a.qf1, a.qf2, a.target_qf1, a.target_qf2)] + [a.log_alpha.clone(), a.adam_q1["m"].clone(), a.pool.obs.clone()]


def test_snapshot_records_the_family_and_refuses_the_other_one(tmp_path):
    """The stub environment of the family's CPU tests stands in for both robots: what is checked is the snapshot's entries and load()'s refusal,
    which comes before anything -- the critics and Adam states included -- is restored."""
    a3, p3 = _trained(tmp_path, "c3.pt", "cassie3d", PD)
    ck = torch.load(p3, weights_only=True)
    assert ck["algo"] == "sac" and ck["env_family"] == "cassie3d" and ck["env_config"] == PD
    a2, p2 = _trained(tmp_path, "c2.pt")
    ck = torch.load(p2, weights_only=True)
    assert ck["env_family"] == "cassie2d" and ck["env_config"] is None
    a2.train_iteration()   # a2 is now past its snapshot: a partial restore would show
    before, t_before = _everything(a2), a2.adam_q1["t"]
    with pytest.raises(ValueError, match="cassie3d.*cassie2d"):
        a2.load(p3)
    assert all(torch.equal(x, y) for x, y in zip(_everything(a2), before)) and a2.adam_q1["t"] == t_before
    before = _everything(a3)
    with pytest.raises(ValueError, match="cassie2d.*cassie3d"):
        a3.load(p2)
    assert all(torch.equal(x, y) for x, y in zip(_everything(a3), before))
    b3 = _snap_sac(7)
    b3.env_family, b3.env_config = "cassie3d", dict(PD)
    _, restored = b3.load(p3)
    assert restored and b3.pool_restored and torch.equal(T.flat_params(b3.qf2), T.flat_params(a3.qf2))
    for other in (dict(PD, control_mode="Torque"), dict(PD, kp=[20.0] * 10)):
        b3.env_config = other
        with pytest.raises(ValueError, match="configured"):
            b3.load(p3)


# ---------------------------------------------------------------------------------------------------------------------- the torch statement at 45 x 10
def test_the_torch_update_runs_at_45_by_10_and_moves_every_block():
    torch.manual_seed(3)
    pol, q1, q2 = _nets(D, A)
    t1, t2 = G.ContinuousMLPQFunction(D, A), G.ContinuousMLPQFunction(D, A)
    nets = (pol, q1, q2, t1, t2)
    n = 64
    batch = (0.7 * torch.randn(n, D), torch.rand(n, A) * 2 - 1, 0.1 * torch.randn(n), (torch.rand(n) < 0.2).float(), 0.7 * torch.randn(n, D))
    la = torch.zeros(1)
    before = [[p.detach().clone() for p in net.parameters()] for net in nets]
    out = S.sac_update_torch_(pol, q1, q2, t1, t2, la, G.new_adam(pol), G.new_adam(q1), G.new_adam(q2), S.new_alpha_adam(la), batch, torch.randn(n, A),
                              torch.randn(n, A))
    assert all(torch.isfinite(x).all() for x in out) and la.item() != 0.0
    assert T.flat_params(pol).numel() == 3188 and T.flat_params(q1).numel() == 2881
    for net, was in zip(nets, before):
        for p, w in zip(net.parameters(), was):
            assert torch.isfinite(p).all() and not torch.equal(p, w)
    assert S.SAC(None, None, pol, q1, q2, 8, D, None, replay_pool_size=8).target_entropy == -10.0
    assert G.ReplayPool.BYTES_PER_ROW(D, A) == 408


# ---------------------------------------------------------------------------------------------------------------------- the library
def test_the_library_exports_the_six_entry_points_and_counts_parameters():
    from cassierl_amd import _lib
    from cassierl_amd import build as B
    L = ct.CDLL(B.build())
    for name in ENTRIES:
        assert hasattr(L, name), "missing export " + name
        assert name in _lib.EXPORTS
    assert "tu_sac3d" in B.UNITS
    count = L.CassieSac3dParamCount   # host only: no device is touched
    assert count(45, 10, G.ACTOR) == 3188 and count(45, 10, G.CRITIC) == 2881
    for shape in ((26, 6), (45, 6), (44, 10), (10, 45), (0, 0)):
        assert count(*shape, G.ACTOR) == 0 and count(*shape, G.CRITIC) == 0
    assert count(45, 10, 2) == 0
