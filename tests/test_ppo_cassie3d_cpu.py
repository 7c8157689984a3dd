"""PPO on Cassie3d, the parts that need no GPU: the builder's refusals (raised before any device is touched), the environment family in
snapshots, and the 45 x 10 policy on the torch statements (parameter alignment for the width-128 kernels, ClipGradKernels' autograd path)."""
import pytest
import torch

from cassierl_amd import ppo as P
from cassierl_amd import trpo as T
from cassierl_amd import vpg as V
from test_ppo_cpu import _snap_ppo, clip_case

D3, A3 = 45, 10


# ---------------------------------------------------------------------------------------------------------------------- the builder
@pytest.mark.parametrize("kw,match", [(dict(terrain=dict(seed=1, files=["a.png"])), "terrain"), (dict(trajectory=object()), "gait"), (dict(kind="stand"), "kind"),
                                      (dict(control_mode="OSC"), "OSC")])
def test_builder_refuses_what_cassie3d_does_not_have(kw, match):
    """terrain, a reference gait, a kind or the OSC mode with env="cassie3d": ValueError, raised before the environment (a device) is created --
    device 123456 does not exist, and nothing gets as far as asking for it."""
    with pytest.raises(ValueError, match=match):
        P.make_cassie_ppo(64, env="cassie3d", device=123456, **kw)


def test_builder_refuses_an_unknown_family_and_the_other_algorithms():
    with pytest.raises(ValueError, match="cassie2d.*cassie3d"):
        P.make_cassie_ppo(64, env="cassie4d", device=123456)
    # the other algorithms refuse Cassie3d (no kernels and no tests at 45 x 10 for them) instead of running on their torch paths
    with pytest.raises(ValueError, match="VPG.*cassie3d.*PPO"):
        V.make_cassie_vpg(64, env="cassie3d", device=123456)
    with pytest.raises(ValueError, match="TRPO.*cassie3d.*PPO"):
        T.make_cassie_trpo(64, env="cassie3d", device=123456)


# ---------------------------------------------------------------------------------------------------------------------- snapshots
PD = dict(control_mode="PD", kp=[10.0] * 10, kd=[5.0] * 10)


def _trained(tmp_path, name, family=None, config=None):
    a = _snap_ppo(2)
    if family is not None:
        a.env_family, a.env_config = family, config
    a.env.g = torch.Generator().manual_seed(2); a.env.reset(); a.obs = None
    a.train_iteration()
    p = str(tmp_path / name)
    a.save(p)
    return a, p


def test_snapshot_records_the_family_and_refuses_the_other_one(tmp_path):
    """The stub environment of the family's CPU tests stands in for both robots: what is checked is the snapshot's entries and load()'s refusal."""
    a3, p3 = _trained(tmp_path, "c3.pt", "cassie3d", PD)
    ck = torch.load(p3, weights_only=True)
    assert ck["env_family"] == "cassie3d" and ck["env_config"] == PD
    a2, p2 = _trained(tmp_path, "c2.pt")
    ck = torch.load(p2, weights_only=True)
    assert ck["env_family"] == "cassie2d" and ck["env_config"] is None
    before = T.flat_params(a2.policy).clone()
    with pytest.raises(ValueError, match="cassie3d.*cassie2d"):
        a2.load(p3)
    assert torch.equal(T.flat_params(a2.policy), before)   # refused before anything was restored
    with pytest.raises(ValueError, match="cassie2d.*cassie3d"):
        a3.load(p2)
    # the same family continues; another control mode or other gains are another run
    b3 = _snap_ppo(7)
    b3.env_family, b3.env_config = "cassie3d", dict(PD)
    _, restored = b3.load(p3)
    assert restored and torch.equal(T.flat_params(b3.policy), T.flat_params(a3.policy))
    for other in (dict(PD, control_mode="Torque"), dict(PD, kp=[20.0] * 10)):
        b3.env_config = other
        with pytest.raises(ValueError, match="configured"):
            b3.load(p3)


def test_a_snapshot_from_before_the_entry_loads_as_cassie2d(tmp_path):
    a2, p2 = _trained(tmp_path, "c2.pt")
    ck = torch.load(p2, weights_only=True)
    del ck["env_family"], ck["env_config"]
    old = str(tmp_path / "old.pt")
    torch.save(ck, old)
    b2 = _snap_ppo(7)
    _, restored = b2.load(old)
    assert restored and torch.equal(T.flat_params(b2.policy), T.flat_params(a2.policy))
    b3 = _snap_ppo(7)
    b3.env_family, b3.env_config = "cassie3d", PD
    with pytest.raises(ValueError, match="cassie2d.*cassie3d"):
        b3.load(old)


# ---------------------------------------------------------------------------------------------------------------------- 45 x 10 on the torch statements
def test_aligned_flat_params_at_45_by_10():
    """log_std (10 floats) sits in front of the mean network: a pad of 2 puts W1 on a 16-byte boundary, and with it b1, W2, b2 and W3 (every
    block before them is a multiple of four floats), which the width-128 kernels read as float4."""
    pol = T.GaussianMLPPolicy(D3, A3, (128, 128), init_std=1.0)
    theta = P.aligned_flat_params(pol)
    assert torch.equal(theta, T.flat_params(pol)) and theta.is_contiguous()
    assert theta.storage_offset() == 2
    off, offs = 0, {}
    for nm, p in pol.named_parameters():
        offs[nm] = off
        off += p.numel()
    assert offs["log_std"] == 0 and offs["mean_net.0.weight"] == A3
    for nm in ("mean_net.0.weight", "mean_net.0.bias", "mean_net.2.weight", "mean_net.2.bias", "mean_net.4.weight"):
        assert (theta.data_ptr() + 4 * offs[nm]) % 16 == 0, nm


@pytest.mark.parametrize("ent", [0.0, 0.01])
def test_clip_grad_kernels_on_cpu_tensors_are_autograd_at_45_by_10(ent):
    pol, obs, act, adv, old_mean, old_ls = clip_case((128, 128), A3, D=D3)
    with torch.no_grad():
        _, _, clipped = P.surrogate_terms(pol.mean_net(obs), pol.log_std, act, adv, old_mean, old_ls, 0.2)
    assert 0.05 < float(clipped.double().mean()) < 0.95
    ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), obs, act, adv, old_mean, old_ls, 0.2, ent)
    assert ck.kind == "autograd"
    g, st = ck.grad()
    ref = P.clipped_grad_closed_form(pol, obs, act, adv, old_mean, old_ls, 0.2, ent)
    assert float((g - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float(st[2]) == float(clipped.sum())
