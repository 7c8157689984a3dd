"""PPO (cassierl_amd/ppo.py) on CPU: GAE(lambda) against hand-worked numbers and its two limits, the closed-form clipped gradient against
autograd of ppo_loss with both clip branches populated, the first gradient against VPG's, learning on the toy env, the minibatch schedule,
snapshot / resume and the refusals."""
import numpy as np
import pytest
import torch

from cassierl_amd import ppo as P
from cassierl_amd import trpo as T
from cassierl_amd import vpg as V
from test_trpo_cpu import SnapshotToyEnv, ToyVecEnv


def test_gae_hand_worked_case_with_a_cut():
    """3 steps, 2 environments, gamma 0.5, lambda 0.5; environment 1 is cut at step 1."""
    rew = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=torch.float64)
    cut = torch.tensor([[False, False], [False, True], [False, False]])
    val = torch.tensor([[0.5, 1.0], [1.5, 2.0], [2.5, 3.0]], dtype=torch.float64)
    last = torch.tensor([4.0, 8.0], dtype=torch.float64)
    ret, adv = P.gae_advantages(rew, cut, val, last, 0.5, 0.5)
    # env 0: delta2 = 5 + .5 * 4 - 2.5 = 4.5; delta1 = 3 + .5 * 2.5 - 1.5 = 2.75; delta0 = 1 + .5 * 1.5 - .5 = 1.25
    #        adv2 = 4.5; adv1 = 2.75 + .25 * 4.5 = 3.875; adv0 = 1.25 + .25 * 3.875 = 2.21875
    #        ret2 = 5 + .5 * 4 = 7; ret1 = 3 + 3.5 = 6.5; ret0 = 1 + 3.25 = 4.25
    # env 1: delta2 = 6 + .5 * 8 - 3 = 7; delta1 = 4 - 2 = 2 (cut: no bootstrap); delta0 = 2 + .5 * 2 - 1 = 2
    #        adv2 = 7; adv1 = 2 (cut: the sum restarts); adv0 = 2 + .25 * 2 = 2.5;  ret2 = 10; ret1 = 4; ret0 = 2 + 2 = 4
    np.testing.assert_allclose(adv.numpy(), [[2.21875, 2.5], [3.875, 2.0], [4.5, 7.0]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(ret.numpy(), [[4.25, 4.0], [6.5, 4.0], [7.0, 10.0]], rtol=0, atol=1e-15)


def test_gae_limits_lambda_one_and_zero():
    g = torch.Generator().manual_seed(0)
    Tn, N, gamma = 8, 50, 0.99
    rew = torch.randn(Tn, N, generator=g, dtype=torch.float64)
    cut = torch.rand(Tn, N, generator=g) < 0.2
    val = torch.randn(Tn, N, generator=g, dtype=torch.float64)
    last = torch.randn(N, generator=g, dtype=torch.float64)
    ret, adv1 = P.gae_advantages(rew, cut, val, last, gamma, 1.0)
    ref = T.discounted_returns(rew, cut, gamma, last)
    tol = lambda x: 1e-12 * (1.0 + float(x.abs().max()))
    assert float((ret - ref).abs().max()) <= tol(ref)
    assert float((adv1 - (ref - val)).abs().max()) <= tol(adv1)
    _, adv0 = P.gae_advantages(rew, cut, val, last, gamma, 0.0)
    v_next = torch.cat([val[1:], last.unsqueeze(0)])
    td = rew + gamma * (~cut).double() * v_next - val
    assert float((adv0 - td).abs().max()) <= tol(td)
    assert float((adv0 - adv1).abs().max()) > 0.1   # the two limits are different things on these inputs


def clip_case(hidden, A, dtype=torch.float64, n=2000, D=26, seed=1, jitter=0.05):
    """A policy, the statistics of its "old" self on a batch, then the policy jittered: ratios spread around 1 on both sides."""
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(D, A, hidden, init_std=1.0, dtype=dtype)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.1 * torch.randn_like(p))
    obs = torch.randn(n, D, dtype=dtype)
    adv = torch.randn(n, dtype=dtype)
    with torch.no_grad():
        old_mean, old_ls = pol.dist_info(obs)
        old_mean, old_ls = old_mean.clone(), old_ls[0].clone()
        act = old_mean + torch.randn_like(old_mean) * old_ls.exp()
        for p in pol.parameters():
            p.add_(jitter * torch.randn_like(p))
    return pol, obs, act, adv, old_mean, old_ls


@pytest.mark.parametrize("hidden", [(32, 32), (128, 128)])
@pytest.mark.parametrize("A", [6, 7])
@pytest.mark.parametrize("ent", [0.0, 0.01])
def test_closed_form_clipped_gradient_matches_autograd(hidden, A, ent):
    pol, obs, act, adv, old_mean, old_ls = clip_case(hidden, A)
    with torch.no_grad():
        _, ratio, clipped = P.surrogate_terms(pol.mean_net(obs), pol.log_std, act, adv, old_mean, old_ls, 0.2)
    share = float(clipped.double().mean())
    print("clipped share %.3f (hidden %r, A %d)" % (share, hidden, A))
    assert 0.10 <= share <= 0.60, share
    assert bool((clipped & (adv > 0)).any()) and bool((clipped & (adv < 0)).any())
    ref = T.flat_grad(P.ppo_loss(pol, obs, act, adv, old_mean, old_ls, 0.2, ent), pol)
    got = P.clipped_grad_closed_form(pol, obs, act, adv, old_mean, old_ls, 0.2, ent)
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    print("closed form against autograd: %.3g relative to the largest entry" % err)
    assert err <= 1e-12, err
    # ClipGradKernels on CPU is autograd of the same loss, and its statistics are the plain sums
    ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), obs, act, adv, old_mean, old_ls, 0.2, ent)
    assert ck.kind == "autograd"
    g, st = ck.grad()
    assert float((g - ref).abs().max()) <= 1e-14 * max(1.0, float(ref.abs().max()))
    assert float(st[2]) == float(clipped.sum()) and float(st[1]) > 0


def test_first_gradient_is_vpgs():
    """epochs = 1 and one minibatch = the batch: at theta = theta_old the ratio is 1 everywhere, nothing is clipped, the gradient is VPG's."""
    torch.manual_seed(2)
    n, D, A = 400, 26, 6
    pol = T.GaussianMLPPolicy(D, A, (32, 32), init_std=1.0, dtype=torch.float64)
    obs, adv = torch.randn(n, D, dtype=torch.float64), torch.randn(n, dtype=torch.float64)
    with torch.no_grad():
        mean, ls = pol.dist_info(obs)
        act = mean + torch.randn_like(mean) * ls.exp()
    ref = V.closed_form_grad(pol, T.AnalyticFisher(pol, obs).vjp, act, mean, ls, adv)
    ck = P.ClipGradKernels(pol, P.aligned_flat_params(pol), obs, act, adv, mean, ls, 0.2, 0.0)
    g, st = ck.grad()
    assert float(st[2]) == 0.0 and abs(float(st[1])) < 1e-12
    assert float((g - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))
    got = P.clipped_grad_closed_form(pol, obs, act, adv, mean, ls, 0.2, 0.0)
    assert float((got - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))


def _toy_ppo(n=64, seed=1, hidden=(32, 32), lr=1e-2, steps=40, **kw):
    env = ToyVecEnv(n, seed)
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(4, 2, hidden, init_std=1.0, dtype=torch.float64)
    return P.PPO(env.step, env.reset, pol, T.LinearFeatureBaseline(), n, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"),
                 batch_size=n * steps, max_path_length=1000, discount=0.99, learning_rate=lr, seed=seed, **kw)


def test_ppo_improves_reward_on_toy_env():
    algo = _toy_ppo(n=128, seed=3, lr=3e-3)
    assert (algo.clip_range, algo.gae_lambda, algo.epochs, algo.minibatch_size, algo.entropy_coeff) == (0.2, 0.95, 4, 128 * 40 // 4, 0.0)
    first = algo.train_iteration()
    for _ in range(30):
        last = algo.train_iteration()
    for k in ("itr", "env_steps", "episodes", "avg_return", "avg_reward", "gathered", "loss_first", "loss_last", "mean_kl", "clip_frac", "grad_norm"):
        assert k in last
    assert algo.adam_t == 31 * 4 * 4 and algo.last_grad_kind == "autograd"
    assert last["avg_reward"] > first["avg_reward"] + 0.05, (first["avg_reward"], last["avg_reward"])


def test_two_epochs_of_four_minibatches_visit_every_sample_once_per_epoch():
    algo = _toy_ppo(n=32, steps=8, epochs=2, minibatch_size=64)
    algo.keep_perms = True
    for it in range(3):
        st = algo.train_iteration()
        assert st["minibatch_steps"] == 8 and 0.0 <= st["clip_frac"] <= 1.0 and st["mean_kl"] >= 0.0 and np.isfinite(st["loss_last"])
        assert len(algo.last_perms) == 2
        for perm in algo.last_perms:
            assert sorted(perm.tolist()) == list(range(256))
        assert not torch.equal(algo.last_perms[0], algo.last_perms[1])
    assert algo.adam_t == 24


def test_indivisible_minibatch_sizes_raise():
    with pytest.raises(ValueError, match="not a multiple"):
        _toy_ppo(n=32, steps=8, minibatch_size=100)
    algo = _toy_ppo(n=32, steps=8, minibatch_size=64)
    algo.minibatch_size = 96   # a batch of another shape than the constructor saw: refused at the first batch
    with pytest.raises(ValueError, match="not a multiple"):
        algo.train_iteration()


def _snap_ppo(seed):
    env = SnapshotToyEnv(32, seed)
    env.g = None
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=torch.float64)
    algo = P.PPO(env.step, env.reset, pol, T.LinearFeatureBaseline(), 32, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"),
                 batch_size=32 * 4, learning_rate=1e-2, epochs=2, minibatch_size=32, seed=seed)
    algo.env = env
    return algo


def test_resumed_ppo_run_is_the_interrupted_run(tmp_path):
    a = _snap_ppo(2)
    a.env.g = torch.Generator().manual_seed(2); a.env.reset(); a.obs = None
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ck = torch.load(p, weights_only=True)
    assert ck["algo"] == "ppo" and ck["hidden_sizes"] == [32, 32] and ck["adam_t"] == 16
    assert (ck["clip_range"], ck["gae_lambda"], ck["epochs"], ck["minibatch_size"], ck["entropy_coeff"], ck["learning_rate"]) == (0.2, 0.95, 2, 32, 0.0, 1e-2)
    ref = a.train_iteration()
    b = _snap_ppo(2)   # (the permutation generator is seeded from the seed; its STATE comes from the snapshot)
    b.env.g = torch.Generator().manual_seed(99)
    b.gen_mb.manual_seed(12345)
    _, restored = b.load(p)
    assert restored and b.adam_t == 16
    got = b.train_iteration()
    assert got["itr"] == ref["itr"] == 2 and b.adam_t == 24
    for k in ("avg_reward", "grad_norm", "loss_first", "loss_last", "mean_kl", "clip_frac"):
        assert got[k] == ref[k], k
    assert torch.equal(T.flat_params(a.policy), T.flat_params(b.policy))
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)


def test_load_refuses_a_vpg_snapshot_and_other_hidden_sizes(tmp_path):
    env = ToyVecEnv(16, 0)
    torch.manual_seed(0)
    pol = T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=torch.float64)
    vpg = V.VPG(env.step, env.reset, pol, T.LinearFeatureBaseline(), 16, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"), batch_size=16 * 2)
    vpg.train_iteration()
    p = str(tmp_path / "vpg.pt")
    vpg.save(p)
    a = _toy_ppo(n=16, steps=4)
    before = T.flat_params(a.policy).clone()
    with pytest.raises(ValueError, match="vpg.*ppo"):
        a.load(p)
    assert torch.equal(T.flat_params(a.policy), before)
    a.train_iteration()
    q = str(tmp_path / "ppo.pt")
    a.save(q)
    with pytest.raises(ValueError, match=r"\(32, 32\).*\(16, 16\)"):
        _toy_ppo(n=16, steps=4, hidden=(16, 16)).load(q)
    with pytest.raises(ValueError, match="ppo.*vpg"):
        vpg.load(q)
