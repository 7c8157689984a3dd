"""PPO's learned value network (cassierl_amd/value.py) on CPU: the closed-form gradient against autograd, the value target of the hand-worked GAE
case, learning on the toy env with the value loss falling inside each update, snapshot / resume and the refusals, the builder's check, the
world-size-2 (gloo) run and the exports."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cassierl_amd import ppo as P
from cassierl_amd import trpo as T
from cassierl_amd import value as VF
from test_trpo_cpu import SnapshotToyEnv, ToyVecEnv

F64 = torch.float64


@pytest.mark.parametrize("D", [26, 45])
@pytest.mark.parametrize("hidden", [(128, 128), (32, 32)])
def test_closed_form_value_gradient_matches_autograd(D, hidden):
    torch.manual_seed(1)
    n = 2000
    vf = VF.MLPValueFunction(D, hidden, dtype=F64)
    with torch.no_grad():
        for p in vf.parameters():
            p.add_(0.1 * torch.randn_like(p))
    obs = torch.randn(n, D, dtype=F64)
    y = vf.predict(obs) + torch.randn(n, dtype=F64)
    assert [tuple(p.shape) for p in vf.parameters()] == [(hidden[0], D), (hidden[0],), (hidden[1], hidden[0]), (hidden[1],), (1, hidden[1]), (1,)]
    ref = T.flat_grad(VF.value_loss(vf, obs, y), vf)
    got = VF.value_grad_closed_form(vf, obs, y)
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    print("closed form against autograd, D %d hidden %r: %.3g relative to the largest entry" % (D, hidden, err))
    assert err <= 1e-12, err
    # scale is 1 / M: the gradient of a shard of a larger minibatch
    half = VF.value_grad_closed_form(vf, obs[:1000], y[:1000], scale=1.0 / n) + VF.value_grad_closed_form(vf, obs[1000:], y[1000:], scale=1.0 / n)
    assert float((half - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # ValueKernels on CPU is autograd of the same loss, and its statistic is the plain sum
    vk = VF.ValueKernels(vf, VF.aligned_value_params(vf))
    assert vk.kind == "autograd"
    vk.set_batch(obs, y)
    g, st = vk.grad()
    assert float((g - ref).abs().max()) <= 1e-14 * max(1.0, float(ref.abs().max()))
    assert abs(float(st) - float(0.5 * ((vf.predict(obs) - y) ** 2).sum())) <= 1e-10 * float(st)


def test_value_function_is_initialised_as_the_mean_network_and_has_no_coefficients():
    torch.manual_seed(3)
    vf = VF.MLPValueFunction(26, (128, 128), dtype=F64)
    for m in vf.net:   # Xavier-uniform weights inside their bound and filling it, zero biases
        if hasattr(m, "bias"):
            bound = (6.0 / (m.in_features + m.out_features)) ** 0.5
            assert float(m.bias.detach().abs().max()) == 0.0 and 0.9 * bound < float(m.weight.detach().abs().max()) <= bound
    assert vf.coeffs is None and vf.hidden_sizes == (128, 128)
    obs = torch.randn(7, 26, dtype=F64) * 50.0
    v = vf.predict(obs, torch.arange(7))
    assert v.dtype == F64 and v.shape == (7,) and torch.equal(v, vf.net(obs).squeeze(-1).detach())   # t ignored, no clipping
    assert vf.fit(obs, None, v) is None and vf.coeffs is None


def test_value_target_of_the_hand_worked_gae_case():
    """test_gae_hand_worked_case_with_a_cut's numbers, with the values handed over by ValueKernels.gae: y = adv + values entry by entry."""
    rew = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=F64)
    cut = torch.tensor([[False, False], [False, True], [False, False]])
    val = torch.tensor([[0.5, 1.0], [1.5, 2.0], [2.5, 3.0]], dtype=F64)
    last = torch.tensor([4.0, 8.0], dtype=F64)
    vf = VF.MLPValueFunction(4, (8, 8), dtype=F64)
    vk = VF.ValueKernels(vf, VF.aligned_value_params(vf))
    ret, adv, y, sums = vk.gae(val, last, rew, cut, 0.5, 0.5)
    assert sums is None
    adv_ref = [[2.21875, 2.5], [3.875, 2.0], [4.5, 7.0]]
    y_ref = [[2.71875, 3.5], [5.375, 4.0], [7.0, 10.0]]
    for t in range(3):
        for i in range(2):
            assert abs(float(adv[t, i]) - adv_ref[t][i]) <= 1e-15 and abs(float(y[t, i]) - y_ref[t][i]) <= 1e-15, (t, i)
    assert torch.equal(ret, torch.tensor([[4.25, 4.0], [6.5, 4.0], [7.0, 10.0]], dtype=F64))
    # no last value: zeros
    _, adv0, y0, _ = vk.gae(val, None, rew, cut, 0.5, 0.5)
    ref0 = P.gae_advantages(rew, cut, val, torch.zeros(2, dtype=F64), 0.5, 0.5)[1]
    assert torch.equal(adv0, ref0) and torch.equal(y0, ref0 + val)


def _toy_ppo(n=64, seed=1, hidden=(32, 32), lr=1e-2, steps=40, value_hidden=(128, 128), **kw):
    env = ToyVecEnv(n, seed)
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(4, 2, hidden, init_std=1.0, dtype=F64)
    vf = VF.MLPValueFunction(4, value_hidden, F64)
    return P.PPO(env.step, env.reset, pol, vf, n, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"),
                 batch_size=n * steps, max_path_length=1000, discount=0.99, learning_rate=lr, seed=seed, **kw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ppo_with_a_value_network_improves_reward_and_lowers_its_value_loss(seed):
    """The settings of test_ppo_improves_reward_on_toy_env with an MLPValueFunction(4, (128, 128), float64): after 31 iterations avg_reward has
    risen by more than the existing test's margin, and at iterations 0, 1, 2 the value loss on the iteration's whole batch is lower after optimize
    than before it."""
    algo = _toy_ppo(n=128, seed=seed, lr=3e-3)
    assert algo.value_kind == "mlp" and algo.value_learning_rate == 1e-3
    fits, drops, optimize = [], [], algo.optimize
    algo.baseline.fit = lambda *a: fits.append(1)

    def watched(d):
        if len(drops) >= 3:
            return optimize(d)
        assert algo._baseline_kernels(d["obs"]) is None
        before = float(VF.value_loss(algo.baseline, d["obs"], d["vtarget"]))
        st = optimize(d)
        drops.append((before, float(VF.value_loss(algo.baseline, d["obs"], d["vtarget"]))))
        return st
    algo.optimize = watched
    first = algo.train_iteration()
    for _ in range(30):
        last = algo.train_iteration()
    for it, (before, after) in enumerate(drops):
        print("seed %d iteration %d: value loss on the batch %.6g -> %.6g (%.1f %%)" % (seed, it, before, after, 100.0 * (1.0 - after / before)))
    print("seed %d: avg_reward %.4f -> %.4f, explained variance %.3f -> %.3f" % (seed, first["avg_reward"], last["avg_reward"], first["explained_variance"],
                                                                               last["explained_variance"]))
    for k in ("itr", "env_steps", "avg_reward", "loss_first", "loss_last", "mean_kl", "clip_frac", "grad_norm", "value_loss_first", "value_loss_last",
              "explained_variance"):
        assert k in last
    assert len(drops) == 3 and all(after < before for before, after in drops), drops
    assert last["avg_reward"] > first["avg_reward"] + 0.05, (first["avg_reward"], last["avg_reward"])
    assert last["value_loss_first"] > 0.0 and last["value_loss_last"] > 0.0 and last["explained_variance"] <= 1.0
    assert algo.adam_t == 31 * 16 and algo.value_adam_t == 31 * 16
    assert algo.last_grad_kind == "autograd" and algo.last_value_kind == "autograd"
    assert algo.baseline.coeffs is None and len(fits) == 31   # process() calls the no-op fit and nothing else


# ---- snapshot / resume
def _snap_ppo(seed, value="mlp", value_hidden=(32, 32)):
    """test_ppo_cpu._snap_ppo's stub env, with the value network swapped in."""
    env = SnapshotToyEnv(32, seed)
    env.g = None
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=F64)
    base = VF.MLPValueFunction(4, value_hidden, F64) if value == "mlp" else T.LinearFeatureBaseline()
    algo = P.PPO(env.step, env.reset, pol, base, 32, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"),
                 batch_size=32 * 4, learning_rate=1e-2, epochs=2, minibatch_size=32, seed=seed, value_learning_rate=2e-3)
    algo.env = env
    return algo


def _started(seed, **kw):
    a = _snap_ppo(seed, **kw)
    a.env.g = torch.Generator().manual_seed(seed); a.env.reset(); a.obs = None
    return a


def test_resumed_run_with_a_value_network_is_the_interrupted_run(tmp_path):
    a = _started(2)
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ck = torch.load(p, weights_only=True)
    assert ck["algo"] == "ppo" and ck["value_kind"] == "mlp" and ck["value_hidden"] == [32, 32] and ck["baseline"] is None
    assert ck["value_adam_t"] == 16 and ck["adam_t"] == 16 and ck["value_learning_rate"] == 2e-3
    assert torch.equal(ck["value_net"], T.flat_params(a.baseline)) and ck["value_adam_m"].shape == ck["value_net"].shape == ck["value_adam_v"].shape
    ref = a.train_iteration()
    b = _snap_ppo(2)
    b.env.g = torch.Generator().manual_seed(99)
    b.gen_mb.manual_seed(12345)
    with torch.no_grad():
        for q in b.baseline.parameters():
            q.add_(1.0)
    b.value_learning_rate = 0.5
    _, restored = b.load(p)
    assert restored and b.adam_t == 16 and b.value_adam_t == 16 and b.value_learning_rate == 2e-3
    got = b.train_iteration()
    assert got["itr"] == ref["itr"] == 2 and b.adam_t == 24 and b.value_adam_t == 24
    for k in ("avg_reward", "grad_norm", "loss_first", "loss_last", "mean_kl", "clip_frac", "value_loss_first", "value_loss_last", "explained_variance"):
        assert got[k] == ref[k], k
    assert torch.equal(T.flat_params(a.policy), T.flat_params(b.policy)) and torch.equal(T.flat_params(a.baseline), T.flat_params(b.baseline))
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert torch.equal(a.value_adam_m, b.value_adam_m) and torch.equal(a.value_adam_v, b.value_adam_v)


def test_load_refuses_the_other_value_kind_and_other_hidden_sizes(tmp_path):
    mlp, lin = _started(2), _started(2, value="linear")
    mlp.train_iteration(); lin.train_iteration()
    pm, pl = str(tmp_path / "mlp.pt"), str(tmp_path / "lin.pt")
    mlp.save(pm); lin.save(pl)
    assert "value_kind" not in torch.load(pl, weights_only=True)   # a linear-baseline snapshot is what it was
    # a value network of the same hidden sizes on another observation width (the other robot's): told by its parameter count
    ck = torch.load(pm, weights_only=True)
    ck["value_net"] = torch.cat([ck["value_net"], torch.zeros(32 * 3, dtype=F64)])
    pw = str(tmp_path / "wide.pt")
    torch.save(ck, pw)
    n_vf = 32 * 4 + 32 + 32 * 32 + 32 + 32 + 1
    for algo, path, pattern in ((_snap_ppo(2, value="linear"), pm, "'mlp'.*'linear'"), (_snap_ppo(2), pl, "'linear'.*'mlp'"),
                                (_snap_ppo(2, value_hidden=(16, 16)), pm, r"\(32, 32\).*\(16, 16\)"),
                                (_snap_ppo(2), pw, "%d parameters.*%d" % (n_vf + 96, n_vf))):
        before = T.flat_params(algo.policy).clone()
        vbefore = None if algo.value_kind == "linear" else T.flat_params(algo.baseline).clone()
        with pytest.raises(ValueError, match=pattern):
            algo.load(path)
        assert torch.equal(T.flat_params(algo.policy), before) and algo.adam_t == 0 and algo.itr == 0
        assert vbefore is None or (torch.equal(T.flat_params(algo.baseline), vbefore) and algo.value_adam_t == 0)
    # a plain TRPO continues the snapshot: the policy comes back, its own linear baseline starts from nothing
    env = SnapshotToyEnv(32, 2)
    torch.manual_seed(7)
    trpo = T.TRPO(env.step, env.reset, T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=F64), T.LinearFeatureBaseline(), 32, 4,
                  T.NormalizedActions([-1, -1], [1, 1], "cpu"), batch_size=32 * 4, seed=2)
    trpo.load(pm, restore_sampler=False)
    assert trpo.baseline.coeffs is None and trpo.itr == 1 and torch.equal(T.flat_params(trpo.policy), T.flat_params(mlp.policy))
    trpo.train_iteration()
    assert trpo.baseline.coeffs is not None


def test_builder_refuses_an_unknown_value_function_before_touching_a_device():
    with pytest.raises(ValueError, match="value must be 'linear' or 'mlp'.*'tree'"):
        P.make_cassie_ppo(64, value="tree", device=123456)


# ---- world size 2
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _run_ppo(i0, n):
    env = ToyVecEnv(n, 3 + i0)
    torch.manual_seed(5)
    pol = T.GaussianMLPPolicy(4, 2, (16, 16), init_std=1.0, dtype=F64)
    vf = VF.MLPValueFunction(4, (16, 16), F64)
    algo = P.PPO(env.step, env.reset, pol, vf, n, 4, T.NormalizedActions([-1, -1], [1, 1], "cpu"), batch_size=64 * 8, learning_rate=1e-2, seed=1,
                 env_id0=i0, epochs=2, minibatch_size=128)
    st = algo.train_iteration()
    return T.flat_params(vf).clone(), T.flat_params(pol).clone(), algo.value_adam_t, st


def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    vtheta, theta, vt, st = _run_ppo(rank * 32, 32)
    q.put((rank, vtheta.numpy(), theta.numpy(), vt, st["value_loss_first"], st["explained_variance"]))
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_value_parameters_after_an_iteration():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict((r[0], r[1:]) for r in (q.get(timeout=180), q.get(timeout=180)))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (v0, t0, n0, l0, e0), (v1, t1, n1, l1, e1) = out[0], out[1]
    assert n0 == n1 == 2 * 4   # epochs x minibatches of 128 / 2 ranks = 64 of a rank's 256 samples
    assert (v0 == v1).all() and (t0 == t1).all()   # bit-identical on both ranks: every gradient is averaged over the ranks
    assert l0 == l1 and e0 == e1 and l0 > 0.0      # the statistics are summed over ranks
    init = T.flat_params(VF.MLPValueFunction(4, (16, 16), F64)).numpy()
    assert v0.shape == init.shape and abs(v0).max() > 0.0


def test_exports_name_the_value_kernels():
    from cassierl_amd import _lib
    for s in ("CassieVfParamCount", "CassieVfPredict", "CassieVfGae", "CassieVfGradRows", "CassieVfGrad"):
        assert s in _lib.EXPORTS, s
