"""ES (cassierl_amd/es.py) on CPU: the torch statements against independent loops, centered ranks, the bookkeeping, learning on the toy env,
the world-size-2 (gloo) run, snapshot / resume, the refusal of a VPG snapshot, the host-side range check of the kernel-call layer and the exports."""
import ctypes as ct
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

from cassierl_amd import es as E
from cassierl_amd import trpo as T
from cassierl_amd import vpg as V
from test_trpo_cpu import SnapshotToyEnv, ToyVecEnv

AMAP = lambda: T.NormalizedActions([-1, -1], [1, 1], "cpu")


# ---- the torch statements
@pytest.mark.parametrize("D,A,hidden", [(26, 6, (32, 32)), (17, 7, (32, 32)), (5, 2, (8, 16))])
def test_perturbed_actions_match_a_network_per_environment(D, A, hidden):
    g = torch.Generator().manual_seed(10 * D + A)
    n, sigma = 10, 0.3
    pol = T.GaussianMLPPolicy(D, A, hidden, dtype=torch.float64)
    theta = T.flat_params(pol.mean_net) + 0.1 * torch.randn(E.param_count(D, hidden, A), dtype=torch.float64, generator=g)
    P = theta.numel()
    assert [n_ for n_, _ in pol.named_parameters() if n_ != "log_std"] == V._MEAN_ORDER
    table = torch.randn(3 * P, generator=g)
    offsets = torch.tensor([0, 2 * P, 7, 7, P - 3], dtype=torch.int64)   # both ends, a shared offset, overlapping slices
    obs = torch.randn(n, D, dtype=torch.float64, generator=g)
    alive = torch.tensor([1, 1, 0, 1, 1, 0, 0, 0, 1, 1], dtype=torch.uint8)
    low, high = -torch.rand(A, dtype=torch.float64, generator=g) - 0.5, torch.rand(A, dtype=torch.float64, generator=g) + 0.5
    amap = T.NormalizedActions(low, high, "cpu")
    got = E.es_actions_torch(theta, table, offsets, sigma, obs, alive, amap, hidden)
    assert got.shape == (n, A) and got.dtype == torch.float64
    for i in range(n):
        eps = table[int(offsets[i >> 1]):int(offsets[i >> 1]) + P].double()
        net = nn.Sequential(nn.Linear(D, hidden[0]), nn.Tanh(), nn.Linear(hidden[0], hidden[1]), nn.Tanh(), nn.Linear(hidden[1], A)).double()
        T.set_flat_params(net, theta + sigma * eps if i % 2 == 0 else theta - sigma * eps)
        with torch.no_grad():
            mean = net(obs[i:i + 1])[0] if alive[i] else torch.zeros(A, dtype=torch.float64)
        ref = torch.minimum(torch.maximum(low + (mean + 1.0) * 0.5 * (high - low), low), high)
        assert (got[i] - ref).abs().max().item() < 1e-12
        if not alive[i]:
            assert torch.equal(got[i], low + (high - low) / 2)
    free = E.es_actions_torch(theta, table, offsets, sigma, obs, None, amap, hidden)
    assert torch.equal(free[alive.bool()], got[alive.bool()]) and not torch.equal(free, got)


def test_gradient_statement_is_the_explicit_matrix_product():
    g = torch.Generator().manual_seed(3)
    P, M, sigma = 301, 9000, 0.07   # more directions than one chunk of es_grad_torch
    table = torch.randn(5000, generator=g).double()
    offsets = torch.randint(0, 5000 - P + 1, (M,), generator=g)
    offsets[0], offsets[-1] = 0, 5000 - P
    w = torch.randn(M, dtype=torch.float64, generator=g)
    Emat = torch.stack([table[int(o):int(o) + P] for o in offsets])
    ref = Emat.T @ w / (2 * M * sigma)
    got = E.es_grad_torch(table, offsets, w, P) / (2 * M * sigma)
    assert (got - ref).abs().max().item() < 1e-12 * max(1.0, ref.abs().max().item())


def test_centered_ranks():
    g = torch.Generator().manual_seed(0)
    f = torch.randn(101, dtype=torch.float64, generator=g)
    u = E.centered_ranks(f)
    assert abs(u.sum().item()) < 1e-12 and u.min().item() == -0.5 and u.max().item() == 0.5
    assert u[f.argmax()].item() == 0.5 and u[f.argmin()].item() == -0.5
    # by hand: values 3 1 2 1 -> ranks 3 0 2 1 (the first of the tied pair gets the lower rank) -> / 3 - 0.5
    hand = E.centered_ranks(torch.tensor([3.0, 1.0, 2.0, 1.0], dtype=torch.float64))
    np.testing.assert_allclose(hand.numpy(), [0.5, -0.5, 1.0 / 6.0, -1.0 / 6.0], rtol=0, atol=1e-15)
    tied = E.centered_ranks(torch.zeros(5, dtype=torch.float64))
    np.testing.assert_allclose(tied.numpy(), [-0.5, -0.25, 0.0, 0.25, 0.5], rtol=0, atol=0)
    assert torch.equal(E.shape_fitness(f), u)
    z = E.shape_fitness(f, "zscore")
    assert abs(z.mean().item()) < 1e-12 and abs(z.std(unbiased=False).item() - 1.0) < 1e-6
    np.testing.assert_allclose(E.pair_weights(hand).numpy(), [1.0, 1.0 / 3.0], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        E.shape_fitness(f, "softmax")


def test_bookkeeping_freezes_after_the_first_done():
    n, steps = 6, 7
    g = torch.Generator().manual_seed(1)
    rew = torch.randn(steps, n, dtype=torch.float64, generator=g)
    done = torch.zeros(steps, n, dtype=torch.bool)
    done[2, 1] = done[4, 1] = done[0, 3] = done[6, 4] = True   # env 1 is done twice (auto-reset): only the first counts
    for dtype in (torch.uint8, torch.bool):
        alive = torch.ones(n, dtype=dtype)
        fitness, length = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.int64)
        for t in range(steps):
            E.es_book_torch(rew[t], done[t], alive, fitness, length)
        first = [steps, 3, steps, 1, steps, steps]   # steps lived: up to and including the first done
        assert length.tolist() == first and alive.tolist() == [1, 0, 1, 0, 0, 1]
        for i in range(n):
            assert abs(fitness[i].item() - rew[:first[i], i].sum().item()) < 1e-14


# ---- ES on the toy env
class PairToyEnv(ToyVecEnv):
    """ToyVecEnv whose reset gives both environments of a pair the same target."""

    def reset(self):
        super().reset()
        self.tg = self.tg[0::2].repeat_interleave(2)
        return self._obs()


def _toy_es(n=128, seed=1, env=None, **kw):
    env = PairToyEnv(n, seed) if env is None else env
    torch.manual_seed(seed)
    pol = T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=torch.float64)
    kw.setdefault("table_size", 1 << 16)
    return E.ES(env.step, env.reset, pol, T.LinearFeatureBaseline(), n, 4, AMAP(), max_path_length=20, seed=seed, **kw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_es_learns_on_the_toy_env(seed):
    algo = _toy_es(n=128, seed=seed, sigma=0.05, learning_rate=0.02, l2_coeff=0.0)
    ls0 = algo.policy.log_std.detach().clone()
    first = algo.train_iteration()
    for _ in range(29):
        last = algo.train_iteration()
    assert sorted(last) == sorted(["itr", "env_steps", "episodes", "avg_return", "max_return", "min_return", "avg_path_length", "grad_norm", "step_norm", "gathered"])
    assert last["itr"] == 29 and last["env_steps"] == 128 * 20 and last["episodes"] == last["gathered"] == 128 and last["avg_path_length"] == 20.0
    assert last["min_return"] <= last["avg_return"] <= last["max_return"] < 0 and algo.adam_t == 30
    assert algo.last_policy_step_kind == algo.last_grad_kind == "torch" and not algo.last_adam_fused and not algo.last_book_fused
    assert torch.equal(algo.policy.log_std.detach(), ls0)   # ES never touches log_std
    print("ES on the toy env, seed %d: avg_return %.3f -> %.3f" % (seed, first["avg_return"], last["avg_return"]))
    assert first["avg_return"] < 0 and last["avg_return"] > 0.1 * first["avg_return"], (first["avg_return"], last["avg_return"])


def test_es_argument_checks():
    with pytest.raises(ValueError, match="even"):
        _toy_es(n=7, env=ToyVecEnv(7, 0))
    with pytest.raises(ValueError, match="fitness_shaping"):
        _toy_es(n=8, fitness_shaping="softmax")
    with pytest.raises(ValueError, match="table_size"):
        _toy_es(n=8, table_size=100)
    algo = _toy_es(n=8, fitness_shaping="zscore")
    assert np.isfinite(algo.train_iteration()["grad_norm"])


# ---- data-parallel: 2 ranks with half the environments each == 1 process with all of them
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


class _ShardEnv:
    """A shard [i0, i0 + n) of one PairToyEnv of 64 envs (the physics of an env does not depend on the shard)."""

    def __init__(self, i0, n):
        self.full, self.i0, self.n = PairToyEnv(64, 0), i0, n

    def reset(self):
        return self.full.reset()[self.i0:self.i0 + self.n]

    def step(self, a):
        big = torch.zeros(64, a.shape[1], dtype=a.dtype)
        big[self.i0:self.i0 + self.n] = a
        o, r, d = self.full.step(big)
        sl = slice(self.i0, self.i0 + self.n)
        return o[sl], r[sl], d[sl]


def _run_es(i0, n, itr=2):
    env = _ShardEnv(i0, n)
    torch.manual_seed(5)
    pol = T.GaussianMLPPolicy(4, 2, (16, 16), init_std=1.0, dtype=torch.float64)
    algo = E.ES(env.step, env.reset, pol, T.LinearFeatureBaseline(), n, 4, AMAP(), max_path_length=20, sigma=0.05, learning_rate=0.02, seed=1,
                table_size=1 << 16, env_id0=i0)
    stats = [algo.train_iteration() for _ in range(itr)]
    return T.flat_params(pol).numpy(), stats


def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    theta, st = _run_es(rank * 32, 32)
    if rank == 0:
        q.put((theta, st))
    dist.destroy_process_group()


def test_two_process_es_equals_one_process():
    ref, st_ref = _run_es(0, 64)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    theta, st = q.get(timeout=180)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    np.testing.assert_allclose(theta, ref, rtol=0, atol=1e-9)
    for a, b in zip(st, st_ref):
        assert a["env_steps"] == b["env_steps"] == 64 * 20 and a["gathered"] == b["gathered"] == 64 and a["episodes"] == b["episodes"] == 64
        assert abs(a["avg_return"] - b["avg_return"]) < 1e-12 * abs(b["avg_return"]) and abs(a["grad_norm"] - b["grad_norm"]) < 1e-9 * max(1.0, b["grad_norm"])


# ---- snapshot / resume
class FixedTargetEnv(SnapshotToyEnv):
    """Every reset starts from the same paired targets (a deterministic reset, as the flat floor's)."""

    def reset(self):
        super().reset()
        self.tg = torch.linspace(-0.9, 0.9, self.n // 2, dtype=torch.float64).repeat_interleave(2)
        return self._obs()


def _snap_es(seed, **kw):
    algo = _toy_es(n=32, seed=seed, env=FixedTargetEnv(32, seed), sigma=0.05, learning_rate=0.02, **kw)
    algo.env = algo.env_step.__self__
    return algo


def test_resumed_es_run_is_the_interrupted_run(tmp_path):
    a = _snap_es(2)
    a.train_iteration(); a.train_iteration()
    p = str(tmp_path / "snap.pt")
    a.save(p)
    ck = torch.load(p, weights_only=True)
    assert ck["algo"] == "es" and ck["hidden_sizes"] == [32, 32] and ck["adam_t"] == 2 and ck["sigma"] == 0.05 and ck["learning_rate"] == 0.02
    assert ck["l2_coeff"] == 0.005 and ck["table_size"] == 1 << 16 and ck["table_seed"] == a.table_seed and ck["gen_off_state"] is not None
    tensors = [v for v in ck.values() if torch.is_tensor(v)] + [v for v in ck["policy"].values()]
    assert tensors and all(t.numel() < ck["table_size"] for t in tensors)   # the table is regenerated from its seed, never stored
    assert os.path.getsize(p) < 4 * ck["table_size"]
    ref = a.train_iteration()
    b = _snap_es(7, table_seed=12345)   # another policy, another table, another offset stream: all three come from the snapshot
    assert not torch.equal(a.table, b.table)
    _, restored = b.load(p)
    assert restored and b.adam_t == 2 and torch.equal(a.table, b.table)
    got = b.train_iteration()
    assert got == ref and got["itr"] == 2 and b.adam_t == 3
    assert torch.equal(T.flat_params(a.policy), T.flat_params(b.policy))
    assert torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v) and torch.equal(a.offsets, b.offsets)


def test_load_refuses_a_vpg_snapshot_and_trpo_continues_an_es_snapshot(tmp_path):
    env = ToyVecEnv(16, 0)
    torch.manual_seed(0)
    pol = T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=torch.float64)
    vpg = V.VPG(env.step, env.reset, pol, T.LinearFeatureBaseline(), 16, 4, AMAP(), batch_size=16 * 2)
    vpg.train_iteration()
    p = str(tmp_path / "vpg.pt")
    vpg.save(p)
    es = _toy_es(n=16)
    before = T.flat_params(es.policy).clone()
    with pytest.raises(ValueError, match="vpg.*es"):
        es.load(p)
    assert torch.equal(T.flat_params(es.policy), before)
    es.train_iteration()
    q = str(tmp_path / "es.pt")
    es.save(q)
    with pytest.raises(ValueError, match="es.*vpg"):
        vpg.load(q)
    env2 = ToyVecEnv(16, 0)
    pol2 = T.GaussianMLPPolicy(4, 2, (32, 32), init_std=1.0, dtype=torch.float64)
    trpo = T.TRPO(env2.step, env2.reset, pol2, T.LinearFeatureBaseline(), 16, 4, AMAP(), batch_size=16 * 2)
    trpo.load(q, restore_sampler=False)   # a TRPO run continues from an ES snapshot: the policy, log_std untouched
    assert torch.equal(T.flat_params(pol2), T.flat_params(es.policy)) and trpo.itr == 1
    assert np.isfinite(trpo.train_iteration()["loss_after"])


# ---- the kernel-call layer's host-side checks (nothing is launched) and the exports
def test_set_directions_refuses_bad_offsets_before_any_launch():
    table = torch.randn(5000)
    ek = E.EsKernels(table, 8, 26, 6)
    P, top = ek.P, 5000 - ek.P
    assert P == 2118 and E.param_count(26, (32, 32), 6) == P
    ek.fn["PolicyStep"] = ek.fn["Grad"] = ek.fn["Book"] = lambda *a: pytest.fail("a kernel was launched")
    good = torch.tensor([0, top, 5, 5], dtype=torch.int64)
    ek.set_directions(good)
    assert ek.offsets is good
    for bad in (torch.tensor([0, -1, 5, 5]), torch.tensor([0, top + 1, 5, 5])):
        with pytest.raises(ValueError, match="offsets must lie in"):
            ek.set_directions(bad)
    with pytest.raises(ValueError, match="int64"):
        ek.set_directions(good.to(torch.int32))
    with pytest.raises(ValueError, match="int64"):
        ek.set_directions(torch.tensor([0, 1, 2, 3, 4, 5, 6, 7])[0::2])   # not contiguous
    with pytest.raises(ValueError, match="one per pair"):
        ek.set_directions(torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="one per pair"):
        ek.set_directions(torch.tensor([0, 1, 2, 3, 4]))
    assert ek.offsets is good   # a refused call changes nothing
    ek.set_directions(torch.tensor([0, 4999, 5, 5]), n_params=1)
    with pytest.raises(ValueError, match="offsets must lie in"):
        ek.set_directions(torch.tensor([0, 5000, 5, 5]), n_params=1)
    for args in ((table, 7, 26, 6), (table, 8, 26, 5), (table, 8, 20, 6), (table.double(), 8, 26, 6), (table[:100], 8, 26, 6)):
        with pytest.raises(ValueError):
            E.EsKernels(*args)


def test_es_symbols_are_exported():
    from cassierl_amd import _lib
    from cassierl_amd import build as B
    L = ct.CDLL(B.build())
    names = [s for s in _lib.EXPORTS if s.startswith("CassieEs")]
    assert set(names) >= {"CassieEsParamCount", "CassieEsPolicyStep", "CassieEsBook", "CassieEsGradRows", "CassieEsGrad"}
    assert set(E.EsKernels.ENTRY.values()) == set(names) and "tu_es" in B.UNITS
    for s in names:
        assert hasattr(L, s), "missing export " + s
    assert [L.CassieEsParamCount(*s) for s in ((26, 6), (26, 7), (17, 7), (17, 6), (26, 5), (20, 6))] == [2118, 2151, 1863, 1830, 0, 0]
    assert [L.CassieEsGradRows(m) for m in (0, 1, 64, 65, 257, 4099, 32768)] == [0, 1, 1, 2, 5, 65, 128] and L.CassieEsPairsPerWorkgroup() >= 1
