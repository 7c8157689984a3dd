"""SAC at the Cassie3d shape, 45 observations and 10 actions (csrc/tu_sac3d.hip on the shape-generic kernels of csrc/sac_kernels.h and csrc/mlp32_tiles.h): the six CassieSac3d* entry points against the
torch statements of cassierl_amd/sac.py, the whole update and the resume on Cassie3dVecEnv, train_sac.py --env cassie3d and sim_policy.py.  -m gpu only.

Networks, pool and bounds are tests/test_gpu_sac.py's; the gradient bound is applied per parameter block, relative to the block's own largest entry,
with the blocks cut where the kernels' layout changes: the two column blocks of W1, the third action quad of the critic's W2, the slots 8 and 9 of
both heads of the actor's W3 / b3.

The hard cases of the gradient kernels and of the policy step at this shape live in tests/test_gpu_offpolicy_edges_cassie3d.py, on
tests/test_gpu_offpolicy_edges.py's method: batches from 1 to 256 and 4099, the log_std clamp on some and on every component, saturated actions, tied
critics, wild rows and the policy step with the wide head, every gradient block (the cuts of _blocks below, column 44 of W1 on its own) against
FLOAT64 autograd, for the critics too.  This file keeps the large batches (up to 32 801), the apply entries (1 to 256 partial rows), the
refusals, the whole update, the resume, the scripts and the timing."""
import copy
import ctypes as ct
import functools
import os
import sys
import time

import numpy as np
import pytest

from test_gpu_ddpg import _run
from test_gpu_sac import _log_alpha, _nets, _pool_with_margin

pytestmark = pytest.mark.gpu

D, A = 45, 10
NPI, NQ = 3188, 2881
EINVAL = -1


def _blocks(net, actor):
    """(name, index tensor into the flat parameter row) of the blocks the gradient bound is applied to."""
    import torch
    shapes = [tuple(p.shape) for p in net.parameters()]   # W1 b1 W2 b2 W3 b3
    start = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    at = lambda k: torch.arange(start[k], start[k + 1]).reshape(shapes[k])
    W1, b1, W2, b2, W3, b3 = (at(k) for k in range(6))
    out = [("W1[:, :32]", W1[:, :32]), ("W1[:, 32:]", W1[:, 32:]), ("b1", b1)]
    if actor:
        out += [("W2", W2), ("b2", b2)]
        for lo, hi in ((0, 8), (8, 10), (10, 18), (18, 20)):
            out += [("W3[%d:%d]" % (lo, hi), W3[lo:hi]), ("b3[%d:%d]" % (lo, hi), b3[lo:hi])]
    else:
        out += [("W2[:, :32]", W2[:, :32]), ("W2[:, 32:40]", W2[:, 32:40]), ("W2[:, 40:]", W2[:, 40:]), ("b2", b2), ("W3", W3), ("b3", b3)]
    assert sum(i.numel() for _, i in out) == start[-1]
    return [(n, i.reshape(-1).cuda()) for n, i in out]


def _check_blocks(what, got, ref32, blocks, ref64=None):
    """got within 2e-4 of ref32 per block, relative to the block's own largest entry; with ref64 the alternative of tests/test_gpu_sac.py: the
    error against float64 at most four times that of float32 autograd against float64."""
    bad = []
    for name, i in blocks:
        g, r = got[i], ref32[i]
        err, top = (g - r).abs().max().item(), r.abs().max().item()
        line = "%s %s: max error %.3g of max %.3g" % (what, name, err, top)
        ok = err < 2e-4 * top
        if ref64 is not None:
            ek, et = (g.double() - ref64[i]).abs().max().item(), (r.double() - ref64[i]).abs().max().item()
            line += "; against float64: kernel %.3g, torch float32 %.3g" % (ek, et)
            ok = ok or ek <= 4 * et
        print(line)
        if not ok:
            bad.append(line)
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _setup(seed=3, wide=False):
    """Networks, the pool built by rejection, the noise of its rows and the kernels: made once, shared by the cases, left unchanged."""
    from cassierl_amd import sac as S
    kw = dict(ls_width=4.0, ls_bias=-9.0) if wide else {}
    nets = _nets(D, A, seed, **kw)
    pool, row_noise, dropped = _pool_with_margin(*nets[:3], D, A, inside=not wide)
    la = _log_alpha()
    return nets, pool, row_noise, dropped, la, S.SacKernels(*nets, la)


def _actor_loss(p, c1, c2, s_, e_, al):
    import torch
    at, lp = p.sample(s_, e_)
    qm = torch.min(c1(s_, at), c2(s_, at))
    return (al * lp - qm).mean(), lp, qm


def _flat_grad(loss, net):
    import torch
    return torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(net.parameters()))])


# ------------------------------------------------------------------------------------------------------------------ policy step
def _boxes():
    from cassierl_amd.vec_env3d import action_space
    pd = action_space("PD")
    k = np.arange(A, dtype=np.float64)
    return {"PD": (pd.low, pd.high), "synthetic": (-1.0 - 0.37 * k, 0.5 + 0.61 * k * k)}   # ten distinct pairs: a permuted slot cannot pass


@pytest.mark.parametrize("box", ["PD", "synthetic"])
@pytest.mark.parametrize("n", [1, 33, 130, 257])
def test_policy_step_matches_the_torch_statement(n, box):
    import torch
    from cassierl_amd import sac as S
    from cassierl_amd import trpo as T
    pol, qf1, qf2, _, _ = _nets(D, A, 7)
    low, high = _boxes()[box]
    assert box == "PD" or (len(set(low.tolist())) == A and len(set(high.tolist())) == A)
    amap = T.NormalizedActions(low, high, "cuda")
    algo = S.SAC(None, None, pol, qf1, qf2, n, D, amap, replay_pool_size=3 * n)
    fused = algo._fused_step(torch.device("cuda:0"))
    assert fused is not None
    step, pool = fused[0], algo.pool
    lo, hi = torch.as_tensor(low, device="cuda"), torch.as_tensor(high, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(n)
    for top in (n, 2 * n, 0):   # the middle of the ring, an append that ends exactly at capacity, the next one at 0
        for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs):
            t.copy_(torch.randn(t.shape, device="cuda", generator=g))
        before = [t.clone() for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs)]
        obs = torch.randn(n, D, dtype=torch.float64, device="cuda", generator=g)
        noise = torch.randn(n, A, device="cuda", generator=g)
        with torch.no_grad():
            a_ref = algo._explore(obs.float(), noise)
        step(obs, noise, top)
        act = pool.act[top:top + n]
        assert torch.equal(pool.obs[top:top + n], obs.float())
        err = (act - a_ref).abs().max().item()
        print("policy step n %d box %s top %d: max action error %.3g" % (n, box, top, err))
        assert err < 5e-6 * (1 + a_ref.abs().max().item())
        assert (algo._env_actions - amap(act)).abs().max().item() < 1e-12
        assert (algo._env_actions >= lo).all() and (algo._env_actions <= hi).all()
        rest = torch.ones(pool.capacity, dtype=torch.bool, device="cuda")
        rest[top:top + n] = False
        for now, was in zip((pool.obs, pool.act), before[:2]):
            assert torch.equal(now[rest], was[rest])
        for now, was in zip((pool.rew, pool.term, pool.nobs), before[2:]):
            assert torch.equal(now, was)


# ------------------------------------------------------------------------------------------------------------------ gradients
def _gradients_case(setup, idx):
    """Both kernels on the batch idx (clamped into the pool for the reference) against autograd; returns the actor's partial and the raw log_std."""
    import torch
    (pol, qf1, qf2, tq1, tq2), pool, row_noise, _, la, k = setup
    batch = idx.numel()
    alpha, gamma = la.exp(), 0.99
    ci = idx.clamp(0, pool.capacity - 1)
    g = torch.Generator(device="cuda").manual_seed(5)
    eps_s = row_noise[ci].contiguous()
    eps_s2 = torch.randn(batch, A, device="cuda", generator=g)
    s, a, r, term, s2 = pool.sample(ci)
    rows = k.L.CassieDdpgPartialRows(batch)
    # ---- critics
    with torch.no_grad():
        a2, lp2 = pol.sample(s2, eps_s2)
        y = r + (1 - term) * gamma * (torch.min(tq1(s2, a2), tq2(s2, a2)) - alpha * lp2)
    k._rows("critic", batch, 2, -1, NQ + 2).fill_(float("nan"))
    part = k.critic_grad(pool, idx, eps_s2, gamma).clone()
    assert part.shape == (2, rows, NQ + 2) and torch.isfinite(part).all()
    for i, qf in enumerate((qf1, qf2)):
        q = qf(s, a)
        loss = ((q - y) ** 2).mean()
        gref = _flat_grad(loss, qf)
        tot = part[i].double().sum(0)
        _check_blocks("batch %d critic %d" % (batch, i + 1), (tot[:NQ] / batch).float(), gref, _blocks(qf, False))
        assert abs(tot[NQ].item() / batch - loss.double().item()) < 1e-5 * abs(loss.item())
        assert abs(tot[NQ + 1].item() / batch - q.double().mean().item()) < 1e-5 * abs(q.double().mean().item())
    assert torch.equal(part, k.critic_grad(pool, idx, eps_s2, gamma))   # fixed-order sums: the same bits twice
    # ---- actor
    loss, lp, qm = _actor_loss(pol, qf1, qf2, s, eps_s, alpha)
    gref = _flat_grad(loss, pol)
    p64, c64a, c64b = (copy.deepcopy(m).double() for m in (pol, qf1, qf2))
    g64 = _flat_grad(_actor_loss(p64, c64a, c64b, s.double(), eps_s.double(), alpha.double())[0], p64)
    k._rows("actor", batch, -1, NPI + 2).fill_(float("nan"))
    part = k.actor_grad(pool, idx, eps_s).clone()
    assert part.shape == (rows, NPI + 2) and torch.isfinite(part).all()
    tot = part.double().sum(0)
    _check_blocks("batch %d actor" % batch, (tot[:NPI] / batch).float(), gref, _blocks(pol, True), g64)
    print("mean log pi %.8g / %.8g; mean min Q %.8g / %.8g" % (tot[NPI].item() / batch, lp.double().mean().item(), tot[NPI + 1].item() / batch, qm.double().mean().item()))
    assert abs(tot[NPI].item() / batch - lp.double().mean().item()) < 1e-5 * abs(lp.double().mean().item())
    assert abs(tot[NPI + 1].item() / batch - qm.double().mean().item()) < 1e-5 * abs(qm.double().mean().item())
    assert torch.equal(part, k.actor_grad(pool, idx, eps_s))
    with torch.no_grad():
        raw = pol.l3(torch.relu(pol.l2(torch.relu(pol.l1(s)))))[:, A:]
    return part, raw


def _indices(pool, batch):
    import torch
    g = torch.Generator(device="cuda").manual_seed(batch)
    idx = torch.randint(0, pool.size, (batch,), device="cuda", generator=g)
    idx[1] = idx[0]
    assert idx.unique().numel() < batch
    return idx


@pytest.mark.parametrize("batch", [77, 1000, 4099, 32801])
def test_gradients_match_autograd(batch):
    """CassieSac3dCriticGrad and CassieSac3dActorGrad against float32 autograd on the gathered batch, per parameter block; a repeated index in each;
    32 801 is one tile past 256 x 4 x 32, so that one wavefront takes a second tile.  At most 3 % of the pool's candidates may be dropped."""
    setup = _setup()
    print("margins: %.2f %% of the candidate rows dropped" % (100 * setup[3]))
    assert setup[3] <= 0.03
    _gradients_case(setup, _indices(setup[1], batch))


def test_gradients_with_wild_indices():
    """Batch 77 with an index below 0 and one at and one above the capacity: the gather clamps them."""
    setup = _setup()
    idx = _indices(setup[1], 77)
    idx[5], idx[40], idx[76] = -3, setup[1].capacity, setup[1].capacity + 12345
    _gradients_case(setup, idx)


def test_gradients_with_the_clamp_active():
    """Batch 130 with a log_std head that crosses both bounds of the clamp; the batch is drawn so that actions 8 and 9 -- the slots of registers 4, 5
    and 12, 13 -- have rows with the clamp active and rows inside it.  Where a component's clamp is active on every row its log_std rows of
    W3 / b3 are exactly zero in every partial row."""
    import torch
    setup = _setup(wide=True)
    pol, pool = setup[0][0], setup[1]
    with torch.no_grad():
        raw = pol.l3(torch.relu(pol.l2(torch.relu(pol.l1(pool.obs)))))[:, A:]
    out = (raw > 2.0) | (raw < -20.0)
    pick = [torch.nonzero(out[:, a])[:8, 0] for a in (8, 9)] + [torch.nonzero(~out[:, a])[:8, 0] for a in (8, 9)]
    idx = _indices(pool, 130)
    head = torch.cat(pick)
    idx[2:2 + head.numel()] = head
    part, raw_b = _gradients_case(setup, idx)
    out_b = (raw_b > 2.0) | (raw_b < -20.0)
    print("clamp active on %s of 130 rows per action; above 2: %d, below -20: %d components" %
          (out_b.sum(0).tolist(), int((raw_b > 2.0).sum()), int((raw_b < -20.0).sum())))
    assert (raw_b > 2.0).any() and (raw_b < -20.0).any()
    for a in (8, 9):
        assert out_b[:, a].any() and (~out_b[:, a]).any()
    W3, b3 = 32 * D + 32 + 32 * 32 + 32, 32 * D + 32 + 32 * 32 + 32 + 20 * 32
    for a in range(A):
        if out_b[:, a].all():
            assert (part[:, W3 + (A + a) * 32:W3 + (A + a + 1) * 32] == 0).all() and (part[:, b3 + A + a] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("rows", [1, 2, 64, 256])
@pytest.mark.parametrize("learn_alpha", [True, False])
def test_apply_matches_adam_and_the_log_alpha_step(learn_alpha, rows):
    """Five steps with gradients spanning 1e-4 .. 1: CassieSac3dActorApply (actor, log_alpha) and CassieSac3dCriticApply (Adam + soft update).
    rows: 2 takes column_sum's tail loop alone, 64 its groups of eight alone, 256 is MAX_BLOCKS, the most partial rows a gradient launch writes."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import sac as S
    from cassierl_amd import trpo as T
    from cassierl_amd.vpg import adam_step_
    pol, qf1, qf2, tq1, tq2 = _nets(D, A, 4)
    la = _log_alpha(0.7)
    k = S.SacKernels(pol, qf1, qf2, tq1, tq2, la)
    assert k.ENTRY["SacApply"] == "CassieSac3dActorApply" and k.ENTRY["Apply"] == "CassieSac3dCriticApply" and (k.np_pi, k.np_q) == (NPI, NQ)
    pol_r, qf_r, tq_r, la_r = copy.deepcopy(pol), copy.deepcopy(qf2), copy.deepcopy(tq2), la.clone()
    adam_pi, adam_pi_r, adam_q, adam_q_r = G.new_adam(pol), G.new_adam(pol_r), G.new_adam(qf2), G.new_adam(qf_r)
    adam_a, adam_a_r = S.new_alpha_adam(la), S.new_alpha_adam(la_r)
    assert T.flat_params(pol).numel() == NPI and T.flat_params(qf2).numel() == NQ
    stats, want = torch.zeros(5, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda")
    lr, alr, tau, scale, tent = 1e-3, 3e-3, 5e-3, 1.0 / 37, -10.0
    torch.manual_seed(5)
    for t in range(1, 6):
        mag = lambda n: 10.0 ** torch.randint(-4, 1, (n,), device="cuda").float()
        part = torch.randn(rows, NPI + 2, device="cuda") * mag(NPI + 2)
        partq = torch.randn(2, rows, NQ + 2, device="cuda") * mag(NQ + 2)
        alpha_before = la.double().exp().item()
        k.actor_apply(part, scale, adam_pi, lr, 0.9, 0.999, 1e-8, adam_a if learn_alpha else None, alr, tent, stats[2:])
        k.critic_apply(1, partq[1], scale, adam_q, lr, 0.9, 0.999, 1e-8, tau, stats)
        G._adam_on(pol_r, part[:, :NPI].sum(0) * scale, adam_pi_r, lr, 0.9, 0.999, 1e-8)
        if learn_alpha:
            adam_a_r["t"] += 1
            adam_step_(la_r, -(part[:, NPI].sum(0, keepdim=True) * scale + tent), adam_a_r["m"], adam_a_r["v"], adam_a_r["t"], alr)
        G._adam_on(qf_r, partq[1, :, :NQ].sum(0) * scale, adam_q_r, lr, 0.9, 0.999, 1e-8)
        G.soft_update_(tq_r, qf_r, tau)
        sums = part[:, NPI:].double().sum(0)
        want += torch.cat([partq[1, :, NQ:].double().sum(0), sums, (alpha_before * sums[0] - sums[1]).reshape(1)])
        assert adam_pi["t"] == adam_q["t"] == t and adam_a["t"] == (t if learn_alpha else 0)
    pairs = [(T.flat_params(pol), T.flat_params(pol_r)), (adam_pi["m"], adam_pi_r["m"]), (adam_pi["v"], adam_pi_r["v"]), (T.flat_params(qf2), T.flat_params(qf_r)),
             (T.flat_params(tq2), T.flat_params(tq_r)), (adam_q["m"], adam_q_r["m"]), (adam_q["v"], adam_q_r["v"]), (la, la_r)]
    if learn_alpha:
        pairs += [(adam_a["m"], adam_a_r["m"]), (adam_a["v"], adam_a_r["v"])]
        assert la.item() != float(np.float32(np.log(0.7)))
    else:
        assert la.item() == float(np.float32(np.log(0.7))) and adam_a["m"].item() == 0
    for a, b in pairs:
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item(), ((a - b).abs().max().item(), b.abs().max().item())
    print("apply statistics: %s / %s" % (stats.tolist(), want.tolist()))
    assert (stats[:4] - want[:4]).abs().max().item() <= 1e-12 * want[:4].abs().max().item()
    assert abs(stats[4].item() - want[4].item()) <= 1e-12 * abs(want[4].item())


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_alone():
    """A null network pointer, batch = 0, a misaligned partial pointer and the shape (26, 6): CASSIE_EINVAL, and nothing is written."""
    import torch
    from cassierl_amd.offpolicy import _P, _ptrs
    (pol, qf1, qf2, tq1, tq2), pool, row_noise, _, la, k = _setup()
    batch = 77
    idx = _indices(pool, batch)
    eps = torch.randn(batch, A, device="cuda")
    rows = k.L.CassieDdpgPartialRows(batch)
    pc = torch.full((2 * rows * (NQ + 2) + 4,), float("nan"), device="cuda")
    pa = torch.full((rows * (NPI + 2) + 4,), float("nan"), device="cuda")
    stream = lambda: ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    off = lambda t, b: ct.c_void_p(t.data_ptr() + b)

    def critic(actor=None, n=batch, shape=(D, A), out=None):
        return k.L.CassieSac3dCriticGrad(_P(pool.obs), _P(pool.act), _P(pool.rew), _P(pool.term), _P(pool.nobs), ct.c_longlong(pool.capacity), _P(idx), n, *shape,
                                         _ptrs(pol) if actor is None else actor[0], _ptrs(tq1), _ptrs(tq2), _ptrs(qf1), _ptrs(qf2), _P(eps), _P(la), ct.c_float(0.99),
                                         _P(pc) if out is None else out, stream())

    def actor(net=None, n=batch, shape=(D, A), out=None):
        return k.L.CassieSac3dActorGrad(_P(pool.obs), ct.c_longlong(pool.capacity), _P(idx), n, *shape, _ptrs(pol) if net is None else net[0], _ptrs(qf1), _ptrs(qf2),
                                        _P(eps), _P(la), _P(pa) if out is None else out, stream())

    holed = (ct.c_void_p * 6)(*[p.data_ptr() for p in (pol.l1.weight, pol.l1.bias, pol.l2.weight)], None, pol.l3.weight.data_ptr(), pol.l3.bias.data_ptr())
    for fn, buf in ((critic, pc), (actor, pa)):
        assert fn((None,)) == EINVAL and fn((holed,)) == EINVAL
        assert fn(n=0) == EINVAL and fn(n=-5) == EINVAL
        assert fn(out=off(buf, 2)) == EINVAL and fn(out=ct.c_void_p(None)) == EINVAL
        assert fn(shape=(26, 6)) == EINVAL and fn(shape=(45, 6)) == EINVAL and fn(shape=(44, 10)) == EINVAL
    # the policy step and the two apply entries
    n = 33
    obs = torch.randn(n, D, dtype=torch.float64, device="cuda")
    low, high = torch.full((A,), -1.0, dtype=torch.float64, device="cuda"), torch.full((A,), 1.0, dtype=torch.float64, device="cuda")
    o32, act, env = (torch.full(s, float("nan"), dtype=dt, device="cuda") for s, dt in (((n, D), torch.float32), ((n, A), torch.float32), ((n, A), torch.float64)))
    step = lambda net=None, m=n, shape=(D, A): k.L.CassieSac3dPolicyStep(_P(obs), m, *shape, _ptrs(pol) if net is None else net[0], _P(eps), _P(low), _P(high), _P(o32),
                                                                      _P(act), _P(env), stream())
    assert step((None,)) == EINVAL and step(m=0) == EINVAL and step(shape=(26, 6)) == EINVAL
    m, v = torch.full((NPI,), float("nan"), device="cuda"), torch.full((NPI,), float("nan"), device="cuda")
    f = lambda *xs: [ct.c_float(x) for x in xs]
    aapply = lambda shape=(D, A), rws=rows, out=None: k.L.CassieSac3dActorApply(rws, *shape, _P(pa) if out is None else out, ct.c_float(1.0), _ptrs(pol), _P(m), _P(v), 1,
                                                                              *f(1e-3, 0.9, 0.999, 1e-8), _P(la), None, None, 0, *f(1e-3, -10.0), None, stream())
    capply = lambda shape=(D, A), rws=rows, out=None: k.L.CassieSac3dCriticApply(rws, *shape, _P(pc) if out is None else out, ct.c_float(1.0), _ptrs(qf1), _ptrs(tq1), _P(m),
                                                                               _P(v), 1, *f(1e-3, 0.9, 0.999, 1e-8, 5e-3), None, stream())
    before = [copy.deepcopy(x.state_dict()) for x in (pol, qf1, tq1)]
    for fn in (aapply, capply):
        assert fn(shape=(26, 6)) == EINVAL and fn(rws=0) == EINVAL and fn(out=off(pa, 2)) == EINVAL and fn(out=ct.c_void_p(None)) == EINVAL
    torch.cuda.synchronize()
    for t in (pc, pa, o32, act, env, m, v):
        assert torch.isnan(t).all()
    for net, sd in zip((pol, qf1, tq1), before):
        assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), sd.values()))
    assert k.L.CassieSacApply(rows, D, A, _P(pa), ct.c_float(1.0), _ptrs(pol), _P(m), _P(v), 1, *f(1e-3, 0.9, 0.999, 1e-8), _P(la), None, None, 0, *f(1e-3, -10.0), None,
                              stream()) == EINVAL   # the 26-wide entries keep refusing this shape
    assert k.L.CassieDdpgParamCount(D, A, 1) == 0 and k.L.CassieSacParamCount(D, A) == 0


# ------------------------------------------------------------------------------------------------------------------ the whole update
def test_fused_update_equals_the_torch_update_on_cassie3d():
    """256 Cassie3d environments, PD mode, 8 vector steps into the pool through the fused policy step, then three updates of batch 256 with
    fused_update True and False from the same state, the same indices and the same noises."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import sac as S
    from cassierl_amd import trpo as T
    algo = S.make_cassie_sac(256, env="cassie3d", control_mode="PD", seed=1, replay_pool_size=256 * 8, batch_size=256, min_pool_size=10 ** 9)
    assert algo.obs_dim == D and algo.act_dim == A and algo.env_family == "cassie3d" and algo.target_entropy == -10.0
    for _ in range(8):
        assert algo.train_step() == 0
    assert algo.last_policy_step_fused and algo.pool.size == 256 * 8 and algo.pool.top == 0
    assert torch.isfinite(algo.pool.obs).all() and torch.isfinite(algo.pool.nobs).all() and torch.isfinite(algo.pool.rew).all()
    assert algo.pool.act.abs().max().item() <= 1.0 and algo.pool.act.std().item() > 0.1
    nets = (algo.policy, algo.qf1, algo.qf2, algo.target_qf1, algo.target_qf2)
    state0 = [copy.deepcopy(n.state_dict()) for n in nets]
    theta0 = [T.flat_params(n).clone() for n in nets] + [algo.log_alpha.clone()]
    draws = [(algo.sample_indices(), algo.sample_noise()) for _ in range(3)]
    res = {}
    for fused in (True, False):
        for n, sd in zip(nets, state0):
            n.load_state_dict(sd)
        algo.log_alpha.copy_(theta0[-1])
        algo.adam_pi, algo.adam_q1, algo.adam_q2 = G.new_adam(algo.policy), G.new_adam(algo.qf1), G.new_adam(algo.qf2)
        algo.adam_alpha = S.new_alpha_adam(algo.log_alpha)
        algo.fused_update = fused
        for idx, noise in draws:
            algo.update(idx, noise)
            assert algo.last_update_kind == ("sac_kernels" if fused else "torch")
        res[fused] = [T.flat_params(n).clone() for n in nets] + [algo.log_alpha.clone()]
    rels = [((a - b).norm() / b.norm()).item() for a, b in zip(res[True], res[False])]
    moved = [(a - t0).norm().item() for a, t0 in zip(res[False], theta0)]
    print("fused vs torch update, relative difference (actor, qf1, qf2, target_qf1, target_qf2, log_alpha): %s; moved by %s" % (rels, moved))
    assert all(m > 0 for m in moved)
    assert all(r < 1e-5 for r in rels), rels
    algo.env.close()


# ------------------------------------------------------------------------------------------------------------------ resume
def _state_of(algo):
    import torch
    from cassierl_amd import trpo as T
    out = [T.flat_params(getattr(algo, n)).clone() for n in ("policy", "qf1", "qf2", "target_qf1", "target_qf2")]
    for a in algo.ADAMS:
        ad = getattr(algo, a)
        out += [ad["m"].clone(), ad["v"].clone(), torch.tensor([ad["t"]])]
    p = algo.pool
    out += [algo.log_alpha.clone(), p.obs.clone(), p.act.clone(), p.rew.clone(), p.term.clone(), p.nobs.clone(), torch.tensor([p.top, p.size]),
            torch.from_numpy(algo.env.get_full_state_host().copy()), algo.obs.clone(), algo.path_t.clone(), algo.path_ret.clone()]
    return out


def test_resume_equals_the_uninterrupted_run(tmp_path):
    """A: two epochs.  B: one epoch, save, a fresh algorithm loads, one more epoch.  Networks, Adam states, log_alpha, the pool and the environment's
    state records are equal bit for bit (the ring wraps at 8 steps, paths are truncated at 10)."""
    import torch
    from cassierl_amd import sac as S
    mk = lambda: S.make_cassie_sac(256, env="cassie3d", control_mode="PD", seed=1, replay_pool_size=256 * 8, batch_size=256, min_pool_size=512, epoch_length=6,
                                   max_path_length=10)
    a = mk()
    a.train_iteration()
    ref = a.train_iteration()
    assert ref["update_kind"] == "sac_kernels" and ref["updates"] == 6 and a.last_policy_step_fused
    want = _state_of(a)
    a.env.close()
    b = mk()
    b.train_iteration()
    snap = str(tmp_path / "snap.pt")
    b.save(snap)
    b.env.close()
    ck = torch.load(snap, map_location="cpu", weights_only=True)
    assert ck["env_family"] == "cassie3d" and ck["env_config"]["control_mode"] == "PD" and ck["env_config"]["kp"] == [10.0] * 10 and ck["algo"] == "sac"
    c = mk()
    _, restored = c.load(snap)
    assert restored and c.pool_restored
    got = c.train_iteration()
    for key in ("itr", "avg_reward", "qf1_loss", "qf2_loss", "policy_loss", "avg_log_pi", "alpha", "avg_q", "episodes"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    for x, y in zip(_state_of(c), want):
        assert torch.equal(x.cpu(), y.cpu())
    c.env.close()
    other = S.make_cassie_sac(64, env="cassie3d", control_mode="PD", kp=20.0, replay_pool_size=64 * 8, batch_size=64)
    with pytest.raises(ValueError, match="configured with"):
        other.load(snap)
    other.env.close()


# ------------------------------------------------------------------------------------------------------------------ scripts
def test_train_sac_on_cassie3d_and_its_snapshot(tmp_path):
    """train_sac.py --env cassie3d for two short epochs at 256 environments; sim_policy.py rolls the snapshot out; a Cassie2d SAC refuses it."""
    from conftest import ROOT
    from cassierl_amd import sac as S
    from cassierl_amd.trajectory import default_gait
    snap = str(tmp_path / "snap.pt")
    st = _run([sys.executable, os.path.join(ROOT, "train_sac.py"), "--env", "cassie3d", "--envs-per-gpu", "256", "--batch-size", "256", "--pool-size", "2048",
               "--min-pool-size", "512", "--epoch-length", "4", "--n-epochs", "2", "--snapshot", snap])
    assert os.path.exists(snap) and len(st) == 2 and st[-1]["update_kind"] == "sac_kernels" and st[-1]["updates"] == 4 and st[-1]["env_steps"] == 256 * 4
    assert all(np.isfinite(st[-1][key]) for key in ("qf1_loss", "qf2_loss", "policy_loss", "avg_log_pi", "alpha", "avg_reward"))
    base = [sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "128", "--max-path-length", "30"]
    det, smp = _run(base + ["--deterministic"])[-1], _run(base)[-1]
    for r, d in ((det, True), (smp, False)):
        assert r["itr"] == 2 and r["envs"] == 128 and r["deterministic"] == d and 0 < r["avg_path_length"] <= 30 and np.isfinite(r["avg_return"])
    assert det["avg_return"] != smp["avg_return"]
    two = S.make_cassie_sac(64, kind="stand", control_mode="Torque", trajectory=default_gait(), replay_pool_size=64 * 8, batch_size=64)
    with pytest.raises(ValueError, match="cassie3d.*cassie2d"):
        two.load(snap)
    two.env.close()


# ------------------------------------------------------------------------------------------------------------------ timing
def test_update_timing_batch_4096():
    """One fused update at batch 4096 against sac_update_torch_ on the same state, alternated, medians of 20 synchronised repeats after a warm-up.
    The kernels replace well over a hundred launches with five: a fused update that loses to the launch-bound torch statement is broken, not slow."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import sac as S
    (pol, qf1, qf2, tq1, tq2), pool, _, _, _, _ = _setup()
    nets = {f: tuple(copy.deepcopy(n) for n in (pol, qf1, qf2, tq1, tq2)) for f in (True, False)}   # copies: the shared setup stays unchanged
    las = {True: _log_alpha(), False: _log_alpha()}
    k = S.SacKernels(*nets[True], las[True])
    idx = torch.randint(0, pool.size, (4096,), device="cuda")
    noise = torch.randn(2, 4096, A, device="cuda")
    adam = {f: (G.new_adam(nets[f][0]), G.new_adam(nets[f][1]), G.new_adam(nets[f][2]), S.new_alpha_adam(las[f])) for f in (True, False)}

    def fused():
        k.update(pool, idx, noise[0], noise[1], 0.99, 3e-4, 3e-4, 3e-4, 5e-3, -10.0, *adam[True])

    def torch_update():
        S.sac_update_torch_(*nets[False], las[False], *adam[False], pool.sample(idx), noise[0], noise[1], 0.99, 3e-4, 3e-4, 3e-4, 5e-3, -10.0)

    out = {}
    for name, fn in (("fused", fused), ("torch", torch_update)) * 2:   # alternated, the second round kept
        for _ in range(5):
            fn()
        ts = []
        for _ in range(20):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        out[name] = float(np.median(ts)) * 1e3
    print("SAC update ms at batch 4096, 45 x 10: %s; torch / fused %.2f" % (out, out["torch"] / out["fused"]))
    assert out["fused"] < out["torch"]
