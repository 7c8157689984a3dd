"""SAC's update kernels at Cassie3d's shape, 45 observations and 10 actions (csrc/tu_sac3d.hip: the <45, 10> instantiation of csrc/sac_kernels.h and
csrc/mlp32_tiles.h), where tests/test_gpu_sac_cassie3d.py does not look: the hard cases of tests/test_gpu_offpolicy_edges.py -- batches of a tile
or less, the log_std clamp on some or all components, saturated actions, tied critics, wild rows, the policy step with the clamp active -- through
the six CassieSac3d* entry points.  -m gpu only.  (The apply entries at 2 and 256 partial rows are cases of
test_gpu_sac_cassie3d.test_apply_matches_adam_and_the_log_alpha_step.)

Method, reference and bounds are test_gpu_offpolicy_edges.py's, through its own helpers: float64 torch autograd of cassierl_amd/sac.py's statements on
networks and data cast up; a gradient max|g_kernel - g_64| < 2e-4 max|g_64|, a statistic column 1e-5 relative, an action 5e-6 (1 + max|a_64|), or
else the kernel's error at most 4 times that of torch's float32 evaluation of the same statement; every gradient launch twice, bit for bit; the
partial rows prefilled with NaN and finite afterwards.  What is this file's own:

  * The gradient bound holds PER PARAMETER BLOCK, relative to the block's own largest float64 entry (the smallest block's largest entry is a few
    per cent of the whole vector's: a bound over the whole vector would let a block be wrong by its full size), for the critics against float64
    too.  The blocks are test_gpu_sac_cassie3d._blocks' cuts -- where the kernels' layout changes -- with W1[:, 32:] cut again at column 44, the
    lone feature of the last first-layer k-step (DESIGN.md 9u says which constant of mlp32_tiles.h's Shape each cut isolates).  No block's float64
    maximum may be 0, except the log_std blocks where every component is clamped: those are exactly 0 in every partial row and both references.
  * A statistic's bound is relative to the statistic, so |mean| >= 0.1 mean|per-sample value| (float64) is asserted of each: a mean that cancels
    would make the bound one on noise.  (A critic's loss is a mean of squares: nothing to cancel.)
  * A condition on the DATA that a draw misses (the 0.1 above, the clamp shares of the `wide` cases) is repaired by another seed of that case's
    index, SEED_BUMP, with the reason next to it -- never by a wider condition or bound.

Networks, pools and kernel objects are test_gpu_offpolicy_edges._sac(45, 10, kind): built once per kind and never written to."""
import copy
import functools

import pytest

import test_gpu_offpolicy_edges as E
import test_gpu_sac as TS
import test_gpu_sac_cassie3d as C

pytestmark = pytest.mark.gpu

D, A, NPI, NQ = C.D, C.A, C.NPI, C.NQ
GAMMA = E.GAMMA
# E.SMALL and: 16 | 17, the lane-half boundary of the transposed operand (gather: sm = s0 + 16 h + s); 128, a workgroup's four full tiles;
# 4099, the grid-stride loop with a ragged last tile
SMALL = [1, 4, 16, 17, 31, 32, 33, 127, 128, 129, 256, 4099]
LS_BLOCKS = ("W3[10:18]", "b3[10:18]", "W3[18:20]", "b3[18:20]")   # the log_std head: registers v + HREG, image rows 16 + a
SEED_BUMP = {}   # (kind, batch) -> added to the seed of that case's index, where the first seed misses a condition on the data asserted below


# ------------------------------------------------------------------------------------------------------------------ blocks
@functools.lru_cache(maxsize=None)
def _cuts(actor):
    """test_gpu_sac_cassie3d._blocks' cuts, W1[:, 32:] cut into the full k-steps 16 .. 21 and column 44, which k-step 22 carries alone."""
    nets = E._sac(D, A, "narrow")[0]
    out = []
    for name, i in C._blocks(nets[0] if actor else nets[1], actor):
        if name == "W1[:, 32:]":
            i = i.reshape(32, D - 32)
            out += [("W1[:, 32:44]", i[:, :12].reshape(-1)), ("W1[:, 44]", i[:, 12].reshape(-1))]
        else:
            out.append((name, i))
    assert sum(i.numel() for _, i in out) == (NPI if actor else NQ) and all(n in [m for m, _ in out] for n in (LS_BLOCKS if actor else ()))
    return out


def _check_blocks(what, part, batch, ref64, ref32, actor, zero=()):
    """The rows of `part` added in float64 and divided by the batch against ref64, block by block with E._check's rule; the blocks named in `zero`
    are exactly 0 in every partial row and in both references, and no other block's float64 maximum is 0.  Every block is looked at before the
    first failure is raised."""
    tot = part.double().sum(0) / batch
    bad = []
    for name, i in _cuts(actor):
        top = ref64[i].abs().max().item()
        if name in zero:
            ok = bool(top == 0 and (ref32[i] == 0).all() and (part[:, i] == 0).all())
            print("%s %s: float64 max %.3g, float32 max %.3g, partial rows max %.3g (%s)" %
                  (what, name, top, ref32[i].abs().max().item(), part[:, i].abs().max().item(), "zero" if ok else "NOT zero"))
            if not ok:
                bad.append("%s %s: not exactly 0" % (what, name))
            continue
        assert top > 0, (what, name)
        try:
            E._check("%s %s" % (what, name), tot[i], ref64[i], ref32[i], 2e-4)
        except AssertionError as e:
            bad.append(str(e).split("\n")[0])   # E._check's (name, kernel error, float32 error, scale)
    assert not bad, bad


def _check_stat(name, got, mean64, mean32, per64, problems):
    """A statistic column with E._check's 1e-5 rule; its float64 per-sample values say whether the mean is one the relative bound means something for."""
    per64 = per64.reshape(-1)
    assert abs(per64.mean().item() - mean64.item()) <= 1e-12 * abs(mean64.item()), name
    ratio = abs(mean64.item()) / per64.abs().mean().item()
    print("%s: |mean| / mean|per-sample value| %.3g" % (name, ratio))
    if ratio < 0.1:
        problems.append((name, "|mean| / mean|per-sample value|", ratio))
    E._check(name, got, mean64, mean32, 1e-5)


# ------------------------------------------------------------------------------------------------------------------ one batch
def _draw(kind, batch, bump=None):
    """The batch of one case: index (positions 0 and 1 the same row), both noises, the gathered rows in float32 and float64, the float64 heads at s
    and s', and the float64 per-sample values of the statistics."""
    import torch
    nets, nets64, pool, row_noise = E._sac(D, A, kind)[:4]
    idx, g = E._indices(pool, batch, seed=5 + (SEED_BUMP.get((kind, batch), 0) if bump is None else bump))
    eps_s = row_noise[idx].contiguous()   # the noise the row met the margins with
    eps_s2 = torch.randn(batch, A, device="cuda", generator=g)
    data = pool.sample(idx)
    d64 = [t.double() for t in data]
    heads = E._head(nets64[0], d64[0], eps_s.double()) + E._head(nets64[0], d64[4], eps_s2.double())
    pol, qf1, qf2 = nets64[:3]
    with torch.no_grad():
        at, lp = pol.sample(d64[0], eps_s.double())
        per = dict(q1=qf1(d64[0], d64[1]), q2=qf2(d64[0], d64[1]), lp=lp, qm=torch.min(qf1(d64[0], at), qf2(d64[0], at)))
    return idx, eps_s, eps_s2, data, d64, heads, per


def _conditions(heads, mixed):
    """Prints the clamp and saturation shares of the batch; returns the misses of the conditions that keep a `wide` case honest."""
    raw, u, raw2, u2 = heads
    share = lambda m: m.double().mean().item()
    print("log_std above 2 / below -20: %.2f %% / %.2f %% at s, %.2f %% / %.2f %% at s'; |u| > 9: %.2f %% / %.2f %%; max |u| %.3g; min |u| %.3g" %
          (100 * share(raw > 2), 100 * share(raw < -20), 100 * share(raw2 > 2), 100 * share(raw2 < -20), 100 * share(u.abs() > 9), 100 * share(u2.abs() > 9),
           u.abs().max().item(), u.abs().min().item()))
    problems = []
    if mixed:
        for where, r_, u_ in (("s", raw, u), ("s'", raw2, u2)):   # E._sac_case's `mixed` conditions
            for what, got, least in (("above 2", share(r_ > 2), 0.01), ("below -20", share(r_ < -20), 0.01), ("|u| > 9", share(u_.abs() > 9), 0.005)):
                if got < least:
                    problems.append((where, what, got))
        out = (raw > 2) | (raw < -20)
        print("clamp active on %s of %d rows per action at s" % (out.sum(0).tolist(), raw.shape[0]))
        for a in (8, 9):   # registers 4 and 5 of lane half 0, log_std in 12 and 13: both sides of `inside` in one batch
            if not (out[:, a].any() and (~out[:, a]).any()):
                problems.append(("s", "action %d: rows with the clamp active and rows inside it" % a, int(out[:, a].sum())))
    return problems


def _case(batch, kind, critics=True, actor=True, mixed=False, clamped=False):
    """CassieSac3dCriticGrad (both blocks) and CassieSac3dActorGrad on one batch against float64 and float32 autograd, per parameter block."""
    import torch
    nets, nets64, pool, row_noise, dropped, la, k = E._sac(D, A, kind)
    assert k.is3d and (k.ENTRY["SacCriticGrad"], k.ENTRY["SacActorGrad"]) == ("CassieSac3dCriticGrad", "CassieSac3dActorGrad") and (k.np_pi, k.np_q) == (NPI, NQ)
    print("margins (%s): %.2f %% of the candidate rows dropped, pool of %d rows" % (kind, 100 * dropped, pool.size))
    assert dropped <= 0.03
    idx, eps_s, eps_s2, data, d64, heads, per = _draw(kind, batch)
    problems = _conditions(heads, mixed)
    alpha = la.exp()
    crit64, (gpi64, lp64, qm64) = E._sac_ref(nets64, d64, eps_s.double(), eps_s2.double(), alpha.double())
    crit32, (gpi32, lp32, qm32) = E._sac_ref(nets, data, eps_s, eps_s2, alpha)
    tag = "%s batch %d" % (kind, batch)
    if critics:
        k._rows("critic", batch, 2, -1, NQ + 2).fill_(float("nan"))
        part = k.critic_grad(pool, idx, eps_s2, GAMMA).clone()
        assert part.shape == (2, E._rows_ok(k, part, batch), NQ + 2) and torch.isfinite(part).all()
        for i in range(2):
            name = "%s critic %d" % (tag, i + 1)
            _check_blocks(name, part[i], batch, crit64[i][0], crit32[i][0], False)
            tot = part[i].double().sum(0) / batch
            E._check(name + " loss", tot[NQ], crit64[i][1], crit32[i][1], 1e-5)
            _check_stat(name + " mean Q", tot[NQ + 1], crit64[i][2], crit32[i][2], per["q%d" % (i + 1)], problems)
        assert torch.equal(part, k.critic_grad(pool, idx, eps_s2, GAMMA))
    if actor:
        k._rows("actor", batch, -1, NPI + 2).fill_(float("nan"))
        part = k.actor_grad(pool, idx, eps_s).clone()
        assert part.shape == (E._rows_ok(k, part, batch), NPI + 2) and torch.isfinite(part).all()
        _check_blocks(tag + " actor", part, batch, gpi64, gpi32, True, zero=LS_BLOCKS if clamped else ())
        tot = part.double().sum(0) / batch
        _check_stat(tag + " mean log pi", tot[NPI], lp64, lp32, per["lp"], problems)
        _check_stat(tag + " mean min Q", tot[NPI + 1], qm64, qm32, per["qm"], problems)
        assert torch.equal(part, k.actor_grad(pool, idx, eps_s))
    assert not problems, problems   # conditions on the data, not on the kernels: another seed (SEED_BUMP), never a wider condition
    return heads, nets, data, eps_s


# ------------------------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("batch", SMALL)
def test_gradients_at_small_batches(batch):
    """1. Batches of less than a workgroup's four tiles (idle wavefronts write a row of zeros; a tile of mostly invalid lanes; the transposed
    operands' own guard on both lane halves), of exactly one and two partial rows, and the grid-stride loop with a ragged last tile: every block of
    both critics and of the actor, so that the second column block of [gW1 | gb1] (NB1 = 2, Tile::xt once per block), k-step 22 with observation 44
    alone (KS1 = 23, NQ1 = 6), the action quad of slots 4 and 5 (NS = 6, NQA = 2) and the rows 8, 9 of both heads (HREG = 8, NQH = 4) are each
    held to their own size."""
    _case(batch, "narrow")


@pytest.mark.parametrize("batch", [130, 1000, 4099])
def test_gradients_with_the_clamp_active_on_some_components(batch):
    """2. The wide log_std head (weights +-4, bias -9): components above 2, below -20 and between in one batch, at s and at s', |u| up to about 30,
    and for the actions 8 and 9 -- registers 4 and 5 of lane half 0, whose log_std sits in 12 and 13 and whose lane-half-1 partners are the dead
    rows 12 and 13 -- rows on both sides of `inside`.  The log_std rows of W3 / b3 are blocks of their own."""
    _case(batch, "wide", mixed=True)


@pytest.mark.parametrize("kind", ["high", "low"])
def test_gradients_with_every_component_clamped(kind):
    """3. log_std bias +5 / -25: the gradient on the log_std rows of W3 and b3 is exactly 0 in every partial row, as in both references (the image
    rows 16 + a of the output tile take no cotangent through K_HEADT); every other block meets its bound."""
    (raw, _, _, _), _, _, _ = _case(1000, kind, clamped=True)
    assert (raw > 2).all() if kind == "high" else (raw < -20).all()


def test_gradients_with_saturated_actions():
    """4. The mean head's bias at +12 (even actions) and -12 (odd ones): float32 tanh and tanh_fast give exactly +-1, 1 - a^2 is exactly 0 in all
    six slots, log pi has its softplus form left; everything stays finite and every block meets its bound."""
    import torch
    (_, u, _, _), nets, data, eps_s = _case(1000, "saturated")
    with torch.no_grad():
        at = nets[0].sample(data[0], eps_s)[0]
    far = u.abs() > 9.1
    print("saturated: min |u| %.3g; |u| > 9.1 on %.2f %% of the components; float32 actions exactly +-1 on %.2f %%" %
          (u.abs().min().item(), 100 * far.double().mean().item(), 100 * (at.abs() == 1).double().mean().item()))
    assert far.double().mean().item() >= 0.99 and u.abs().min().item() > 6.0
    assert (at[far].abs() == 1).all() and torch.equal(at.sign(), u.sign().float())


def test_actor_gradient_with_tied_critics():
    """5. qf2 is a copy of qf1: every row takes actor_grad_kernel's `qa <= qb` branch on equal values, and dQ/da of the six slots comes from the
    first critic's K_DA image."""
    import torch
    _, nets, data, eps_s = _case(1000, "tied", critics=False)
    with torch.no_grad():
        at = nets[0].sample(data[0], eps_s)[0]
        assert torch.equal(nets[1](data[0], at), nets[2](data[0], at))


def test_gradient_kernels_clamp_wild_rows():
    """6. test_gpu_offpolicy_edges.test_gradient_kernels_clamp_wild_rows' index through CassieSac3dCriticGrad and CassieSac3dActorGrad: bit for bit the
    rows of the clamped index, for the lane's own sample and for the transposed operand of both column blocks."""
    import torch
    pool, g = E._random_pool(D, A)
    cap = pool.capacity
    idx = torch.tensor([-7, 0, 3, cap - 1, cap, cap + 1000, 2 ** 40, 17, 17], dtype=torch.int64, device="cuda")
    good = idx.clamp(0, cap - 1)
    k = E._sac(D, A)[-1]
    eps = torch.randn(idx.numel(), A, device="cuda", generator=g)
    calls = {"CassieSac3dCriticGrad": (lambda i: k.critic_grad(pool, i, eps, GAMMA), ("critic", idx.numel(), 2, -1, NQ + 2)),
             "CassieSac3dActorGrad": (lambda i: k.actor_grad(pool, i, eps), ("actor", idx.numel(), -1, NPI + 2))}
    for name, (fn, rows) in calls.items():
        k._rows(*rows).fill_(float("nan"))
        a = fn(idx).clone()
        k._rows(*rows).fill_(float("nan"))
        b = fn(good).clone()
        assert torch.isfinite(a).all() and a.abs().max().item() > 0, name
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------------------------ policy step
@pytest.mark.parametrize("box", ["PD", "synthetic"])
@pytest.mark.parametrize("n", [33, 1000])
def test_policy_step_with_the_clamp_active(n, box):
    """7. CassieSac3dPolicyStep with the wide log_std head: the clamp of policy_step on both sides in all six slots, actions of exactly +-1 and never
    beyond, the environment's actions in their box -- ten distinct bound pairs in the synthetic one, so that a permuted slot cannot pass."""
    import torch
    from cassierl_amd import sac as S
    from cassierl_amd import trpo as T
    pol, qf1, qf2, _, _ = TS._nets(D, A, 7, **E.WIDE)
    pol64 = copy.deepcopy(pol).double()
    low, high = C._boxes()[box]
    assert box == "PD" or (len(set(low.tolist())) == A and len(set(high.tolist())) == A)
    amap = T.NormalizedActions(low, high, "cuda")
    algo = S.SAC(None, None, pol, qf1, qf2, n, D, amap, replay_pool_size=3 * n)
    fused = algo._fused_step(torch.device("cuda:0"))
    assert fused is not None and algo.STEP_ENTRY[D] == "CassieSac3dPolicyStep"
    step, pool = fused[0], algo.pool
    lo, hi = torch.as_tensor(low, device="cuda"), torch.as_tensor(high, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(n)
    exact = above = below = 0
    for top in (n, 2 * n, 0):   # the middle of the ring, an append that ends exactly at capacity, the next one at 0
        for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs):
            t.copy_(torch.randn(t.shape, device="cuda", generator=g))
        before = [t.clone() for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs)]
        obs = torch.randn(n, D, dtype=torch.float64, device="cuda", generator=g)
        noise = torch.randn(n, A, device="cuda", generator=g)
        with torch.no_grad():
            a32 = algo._explore(obs.float(), noise)
            a64 = pol64.sample(obs.float().double(), noise.double())[0]   # the statement's input is the float32 observation
        raw, _ = E._head(pol64, obs.float().double(), noise.double())
        step(obs, noise, top)
        act = pool.act[top:top + n]
        assert torch.equal(pool.obs[top:top + n], obs.float())
        E._check("policy step n %d box %s top %d, actions" % (n, box, top), act, a64, a32, 5e-6, plus=1.0)   # 5e-6 (1 + max|a_64|)
        assert act.min().item() >= -1.0 and act.max().item() <= 1.0
        assert (algo._env_actions - amap(act)).abs().max().item() < 1e-12
        assert (algo._env_actions >= lo).all() and (algo._env_actions <= hi).all()
        rest = torch.ones(pool.capacity, dtype=torch.bool, device="cuda")
        rest[top:top + n] = False
        for now, was in zip((pool.obs, pool.act), before[:2]):
            assert torch.equal(now[rest], was[rest])
        for now, was in zip((pool.rew, pool.term, pool.nobs), before[2:]):
            assert torch.equal(now, was)
        exact += int((act.abs() == 1).sum().item()); above += int((raw > 2).sum().item()); below += int((raw < -20).sum().item())
    print("policy step n %d box %s: over the three appends %d actions exactly +-1, %d log_std above 2, %d below -20, of %d" % (n, box, exact, above, below, 3 * n * A))
    assert exact > 0 and above > 0 and below > 0
