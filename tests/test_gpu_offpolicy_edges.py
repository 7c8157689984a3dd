"""The DDPG and SAC update kernels (csrc/tu_ddpg.hip, tu_sac.hip, mlp32_tiles.h) where training runs them and tests/test_gpu_ddpg.py and
tests/test_gpu_sac.py do not look: batches of a tile or less, shape (17, 7), log_std outside the clamp's bounds, saturated actions, pool rows outside
the pool, tied critics.  -m gpu only.

The reference of every comparison is FLOAT64 torch autograd of the modules' own statements (cassierl_amd/ddpg.py, sac.py) on networks cast up and
data cast up.  Bounds: a gradient max|g_kernel - g_64| < 2e-4 max|g_64|, a statistic column 1e-5 relative, an action 5e-6 (1 + max|a_64|).  Where a
case misses its bound the project's other rule decides (test_gpu_sac.test_sac_gradients_match_autograd, test_gpu_ppo's whole update): the kernel's
error against float64 may be at most 4 times that of torch's float32 evaluation of the same statement on the same inputs (two float32 evaluations
that differ in summation order).  Every line printed says which of the two held ("bound" or "4x").  Every gradient launch is made twice and must
repeat bit for bit.

Networks, pools and kernel objects are built once per shape and kind (lru_cache) and are never written to."""
import copy
import functools

import numpy as np
import pytest

import test_gpu_ddpg as TD
import test_gpu_sac as TS

pytestmark = pytest.mark.gpu

GAMMA = 0.99
SMALL = [1, 4, 31, 32, 33, 127, 129, 256]   # per-rank shares of the default batches; a short, a full, a full + 1 tile; one / two partial rows; SAC's default
CASES_A = [(b, D, A) for D, A in ((26, 6), (17, 7)) for b in SMALL] + [(4099, 17, 7)]   # the last: grid-stride loop, ragged last tile


# ------------------------------------------------------------------------------------------------------------------ helpers
def _flat_grad(loss, net):
    import torch
    return torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(net.parameters()))]).double()


def _check(name, got, ref64, ref32, rel, plus=0.0):
    """got (kernel) and ref32 (torch float32) against ref64: the fixed bound rel * (plus + max|ref64|), else the 4x rule.  Returns the errors and the rule."""
    import torch
    got, ref64, ref32 = (torch.as_tensor(x).double().reshape(-1) for x in (got, ref64, ref32))
    assert torch.isfinite(got).all() and torch.isfinite(ref64).all(), name
    err_k, err_t, scale = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item(), plus + ref64.abs().max().item()
    rule = "bound" if err_k < rel * scale else "4x"
    print("%s: against float64 kernel %.3g, torch float32 %.3g, of max %.3g (%s, bound %.3g)" % (name, err_k, err_t, scale, rule, rel * scale))
    assert err_k < rel * scale or err_k <= 4 * err_t, (name, err_k, err_t, scale)
    return err_k, err_t, rule


def _indices(pool, batch, seed=5):
    """With replacement; positions 0 and 1 hold the same row."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = torch.randint(0, pool.size, (batch,), device="cuda", generator=g)
    if batch >= 2:
        idx[1] = idx[0]
        assert idx.unique().numel() < batch
    return idx, g


def _rows_ok(k, part, batch):
    rows = k.L.CassieDdpgPartialRows(batch)
    assert part.shape[-2] == rows == min((batch + 127) // 128, 256)   # one row per workgroup of four tiles of 32
    return rows


# ------------------------------------------------------------------------------------------------------------------ DDPG
@functools.lru_cache(maxsize=None)
def _ddpg(D, A):
    from cassierl_amd import ddpg as G
    nets = TD._nets(D, A, 3)
    pool, dropped = TD._pool_with_margin(nets[0], nets[1], D, A)
    return nets, [copy.deepcopy(m).double() for m in nets], pool, dropped, G.DdpgKernels(*nets)


def _ddpg_ref(nets, data):
    """ddpg_update_torch_'s two losses in the dtype of nets and data: (critic gradient, loss, mean Q), (actor gradient, mean Q(s, mu(s)))."""
    import torch
    pol, qf, tpol, tqf = nets
    s, a, r, term, s2 = data
    with torch.no_grad():
        y = r + (1.0 - term) * GAMMA * tqf(s2, tpol(s2))
    q = qf(s, a)
    loss = ((q - y) ** 2).mean()
    gq = _flat_grad(loss, qf)
    qa = qf(s, pol(s))
    gpi = _flat_grad(-qa.mean(), pol)
    return (gq, loss.detach().double(), q.detach().double().mean()), (gpi, qa.detach().double().mean())


@pytest.mark.parametrize("batch,obs_dim,act_dim", CASES_A)
def test_ddpg_gradients_at_small_batches(batch, obs_dim, act_dim):
    """A. CassieDdpgCriticGrad and CassieDdpgActorGrad on batches of less than a workgroup's four tiles (idle wavefronts write a row of zeros that
    reduce_rows adds; a tile of mostly invalid lanes; the transposed operands' own guard) and on shape (17, 7)."""
    import torch
    nets, nets64, pool, dropped, k = _ddpg(obs_dim, act_dim)
    print("ReLU margin: %.2f %% of the candidate rows dropped" % (100 * dropped))
    assert dropped <= 0.03
    idx, _ = _indices(pool, batch)
    data = pool.sample(idx)
    (gq64, loss64, q64), (gpi64, qa64) = _ddpg_ref(nets64, [t.double() for t in data])
    (gq32, loss32, q32), (gpi32, qa32) = _ddpg_ref(nets, data)
    part = k.critic_grad(pool, idx, GAMMA).clone()
    NP = gq64.numel()
    assert part.shape == (_rows_ok(k, part, batch), NP + 2)
    tot = part.double().sum(0) / batch
    _check("critic gradient", tot[:NP], gq64, gq32, 2e-4)
    _check("critic loss", tot[NP], loss64, loss32, 1e-5)
    _check("mean Q", tot[NP + 1], q64, q32, 1e-5)
    assert torch.equal(part, k.critic_grad(pool, idx, GAMMA))
    part = k.actor_grad(pool, idx).clone()
    NP = gpi64.numel()
    assert part.shape == (_rows_ok(k, part, batch), NP + 1)
    tot = part.double().sum(0) / batch
    _check("actor gradient", tot[:NP], gpi64, gpi32, 2e-4)
    _check("mean Q(s, mu(s))", tot[NP], qa64, qa32, 1e-5)
    assert torch.equal(part, k.actor_grad(pool, idx))


# ------------------------------------------------------------------------------------------------------------------ SAC
WIDE = dict(ls_width=4.0, ls_bias=-9.0)   # a log_std head that crosses both bounds of the clamp and saturates tanh on a few per cent of the components
KINDS = {"narrow": ({}, True), "wide": (WIDE, False), "high": (dict(ls_bias=5.0), False), "low": (dict(ls_bias=-25.0), False), "tied": ({}, True),
         "saturated": (None, True)}


@functools.lru_cache(maxsize=None)
def _sac(D, A, kind="narrow"):
    """(nets, nets in float64, pool, the pool rows' noise, share of candidates dropped, log_alpha, kernels) of one shape and kind of actor."""
    from cassierl_amd import sac as S
    kw, inside = KINDS[kind]
    if kind == "saturated":
        kw = dict(mean_bias=[12.0 if a % 2 == 0 else -12.0 for a in range(A)])
    nets = TS._nets(D, A, 3, **kw)
    if kind == "tied":   # the second critic and its target are the first: every row is a tie
        nets[2], nets[4] = copy.deepcopy(nets[1]), copy.deepcopy(nets[3])
    pool, row_noise, dropped = TS._pool_with_margin(nets[0], nets[1], nets[2], D, A, inside=inside, untied=kind != "tied")
    la = TS._log_alpha()
    return nets, [copy.deepcopy(m).double() for m in nets], pool, row_noise, dropped, la, S.SacKernels(*nets, la)


def _sac_ref(nets, data, eps_s, eps_s2, alpha):
    """sac_update_torch_'s losses in the dtype of the arguments: [(critic k's gradient, loss, mean Q)] and (actor gradient, mean log pi, mean min Q)."""
    import torch
    pol, qf1, qf2, tq1, tq2 = nets
    s, a, r, term, s2 = data
    with torch.no_grad():
        a2, lp2 = pol.sample(s2, eps_s2)
        y = r + (1.0 - term) * GAMMA * (torch.min(tq1(s2, a2), tq2(s2, a2)) - alpha * lp2)
    critics = []
    for qf in (qf1, qf2):
        q = qf(s, a)
        loss = ((q - y) ** 2).mean()
        critics.append((_flat_grad(loss, qf), loss.detach().double(), q.detach().double().mean()))
    at, lp = pol.sample(s, eps_s)
    qm = torch.min(qf1(s, at), qf2(s, at))
    gpi = _flat_grad((alpha * lp - qm).mean(), pol)
    return critics, (gpi, lp.detach().double().mean(), qm.detach().double().mean())


def _head(pol64, s, eps):
    """float64: the raw log_std head and u = mean + exp(clamp(log_std)) eps."""
    import torch
    with torch.no_grad():
        out = pol64.l3(torch.relu(pol64.l2(torch.relu(pol64.l1(s)))))
        raw = out[:, pol64.act_dim:]
        return raw, out[:, :pol64.act_dim] + raw.clamp(-20.0, 2.0).exp() * eps


def _ls_part(D, A):
    """Positions of the log_std rows of W3 and of b3[A:] in the actor's row [W1 | b1 | W2 | b2 | W3 | b3]."""
    import torch
    w3 = 32 * D + 32 + 32 * 32 + 32
    b3 = w3 + 2 * A * 32
    return torch.cat([torch.arange(w3 + A * 32, b3), torch.arange(b3 + A, b3 + 2 * A)]).cuda()


def _sac_case(batch, D, A, kind, critics=True, actor=True, mixed=False, clamped=False):
    """CassieSacCriticGrad (both blocks) and CassieSacActorGrad on one batch against float64 and float32 autograd; returns what the callers look at."""
    import torch
    nets, nets64, pool, row_noise, dropped, la, k = _sac(D, A, kind)
    print("margins (%s): %.2f %% of the candidate rows dropped" % (kind, 100 * dropped))
    assert dropped <= 0.03
    idx, g = _indices(pool, batch)
    eps_s = row_noise[idx].contiguous()   # the noise the row met the margins with
    eps_s2 = torch.randn(batch, A, device="cuda", generator=g)
    data = pool.sample(idx)
    alpha = la.exp()
    crit64, (gpi64, lp64, qm64) = _sac_ref(nets64, [t.double() for t in data], eps_s.double(), eps_s2.double(), alpha.double())
    crit32, (gpi32, lp32, qm32) = _sac_ref(nets, data, eps_s, eps_s2, alpha)
    raw, u = _head(nets64[0], data[0].double(), eps_s.double())
    raw2, u2 = _head(nets64[0], data[4].double(), eps_s2.double())
    share = lambda m: m.double().mean().item()
    print("log_std above 2 / below -20: %.2f %% / %.2f %% at s, %.2f %% / %.2f %% at s'; |u| > 9: %.2f %% / %.2f %%; max |u| %.3g; min |u| %.3g" %
          (100 * share(raw > 2), 100 * share(raw < -20), 100 * share(raw2 > 2), 100 * share(raw2 < -20), 100 * share(u.abs() > 9), 100 * share(u2.abs() > 9),
           u.abs().max().item(), u.abs().min().item()))
    if mixed:   # the conditions that keep the mixed-clamp test honest
        for r_, u_ in ((raw, u), (raw2, u2)):
            assert share(r_ > 2) >= 0.01 and share(r_ < -20) >= 0.01 and share(u_.abs() > 9) >= 0.005
    if critics:
        part = k.critic_grad(pool, idx, eps_s2, GAMMA).clone()
        NP = crit64[0][0].numel()
        assert part.shape == (2, _rows_ok(k, part, batch), NP + 2)
        for i in range(2):
            tot = part[i].double().sum(0) / batch
            _check("critic %d gradient" % (i + 1), tot[:NP], crit64[i][0], crit32[i][0], 2e-4)
            _check("critic %d loss" % (i + 1), tot[NP], crit64[i][1], crit32[i][1], 1e-5)
            _check("critic %d mean Q" % (i + 1), tot[NP + 1], crit64[i][2], crit32[i][2], 1e-5)
        assert torch.equal(part, k.critic_grad(pool, idx, eps_s2, GAMMA))
    if actor:
        part = k.actor_grad(pool, idx, eps_s).clone()
        NP = gpi64.numel()
        assert part.shape == (_rows_ok(k, part, batch), NP + 2)
        tot = part.double().sum(0) / batch
        ls = _ls_part(D, A)
        if clamped:   # no gradient reaches the log_std head: exactly, in the kernel and in the reference, and the rest meets the bound
            rest = torch.ones(NP, dtype=torch.bool, device="cuda")
            rest[ls] = False
            assert (gpi64[ls] == 0).all() and (gpi32[ls] == 0).all()
            assert (part[:, ls] == 0).all()
            _check("actor gradient without the log_std head", tot[:NP][rest], gpi64[rest], gpi32[rest], 2e-4)
        else:
            _check("actor gradient", tot[:NP], gpi64, gpi32, 2e-4)
        if mixed:
            _check("actor gradient, log_std rows of W3 and b3", tot[:NP][ls], gpi64[ls], gpi32[ls], 2e-4)
        _check("mean log pi", tot[NP], lp64, lp32, 1e-5)
        _check("mean min Q", tot[NP + 1], qm64, qm32, 1e-5)
        assert torch.equal(part, k.actor_grad(pool, idx, eps_s))
    return raw, u, nets, data, eps_s


@pytest.mark.parametrize("batch,obs_dim,act_dim", CASES_A)
def test_sac_gradients_at_small_batches(batch, obs_dim, act_dim):
    """A. CassieSacCriticGrad (both blocks) and CassieSacActorGrad on the batches and shapes of test_ddpg_gradients_at_small_batches."""
    _sac_case(batch, obs_dim, act_dim, "narrow")


@pytest.mark.parametrize("batch", [1000, 4099])
@pytest.mark.parametrize("obs_dim,act_dim", [(26, 6), (26, 7), (17, 6)])
def test_sac_gradients_with_the_clamp_active_on_some_components(obs_dim, act_dim, batch):
    """B. A wide log_std head (weights +-4, bias -9): in one batch, components above 2, below -20 and between, and |u| up to about 30.  squash()'s
    `inside` flag and the branch of actor_grad_kernel that drops the log_std cotangent take both sides; tanh_fast returns exactly +-1 on some
    components, where 1 - a^2 is exactly 0 and log pi has only its softplus form left.  The log_std rows of the gradient are checked on their own
    too: against the whole vector's maximum an error in them alone could hide."""
    _sac_case(batch, obs_dim, act_dim, "wide", mixed=True)


@pytest.mark.parametrize("kind", ["high", "low"])
@pytest.mark.parametrize("obs_dim,act_dim", [(26, 6), (17, 7)])
def test_sac_gradients_with_every_component_clamped(obs_dim, act_dim, kind):
    """B. log_std bias +5 (every component above 2) and -25 (every component below -20): the gradient on W3[A:] and b3[A:] is exactly 0 in every
    partial row, as it is in the float64 and the float32 reference; the rest meets the bound."""
    raw, _, _, _, _ = _sac_case(1000, obs_dim, act_dim, kind, clamped=True)
    assert (raw > 2).all() if kind == "high" else (raw < -20).all()


@pytest.mark.parametrize("obs_dim,act_dim", [(26, 6), (17, 7)])
def test_sac_gradients_with_saturated_actions(obs_dim, act_dim):
    """B. The mean head's bias at +12 (even actions) and -12 (odd ones), the usual narrow log_std head: |u| > 9.1 on 99 % of the components and more
    (the rest of the head moves the mean by a few units at the most), past the point where float32 tanh and tanh_fast round to exactly +-1.
    log pi, both statistic columns and the actor's gradient stay finite and meet their bounds; the critics' y takes alpha log pi of such samples."""
    import torch
    _, u, nets, data, eps_s = _sac_case(1000, obs_dim, act_dim, "saturated")
    with torch.no_grad():
        at = nets[0].sample(data[0], eps_s)[0]
    far = u.abs() > 9.1
    print("saturated: min |u| %.3g; |u| > 9.1 on %.2f %% of the components; float32 actions exactly +-1 on %.2f %%" %
          (u.abs().min().item(), 100 * far.double().mean().item(), 100 * (at.abs() == 1).double().mean().item()))
    assert far.double().mean().item() >= 0.99 and u.abs().min().item() > 6.0
    assert (at[far].abs() == 1).all() and torch.equal(at.sign(), u.sign().float())


def test_sac_actor_gradient_with_tied_critics():
    """D. qf2 is a copy of qf1: every row takes actor_grad_kernel's `qa <= qb` branch on equal values.  float64 autograd of torch.min splits the
    cotangent evenly between two identical critics, which is the gradient through either one."""
    import torch
    _, _, nets, data, eps_s = _sac_case(1000, 26, 6, "tied", critics=False)
    with torch.no_grad():
        at = nets[0].sample(data[0], eps_s)[0]
        assert torch.equal(nets[1](data[0], at), nets[2](data[0], at))


@pytest.mark.parametrize("n", [1000, 33])
@pytest.mark.parametrize("control_mode,adim", [("PD", 6), ("OSC", 7)])
def test_sac_policy_step_with_the_clamp_active(control_mode, adim, n):
    """B. CassieSacPolicyStep with the wide log_std head, as test_gpu_sac.test_sac_policy_step_matches_the_torch_statement: the clamp of
    policy_step_kernel on both sides, actions of exactly +-1 (and never beyond), the environment's actions inside their box."""
    import torch
    from cassierl_amd import sac as S
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env import action_space
    pol, qf1, qf2, _, _ = TS._nets(26, adim, 7, **WIDE)
    pol64 = copy.deepcopy(pol).double()
    box = action_space(control_mode)
    amap = T.NormalizedActions(box.low, box.high, "cuda")
    algo = S.SAC(None, None, pol, qf1, qf2, n, 26, amap, replay_pool_size=3 * n)
    fused = algo._fused_step(torch.device("cuda:0"))
    assert fused is not None
    step = fused[0]
    pool = algo.pool
    lo, hi = torch.as_tensor(box.low, device="cuda"), torch.as_tensor(box.high, device="cuda")
    exact = above = below = 0
    for top in (n, 2 * n, 0):
        for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs):
            t.copy_(torch.randn_like(t))
        before = [t.clone() for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs)]
        obs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
        noise = torch.randn(n, adim, device="cuda")
        with torch.no_grad():
            a32 = algo._explore(obs.float(), noise)
            a64 = pol64.sample(obs.float().double(), noise.double())[0]   # the statement's input is the float32 observation
        raw, _ = _head(pol64, obs.float().double(), noise.double())
        step(obs, noise, top)
        act = pool.act[top:top + n]
        assert torch.equal(pool.obs[top:top + n], obs.float())
        _check("policy step n %d A %d top %d, actions" % (n, adim, top), act, a64, a32, 5e-6, plus=1.0)   # 5e-6 (1 + max|a_64|)
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
    print("policy step n %d A %d: over the three appends %d actions exactly +-1, %d log_std above 2, %d below -20, of %d" % (n, adim, exact, above, below, 3 * n * adim))
    assert exact > 0 and above > 0 and below > 0


# ------------------------------------------------------------------------------------------------------------------ wild rows
def _random_pool(D, A, cap=500, seed=13):
    import torch
    from cassierl_amd import ddpg as G
    g = torch.Generator(device="cuda").manual_seed(seed)
    pool = G.ReplayPool(cap, 1, D, A, "cuda")
    pool.obs.copy_(0.7 * torch.randn(cap, D, device="cuda", generator=g)); pool.act.copy_(torch.rand(cap, A, device="cuda", generator=g) * 2 - 1)
    pool.rew.copy_(torch.randn(cap, device="cuda", generator=g) * 0.1); pool.term.copy_((torch.rand(cap, device="cuda", generator=g) < 0.2).float())
    pool.nobs.copy_(0.7 * torch.randn(cap, D, device="cuda", generator=g))
    pool.size = cap
    return pool, g


@pytest.mark.parametrize("obs_dim,act_dim", [(26, 6), (17, 7)])
def test_gradient_kernels_clamp_wild_rows(obs_dim, act_dim):
    """C. Row numbers outside [0, capacity) are clamped (test_gpu_ppo.test_clip_grad_clamps_a_wild_index says so of CassieDdpg*Grad): all four
    gradient entry points return, bit for bit, the rows of the clamped index -- for the lane's own sample and for the transposed operand."""
    import torch
    pool, g = _random_pool(obs_dim, act_dim)
    cap = pool.capacity
    idx = torch.tensor([-7, 0, 3, cap - 1, cap, cap + 1000, 2 ** 40, 17, 17], dtype=torch.int64, device="cuda")
    good = idx.clamp(0, cap - 1)
    kd, ks = _ddpg(obs_dim, act_dim)[-1], _sac(obs_dim, act_dim)[-1]
    eps = torch.randn(idx.numel(), act_dim, device="cuda", generator=g)
    calls = {"CassieDdpgCriticGrad": lambda i: kd.critic_grad(pool, i, GAMMA), "CassieDdpgActorGrad": lambda i: kd.actor_grad(pool, i),
             "CassieSacCriticGrad": lambda i: ks.critic_grad(pool, i, eps, GAMMA), "CassieSacActorGrad": lambda i: ks.actor_grad(pool, i, eps)}
    for name, fn in calls.items():
        a = fn(idx).clone()
        b = fn(good).clone()
        assert torch.isfinite(a).all() and a.abs().max().item() > 0, name
        assert torch.equal(a, b), name
