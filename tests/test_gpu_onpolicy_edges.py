"""The on-policy kernels (csrc/tu_trpo.hip, tu_pg.hip, tu_pg_trpo.hip, tu_ppo.hip, tu_trpo_baseline.hip) where VPG, TRPO and PPO run them and
tests/test_gpu_trpo_fused.py, test_gpu_trpo_wide.py, test_gpu_vpg.py and test_gpu_ppo.py do not look: batches of a tile or less and of full tiles
only, shape (17, 7), saturated and near-zero hidden units, log_std far from 0, minibatches with every / no sample clipped, the CG vector kernels
on their own, the baseline kernels below one MFMA step and on clipped features.  -m gpu only; the counterpart of test_gpu_offpolicy_edges.py.

The reference of every comparison is FLOAT64 torch (AnalyticFisher, autograd, the statements of trpo.py and ppo.py) on networks cast up and data
cast up.  Bounds, all of them this project's: a gradient or product max|got - ref64| < 2e-4 max|ref64|; a surrogate loss or mean KL 2e-5 on the
scales of test_fused_surrogate_matches_the_torch_line_search_evaluation; an action or mean 5e-6 (1 + max|ref64|); the float64 sums of a
minibatch as test_gpu_ppo compares them.  Where a case misses its bound the project's other rule decides: the kernel's error against float64 may
be at most 4 times that of torch's float32 evaluation of the same statement on the same inputs.  Every line printed says which of the two held
("bound" or "4x").  Every launch is made twice and must repeat bit for bit.

Every input is drawn on the CPU (a torch.Generator of its own per bundle) and moved to the device: the input-dependent conditions asserted below
(saturation shares, clipped-feature share, |ll| < 20, no ratio within 1e-4 of a clip boundary, every sample clipped with a margin, a clipped
share inside (0, 1)) depend on the float64 reference alone and hold wherever the file runs.  Networks, data and kernel objects are built once per
shape, width and regime (lru_cache) and are never written to."""
import copy
import ctypes as ct
import functools
import math
import types

import pytest

from test_gpu_offpolicy_edges import _check, _flat_grad

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
CLIP = 0.2
SHAPES = [(26, 6), (17, 7)]
WIDTHS = [32, 128]
SMALL = [1, 4, 31, 32, 33, 127, 128, 129, 256]   # a short tile; one full tile (three idle wavefronts); a tile + 1; a width-128 group of 4 tiles, - 1, + 1; two groups
CASES_A = [(n, D, A) for D, A in SHAPES for n in SMALL] + [(4099, 17, 7)]   # the last: grid-stride loop, ragged last tile
NMAX = 4099
NCLIP = 300   # the batch that the minibatches of group A are drawn from
KIND = {32: "trpo_clip", 128: "pg_clip"}
# saturated: every second hidden unit of both layers has its row of W and its bias multiplied by SAT.  One common factor cannot meet both shares
# that the regime asks for: pre-activations N(0, s^2) have P(|z| < 2) >= 0.2 only for s <= 7.9 and P(|z| > 9) >= 0.3 only for s >= 8.7.
SAT = 60.0
LS = [-5.0, 2.0, -5.0, 2.0, -5.0, 2.0, -5.0]       # log_std of the `logstd` regime: precisions from 4e4 to 2e-2
LS_OFF = [-1.0, 0.4, -0.6, 0.3, -0.3, 0.2, -0.8]   # old log_std = LS + LS_OFF.  Positive offsets stay small: with the actions drawn from the old Gaussian
#                                                    a component adds -(e^(2 off) - 1) noise^2 / 2 to ll_new - ll_old, -3.2 noise^2 at off = 1
SEED_BUMP = {}   # (D, A, width, regime) -> added to the bundle's seed where the first seed misses a condition asserted below


# ------------------------------------------------------------------------------------------------------------------ networks and data
def _linears(pol):
    from torch import nn
    return [m for m in pol.mean_net if isinstance(m, nn.Linear)]


def _regime_(pol, regime):
    import torch
    lin = _linears(pol)
    with torch.no_grad():
        for l in lin[:2]:
            if regime == "saturated":
                l.weight[0::2] *= SAT; l.bias[0::2] *= SAT
            elif regime == "tiny":
                l.weight *= 1e-3; l.bias *= 1e-3
        if regime == "logstd":
            pol.log_std.copy_(torch.tensor(LS[:pol.log_std.numel()]))
    return pol


@functools.lru_cache(maxsize=None)
def _bundle(D, A, width, regime="default"):
    """One policy (the default initialisation + N(0, 0.1) jitter, then the regime), its candidates of a line search (`sur`) and of a PPO step
    (`clip`), a batch of NMAX samples whose old statistics are the policy's, a direction v and cotangents w; float32 on DEV, the networks in
    float64 too.  The candidates move the UNSCALED parameters by 0.02 / 0.05 N(0, 1) (logstd: 5e-4, see _ll_ok) before the regime is applied."""
    import torch
    from cassierl_amd import trpo as T
    g = torch.Generator().manual_seed(1000 * D + 10 * A + width + {"default": 0, "saturated": 1, "tiny": 2, "logstd": 3}[regime] * 100000
                                      + SEED_BUMP.get((D, A, width, regime), 0))
    randn = lambda *s: torch.randn(*s, generator=g)
    base = T.GaussianMLPPolicy(D, A, (width, width), init_std=1.0)
    with torch.no_grad():
        for l in _linears(base):   # GaussianMLPPolicy's own initialisation (Xavier-uniform, zero bias), from this generator
            a = math.sqrt(6.0 / (l.in_features + l.out_features))
            l.weight.copy_((torch.rand(l.weight.shape, generator=g) * 2 - 1) * a); l.bias.zero_()
        for p in base.parameters():
            p.add_(0.1 * randn(p.shape))
    delta = [randn(p.shape) for p in base.parameters()]

    def variant(eps):
        pol = copy.deepcopy(base)
        with torch.no_grad():
            for p, d in zip(pol.parameters(), delta):
                p.add_(eps * d)
        return _regime_(pol, regime)

    small = regime == "logstd"
    pols = dict(pol=variant(0.0), sur=variant(5e-4 if small else 0.02), clip=variant(5e-4 if small else 0.05))
    b = types.SimpleNamespace(D=D, A=A, width=width, regime=regime)
    obs, noise = 0.7 * randn(NMAX, D), randn(NMAX, A)
    with torch.no_grad():
        old_mean = pols["pol"].mean_net(obs)
        old_ls = pols["pol"].log_std.detach().clone() + (torch.tensor(LS_OFF[:A]) if small else 0.0)
        act = old_mean + noise * old_ls.exp()
    data = dict(obs=obs, old_mean=old_mean, old_ls=old_ls, act=act, adv=randn(NMAX), w=randn(NMAX, A), v=randn(sum(p.numel() for p in base.parameters())))
    for k, t in data.items():
        setattr(b, k, t.to(DEV).contiguous())
    for k, p in pols.items():
        setattr(b, k, p.to(DEV)); setattr(b, k + "64", copy.deepcopy(p).double().to(DEV))
    i0 = 0
    for n, p in base.named_parameters():
        if n == "log_std":
            b.ls_slot = slice(i0, i0 + p.numel())
        i0 += p.numel()
    return b


def _shares(b, n):
    """float64: per hidden layer the shares of pre-activations with |z| > 9 and with |z| < 2 on the first n rows."""
    import torch
    lin = _linears(b.pol64)
    with torch.no_grad():
        z1 = lin[0](b.obs[:n].double())
        z2 = lin[1](torch.tanh(z1))
    return [((z.abs() > 9).double().mean().item(), (z.abs() < 2).double().mean().item(), z.abs().max().item()) for z in (z1, z2)]


# ------------------------------------------------------------------------------------------------------------------ the four kernels
def _fisher(width, pol, obs):
    from cassierl_amd import trpo as T
    return (T.FusedFisher if width == 32 else T.PgFisher)(pol, obs)


@functools.lru_cache(maxsize=None)
def _fisher_of(D, A, width, regime, n):
    b = _bundle(D, A, width, regime)
    return _fisher(width, b.pol, b.obs[:n])


def _pg_vjp(pol, obs, w):
    from cassierl_amd import vpg as V
    pk = V.PolicyGradKernels(pol, obs)
    assert pk.kind == "pg_vjp"
    return pk._pg_vjp(w)


def _partial_ok(F, n, width):
    """The row count is the library's and the launch's; a width-32 wavefront r owns the tiles r, r + rows, ..: rows past the last tile are zeros.
    (A width-128 row belongs to a workgroup of four tiles, and the grid has no workgroup without one.)"""
    tiles = (n + 31) // 32
    rows = F.partial.shape[0]
    assert rows == F._partial_rows(n) == (4 if width == 32 else 1) * min((tiles + 3) // 4, 512 if width == 32 else 256)
    if width == 32:
        assert (F.partial[tiles:] == 0).all()
        assert rows - tiles == (-tiles) % 4 or tiles > rows
    return rows


def _vjp_ref(pol, obs, w):
    import torch
    g = torch.autograd.grad((pol.mean_net(obs) * w).sum(), list(pol.parameters()), allow_unused=True)
    return torch.cat([torch.zeros_like(p).reshape(-1) if x is None else x.reshape(-1) for x, p in zip(g, pol.parameters())]).double()


def _fisher_and_vjp(b, n, tag, ls_block=False):
    import torch
    from cassierl_amd import trpo as T
    obs = b.obs[:n]
    F = _fisher_of(b.D, b.A, b.width, b.regime, n)
    ref64, ref32 = T.AnalyticFisher(b.pol64, obs.double())(b.v.double()), T.AnalyticFisher(b.pol, obs)(b.v)
    got = F(b.v).clone()
    out = [_check("%s Fisher product" % tag, got, ref64, ref32, 2e-4)]
    if ls_block:
        out.append(_check("%s Fisher product, log_std block" % tag, got[b.ls_slot], ref64[b.ls_slot], ref32[b.ls_slot], 2e-4))
    _partial_ok(F, n, b.width)
    assert torch.equal(got, F(b.v))
    w = (b.w / n)[:n]   # like obs: the first rows of a longer buffer, so that a lane or a row past n reads real numbers, not zeros
    vjp = F.vjp if b.width == 32 else (lambda w_: _pg_vjp(b.pol, obs, w_))
    got = vjp(w).clone()
    out.append(_check("%s J' w" % tag, got, _vjp_ref(b.pol64, obs.double(), w.double()), _vjp_ref(b.pol, obs, w), 2e-4))
    assert (got[b.ls_slot] == 0).all()
    if b.width == 32:
        _partial_ok(F, n, b.width)
    assert torch.equal(got, vjp(w))
    return out


def _sur_ref(pol, b, rows, dt):
    """The torch expressions of TRPO.optimize's surrogate() in dtype dt on the rows given: (loss, mean KL, ll_new - ll_old, ratio adv)."""
    import torch
    with torch.no_grad():
        obs, act, adv, om = (x[rows].to(dt) for x in (b.obs, b.act, b.adv, b.old_mean))
        ols, mean = b.old_ls.to(dt), pol.mean_net(obs)
        ll = pol.log_likelihood(act, mean, pol.log_std) - pol.log_likelihood(act, om, ols)
        lr = ll.exp()
        return -(lr * adv).mean().double(), pol.kl(om, ols, mean, pol.log_std).mean().double(), ll.double(), (lr * adv).double()


def _surrogate(b, n, tag):
    import torch
    F = _fisher_of(b.D, b.A, b.width, b.regime, n)
    rows = slice(0, n)
    l64, k64, ll, ra = _sur_ref(b.sur64, b, rows, torch.float64)
    l32, k32, _, _ = _sur_ref(b.sur, b, rows, torch.float32)
    call = lambda: torch.stack(F.surrogate(b.sur, b.act[:n], b.adv[:n], b.old_mean[:n], b.old_ls))
    got = call().clone()
    scale, k = ra.abs().mean().item(), k64.item()
    out = [_check("%s surrogate loss" % tag, got[0], l64, l32, 2e-5, plus=scale - abs(l64.item())),      # bound 2e-5 mean|ratio adv|
           _check("%s mean KL" % tag, got[1], k64, k32, 2e-5, plus=max(k, 1e-3) - k)]                    # bound 2e-5 max(KL, 1e-3)
    assert torch.equal(got, call())
    return out, ll


def _near(ratio, clip):
    return ((ratio - (1.0 + clip)).abs() < 1e-4) | ((ratio - (1.0 - clip)).abs() < 1e-4)


def _ratio64(b, pol64, rows, adv, clip):
    import torch
    from cassierl_amd import ppo as P
    with torch.no_grad():
        _, ratio, clipped = P.surrogate_terms(pol64.mean_net(b.obs[rows].double()), pol64.log_std, b.act[rows].double(), adv[rows].double(),
                                              b.old_mean[rows].double(), b.old_ls.double(), clip)
    return ratio, clipped


def _clip_partial(ck, m):
    return ck._bufs[ck._rows(m)][0]


def _clip_rows_ok(ck, m, width):
    """One row per wavefront (width 32) or per workgroup of four tiles (width 128), as the library reports."""
    assert _clip_partial(ck, m).shape[0] == ck._rows(m) == (4 if width == 32 else 1) * ((((m + 31) // 32) + 3) // 4)


def _clip_grad(b, nb, idx, m, tag, clip=CLIP, ent=0.0, adv=None, loss64=None):
    """ClipGradKernels.grad(idx, m) on the batch of the first nb rows at the candidate `clip` against float64 and float32 autograd of ppo_loss
    (loss64: another float64 loss of (pol64, obs, act, adv, old_mean, old_ls)) and minibatch_stats.  Returns (ck, gradient, stats, checks)."""
    import torch
    from cassierl_amd import ppo as P
    adv = b.adv if adv is None else adv
    obs, act, adv, om = b.obs[:nb], b.act[:nb], adv[:nb].contiguous(), b.old_mean[:nb]
    ck = P.ClipGradKernels(b.clip, P.aligned_flat_params(b.clip), obs, act, adv, om, b.old_ls, clip, ent)
    assert ck.kind == KIND[b.width]
    sel = slice(0, m) if idx is None else idx
    rows = lambda dt: [x[sel].to(dt) for x in (obs, act, adv, om)]
    loss = lambda pol, dt: (P.ppo_loss(pol, *rows(dt), b.old_ls.to(dt), clip, ent) if loss64 is None else loss64(pol, *rows(dt), b.old_ls.to(dt)))
    ref, g32 = _flat_grad(loss(b.clip64, torch.float64), b.clip64), _flat_grad(loss(b.clip, torch.float32), b.clip)
    st64, st32 = P.minibatch_stats(b.clip64, *rows(torch.float64), b.old_ls.double(), clip), P.minibatch_stats(b.clip, *rows(torch.float32), b.old_ls, clip)
    got, st = ck.grad(idx, m=m)
    got, st = got.clone(), st.clone()
    _clip_rows_ok(ck, m, b.width)
    ratio, _ = _ratio64(b, b.clip64, sel, adv, clip)
    sur_scale, kl = (ratio * adv[sel].double()).abs().mean().item(), st64[1].item() / m
    out = [_check("%s gradient" % tag, got, ref, g32, 2e-4)]
    if sur_scale > 0:
        out.append(_check("%s loss" % tag, st[0] / m, st64[0] / m, st32[0] / m, 2e-5, plus=sur_scale - abs(st64[0].item()) / m))
    out.append(_check("%s mean KL" % tag, st[1] / m, st64[1] / m, st32[1] / m, 2e-5, plus=max(kl, 1e-3) - kl))
    print("%s clipped samples: kernel %d, float64 %d of %d" % (tag, st[2].item(), st64[2].item(), m))
    assert st[2].item() == st64[2].item()
    got2, st2 = ck.grad(idx, m=m)
    assert torch.equal(got, got2) and torch.equal(st, st2)
    return ck, got, st, out


def _away_from_the_boundaries(b, n, clip=CLIP):
    """The rows of the first n whose float64 ratio is not within 1e-4 of a clip boundary (those can fall on either side in float32), as an index;
    at most 1 % may be taken out (test_gpu_ppo.test_clip_grad_matches_float64_autograd)."""
    ratio, _ = _ratio64(b, b.clip64, slice(0, n), b.adv, clip)
    keep = (~_near(ratio, clip)).nonzero().squeeze(-1).contiguous()
    print("%d of %d samples within 1e-4 of a clip boundary taken out" % (n - keep.numel(), n))
    assert n - keep.numel() <= 0.01 * n
    return keep


# ------------------------------------------------------------------------------------------------------------------ A. small batches
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n,obs_dim,act_dim", CASES_A)
def test_fisher_vjp_and_surrogate_at_small_batches(n, obs_dim, act_dim, width):
    """A. CassieTrpoFvp / Vjp / Surrogate and CassiePgFvp / Vjp / Surrogate on fewer samples than a tile, on one full tile (three wavefronts write
    a row of zeros), on a width-128 group of fewer than four tiles, on full tiles only, and on shape (17, 7) (three live actions and a dead one in
    the upper lane half, the ones-column at lane 17, an odd last k-step)."""
    b = _bundle(obs_dim, act_dim, width)
    tag = "n %d D %d A %d width %d:" % (n, obs_dim, act_dim, width)
    _fisher_and_vjp(b, n, tag)
    _surrogate(b, n, tag)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mode", ["rows", "repeats"])
@pytest.mark.parametrize("obs_dim,act_dim", SHAPES)
@pytest.mark.parametrize("m", SMALL)
def test_clip_grad_at_small_minibatches(m, obs_dim, act_dim, mode, width):
    """A. CassieTrpoClipGrad / CassiePgClipGrad on minibatches of SMALL rows of a batch of 300: `rows` idx = NULL, `repeats` an index drawn with
    replacement whose positions 0 and 1 hold the same row (entropy bonus 0.01).  No sample can be taken out at these sizes: no float64 ratio of
    the batch lies within 1e-4 of a clip boundary."""
    import torch
    b = _bundle(obs_dim, act_dim, width)
    ratio, clipped = _ratio64(b, b.clip64, slice(0, NCLIP), b.adv, CLIP)
    assert not _near(ratio, CLIP).any()
    idx = None
    if mode == "repeats":
        idx = torch.randint(0, NCLIP, (m,), generator=torch.Generator().manual_seed(5 + m))
        if m >= 2:
            idx[1] = idx[0]
            assert idx.unique().numel() < m
        idx = idx.to(DEV)
    share = clipped[slice(0, m) if idx is None else idx].double().mean().item()
    tag = "m %d D %d A %d width %d %s:" % (m, obs_dim, act_dim, width, mode)
    print("%s clipped share %.3f" % (tag, share))
    if m >= 127:
        assert 0.0 < share < 1.0
    _clip_grad(b, NCLIP, idx, m, tag, ent=0.01 if mode == "repeats" else 0.0)


# ------------------------------------------------------------------------------------------------------------------ B. saturated and near-zero hidden units
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("obs_dim,act_dim", SHAPES)
@pytest.mark.parametrize("n", [33, 129, 1000])
@pytest.mark.parametrize("regime", ["saturated", "tiny"])
def test_kernels_with_saturated_and_near_zero_hidden_units(regime, n, obs_dim, act_dim, width):
    """B. `saturated`: in float64 at least 30 % of each layer's pre-activations have |z| > 9 (tanh_fast's exact ends e = inf and e = 0; 1 - h^2
    exactly 0 in the forward-mode and the reverse pass, the Fisher product's tangent through a dead unit) and at least 20 % have |z| < 2.
    `tiny`: W1, b1, W2, b2 times 1e-3, pre-activations of about 1e-3, where tanh_fast = 1 - 2 / (e + 1) has an absolute error of about 1e-7, a
    relative one of about 1e-4 on the activation."""
    b = _bundle(obs_dim, act_dim, width, regime)
    sh = _shares(b, n)
    tag = "%s n %d D %d A %d width %d:" % (regime, n, obs_dim, act_dim, width)
    print("%s pre-activations |z| > 9 / |z| < 2 / max: layer 1 %.3f / %.3f / %.3g, layer 2 %.3f / %.3f / %.3g" % (tag, *sh[0], *sh[1]))
    for far, close, top in sh:
        if regime == "saturated":
            assert far >= 0.30 and close >= 0.20
        else:
            assert top < 2e-2
    _fisher_and_vjp(b, n, tag)
    _surrogate(b, n, tag)
    keep = _away_from_the_boundaries(b, n)
    _clip_grad(b, n, keep, keep.numel(), tag)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("regime", ["default", "saturated"])
@pytest.mark.parametrize("control_mode,adim", [("PD", 6), ("OSC", 7)])
def test_policy_step_at_small_batches_and_saturated_units(control_mode, adim, regime, width):
    """B. CassieTrpoPolicyStep / CassiePgPolicyStep through TRPO._fused_policy_step on 1, 31, 33, 129 and 1000 environments: means and actions
    against the float64 policy on the float32-rounded observation, the float32 view bit for bit, the environment's actions inside their box and
    equal to NormalizedActions(act), nothing written behind row n (n + 32 rows of a sentinel, views of the first n passed)."""
    import torch
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env import action_space
    b = _bundle(26, adim, width, regime)
    if regime == "saturated":
        sh = _shares(b, 1000)
        assert all(far >= 0.30 and close >= 0.20 for far, close, _ in sh), sh
    box = action_space(control_mode)
    amap = T.NormalizedActions(box.low, box.high, DEV)
    lo, hi = torch.as_tensor(box.low, device=DEV), torch.as_tensor(box.high, device=DEV)
    g = torch.Generator().manual_seed(70 + adim + width)
    for n in (1, 31, 33, 129, 1000):
        obs = torch.randn(n, 26, dtype=torch.float64, generator=g).to(DEV)
        noise = torch.randn(n, adim, generator=g).to(DEV)
        algo = T.TRPO(None, None, b.pol, T.LinearFeatureBaseline(), n, 26, amap)
        SENT = 777.0
        o32, mean, act = (torch.full((n + 32, k), SENT, device=DEV) for k in (26, adim, adim))
        env = torch.full((n + 32, adim), SENT, dtype=torch.float64, device=DEV)
        algo._env_actions = env[:n]
        step = algo._fused_policy_step(torch.device(DEV, 0), torch.float32)
        assert step is not None and algo.policy_step_entry == ("CassieTrpoPolicyStep" if width == 32 else "CassiePgPolicyStep")
        assert algo._env_actions.data_ptr() == env.data_ptr()
        step(obs, noise, o32[:n], mean[:n], act[:n])
        first = [t.clone() for t in (o32, mean, act, env)]
        with torch.no_grad():
            a32, m32, _ = b.pol.get_actions(obs.float(), noise=noise)
            a64, m64, _ = b.pol64.get_actions(obs.float().double(), noise=noise.double())
        tag = "policy step %s n %d A %d width %d:" % (regime, n, adim, width)
        _check("%s mean" % tag, mean[:n], m64, m32, 5e-6, plus=1.0)
        _check("%s action" % tag, act[:n], a64, a32, 5e-6, plus=1.0)
        assert torch.equal(o32[:n], obs.float())
        assert (env[:n] - amap(act[:n])).abs().max().item() < 1e-12
        assert (env[:n] >= lo).all() and (env[:n] <= hi).all()
        for t in (o32, mean, act, env):
            assert (t[n:] == SENT).all()
        step(obs, noise, o32[:n], mean[:n], act[:n])
        assert all(torch.equal(x, y) for x, y in zip(first, (o32, mean, act, env)))


# ------------------------------------------------------------------------------------------------------------------ C. log_std and clip extremes
def _ll_ok(b, n):
    """The accuracy tests of group C are not about overflow: in float64 |ll_new - ll_old| < 20 on every sample, at both candidates."""
    import torch
    for pol in (b.sur64, b.clip64):
        ll = _sur_ref(pol, b, slice(0, n), torch.float64)[2]
        print("log_std regime n %d: max |ll_new - ll_old| %.3g" % (n, ll.abs().max().item()))
        assert ll.abs().max().item() < 20.0


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("obs_dim,act_dim", SHAPES)
@pytest.mark.parametrize("n", [129, 1000])
def test_kernels_with_log_std_far_from_zero(n, obs_dim, act_dim, width):
    """C. log_std alternating -5 and +2 (prec, kden, kvar, pr[v] and expf(log_std) far from 1), the old log_std off by up to 1 per component,
    actions drawn from the OLD Gaussian: the Fisher product with its log_std block, the surrogate, and the clip gradient with g_log_std."""
    b = _bundle(obs_dim, act_dim, width, "logstd")
    tag = "log_std n %d D %d A %d width %d:" % (n, obs_dim, act_dim, width)
    _ll_ok(b, n)
    _fisher_and_vjp(b, n, tag, ls_block=True)
    _surrogate(b, n, tag)
    keep = _away_from_the_boundaries(b, n)
    _, got, _, _ = _clip_grad(b, n, keep, keep.numel(), tag, ent=0.01)
    import torch
    from cassierl_amd import ppo as P
    rows = lambda dt: [x[:n][keep].to(dt) for x in (b.obs, b.act, b.adv, b.old_mean)]
    ref = _flat_grad(P.ppo_loss(b.clip64, *rows(torch.float64), b.old_ls.double(), CLIP, 0.01), b.clip64)
    g32 = _flat_grad(P.ppo_loss(b.clip, *rows(torch.float32), b.old_ls, CLIP, 0.01), b.clip)
    _check("%s g_log_std" % tag, got[b.ls_slot], ref[b.ls_slot], g32[b.ls_slot], 2e-4)   # on its own: against the whole vector's maximum it could hide


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("obs_dim,act_dim", SHAPES)
@pytest.mark.parametrize("n", [129, 1000])
def test_clip_grad_with_every_sample_clipped(n, obs_dim, act_dim, width):
    """C. clip = 1e-3 and the advantage's sign taken from the float64 ratio, on the first n samples whose ratio is at least 1e-2 beyond the
    boundary: every sample is clipped, so every partial row of the mean network's gradient and of g_log_std is exactly 0, the gradient is the
    entropy bonus's constant and nothing else, the clip count is m and the loss still matches."""
    import torch
    b = _bundle(obs_dim, act_dim, width, "logstd")
    clip, margin = 1e-3, 1e-2
    ratio, _ = _ratio64(b, b.clip64, slice(0, NMAX), b.adv, clip)
    ok = ((ratio > 1.0 + clip + margin) | (ratio < 1.0 - clip - margin)).nonzero().squeeze(-1)
    assert ok.numel() >= n and ok[n - 1].item() < 1.1 * n + 40, (ok.numel(), ok[n - 1].item())   # a few per cent of the candidates lie inside the margin
    idx = ok[:n].contiguous()
    adv = torch.where(ratio > 1.0, b.adv.abs() + 0.1, -b.adv.abs() - 0.1).float().contiguous()
    r, clipped = ratio[idx], (((adv[idx] > 0) & (ratio[idx] > 1.0 + clip)) | ((adv[idx] < 0) & (ratio[idx] < 1.0 - clip)))
    assert clipped.all() and ((r - 1.0).abs() >= clip + margin).all()
    last = int(idx[-1].item()) + 1
    _ll_ok(b, last)
    tag = "every sample clipped n %d D %d A %d width %d:" % (n, obs_dim, act_dim, width)
    for ent in (0.0, 0.01):
        ck, got, st, _ = _clip_grad(b, last, idx, n, "%s ent %g" % (tag, ent), clip=clip, ent=ent, adv=adv)
        assert st[2].item() == n
        assert (_clip_partial(ck, n) == 0).all()
        want = torch.zeros_like(got)
        want[b.ls_slot] = -ent
        assert torch.equal(got, want)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("obs_dim,act_dim", SHAPES)
@pytest.mark.parametrize("n", [129, 1000])
def test_clip_grad_with_no_sample_clipped_and_with_zero_advantages(n, obs_dim, act_dim, width):
    """C. clip = 1e6: no sample is clipped and the gradient is that of -(ratio adv).mean().  Then clip = 0.2 with adv == 0 on every third row:
    those rows contribute nothing and count as unclipped, whatever their ratio."""
    import torch
    from cassierl_amd import ppo as P
    b = _bundle(obs_dim, act_dim, width, "logstd")
    _ll_ok(b, n)
    tag = "D %d A %d width %d n %d:" % (obs_dim, act_dim, width, n)

    def plain(pol, obs, act, adv, om, ols):
        _, ratio, _ = P.surrogate_terms(pol.mean_net(obs), pol.log_std, act, adv, om, ols, 1e6)
        return -(ratio * adv).mean()

    _, _, st, _ = _clip_grad(b, n, None, n, "no sample clipped " + tag, clip=1e6, loss64=plain)
    assert st[2].item() == 0
    keep = _away_from_the_boundaries(b, n)
    adv = b.adv.clone()
    adv[0::3] = 0.0
    ratio, _ = _ratio64(b, b.clip64, keep, adv, CLIP)
    zero = adv[keep] == 0
    outside = zero & ((ratio > 1.0 + CLIP) | (ratio < 1.0 - CLIP))
    print("zero advantages %s %d rows with adv == 0, %d of them with a ratio outside the clip range" % (tag, int(zero.sum()), int(outside.sum())))
    assert zero.sum().item() >= keep.numel() // 4 and outside.any()
    ck, got, st, _ = _clip_grad(b, n, keep, keep.numel(), "zero advantages " + tag, adv=adv)
    _, clipped = _ratio64(b, b.clip64, keep, adv, CLIP)
    assert st[2].item() == clipped[~zero].sum().item() and not clipped[zero].any()


# ------------------------------------------------------------------------------------------------------------------ D. the CG vector kernels
def _cg_iteration(Apm, hls, p, r, x, rr, ls_off, n_ls, reg, tol):
    """One pass of trpo.conjugate_gradient's loop body in the dtype of the arguments, the product assembled as CassieTrpoCgUpdate documents it."""
    import torch
    n = p.numel()
    Ap = torch.empty_like(p)
    Ap[ls_off:ls_off + n_ls] = hls * p[ls_off:ls_off + n_ls]
    rest = torch.ones(n, dtype=torch.bool, device=p.device)
    rest[ls_off:ls_off + n_ls] = False
    Ap[rest] = Apm
    Ap = Ap + reg * p
    alpha = rr / (p @ Ap)
    x, r = x + alpha * p, r - alpha * Ap
    rr_new = r @ r
    running = bool(rr_new >= tol)
    return x, r, (r + (rr_new / rr) * p) if running else r.clone(), rr_new, running


@pytest.mark.parametrize("width,sizes", [(32, [13, 1024, 1025, 2124, 3072]), (128, [1025, 20878, 21504])])
def test_cg_update_kernels_called_directly(width, sizes):
    """D. CassieTrpoCgUpdate / CassiePgCgUpdate on sizes on both sides of a 1024 boundary and at their maxima, with the log_std block in front
    (ls_off = 0: Apm[i - n_ls]) and behind (ls_off = n - n_ls), against one iteration of trpo.conjugate_gradient in float64 on the same float32
    values.  Apm = d o p + 0.1 N(0, 1) with d in [0.5, 1.5]: positive along p, as a Fisher product is, so that the step length is not a quotient
    of a cancelled sum.  Then the frozen state: a tolerance above the new residual gives scal[1] = 0 and p = r, and from then on x and r keep
    their bits; so they do with scal[1] = 0 on entry."""
    import torch
    from cassierl_amd import _lib
    L = _lib.load()
    entry = L.CassieTrpoCgUpdate if width == 32 else L.CassiePgCgUpdate
    P = lambda t: ct.c_void_p(t.data_ptr())
    reg = 1e-5
    g = torch.Generator().manual_seed(40 + width)
    call = lambda n, ls_off, n_ls, Apm, hls, tol, x, r, p, scal: entry(n, ls_off, n_ls, P(Apm), P(hls), ct.c_float(reg), ct.c_float(tol), P(x), P(r), P(p), P(scal), None)
    for n in sizes:
        for n_ls in (6, 7):
            for ls_off in (0, n - n_ls):
                p, r, x = (torch.randn(n, generator=g).to(DEV) for _ in range(3))
                hls = (0.5 + torch.rand(n_ls, generator=g)).to(DEV)
                rest = torch.ones(n, dtype=torch.bool)
                rest[ls_off:ls_off + n_ls] = False
                Apm = ((0.5 + torch.rand(n - n_ls, generator=g)) * p.cpu()[rest] + 0.1 * torch.randn(n - n_ls, generator=g)).to(DEV).contiguous()
                rr = r @ r
                tag = "CG width %d n %d n_ls %d ls_off %d:" % (width, n, n_ls, ls_off)
                for tol in (1e-10, 1e30):
                    d = lambda t: t.double()
                    x64, r64, p64, rr64, run64 = _cg_iteration(d(Apm), d(hls), d(p), d(r), d(x), d(rr), ls_off, n_ls, reg, tol)
                    x32, r32, p32, rr32, _ = _cg_iteration(Apm, hls, p, r, x, rr, ls_off, n_ls, reg, tol)
                    xk, rk, pk = x.clone(), r.clone(), p.clone()
                    scal = torch.stack([rr, torch.ones((), device=DEV)]).contiguous()
                    assert call(n, ls_off, n_ls, Apm, hls, tol, xk, rk, pk, scal) == 0
                    for nm, got, r64_, r32_ in (("x", xk, x64, x32), ("r", rk, r64, r32), ("p", pk, p64, p32), ("r.r", scal[0], rr64, rr32)):
                        _check("%s tol %g %s" % (tag, tol, nm), got, r64_, r32_, 1e-5)
                    assert scal[1].item() == (1.0 if run64 else 0.0) and run64 == (tol < 1.0)
                    again = [t.clone() for t in (xk, rk, pk, scal)]
                    xk2, rk2, pk2, scal2 = x.clone(), r.clone(), p.clone(), torch.stack([rr, torch.ones((), device=DEV)]).contiguous()
                    assert call(n, ls_off, n_ls, Apm, hls, tol, xk2, rk2, pk2, scal2) == 0
                    assert all(torch.equal(a, b_) for a, b_ in zip(again, (xk2, rk2, pk2, scal2)))   # fixed-order sums: the same bits twice
                    if tol > 1.0:   # stopped: p = r, and a further call moves neither x nor r
                        assert torch.equal(pk, rk)
                        assert call(n, ls_off, n_ls, Apm, hls, tol, xk, rk, pk, scal) == 0
                        assert torch.equal(xk, again[0]) and torch.equal(rk, again[1]) and scal[1].item() == 0.0
                # frozen on entry
                xk, rk, pk = x.clone(), r.clone(), p.clone()
                scal = torch.stack([rr, torch.zeros((), device=DEV)]).contiguous()
                assert call(n, ls_off, n_ls, Apm, hls, 1e-10, xk, rk, pk, scal) == 0
                assert torch.equal(xk, x) and torch.equal(rk, r) and scal[1].item() == 0.0
    # refusals
    z = lambda k: torch.zeros(k, device=DEV)
    x, r, p, scal, apm, hls = z(21600), z(21600), z(21600), z(2), z(21600), z(7)
    bad = lambda n, ls_off, n_ls: call(n, ls_off, n_ls, apm, hls, 1e-10, x, r, p, scal)
    assert bad(3073 if width == 32 else 21505, 0, 7) == EINVAL
    assert bad(100, 95, 7) == EINVAL and bad(100, -1, 7) == EINVAL and bad(1000, 1000, 1) == EINVAL
    torch.cuda.synchronize()
    assert (x == 0).all() and (r == 0).all() and (p == 0).all()


# ------------------------------------------------------------------------------------------------------------------ E. the baseline kernels
GRAM_M = [1, 15, 16, 17, 63, 65, 255, 257]
BASE_SEED = {26: 4, 17: 4}   # seeds for which the clipped share of every prefix of GRAM_M rows lies in [3 %, 30 %] (row 0 on its own included)


@functools.lru_cache(maxsize=None)
def _baseline_data(D):
    """257 observations of which about 10 % of the entries lie beyond +-10 (N(0, 6.08^2): P(|z| > 1.645) = 0.1), path clocks up to 999 (row 0
    holds 999: a cube of 997), targets and coefficients in float64."""
    import torch
    g = torch.Generator().manual_seed(BASE_SEED[D])
    m = max(GRAM_M)
    obs = 6.08 * torch.randn(m, D, generator=g)
    t = torch.randint(0, 1000, (m,), generator=g)
    t[0] = 999
    y = torch.randn(m, dtype=torch.float64, generator=g)
    coeffs = torch.randn(2 * D + 4, dtype=torch.float64, generator=g)
    return tuple(x.to(DEV).contiguous() for x in (obs, t, y, coeffs))


@pytest.mark.parametrize("D", [26, 17])
def test_baseline_gram_and_predict_below_one_mfma_step_and_on_clipped_features(D):
    """E. CassieTrpoBaselineGram and CassieTrpoBaselinePredict on 1 .. 257 samples (below, at and above the 16 rows of one MFMA step) whose
    observations are clipped on about a tenth of the entries and whose path clocks reach 999, with the bounds of
    test_baseline_kernels_match_the_torch_expressions and of the GAE test's predictions."""
    import torch
    from cassierl_amd import trpo as T
    obs_, t_, y_, coeffs = _baseline_data(D)
    bk = T.BaselineKernels(torch.device(DEV, 0), D)
    for m in GRAM_M:
        obs, t, y = obs_[:m], t_[:m], y_[:m]
        share = (obs.abs() > 10).double().mean().item()
        assert 0.03 <= share <= 0.30 and t.max().item() == 999
        X = T.LinearFeatureBaseline.features(obs, t).double()
        Ar, br = T.gram(X, y)
        A, b = (z.clone() for z in bk.gram(obs, t, y))
        top = Ar.abs().max().item()
        e_max, e_entry = (A - Ar).abs().max().item() / top, ((A - Ar).abs() / (Ar.abs() + 1e-3 * top)).max().item()
        e_b = (b - br).abs().max().item() / (br.abs().max().item() + top ** 0.5)
        print("gram D %d m %d: clipped share %.3f, X'X %.3g of the maximum (bound 1e-10), entry by entry %.3g (1e-9), X'y %.3g (1e-10)" % (D, m, share, e_max, e_entry, e_b))
        assert e_max < 1e-10 and e_entry < 1e-9 and e_b < 1e-10
        assert torch.equal(A, A.T)
        A2, b2 = bk.gram(obs, t, y)
        assert torch.equal(A, A2) and torch.equal(b, b2)
        pr, got = X @ coeffs, bk.predict(obs, t, coeffs)
        e_p = (got - pr).abs().max().item()
        print("predict D %d m %d: %.3g of 1 + max %.3g (bound 1e-12)" % (D, m, e_p, 1 + pr.abs().max().item()))
        assert e_p <= 1e-12 * (1.0 + pr.abs().max().item())
        assert torch.equal(got, bk.predict(obs, t, coeffs))


@pytest.mark.parametrize("D", [26, 17])
@pytest.mark.parametrize("T_,N", [(1, 1), (3, 255), (5, 257)])
def test_returns_and_advantages_at_small_batches(T_, N, D):
    """E. CassieTrpoReturnsAdvantages with and without coefficients and a last value, on paths that all end, never end and end at random, against
    discounted_returns and the torch expressions of TRPO.process in float64; the sums as the GAE test compares them."""
    import torch
    from cassierl_amd import trpo as T
    g = torch.Generator().manual_seed(17 + T_ + D)
    obs = (6.08 * torch.randn(T_, N, D, generator=g)).to(DEV)
    t = torch.randint(0, 1000, (T_, N), generator=g).to(DEV)
    rew = torch.randn(T_, N, dtype=torch.float64, generator=g).to(DEV)
    coeffs, last = torch.randn(2 * D + 4, dtype=torch.float64, generator=g).to(DEV), torch.randn(N, dtype=torch.float64, generator=g).to(DEV)
    cuts = {"all": torch.ones(T_, N, dtype=torch.bool), "none": torch.zeros(T_, N, dtype=torch.bool), "random": torch.rand(T_, N, generator=g) < 0.3}
    bk = T.BaselineKernels(torch.device(DEV, 0), D)
    for name, cut in cuts.items():
        cut = cut.to(DEV)
        for fitted in (False, True):
            c, lv = (coeffs, last) if fitted else (None, None)
            ret, adv, sums = bk.returns_advantages(obs, t, rew, cut, c, lv, 0.99)
            ret_ref = T.discounted_returns(rew, cut, 0.99, lv)
            values = (T.LinearFeatureBaseline.features(obs.view(-1, D), t.view(-1)).double() @ coeffs).view(T_, N) if fitted else torch.zeros_like(rew)
            adv_ref = ret_ref - values
            e_ret, e_adv = (ret - ret_ref).abs().max().item(), (adv - adv_ref).abs().max().item()
            print("returns T %d N %d D %d cut %s fitted %s: |returns| err %.3g, |adv| err %.3g of max %.3g" % (T_, N, D, name, fitted, e_ret, e_adv, adv_ref.abs().max().item()))
            assert e_ret <= 1e-12 * (1.0 + ret_ref.abs().max().item())
            assert e_adv <= 1e-12 * (1.0 + adv_ref.abs().max().item())
            s1, s2 = adv_ref.sum().item(), (adv_ref ** 2).sum().item()
            assert abs(sums[0].item() - s1) <= 1e-10 * abs(s1) and abs(sums[1].item() - s2) <= 1e-10 * s2
            ret2, adv2, sums2 = bk.returns_advantages(obs, t, rew, cut, c, lv, 0.99)
            assert torch.equal(ret, ret2) and torch.equal(adv, adv2) and torch.equal(sums, sums2)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_sampler_step_at_small_batches(n):
    """E. CassieTrpoSamplerStep on 1, 255 and 257 environments (one workgroup short of, and one lane past, 256) with max_path_length = 3 over five
    steps, against the element-wise torch bookkeeping of TRPO.collect (TRPO._book_step without the kernel): every row, the clocks, the running
    returns, the episode count and the summed returns."""
    import torch
    from cassierl_amd import trpo as T
    g = torch.Generator().manual_seed(23 + n)
    pol = _bundle(26, 6, 32).pol
    fused, plain = (T.TRPO(None, None, pol, T.LinearFeatureBaseline(), n, 26, None, max_path_length=3) for _ in range(2))
    book = fused._fused_sampler_step(torch.device(DEV, 0))
    assert book is not None and fused._book_partial.shape == (max(1, (n + 255) // 256), 2)
    ep = [torch.zeros(2, dtype=torch.float64, device=DEV) for _ in range(2)]
    truncated = 0
    for step in range(5):
        rew = torch.randn(n, dtype=torch.float64, generator=g).to(DEV)
        done = (torch.rand(n, generator=g) < 0.2).to(torch.uint8).to(DEV)
        rows = [[torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.bool, device=DEV)] for _ in range(2)]
        cut, _ = fused._book_step(book, rew, done, *rows[0], ep[0])
        cut_ref, _ = plain._book_step(None, rew, done, *rows[1], ep[1])
        for a, b_ in zip(rows[0], rows[1]):
            assert torch.equal(a, b_), step
        assert torch.equal(cut.bool(), cut_ref.bool())
        assert torch.equal(fused.path_t, plain.path_t) and torch.equal(fused.path_ret, plain.path_ret)
        assert ep[0][0].item() == ep[1][0].item()
        assert abs(ep[0][1].item() - ep[1][1].item()) <= 1e-9 * (1.0 + abs(ep[1][1].item()))
        truncated += int((cut_ref.bool() & ~done.bool()).sum())
    print("sampler step n %d: %d paths ended, %d of them by truncation" % (n, int(ep[1][0].item()), truncated))
    assert ep[1][0].item() > 0 and (truncated > 0 or n == 1)
