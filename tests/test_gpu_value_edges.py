"""PPO's value network (csrc/tu_vf.hip: CassieVfPredict, CassieVfGae, CassieVfGrad) and the Adam kernel it leans on (csrc/tu_pg.hip:
CassiePgAdam) where tests/test_gpu_ppo_value.py and test_gpu_vpg.py do not look: minibatches of a lone sample, one full tile (three idle
wavefronts), a tile +- 1, one group of four tiles +- 1 and two workgroups; one hot residual per tile position; a `scale` that is not 1 / m;
saturated and near-zero hidden units; residuals of 1e2 .. 1e4; GAE at the partial rows' edges with lambda and gamma 0 and 1, every / no / only the
last step cut and values of 1e4; Adam at sizes around its block, at large t, on a zero gradient and on one whose square underflows; one whole
update below a tile.  -m gpu only; the counterpart of test_gpu_onpolicy_edges.py for this unit, at both widths of observation (26 and 45).

The reference of every comparison is FLOAT64 torch: value.value_loss through autograd on a .double() copy of the network, MLPValueFunction.predict
of that copy, ppo.gae_advantages, adam.adam_step_ on float64 copies; the kernels' float32 inputs (observations, targets, values, state) are cast
up, so both sides see the same numbers.  Bounds, all of them this project's:
  gradient    per parameter block of test_gpu_ppo_value._blocks (W1 split at column 32 for D = 45) and per 32-row quarter of the 128-row blocks:
              max|got - ref64| < 2e-4 max|ref64| of the block; where a block misses it, err_kernel <= 4 err_torch32 decides, torch32
              being float32 autograd of the same statement on the same float32 inputs.  _check prints which rule held ("bound" or "4x").
  prediction  5e-6 (1 + max|V64|).
  statistic   |stat - stat64| / m <= 2e-5 mean(r^2) / 2 + 5e-6 (1 + max|V64|) mean|r|, r the float64 residual: the bound of test_gpu_ppo_value plus
              the prediction bound carried through d(r^2 / 2) = |r| dV.
  GAE         1e-12 (1 + max|ref|) for returns, adv and vtarget, 1e-10 relative for the two sums.
  Adam        max|got - ref64| < 1e-6 max|ref64| per tensor (test_pg_adam_matches_the_torch_adam's bound), else 4 x the float32 statement's error.
Every launch is made twice and must repeat bit for bit; every output buffer is longer than the launch needs and the tail must keep its fill.

Every input is drawn on the CPU from a torch.Generator seeded per case and moved to the device, so every precondition asserted below (|g_ref[b3]|
against mean|r|, the cold rows' share of a hot-residual case, the saturation shares, |z| < 2) depends on the float64 reference alone.  Networks,
batches and ValueKernels objects are built once per (D, regime) (lru_cache) and are not written to afterwards.

What the file found when it was written ("Edges", has the figures): the `tiny` regime's W3 block missed both gradient rules at
five of its six cases (tanh_fast's absolute error of 1e-7 on activations of 1e-4; now tanh_near0 in this unit), and with values of 1e4 the value
target a + value lost four digits to cancellation (now the lambda-return's own recurrence; _lambda_return below is the reference for it)."""
import copy
import ctypes as ct
import functools
import math
import types

import pytest

from test_gpu_offpolicy_edges import _check, _flat_grad
from test_gpu_ppo_value import _blocks, _make

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1
SENT = -777.0
SMALL = [1, 4, 31, 32, 33, 127, 128, 129, 256]   # a lone sample; a short tile; a tile - 1, a full tile (three idle wavefronts), + 1; a group of four tiles - 1, full, + 1; two workgroups
NROWS = 300      # the batch that the minibatches of groups A and C are rows of
NBATCH = 1200    # rows drawn per (D, regime)
SAT = 60.0       # test_gpu_onpolicy_edges.SAT: every second hidden unit's row of W and its bias times 60
REGIMES = {"default": 0, "saturated": 1, "tiny": 2}
SEED_BUMP = {}   # (D, regime) -> added to the bundle's seed, ("idx", D, m) -> added to a `repeats` index's seed, where the first seed misses a condition asserted below


# ------------------------------------------------------------------------------------------------------------------ networks and data
def _linears(vf):
    from torch import nn
    return [m for m in vf.net if isinstance(m, nn.Linear)]


@functools.lru_cache(maxsize=None)
def _net_and_data(D, regime="default"):
    """On the CPU, from one generator: the value network (Xavier-uniform weights, zero biases, + N(0, 0.1) jitter, then the regime), NBATCH
    observations 0.7 N(0, 1), N(0, 1) noise for the targets (float64), the float64 copy of the network and its values."""
    import torch
    from cassierl_amd import value as VF
    g = torch.Generator().manual_seed(7000 + 10 * D + REGIMES[regime] + SEED_BUMP.get((D, regime), 0))
    vf = VF.MLPValueFunction(D, (128, 128))
    with torch.no_grad():
        for l in _linears(vf):   # MLPValueFunction's own initialisation, from this generator
            a = math.sqrt(6.0 / (l.in_features + l.out_features))
            l.weight.copy_((torch.rand(l.weight.shape, generator=g) * 2 - 1) * a); l.bias.zero_()
        for p in vf.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        for l in _linears(vf)[:2]:
            if regime == "saturated":
                l.weight[0::2] *= SAT; l.bias[0::2] *= SAT
            elif regime == "tiny":
                l.weight *= 1e-3; l.bias *= 1e-3
    obs = 0.7 * torch.randn(NBATCH, D, generator=g)
    noise = torch.randn(NBATCH, dtype=torch.float64, generator=g)
    vf64 = copy.deepcopy(vf).double()
    return vf, vf64, obs, noise, vf64.predict(obs.double())


def _shares(vf64, obs):
    """float64: per hidden layer the shares of pre-activations with |z| > 9 and with |z| < 2, and max|z|."""
    import torch
    lin = _linears(vf64)
    with torch.no_grad():
        z1 = lin[0](obs.double())
        z2 = lin[1](torch.tanh(z1))
    return [((z.abs() > 9).double().mean().item(), (z.abs() < 2).double().mean().item(), z.abs().max().item()) for z in (z1, z2)]


@functools.lru_cache(maxsize=None)
def _bundle(D, regime="default"):
    """_net_and_data on the device with the kernels: vf, vf64, obs [NBATCH, D], noise, v64 (the float64 network's values, evaluated on the device),
    y = float32(V64 + 0.5 + noise) -- the offset keeps b3's reference, mean(r), from being a cancelling mean --, theta, vk (its batch: the first
    NROWS rows)."""
    import torch
    from cassierl_amd import value as VF
    vf, vf64, obs, noise, v64 = _net_and_data(D, regime)
    b = types.SimpleNamespace(D=D, regime=regime, vf=copy.deepcopy(vf).to(DEV), vf64=copy.deepcopy(vf64).to(DEV), obs=obs.to(DEV).contiguous(), noise=noise.to(DEV),
                              y=(v64 + 0.5 + noise).float().to(DEV).contiguous())
    b.v64 = b.vf64.predict(b.obs.double())
    b.theta = VF.aligned_value_params(b.vf)
    b.vk = VF.ValueKernels(b.vf, b.theta)
    assert b.vk.kind == "vf_grad" and b.theta.data_ptr() % 16 == 0
    b.vk.set_batch(b.obs[:NROWS], b.y[:NROWS])
    return b


# ------------------------------------------------------------------------------------------------------------------ launches and references
def _grad_launch(b, obs, y, idx, m, scale=None):
    """CassieVfGrad called directly, twice, on buffers with 3 rows of SENT behind CassieVfGradRows(m): (gradient, statistic)."""
    import torch
    from cassierl_amd._lib import ptr
    vk = b.vk
    rows = vk.fn["GradRows"](m)
    assert rows == min((m + 127) // 128, 256)
    assert obs.is_contiguous() and obs.dtype == torch.float32 and y.is_contiguous() and y.dtype == torch.float32 and y.numel() == obs.shape[0]
    assert (idx is None and m <= obs.shape[0]) or (idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == m and 0 <= int(idx.min()) and int(idx.max()) < obs.shape[0])
    out = []
    for _ in range(2):
        partial = torch.full((rows + 3, vk.NP), SENT, device=DEV)
        stats = torch.full((rows + 3,), SENT, dtype=torch.float64, device=DEV)
        vk._call("Grad", ptr(obs), obs.shape[0], b.D, *vk._net(), ptr(idx), m, ptr(y), ct.c_float(1.0 / m if scale is None else scale), ptr(partial), ptr(stats))
        assert bool((partial[rows:] == SENT).all()) and bool((stats[rows:] == SENT).all())   # rows behind the launch's own keep their fill
        out.append((partial[:rows].sum(0), stats[:rows].sum()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])   # fixed-order sums: the same bits twice
    assert torch.isfinite(out[0][0]).all() and torch.isfinite(out[0][1])
    return out[0]


def _refs(b, obs, y, sel):
    """float64 and float32 autograd of value_loss on the rows sel of (obs, y); the float64 residuals r = V64 - y, the float64 statistic, max|V64|."""
    import torch
    from cassierl_amd import value as VF
    o, t = obs[sel], y[sel]
    ref = _flat_grad(VF.value_loss(b.vf64, o.double(), t.double()), b.vf64)
    g32 = _flat_grad(VF.value_loss(b.vf, o, t), b.vf)
    v = b.vf64.predict(o.double())
    r = v - t.double()
    return ref, g32, r, 0.5 * (r * r).sum(), v.abs().max().item()


def _judge(tag, D, got, ref, g32):
    """The gradient rule per block and per 32-row quarter; prints one summary line (worst err / max|ref64| of a block, whether the 4x rule was needed)."""
    worst, rules = 0.0, set()
    for name, o, r, c, cols in _blocks(D):
        blk = lambda g: g[o:o + r * c].view(r, c)[:, cols]
        parts = [(name, blk(got), blk(ref), blk(g32))]
        if r == 128:   # the 32-row quarters, one per wavefront
            parts += [("%s quarter %d" % (name, q), blk(got)[32 * q:32 * q + 32], blk(ref)[32 * q:32 * q + 32], blk(g32)[32 * q:32 * q + 32]) for q in range(4)]
        for nm, a, r64, r32 in parts:
            e_k, _, rule = _check("%s %s" % (tag, nm), a, r64, r32, 2e-4)
            top = r64.abs().max().item()
            worst = max(worst, e_k / top if top > 0 else 0.0)
            rules.add(rule)
    print("EDGES %s worst block %.3g of its max|g_ref| (bound 2e-4), rules %s" % (tag, worst, sorted(rules)))
    return worst


def _stat_ok(tag, st, st64, r, vmax, m):
    err = abs(st.item() - st64.item()) / m
    bound = 2e-5 * (r * r).mean().item() / 2 + 5e-6 * (1 + vmax) * r.abs().mean().item()
    print("EDGES %s statistic: kernel %.12g, float64 %.12g, |diff| / m %.3g (bound %.3g)" % (tag, st.item(), st64.item(), err, bound))
    assert err <= bound, (tag, st.item(), st64.item(), err, bound)


def _grad_case(tag, b, obs, y, idx, m, b3_floor=None):
    """One minibatch under the gradient rule and the statistic bound; b3_floor: the precondition |g_ref[b3]| >= b3_floor mean|r| on the float64 side."""
    sel = slice(0, m) if idx is None else idx
    ref, g32, r, st64, vmax = _refs(b, obs, y, sel)
    if b3_floor is not None:
        print("%s |g_ref[b3]| %.3g, mean|r| %.3g" % (tag, ref[-1].abs().item(), r.abs().mean().item()))
        assert ref[-1].abs().item() >= b3_floor * r.abs().mean().item()   # a reference-only condition: bump the seed (SEED_BUMP), not the bound
    got, st = _grad_launch(b, obs, y, idx, m)
    _judge(tag, b.D, got, ref, g32)
    _stat_ok(tag, st, st64, r, vmax, m)
    return got, st, ref, g32


# ------------------------------------------------------------------------------------------------------------------ A. small minibatches
@pytest.mark.parametrize("D", [26, 45])
@pytest.mark.parametrize("mode", ["rows", "repeats", "all"])
@pytest.mark.parametrize("m", SMALL)
def test_value_grad_at_small_minibatches(m, mode, D):
    """A. CassieVfGrad on minibatches of SMALL rows: `rows` idx = NULL and rows 0 .. m - 1 of a batch of 300 (a lane past m would read real
    numbers), `repeats` an index drawn with replacement whose positions 0 and 1 hold the same row, `all` idx = NULL on a batch of exactly m rows.
    Targets V64 + 0.5 + N(0, 1): from m = 31 on |g_ref[b3]| >= 0.1 mean|r| is asserted, so no block's reference is a cancelling mean."""
    import torch
    b = _bundle(D)
    idx = None
    if mode == "all":
        obs, y = b.obs[:m].clone(), b.y[:m].clone()
    else:
        obs, y = b.obs[:NROWS], b.y[:NROWS]
    if mode == "repeats":
        idx = torch.randint(0, NROWS, (m,), generator=torch.Generator().manual_seed(11 + 100 * m + D + SEED_BUMP.get(("idx", D, m), 0)))
        if m >= 2:
            idx[1] = idx[0]
            assert idx.unique().numel() < m
        idx = idx.to(DEV)
    got, st, _, _ = _grad_case("A D %d m %d %s:" % (D, m, mode), b, obs, y, idx, m, b3_floor=0.1 if m >= 31 else None)
    if mode != "all":   # the Python wrapper on its own buffers: the same bits
        gw, sw = b.vk.grad(idx, m=m)
        assert torch.equal(gw, got) and torch.equal(sw, st)


# ------------------------------------------------------------------------------------------------------------------ B. one hot residual
@pytest.mark.parametrize("D", [26, 45])
@pytest.mark.parametrize("hot", [0, 31, 32, 63, 96, 127, 128])
def test_value_grad_with_one_hot_residual(hot, D):
    """B. m = 129, no index; the target is float32(V64) on every row but `hot` (the first and last lane of a tile, the last tile of the first group,
    the lone sample of the second group), where it is V64 - 100.  The gradient must be the float64 single-sample gradient of that row with scale
    1 / m: a cotangent delivered to another sample, tile or wavefront shows as itself, not as "a large error".  The cold rows' residuals are float32
    roundings of V: sum|r_cold| <= 1e-5 x 100 is asserted on the float64 side before the kernel is judged."""
    import torch
    from cassierl_amd import value as VF
    m = 129
    b = _bundle(D)
    obs = b.obs[:m].clone()
    y = b.v64[:m].float()
    y[hot] = (b.v64[hot] - 100.0).float()
    y = y.contiguous()
    r = b.v64[:m] - y.double()
    cold = r.abs().sum().item() - r[hot].abs().item()
    tag = "B D %d hot row %d:" % (D, hot)
    print("%s residual of the hot row %.9g, sum|r| of the others %.3g" % (tag, r[hot].item(), cold))
    assert abs(r[hot].item() - 100.0) < 1e-4 and cold <= 1e-5 * 100.0
    ref = _flat_grad(VF.value_loss(b.vf64, obs[hot:hot + 1].double(), y[hot:hot + 1].double()) / m, b.vf64)   # (1 / m) r dV / dtheta of the one row
    g32 = _flat_grad(VF.value_loss(b.vf, obs, y), b.vf)
    got, st = _grad_launch(b, obs, y, None, m)
    _judge(tag, D, got, ref, g32)
    _stat_ok(tag, st, 0.5 * (r * r).sum(), r, b.v64[:m].abs().max().item(), m)


# ------------------------------------------------------------------------------------------------------------------ C. scale
@pytest.mark.parametrize("D", [26, 45])
def test_value_grad_scale_is_the_argument(D):
    """C. The kernel's `scale` is an argument, not 1 / m: at 0.37 / m and -1 / m the gradient is 0.37 times and -1 times the reference's under the
    gradient rule and the statistic keeps the bits of the 1 / m launch; at 0 every entry is exactly 0 (+0 or -0) and the statistic is unchanged."""
    import torch
    m = 129
    b = _bundle(D)
    obs, y = b.obs[:NROWS], b.y[:NROWS]
    ref, g32, r, st64, vmax = _refs(b, obs, y, slice(0, m))
    g1, st1 = _grad_launch(b, obs, y, None, m)
    _judge("C D %d scale 1 / m:" % D, D, g1, ref, g32)
    _stat_ok("C D %d:" % D, st1, st64, r, vmax, m)
    for s in (0.37, -1.0):
        g, st = _grad_launch(b, obs, y, None, m, scale=s / m)
        _judge("C D %d scale %g / m:" % (D, s), D, g, s * ref, s * g32)
        assert torch.equal(st, st1)
    g, st = _grad_launch(b, obs, y, None, m, scale=0.0)
    assert bool((g == 0).all()) and torch.equal(st, st1)


# ------------------------------------------------------------------------------------------------------------------ D. network regimes
def _regime_ok(b, tag):
    sh = _shares(b.vf64, b.obs[:1000])
    print("%s pre-activations |z| > 9 / |z| < 2 / max: layer 1 %.3f / %.3f / %.3g, layer 2 %.3f / %.3f / %.3g" % (tag, *sh[0], *sh[1]))
    for far, close, top in sh:
        if b.regime == "saturated":
            assert far >= 0.30 and close >= 0.20
        elif b.regime == "tiny":
            assert top < 2.0


@pytest.mark.parametrize("D", [26, 45])
@pytest.mark.parametrize("m", [33, 129, 1000])
@pytest.mark.parametrize("regime", ["saturated", "tiny"])
def test_value_grad_with_saturated_and_near_zero_hidden_units(regime, m, D):
    """D. `saturated`: every second row of W1, b1, W2, b2 times 60; in float64 at least 30 % of each layer's pre-activations have |z| > 9 (1 - H^2
    exactly 0 in float32, tanh_fast's ends) and at least 20 % |z| < 2.  `tiny`: both hidden layers times 1e-3, every |z| < 2 (about 1e-3: tanh_fast =
    1 - 2 / (e + 1) has an absolute error of about 1e-7 there).  idx: a random subset of the batch."""
    import torch
    b = _bundle(D, regime)
    tag = "D %s D %d m %d:" % (regime, D, m)
    _regime_ok(b, tag)
    idx = torch.randperm(NBATCH, generator=torch.Generator().manual_seed(31 + m + D))[:m].contiguous().to(DEV)
    _grad_case(tag, b, b.obs, b.y, idx, m)


def _predict_case(tag, b, obs, n):
    """CassieVfPredict on the first n rows of obs, twice, 40 rows of SENT behind n; obs is longer than n, so a lane past n reads real numbers."""
    import torch
    from cassierl_amd._lib import ptr
    v64 = b.vf64.predict(obs[:n].double())
    with torch.no_grad():
        v32 = b.vf(obs[:n])
    outs = []
    for _ in range(2):
        out = torch.full((n + 40,), SENT, device=DEV)
        b.vk._call("Predict", ptr(obs), n, b.D, *b.vk._net(), ptr(out))
        assert bool((out[n:] == SENT).all())
        outs.append(out[:n])
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all() and torch.isfinite(v64).all()
    err, e32, top = (outs[0].double() - v64).abs().max().item(), (v32.double() - v64).abs().max().item(), v64.abs().max().item()
    print("EDGES %s prediction err %.3g (float32 torch %.3g), max|V64| %.3g, bound %.3g" % (tag, err, e32, top, 5e-6 * (1 + top)))
    assert err < 5e-6 * (1 + top)


@pytest.mark.parametrize("D", [26, 45])
@pytest.mark.parametrize("n", [1, 32, 33, 128, 129, 257])
@pytest.mark.parametrize("regime", ["default", "saturated", "tiny"])
def test_predict_at_full_tiles_and_in_the_regimes(regime, n, D):
    """D. CassieVfPredict at a lone row, a full tile, a full workgroup and each + 1, in the default network and both regimes."""
    b = _bundle(D, regime)
    tag = "D predict %s D %d n %d:" % (regime, D, n)
    _regime_ok(b, tag)
    _predict_case(tag, b, b.obs, n)


@pytest.mark.parametrize("D", [26, 45])
def test_predict_on_observations_of_a_thousand(D):
    """D. Observations times 1e3, which nothing clips: (nearly) every unit of the first layer saturates, tanh_fast's e overflows to inf or
    underflows to 0, and V stays finite and within the prediction bound."""
    b = _bundle(D)
    obs = (1e3 * b.obs[:300]).contiguous()
    sh = _shares(b.vf64, obs)
    print("D predict obs x 1e3 D %d: layer 1 |z| > 9 share %.3f, max|z| %.3g" % (D, sh[0][0], sh[0][2]))
    assert sh[0][0] >= 0.95
    _predict_case("D predict obs x 1e3 D %d n 257:" % D, b, obs, 257)


# ------------------------------------------------------------------------------------------------------------------ E. residual scale
@pytest.mark.parametrize("D", [26, 45])
@pytest.mark.parametrize("m", [129, 1000])
@pytest.mark.parametrize("kind", ["large", "mixed"])
def test_value_grad_with_large_and_mixed_residuals(kind, m, D):
    """E. `large`: y = V64 + 300 + 100 N(0, 1), the returns of early training against V = 0.  `mixed`: every 16th row's residual is 1e4 N(0, 1),
    the others N(0, 1).  The float32 cotangent, its sums and the float64 statistic under the same rules; everything finite (_grad_launch)."""
    b = _bundle(D)
    resid = 300.0 + 100.0 * b.noise if kind == "large" else b.noise.clone()
    if kind == "mixed":
        resid[0::16] *= 1e4
    y = (b.v64 + resid).float().contiguous()
    _grad_case("E %s D %d m %d:" % (kind, D, m), b, b.obs, y, None, m)


# ------------------------------------------------------------------------------------------------------------------ F. GAE
GAE_SHAPES = [(1, 1), (3, 255), (5, 256), (5, 257), (2, 513)]   # one lane; a workgroup - 1, full, + 1 (a second partial row of one lane); a third row of one lane
GAE_COEFFS = [(0.99, 0.0), (0.99, 1.0), (0.0, 0.95), (1.0, 1.0), (0.99, 0.95)]


def _gae_launch(vk, val, last, rew, cut, gamma, lam):
    """CassieVfGae called directly, twice, the three outputs 8 entries longer and `partial` one row longer than the launch needs."""
    import torch
    from cassierl_amd._lib import ptr
    T_, N = rew.shape
    rows = (N + 255) // 256
    res = []
    for _ in range(2):
        o3 = [torch.full((T_ * N + 8,), SENT, dtype=torch.float64, device=DEV) for _ in range(3)]
        partial = torch.full((rows + 1, 2), SENT, dtype=torch.float64, device=DEV)
        vk._call("Gae", ptr(val), ptr(last), ptr(rew), ptr(cut), T_, N, ct.c_double(gamma), ct.c_double(lam), *[ptr(x) for x in o3], ptr(partial))
        assert all(bool((x[T_ * N:] == SENT).all()) for x in o3) and bool((partial[rows:] == SENT).all())
        res.append([x[:T_ * N].view(T_, N) for x in o3] + [partial[:rows].sum(0)])
    assert all(torch.equal(a, b_) for a, b_ in zip(*res))
    return res[0]


def _lambda_return(rew, live, values, last, gamma, lam):
    """float64: the value target adv + values of ppo.gae_advantages by the lambda-return's own recurrence y_t = r_t + gamma live_t ((1 - lambda)
    v_{t+1} + lambda y_{t+1}), y_T = v_T = last.  The same number in exact arithmetic (adv_t + v_t = r_t + gamma live_t (v_{t+1} + lambda adv_{t+1})),
    but without the cancellation of adv + values: with values of 1e4 and lambda = 1 the sum adv + values is a return of order 5 formed from two
    numbers of order 1e4, whose float64 rounding alone (1e-11) is above the bound 1e-12 (1 + max|vtarget|) that this reference is used with."""
    import torch
    y, out = last, torch.empty_like(rew)
    for t in range(rew.shape[0] - 1, -1, -1):
        v_next = values[t + 1] if t + 1 < rew.shape[0] else last
        y = rew[t] + gamma * live[t] * ((1.0 - lam) * v_next + lam * y)
        out[t] = y
    return out


@pytest.mark.parametrize("vscale", [1.0, 1e4])
@pytest.mark.parametrize("T_,N", GAE_SHAPES)
def test_gae_at_the_partial_rows_edges_and_coefficient_ends(T_, N, vscale):
    """F. CassieVfGae with and without last_value, lambda and gamma at 0 and 1, no / every / a fifth of the samples / only the last step cut, values
    N(0, 1) and 1e4 N(0, 1), against ppo.gae_advantages, and the identities: lambda = 1: vtarget = returns; lambda = 0: adv = rew + gamma live
    v_next - value; every sample cut: returns == rew exactly; the last step cut: last_value is dead, with and without it the same bits."""
    import torch
    from cassierl_amd import ppo as P
    vk = _bundle(26).vk
    g = torch.Generator().manual_seed(1000 * T_ + N + (7 if vscale > 1 else 0))
    rew = torch.randn(T_, N, dtype=torch.float64, generator=g).to(DEV)
    val = (vscale * torch.randn(T_, N, generator=g)).to(DEV)
    last = (vscale * torch.randn(N, generator=g)).to(DEV)
    only_last = torch.zeros(T_, N, dtype=torch.bool)
    only_last[-1] = True
    cuts = {"none": torch.zeros(T_, N, dtype=torch.bool), "all": torch.ones(T_, N, dtype=torch.bool), "random": torch.rand(T_, N, generator=g) < 0.2, "last": only_last}
    worst = 0.0
    for cname, cut in cuts.items():
        cut = cut.to(DEV).contiguous()
        live = (~cut).double()
        for gamma, lam in GAE_COEFFS:
            got = {}
            for with_last in (True, False):
                lv = last if with_last else None
                ret, adv, vt, sums = got[with_last] = _gae_launch(vk, val, lv, rew, cut, gamma, lam)
                last64 = last.double() if with_last else torch.zeros(N, dtype=torch.float64, device=DEV)
                ret_r, adv_r = P.gae_advantages(rew, cut, val.double(), last64, gamma, lam)
                vt_r = _lambda_return(rew, live, val.double(), last64, gamma, lam)
                tag = "F T %d N %d values x %g cut %s gamma %g lambda %g last %s" % (T_, N, vscale, cname, gamma, lam, with_last)
                for name, a, r_ in (("returns", ret, ret_r), ("adv", adv, adv_r), ("vtarget", vt, vt_r)):
                    err, top = (a - r_).abs().max().item(), r_.abs().max().item()
                    worst = max(worst, err / (1 + top))
                    assert err <= 1e-12 * (1 + top), (tag, name, err, top)
                # ... and the statement of value.py, adv + values, on the scale of its operands (its own float64 rounding)
                assert (vt - (adv_r + val.double())).abs().max().item() <= 1e-12 * (1 + max(adv_r.abs().max().item(), val.abs().max().item())), tag
                s_r = torch.stack([adv_r.sum(), (adv_r * adv_r).sum()])
                assert bool(((sums - s_r).abs() <= 1e-10 * s_r.abs()).all()), (tag, sums, s_r)
                if lam == 1.0:
                    assert (vt - ret).abs().max().item() <= 1e-12 * (1 + ret_r.abs().max().item()), tag
                if lam == 0.0:
                    v_next = torch.cat([val[1:].double(), last64.unsqueeze(0)])
                    assert (adv - (rew + gamma * live * v_next - val.double())).abs().max().item() <= 1e-12 * (1 + adv_r.abs().max().item()), tag
                if cname == "all":
                    assert torch.equal(ret, rew), tag
            if cname == "last":
                assert all(torch.equal(a, b_) for a, b_ in zip(got[True], got[False])), (T_, N, gamma, lam)
    print("EDGES F T %d N %d values x %g: worst err / (1 + max|ref|) %.3g (bound 1e-12)" % (T_, N, vscale, worst))


# ------------------------------------------------------------------------------------------------------------------ G. Adam
ADAM_N = [1, 255, 256, 257, 20097, 22529]   # around the block of 256; the value network's parameter counts at D = 26 and D = 45
ADAM_T = [1, 2, 1000, 100000]
LR = 1e-3


def _f32(x):
    import torch
    return float(torch.tensor(x, dtype=torch.float32))


def _adam_launch(n, g, m, v, theta, t, lr=LR):
    import torch
    from cassierl_amd import _lib
    P = lambda x: None if x is None else ct.c_void_p(x.data_ptr())
    return _lib.load().CassiePgAdam(n, P(g), P(m), P(v), P(theta), t, ct.c_float(lr), ct.c_float(0.9), ct.c_float(0.999), ct.c_float(1e-8),
                                    ct.c_void_p(torch.cuda.current_stream().cuda_stream))


def _adam_twice(n, g, m, v, theta, t):
    """CassiePgAdam on copies of the state with 8 entries of SENT behind n, twice: the new (m, v, theta), first n entries."""
    import torch
    pad = lambda x: torch.cat([x, torch.full((8,), SENT, device=DEV)]).contiguous()
    res = []
    for _ in range(2):
        gp, mp, vp, tp = (pad(x) for x in (g, m, v, theta))
        assert _adam_launch(n, gp, mp, vp, tp, t) == 0
        assert all(bool((x[n:] == SENT).all()) for x in (gp, mp, vp, tp)) and torch.equal(gp[:n], g)
        res.append((mp[:n], vp[:n], tp[:n]))
    assert all(torch.equal(a, b_) for a, b_ in zip(*res))
    return res[0]


def _adam_statement(g, m, v, theta, t, dtype):
    """adam.adam_step_ on copies in `dtype`, the betas, eps and lr as float32 holds them (given explicitly: in float64 1 - 0.999 differs from
    1 - float32(0.999) by 1.3e-5 of itself, and the comparison would measure that)."""
    from cassierl_amd import adam as A
    g_, m_, v_, th_ = (x.to(dtype).clone() for x in (g, m, v, theta))
    A.adam_step_(th_, g_, m_, v_, t, _f32(LR), _f32(0.9), _f32(0.999), _f32(1e-8))
    return m_, v_, th_


@pytest.mark.parametrize("t", ADAM_T)
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_kernel_around_its_block_and_at_large_t(n, t):
    """G. One step at step count t from a state of the gradient's scale: gradients of five decades of magnitude, m = 0.3 N(0, 1) x the same
    magnitudes, v = U(0, 1) x their squares, theta N(0, 1)."""
    import torch
    gen = torch.Generator().manual_seed(50 + n + t)
    mag = 10.0 ** torch.randint(-4, 1, (n,), generator=gen).float()
    g, m0, v0, th0 = (x.to(DEV) for x in (torch.randn(n, generator=gen) * mag, 0.3 * torch.randn(n, generator=gen) * mag, torch.rand(n, generator=gen) * mag * mag,
                                          torch.randn(n, generator=gen)))
    got = _adam_twice(n, g, m0, v0, th0, t)
    ref64, ref32 = _adam_statement(g, m0, v0, th0, t, torch.float64), _adam_statement(g, m0, v0, th0, t, torch.float32)
    worst = 0.0
    for name, a, r64, r32 in zip(("m", "v", "theta"), got, ref64, ref32):
        e_k, _, _ = _check("G Adam n %d t %d %s" % (n, t, name), a, r64, r32, 1e-6)
        worst = max(worst, e_k / r64.abs().max().item())
    print("EDGES G Adam n %d t %d: worst err / max|ref64| %.3g (bound 1e-6)" % (n, t, worst))


@pytest.mark.parametrize("n", [1, 257, 22529])
def test_adam_kernel_on_a_zero_gradient_and_on_one_whose_square_underflows(n):
    """G. A zero gradient on zero state: theta keeps its bits, m and v stay exactly 0.  A gradient of 1e-25 on zero state: g^2 underflows, v stays
    0, the step is a m / eps in the kernel and in the statement; theta = 1e-20 N(0, 1), so that the step of about 3e-22 shows: within 4 ulp of the
    float32 statement's theta."""
    import torch
    gen = torch.Generator().manual_seed(60 + n)
    zero = torch.zeros(n, device=DEV)
    for t in (1, 1000):
        th0 = torch.randn(n, generator=gen).to(DEV)
        m, v, th = _adam_twice(n, zero, zero, zero, th0, t)
        assert torch.equal(th, th0) and bool((m == 0).all()) and bool((v == 0).all())
        th0 = (1e-20 * torch.randn(n, generator=gen)).to(DEV)
        g = torch.full((n,), 1e-25, device=DEV)
        m, v, th = _adam_twice(n, g, zero, zero, th0, t)
        m32, v32, th32 = _adam_statement(g, zero, zero, th0, t, torch.float32)
        ulp = torch.nextafter(th32.abs(), torch.full_like(th32, math.inf)) - th32.abs()
        moved = (th32 != th0).double().mean().item()
        err = ((th - th32).abs() / ulp).max().item()
        print("EDGES G Adam n %d t %d g 1e-25: theta moved on %.2f of the entries, kernel within %.3g ulp of the float32 statement" % (n, t, moved, err))
        assert bool((v == 0).all()) and bool((v32 == 0).all()) and moved > 0.9 and err <= 4.0
        assert (m - m32).abs().max().item() <= 1e-6 * m32.abs().max().item() and bool((m > 0).all())


def test_adam_kernel_refuses_bad_arguments_before_anything_is_written():
    """G. t = 0, n = 0 and a null pointer return CASSIE_EINVAL and write nothing."""
    import torch
    n = 257
    g, m, v, th = (torch.full((n,), SENT, device=DEV) for _ in range(4))
    rcs = [_adam_launch(n, g, m, v, th, 0), _adam_launch(n, g, m, v, th, -1), _adam_launch(0, g, m, v, th, 1), _adam_launch(-5, g, m, v, th, 1),
           _adam_launch(n, None, m, v, th, 1), _adam_launch(n, g, None, v, th, 1), _adam_launch(n, g, m, None, th, 1), _adam_launch(n, g, m, v, None, 1)]
    torch.cuda.synchronize()
    assert all(rc == EINVAL for rc in rcs), rcs
    assert all(bool((x == SENT).all()) for x in (g, m, v, th))
    g.fill_(1.0); v.fill_(1.0)   # (a second moment is not negative)
    assert _adam_launch(n, g, m, v, th, 1) == 0   # ... and the same call with good arguments runs
    torch.cuda.synchronize()
    assert torch.isfinite(th).all() and not bool((m == SENT).any()) and not bool((th == SENT).any())


# ------------------------------------------------------------------------------------------------------------------ H. one whole update below a tile
@pytest.mark.parametrize("family", ["cassie3d", "cassie2d"])
def test_fused_update_below_a_tile_is_as_close_to_float64_as_the_torch_update(family):
    """H. test_gpu_ppo_value.test_fused_update_is_as_close_to_float64_as_the_torch_update at 32 envs x 4 steps, minibatch_size 16, one epoch: eight
    minibatch steps of half a tile each, fused, forced-torch float32 and torch float64 from the same parameters, batch and permutation.  Required
    of the policy's and the value network's vector: |theta_fused - theta_64| <= 4 |theta_torch32 - theta_64|; both Adam clocks stand at 8."""
    import torch
    from cassierl_amd import trpo as T
    algo = _make(family, 32, batch_size=32 * 4, epochs=1, minibatch_size=16)
    assert algo.value_kind == "mlp" and algo.obs_dim == (45 if family == "cassie3d" else 26)
    d = algo.process(algo.collect())
    assert algo.last_gae_fused and algo.last_value_kind == "vf_grad" and set(d) >= {"vtarget", "v_old"}
    assert d["vtarget"].dtype == torch.float64 and torch.isfinite(d["vtarget"]).all() and torch.isfinite(d["adv"]).all()
    pol32, vf32 = algo.policy, algo.baseline
    theta0, vtheta0 = T.flat_params(pol32).clone(), T.flat_params(vf32).clone()
    gen0 = algo.gen_mb.get_state()
    res = {}
    for name in ("fused", "torch32", "torch64"):
        algo.adam_t, algo.adam_m, algo.adam_v = 0, None, None
        algo.value_adam_t, algo.value_adam_m, algo.value_adam_v = 0, None, None
        algo.gen_mb.set_state(gen0)
        algo.fused_grad = algo.fused_adam = algo.fused_value = name == "fused"
        if name == "torch64":
            algo.policy, algo.baseline = copy.deepcopy(pol32).double(), copy.deepcopy(vf32).double()
            T.set_flat_params(algo.policy, theta0.double()); T.set_flat_params(algo.baseline, vtheta0.double())
            st = algo.optimize({k: v.double() for k, v in d.items()})
        else:
            T.set_flat_params(pol32, theta0); T.set_flat_params(vf32, vtheta0)
            st = algo.optimize(d)
        assert algo.last_value_kind == ("vf_grad" if name == "fused" else "autograd") and algo.last_adam_fused == (name == "fused")
        assert st["minibatch_steps"] == 8 and algo.adam_t == 8 and algo.value_adam_t == 8
        res[name] = (T.flat_params(algo.policy).double().clone(), T.flat_params(algo.baseline).double().clone(), st)
    algo.policy, algo.baseline = pol32, vf32
    for which, i, start in (("policy", 0, theta0), ("value", 1, vtheta0)):
        t64 = res["torch64"][i]
        e_f, e_t, step = (res["fused"][i] - t64).norm().item(), (res["torch32"][i] - t64).norm().item(), (t64 - start.double()).norm().item()
        print("EDGES H %s %s: |theta_fused - theta_64| %.4g, |theta_torch32 - theta_64| %.4g, |step_64| %.4g" % (family, which, e_f, e_t, step))
        assert step > 0 and e_f <= 4.0 * e_t, (which, e_f, e_t)
    algo.env.close()
