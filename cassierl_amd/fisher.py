"""Fisher-vector products of the Gaussian tanh-MLP policy and the conjugate gradient that uses them: the closed form in torch operations
(AnalyticFisher), as one launch per product (FusedFisher for 32 x 32 hidden units, csrc/tu_trpo.hip; PgFisher for 128 x 128, csrc/tu_pg_trpo.hip).
The same objects give J' w, the policy gradient of VPG and TRPO."""
import ctypes as ct

import torch

from ._lib import Kernels
from .baseline import tmatmul
from .comm import all_mean_
from .policy import _MEAN_ORDER, _two_layer_tanh


def conjugate_gradient(Avp, b, iters=10, tol=1e-10):
    """rllab/misc/krylov.py:cg -- including its early exit on the residual, but WITHOUT asking the device for it: once
    r.r < tol the step length is zero from then on (x and r stay what they were at the break), so no iteration waits for a
    host-side comparison (r04: ten synchronisations per update were most of what the CG loop cost around its products)."""
    x = torch.zeros_like(b)
    r, p = b.clone(), b.clone()
    rr = r @ r
    zero = torch.zeros((), dtype=b.dtype, device=b.device)
    running = torch.ones((), dtype=torch.bool, device=b.device)
    for _ in range(iters):
        Ap = Avp(p)
        alpha = torch.where(running, rr / (p @ Ap), zero)
        x.addcmul_(alpha, p)
        r.addcmul_(alpha, Ap, value=-1.0)
        rr_new = r @ r
        running = running & (rr_new >= tol)
        p = torch.addcmul(r, torch.where(running, rr_new / rr, zero), p)   # (stopped: p = r, finite whatever rr is)
        rr = rr_new
    return x


class AnalyticFisher:
    """Fisher-vector products of the Gaussian tanh-MLP policy in closed form (what rllab's `hvp_approach` gets by double
    backprop through mean-KL): F v = (1/N) J' S J v for the mean network (J = d mean / d theta by forward mode, S the
    precision of the old Gaussian) plus a diagonal block for log_std.  Activations of the OLD policy are computed once per
    TRPO update; a product is then ~8 GEMMs and a handful of element-wise kernels instead of ~100 autograd kernels."""
    kind = "analytic"

    def __init__(self, policy, obs, eps=1e-8):
        lin = _two_layer_tanh(policy)
        if lin is None:
            raise ValueError("AnalyticFisher covers the two-hidden-layer tanh policy of trpo_cassie.py only")
        self.names = [n for n, _ in policy.named_parameters()]
        self.shapes = [tuple(p.shape) for p in policy.parameters()]
        with torch.no_grad():
            self.W = [l.weight.detach().clone() for l in lin]
            self.X = obs
            self.H1 = torch.tanh(torch.addmm(lin[0].bias, obs, self.W[0].T))
            self.H2 = torch.tanh(torch.addmm(lin[1].bias, self.H1, self.W[1].T))
            self.D1, self.D2 = 1 - self.H1 * self.H1, 1 - self.H2 * self.H2
            var = (2 * policy.log_std.detach()).exp()
            self.prec = 2.0 / (2.0 * var + eps)                                   # d2 KL / d mean^2 (with kl()'s epsilon)
            self.h_ls = 4.0 * var * (2.0 * var - eps) / (2.0 * var + eps) ** 2     # d2 KL / d log_std^2
            self.n = obs.shape[0]

    @torch.no_grad()
    def __call__(self, v):
        parts, i = {}, 0
        for n, shp in zip(self.names, self.shapes):
            k = int(torch.tensor(shp).prod()) if len(shp) else 1
            parts[n] = v[i:i + k].view(shp)
            i += k
        dW1, db1 = parts["mean_net.0.weight"], parts["mean_net.0.bias"]
        dW2, db2 = parts["mean_net.2.weight"], parts["mean_net.2.bias"]
        dW3, db3 = parts["mean_net.4.weight"], parts["mean_net.4.bias"]
        X, H1, H2, D1, D2 = self.X, self.H1, self.H2, self.D1, self.D2
        W1, W2, W3 = self.W
        # forward mode: directional derivative of the mean
        dH1 = D1 * torch.addmm(db1, X, dW1.T)
        dH2 = D2 * (torch.addmm(db2, dH1, W2.T) + H1 @ dW2.T)
        dmu = torch.addmm(db3, dH2, W3.T) + H2 @ dW3.T
        w = dmu * (self.prec / self.n)
        return self._reverse(w, self.h_ls * parts["log_std"])

    @torch.no_grad()
    def _reverse(self, w, log_std_part):
        """J' w (reverse mode through the cached activations) with `log_std_part` in the log_std slot, in flat parameter order."""
        X, H1, H2, D1, D2 = self.X, self.H1, self.H2, self.D1, self.D2
        W1, W2, W3 = self.W
        out = {"log_std": log_std_part}
        out["mean_net.4.weight"], out["mean_net.4.bias"] = tmatmul(w, H2), w.sum(0)
        g2 = (w @ W3) * D2
        out["mean_net.2.weight"], out["mean_net.2.bias"] = tmatmul(g2, H1), g2.sum(0)
        g1 = (g2 @ W2) * D1
        out["mean_net.0.weight"], out["mean_net.0.bias"] = tmatmul(g1, X), g1.sum(0)
        return torch.cat([out[n].reshape(-1) for n in self.names])

    @torch.no_grad()
    def vjp(self, w):
        """J' w for per-sample cotangents w [n, act_dim] on the mean; the log_std slot is zero."""
        return self._reverse(w, torch.zeros_like(self.h_ls))


class FusedFisher(Kernels):
    """The same Fisher-vector products as AnalyticFisher, each in ONE launch of the fused HIP kernel (csrc/tu_trpo.hip,
    include/cassie_trpo.h): forward mode along the direction, precision of the old Gaussian, reverse mode and the outer-product
    accumulation per wavefront; obs is the only per-sample tensor read.  `vjp(w)` gives J' w for per-sample cotangents (the policy
    gradient).  CUDA float32 policies of the supported shapes only (ValueError otherwise: the caller falls back to AnalyticFisher).
    PgFisher is the same object for the 128 x 128 policy: it swaps the entry points (ENTRY) and the hidden width."""
    kind, hidden = "trpo_fvp", 32
    ENTRY = dict(ParamCount="CassieTrpoParamCount", PartialRows="CassieTrpoPartialRows", SurrogateRows="CassieTrpoPartialRows", Fvp="CassieTrpoFvp",
                 Vjp="CassieTrpoVjp", Surrogate="CassieTrpoSurrogate", CgUpdate="CassieTrpoCgUpdate")

    def __init__(self, policy, obs, eps=1e-8):
        name, H = type(self).__name__, self.hidden
        lin = _two_layer_tanh(policy)
        if lin is None:
            raise ValueError("%s covers the two-hidden-layer tanh policy of trpo_cassie.py only" % name)
        if not obs.is_cuda or obs.dtype != torch.float32 or lin[0].out_features != H or lin[1].out_features != H:
            raise ValueError("%s needs a float32 CUDA batch and %d x %d hidden units" % (name, H, H))
        super().__init__(obs.device)
        self.D, self.A = lin[0].in_features, lin[2].out_features
        self.NP = self.fn["ParamCount"](self.D, self.A)
        if self.NP == 0:
            raise ValueError("%s: unsupported policy shape %d -> %d" % (name, self.D, self.A))
        self.obs = obs.contiguous()
        self.n = obs.shape[0]
        self.names = [n for n, _ in policy.named_parameters()]
        self.shapes = [tuple(p.shape) for p in policy.parameters()]
        self.order = _MEAN_ORDER
        with torch.no_grad():
            self.theta = {n: p.detach().clone().contiguous() for n, p in policy.named_parameters()}
            var = (2 * policy.log_std.detach()).exp()
            self.prec = (2.0 / (2.0 * var + eps)).to(torch.float32).contiguous()
            self.h_ls = 4.0 * var * (2.0 * var - eps) / (2.0 * var + eps) ** 2
        self.rows = self._partial_rows(self.n)
        self.partial = torch.empty((self.rows, self.NP), dtype=torch.float32, device=obs.device)
        # offsets of the kernel's row layout [gW1 | gb1 | gW2 | gb2 | gW3 | gb3]
        self.sizes = [H * self.D, H, H * H, H, self.A * H, self.A]

    def _partial_rows(self, n):
        return self.fn["PartialRows"](n)

    def _fvp(self, parts):
        """The mean network's F v for this rank's samples into self.partial (one row per wavefront)."""
        self._call("Fvp", self._p(self.obs), self.n, self.D, self.A, *self._ptrs(self.theta), *self._ptrs(parts), self._p(self.prec), ct.c_float(1.0 / self.n),
                   self._p(self.partial))

    def _split(self, v):
        parts, i = {}, 0
        for n, shp in zip(self.names, self.shapes):
            k = 1
            for d in shp:
                k *= d
            parts[n] = v[i:i + k]
            i += k
        return parts

    def _assemble(self, flat_mean, log_std_part):
        pieces = dict(zip(self.order, torch.split(flat_mean, self.sizes)))
        pieces["log_std"] = log_std_part
        return torch.cat([pieces[n].reshape(-1) for n in self.names])

    def _ptrs(self, d):
        return [self._p(d[n]) for n in self.order]

    @torch.no_grad()
    def __call__(self, v):
        v = v.to(torch.float32).contiguous()
        parts = self._split(v)
        self._fvp(parts)
        return self._assemble(self.partial.sum(0), self.h_ls * parts["log_std"])

    @torch.no_grad()
    def mean_product(self, v):
        """The mean network's part of F v for this rank's samples, [NP] float32 in the kernel's order (no log_std block, no damping)."""
        self._fvp(self._split(v))
        return self.partial.sum(0)

    @torch.no_grad()
    def conjugate_gradient(self, b, iters, reg, tol=1e-10):
        """conjugate_gradient(lambda v: all_mean_(self(v)) + reg * v, b, iters) with the vector work of an iteration as ONE launch
        (CassieTrpoCgUpdate): per iteration the product, the sum of its partial rows, the all-reduce over ranks, the update.  None if
        the parameter vector is not laid out as [.. log_std ..] around a contiguous mean-network block in the kernel's order."""
        names = self.names
        if "log_std" not in names or [n for n in names if n != "log_std"] != self.order or b.dtype != torch.float32 or not b.is_contiguous():
            return None
        k = names.index("log_std")
        if k not in (0, len(names) - 1):
            return None
        ls_off = 0 if k == 0 else self.NP
        n = b.numel()
        x = torch.zeros_like(b)
        r, p = b.clone(), b.clone()
        scal = torch.stack([r @ r, torch.ones((), dtype=b.dtype, device=b.device)]).contiguous()
        hls = self.h_ls.to(torch.float32).contiguous()
        P = self._p
        for _ in range(iters):
            apm = all_mean_(self.mean_product(p), "fvp_all_reduce")
            self._call("CgUpdate", n, ls_off, self.A, P(apm), P(hls), ct.c_float(reg), ct.c_float(tol), P(x), P(r), P(p), P(scal))
        return x

    @torch.no_grad()
    def vjp(self, w):
        """J' w for w [n, act_dim] float32 (cotangents on the mean); the log_std slot of the result is zero."""
        w = w.to(torch.float32).contiguous()
        self._call("Vjp", self._p(self.obs), self.n, self.D, self.A, *self._ptrs(self.theta), self._p(w), self._p(self.partial))
        return self._assemble(self.partial.sum(0), torch.zeros_like(self.theta["log_std"]))

    @torch.no_grad()
    def surrogate(self, policy, act, adv, old_mean, old_log_std):
        """(surrogate loss, mean KL) of `policy` AS IT IS NOW against the old Gaussian on this batch, in one launch (CassieTrpoSurrogate):
        the line search's evaluation.  old_log_std: the [act_dim] vector of the state-independent old log-std.  Two float64 scalars on the device."""
        live = dict(policy.named_parameters())
        if not hasattr(self, "_sur"):
            self._sur = torch.empty((self.fn["SurrogateRows"](self.n), 2), dtype=torch.float64, device=self.obs.device)
        P = self._p
        act, adv, old_mean = act.contiguous(), adv.to(torch.float32).contiguous(), old_mean.contiguous()
        old_ls = old_log_std.to(torch.float32).contiguous()
        self._call("Surrogate", P(self.obs), self.n, self.D, self.A, *[P(live[k].detach()) for k in self.order], P(live["log_std"].detach()), P(old_ls),
                   P(act), P(adv), P(old_mean), P(self._sur))
        s = self._sur.sum(0) / self.n
        return s[0], s[1]


class PgFisher(FusedFisher):
    """FusedFisher for the 128 x 128 policy (csrc/tu_pg_trpo.hip): the product is CassiePgFvp (forward mode into a [n, act_dim] cotangent,
    then CassiePgVjp), the CG step CassiePgCgUpdate, the line search CassiePgSurrogate and the gradient CassiePgVjp.  Same interface."""
    kind, hidden = "pg_fvp", 128
    ENTRY = {k: "CassiePg" + k for k in ("ParamCount", "PartialRows", "SurrogateRows", "Fvp", "Vjp", "Surrogate", "CgUpdate")}

    def _fvp(self, parts):
        if not hasattr(self, "_work"):
            self._work = torch.empty((self.n, self.A), dtype=torch.float32, device=self.obs.device)
        # the kernel reads db1, dW2, db2, dW3 as float4: in the flat parameter vector they sit behind log_std (act_dim floats), so the
        # direction's mean-network part is copied into a fresh buffer, where every block starts on a 16-byte boundary
        direction = dict(zip(self.order, torch.split(torch.cat([parts[k].reshape(-1) for k in self.order]), self.sizes)))
        self._call("Fvp", self._p(self.obs), self.n, self.D, self.A, *self._ptrs(self.theta), *self._ptrs(direction), self._p(self.prec),
                   ct.c_float(1.0 / self.n), self._p(self._work), self._p(self.partial))
