"""PPO's learned value function: a tanh MLP V(s) in the `baseline` slot of PPO, trained by minibatch Adam steps beside the policy's.

There is no reference counterpart (ppo.py: PPO is the project's own algorithm): the torch statements in this module are the specification, the
kernels of csrc/tu_vf.hip evaluate them for the 128 x 128 network at 26 and 45 observations.

  network     Linear -> tanh -> Linear -> tanh -> Linear(1); parameters [W1, b1, W2, b2, W3, b3]; initialised as the policy's mean network
              (Xavier-uniform weights, zero biases).  predict(obs, t): V as float64 [n]; t is ignored, observations are not clipped.
  advantages  ppo.gae_advantages on values = V of every sample and last_value = V of the sampler's current observation, both predicted in the
              network's precision and promoted to float64 (CassieVfPredict, CassieVfGae); a cut is terminal, as for the linear baseline.
  target      y = adv + values, the lambda-return, with adv the GAE advantage BEFORE process() centres it; float64, handed to the update in the
              network's precision.  CassieVfGae evaluates the same number by the lambda-return's own recurrence
              y_t = r_t + gamma live_t ((1 - lambda) v_{t+1} + lambda y_{t+1}), y_T = last_value, which does not cancel where |values| is large.
  loss        of one minibatch of M samples (all ranks together):  value_loss = (1 / 2M) sum (V(s_i) - y_i)^2.   No value clipping.
  gradient    in closed form (value_grad_closed_form; CassieVfGrad evaluates it in one launch): the reverse pass of the network with the
              cotangent scale (V - y), scale = 1 / M.
  update      PPO.optimize: in every minibatch step, after the policy's Adam step and on the same rows: value gradient -> mean over ranks ->
              one Lasagne Adam step on the value network's flat vector with its own learning rate and its own (m, v, t).
  nothing is fitted in process(): fit() is a no-op and OnPolicy._baseline_kernels is None for this baseline (no Gram, no ridge solve).
"""
import ctypes as ct

import torch
from torch import nn

from ._lib import Kernels, available, ptr
from .baseline import tmatmul
from .policy import flat_grad, flat_params, set_flat_params


class MLPValueFunction(nn.Module):
    def __init__(self, obs_dim, hidden_sizes=(128, 128), dtype=torch.float32):
        super().__init__()
        layers, d = [], obs_dim
        for h in hidden_sizes:
            layers += [nn.Linear(d, h), nn.Tanh()]
            d = h
        layers.append(nn.Linear(d, 1))
        self.net = nn.Sequential(*layers)
        for m in self.net:
            if isinstance(m, nn.Linear):   # as GaussianMLPPolicy's mean network
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)
        self.to(dtype)

    @property
    def coeffs(self):
        """Always None: there is no regression.  A snapshot's "baseline" entry stays None, and a TRPO run that continues it starts its own
        linear baseline from nothing."""
        return None

    @property
    def hidden_sizes(self):
        return tuple(m.out_features for m in self.net if isinstance(m, nn.Linear))[:-1]

    def forward(self, obs):
        return self.net(obs).squeeze(-1)

    @torch.no_grad()
    def predict(self, obs, t=None):
        return self(obs.to(next(self.parameters()).dtype)).double()

    def fit(self, obs, t, returns):
        """Nothing is fitted per iteration: the network learns in PPO.optimize."""


def _linears(vf):
    """The three Linear layers of a two-hidden-layer tanh value network, else None."""
    lin = [m for m in vf.net if isinstance(m, nn.Linear)]
    ok = len(lin) == 3 and all(isinstance(m, (nn.Linear, nn.Tanh)) for m in vf.net) and lin[2].out_features == 1
    return lin if ok else None


def value_loss(vf, obs, y):
    """(1 / 2M) sum (V(s_i) - y_i)^2 over the M rows given, through autograd: any dtype, any device."""
    d = vf(obs) - y
    return 0.5 * (d * d).mean()


def value_grad_closed_form(vf, obs, y, scale=None):
    """The gradient of value_loss in closed form (what CassieVfGrad evaluates), flat in parameter order; scale = 1 / M (default: the rows given).
    AnalyticFisher._reverse's pass with the one-column cotangent scale (V - y)."""
    lin = _linears(vf)
    if lin is None:
        raise ValueError("value_grad_closed_form covers the two-hidden-layer tanh value network only")
    with torch.no_grad():
        scale = 1.0 / obs.shape[0] if scale is None else scale
        W2, W3 = lin[1].weight, lin[2].weight
        H1 = torch.tanh(torch.addmm(lin[0].bias, obs, lin[0].weight.T))
        H2 = torch.tanh(torch.addmm(lin[1].bias, H1, W2.T))
        V = torch.addmm(lin[2].bias, H2, W3.T)
        w = scale * (V - y.unsqueeze(-1))
        g2 = (w @ W3) * (1 - H2 * H2)
        g1 = (g2 @ W2) * (1 - H1 * H1)
        parts = [tmatmul(g1, obs), g1.sum(0), tmatmul(g2, H1), g2.sum(0), tmatmul(w, H2), w.sum(0)]
        return torch.cat([p.reshape(-1) for p in parts])


def aligned_value_params(vf):
    """flat_params(vf) in a buffer of its own: it starts on an allocation boundary, and with 128 hidden units every block behind W1 starts on a
    16-byte boundary (the kernels read b1, W2, b2, W3 as float4): pointers into it reach the kernels as they are."""
    return flat_params(vf).clone().contiguous()


class ValueKernels(Kernels):
    """V, GAE and the gradient of value_loss at the parameters in `theta` (a flat, 16-byte-aligned vector in parameter order that the caller updates in
    place: aligned_value_params): the 128 x 128 network on float32 CUDA tensors at 26 or 45 observations -> CassieVfPredict, CassieVfGae,
    CassieVfGrad, one launch each; CPU tensors, other shapes, fused=False or a library without the symbols -> the torch statements.  The kernel's
    row [gW1 | gb1 | gW2 | gb2 | gW3 | gb3] is the parameter order: no permutation.  `kind`: "vf_grad" or "autograd"."""

    ENTRY = {k: "CassieVf" + k for k in ("ParamCount", "Predict", "Gae", "GradRows", "Grad")}

    def __init__(self, vf, theta, fused=True):
        self.vf, self.theta, self.kind = vf, theta, "autograd"
        self.obs = self.target = None
        lin = _linears(vf)
        if not fused or lin is None or not theta.is_cuda or theta.dtype != torch.float32 or not available(*self.ENTRY.values()):
            return
        D, H = lin[0].in_features, 128
        if (lin[0].out_features, lin[1].out_features) != (H, H) or theta.data_ptr() % 16 != 0 or not theta.is_contiguous():
            return
        super().__init__(theta.device)
        NP = self.fn["ParamCount"](D)
        if NP == 0 or NP != theta.numel():
            return
        self.D, self.NP = D, NP
        self.off, o = [], 0
        for sz in (H * D, H, H * H, H, H, 1):
            self.off.append(o)
            o += sz
        self._bufs = {}
        self.kind = "vf_grad"

    def _net(self):
        base = self.theta.data_ptr()
        return [ct.c_void_p(base + 4 * o) for o in self.off]

    def set_batch(self, obs, target):
        """The batch the gradient's minibatches are rows of: obs [n, D], target [n] (the value target y in the network's precision)."""
        self.obs, self.target = obs.contiguous(), target.to(self.theta.dtype).contiguous()

    def _check(self, obs):
        if not (obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.dim() == 2 and obs.shape[1] == self.D):
            raise TypeError("CassieVf*: observations must be a contiguous float32 CUDA tensor [n, %d] (got %s %r)" % (self.D, obs.dtype, tuple(obs.shape)))

    def predict(self, obs):
        """V(obs) [n] at the parameters in theta, in the network's precision."""
        if self.kind == "vf_grad":
            self._check(obs)
            n = obs.shape[0]
            out = torch.empty(n, dtype=torch.float32, device=obs.device)
            self._call("Predict", ptr(obs), n, self.D, *self._net(), ptr(out))
            return out
        set_flat_params(self.vf, self.theta)
        with torch.no_grad():
            return self.vf(obs.to(self.theta.dtype))

    def gae(self, values, last_value, rew, cut, gamma, lam, fused=True):
        """(returns, adv, vtarget [T, n] float64, (sum adv, sum adv^2) or None) from values [T, n] and last_value [n] (None: zeros) in the network's
        precision: CassieVfGae, or ppo.gae_advantages on the promoted values."""
        if fused and self.kind == "vf_grad":
            T, n = rew.shape
            assert values.is_contiguous() and rew.is_contiguous() and cut.is_contiguous() and (last_value is None or last_value.is_contiguous())
            assert values.dtype == torch.float32 and values.shape == rew.shape and rew.dtype == torch.float64 and cut.dtype in (torch.bool, torch.uint8)
            assert last_value is None or (last_value.dtype == torch.float32 and last_value.numel() == n)
            returns, adv, vt = torch.empty_like(rew), torch.empty_like(rew), torch.empty_like(rew)
            partial = torch.empty(((n + 255) // 256, 2), dtype=torch.float64, device=rew.device)
            self._call("Gae", ptr(values), ptr(last_value), ptr(rew), ptr(cut), T, n, ct.c_double(gamma), ct.c_double(lam), ptr(returns), ptr(adv), ptr(vt),
                       ptr(partial))
            return returns, adv, vt, partial.sum(0)
        from .ppo import gae_advantages
        v64 = values.double()
        last = torch.zeros_like(v64[0]) if last_value is None else last_value.double()
        returns, adv = gae_advantages(rew, cut, v64, last, gamma, lam)
        return returns, adv, adv + v64, None

    def grad(self, idx=None, m=None, stats_out=None):
        """(gradient of the minibatch's value_loss with 1/M = 1/m, flat in parameter order; float64 sum of (V - y)^2 / 2 over the rows) for the rows
        idx [m] of the batch (None: rows 0 .. m - 1, m = the batch by default) at the parameters in theta.  stats_out: a float64 scalar view."""
        obs, y = self.obs, self.target
        m = (obs.shape[0] if idx is None else idx.numel()) if m is None else m
        if self.kind == "vf_grad":
            self._check(obs)
            n = obs.shape[0]
            assert y.dtype == torch.float32 and y.is_contiguous() and y.numel() == n
            rows = self.fn["GradRows"](m)
            if rows not in self._bufs:
                self._bufs[rows] = (torch.empty((rows, self.NP), dtype=torch.float32, device=obs.device), torch.empty(rows, dtype=torch.float64, device=obs.device))
            partial, stats = self._bufs[rows]
            if idx is not None:
                assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == m
            self._call("Grad", ptr(obs), n, self.D, *self._net(), ptr(idx), m, ptr(y), ct.c_float(1.0 / m), ptr(partial), ptr(stats))
            g = partial.sum(0)
            if stats_out is None:
                return g, stats.sum()
            torch.sum(stats, 0, out=stats_out)
            return g, stats_out
        vf = self.vf
        set_flat_params(vf, self.theta)
        sl = slice(0, m) if idx is None else idx
        loss = value_loss(vf, obs[sl], y[sl])
        g = flat_grad(loss, vf).detach()
        st = loss.detach().double() * m
        if stats_out is not None:
            stats_out.copy_(st)
            st = stats_out
        return g, st
