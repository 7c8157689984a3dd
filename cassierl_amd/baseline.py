"""rllab's LinearFeatureBaseline on the batch: the torch statements, the chunked reductions they need on tall-skinny matrices, and the HIP kernels
of csrc/tu_trpo_baseline.hip that evaluate them on the device batch (prediction, returns / advantages / GAE, the normal equations, the solve)."""
import ctypes as ct

import torch

from ._lib import Kernels
from .comm import all_sum_


def gram(X, y, chunk=2048):
    """(X'X, X'y) for a tall-skinny X [N, F].  One GEMM with K = N is pathological in rocBLAS (56 ms for 524 288 x 58 in
    FP64 on MI355X); a batch of K = `chunk` GEMMs summed afterwards does the same arithmetic in 0.2 ms."""
    Z = torch.cat([X, y.unsqueeze(-1)], dim=-1)
    n, f = Z.shape
    m = (n // chunk) * chunk
    G = torch.zeros((f, f), dtype=Z.dtype, device=Z.device)
    if m:
        Zc = Z[:m].view(n // chunk, chunk, f)
        G += torch.bmm(Zc.transpose(1, 2), Zc).sum(0)
    if m < n:
        G += Z[m:].T @ Z[m:]
    return G[:-1, :-1], G[:-1, -1]


def tmatmul(A, B, chunk=2048):
    """A' B for tall-skinny A [N, p], B [N, q] (a reduction over N): chunked for the same reason as gram()."""
    n = A.shape[0]
    m = (n // chunk) * chunk
    out = torch.zeros((A.shape[1], B.shape[1]), dtype=A.dtype, device=A.device)
    if m:
        out += torch.bmm(A[:m].view(n // chunk, chunk, -1).transpose(1, 2), B[:m].view(n // chunk, chunk, -1)).sum(0)
    if m < n:
        out += A[m:].T @ B[m:]
    return out


class LinearFeatureBaseline:
    """Ridge regression of the discounted return on [o, o^2, t, t^2, t^3, 1], o clipped to [-10, 10], t = step/100."""

    def __init__(self, reg_coeff=1e-5):
        self.coeffs, self.reg_coeff = None, reg_coeff

    @staticmethod
    def features(obs, t):
        o = obs.clamp(-10, 10)
        al = (t.to(obs.dtype) / 100.0).unsqueeze(-1)
        return torch.cat([o, o * o, al, al ** 2, al ** 3, torch.ones_like(al)], dim=-1)

    def fit(self, obs, t, returns):
        X = self.features(obs, t).double()
        y = returns.double()
        A, b = gram(X, y)
        self.fit_normal_equations(A, b)

    def fit_normal_equations(self, A, b, solver=None):
        """coeffs from this rank's X'X [F, F] and X'y [F] (summed over ranks here).  solver(A, b, reg): the same rule on the device."""
        A, b = all_sum_(A.contiguous(), "baseline_all_reduce"), all_sum_(b.contiguous(), "baseline_all_reduce")
        if solver is not None:
            self.coeffs = solver(A, b, self.reg_coeff)
            return
        reg = self.reg_coeff
        eye = torch.eye(A.shape[0], dtype=A.dtype, device=A.device)
        for _ in range(5):
            sol = torch.linalg.solve(A + reg * eye, b)
            if torch.isfinite(sol).all():
                break
            reg *= 10
        self.coeffs = sol

    def predict(self, obs, t):
        if self.coeffs is None:
            return torch.zeros(obs.shape[0], dtype=torch.float64, device=obs.device)
        return self.features(obs, t).double() @ self.coeffs


class BaselineKernels(Kernels):
    """LinearFeatureBaseline on the device batch as three HIP kernels (csrc/tu_trpo_baseline.hip, include/cassie_trpo.h): prediction,
    returns / advantages of the [T, n] batch in one pass, and the regression's normal equations on the FP64 matrix cores -- the feature
    matrix is never materialised.  CUDA float32 observations of a supported width only (ValueError otherwise: OnPolicy.process falls back to
    the torch expressions of LinearFeatureBaseline)."""

    ENTRY = {k: "CassieTrpo" + k for k in ("BaselineFeatures", "GramRows", "GramRowSize", "BaselinePredict", "ReturnsAdvantages", "Gae", "BaselineGram",
                                            "RidgeSolve")}

    def __init__(self, dev, obs_dim):
        if dev.type != "cuda":
            raise ValueError("BaselineKernels need a CUDA device")
        super().__init__(dev)
        self.D = obs_dim
        self.F = self.fn["BaselineFeatures"](obs_dim)
        if self.F == 0:
            raise ValueError("BaselineKernels: unsupported observation width %d" % obs_dim)
        rows, size = self.fn["GramRows"](), self.fn["GramRowSize"](obs_dim)
        self.gram_partial = torch.empty((rows, size), dtype=torch.float64, device=dev)
        # full symmetric matrix from the upper 16 x 16 blocks (r <= c, r-major, each row-major): one gather
        nb = ((self.F + 1) + 15) // 16
        order, k = {}, 0
        for r in range(nb):
            for c in range(r, nb):
                order[(r, c)] = k
                k += 1
        idx = torch.empty((16 * nb, 16 * nb), dtype=torch.int64)
        for I in range(16 * nb):
            for J in range(16 * nb):
                r, c, i, j = I // 16, J // 16, I % 16, J % 16
                idx[I, J] = order[(r, c)] * 256 + i * 16 + j if r <= c else order[(c, r)] * 256 + j * 16 + i
        self.idx = idx.reshape(-1).to(dev)
        self.nz = 16 * nb

    def predict(self, obs32, t, coeffs):
        m = obs32.shape[0]
        out = torch.empty(m, dtype=torch.float64, device=self.dev)
        self._call("BaselinePredict", self._p(obs32.contiguous()), self._p(t.contiguous()), m, self.D, self._p(coeffs.contiguous()), self._p(out))
        return out

    def _advantages(self, key, lam, obs_b, t_b, rew_b, cut_b, coeffs, last_value, gamma):
        """The one body of returns_advantages (lam = (): CassieTrpoReturnsAdvantages) and gae (lam = (lambda,): CassieTrpoGae)."""
        T, n = rew_b.shape
        assert obs_b.is_contiguous() and t_b.is_contiguous() and rew_b.is_contiguous() and cut_b.is_contiguous()
        assert obs_b.dtype == torch.float32 and t_b.dtype == torch.int64 and rew_b.dtype == torch.float64 and cut_b.dtype in (torch.bool, torch.uint8)
        returns, adv = torch.empty_like(rew_b), torch.empty_like(rew_b)
        partial = torch.empty(((n + 255) // 256, 2), dtype=torch.float64, device=self.dev)
        self._call(key, self._p(obs_b), self._p(t_b), self._p(rew_b), self._p(cut_b), T, n, self.D,
                   self._p(None if coeffs is None else coeffs.contiguous()), self._p(None if last_value is None else last_value.contiguous()),
                   ct.c_double(gamma), *[ct.c_double(x) for x in lam], self._p(returns), self._p(adv), self._p(partial))
        return returns, adv, partial.sum(0)

    def returns_advantages(self, obs_b, t_b, rew_b, cut_b, coeffs, last_value, gamma):
        """[T, n] batch -> returns [T, n], advantages [T, n] (float64) and (sum adv, sum adv^2) as a float64 pair on the device."""
        return self._advantages("ReturnsAdvantages", (), obs_b, t_b, rew_b, cut_b, coeffs, last_value, gamma)

    def gae(self, obs_b, t_b, rew_b, cut_b, coeffs, last_value, gamma, lam):
        """returns_advantages with GAE(lambda) advantages (CassieTrpoGae; cassierl_amd/ppo.py: gae_advantages is its torch statement)."""
        return self._advantages("Gae", (lam,), obs_b, t_b, rew_b, cut_b, coeffs, last_value, gamma)

    def gram(self, obs32, t, y):
        """(X'X [F, F], X'y [F]) of the baseline's features on m samples."""
        m = obs32.shape[0]
        assert obs32.is_contiguous() and t.is_contiguous() and y.is_contiguous() and y.dtype == torch.float64
        self._call("BaselineGram", self._p(obs32), self._p(t), self._p(y), m, self.D, self._p(self.gram_partial))
        G = self.gram_partial.sum(0)[self.idx].view(self.nz, self.nz)
        return G[:self.F, :self.F], G[:self.F, self.F]

    def ridge_solve(self, A, b, reg):
        """(A + reg I)^-1 b on the device (Cholesky, with fit's retry rule inside the kernel: no read-back)."""
        A, b = A.contiguous(), b.contiguous()
        x = torch.empty_like(b)
        self._call("RidgeSolve", self._p(A), self._p(b), A.shape[0], ct.c_double(reg), self._p(x))
        return x


def discounted_returns(rewards, dones, gamma, last_value=None):
    """rewards, dones: [T, N].  Return-to-go that restarts after a done (path boundary)."""
    T = rewards.shape[0]
    out = torch.zeros_like(rewards)
    run = torch.zeros_like(rewards[0]) if last_value is None else last_value.clone()
    for t in range(T - 1, -1, -1):
        run = rewards[t] + gamma * run * (~dones[t]).to(rewards.dtype)
        out[t] = run
    return out
