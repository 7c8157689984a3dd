"""Evolution strategy (OpenAI-ES style) over the batched environment: every environment runs its own antithetically perturbed copy of the policy
for a whole episode, nothing is stored per step, and the update is one weighted sum of noise vectors.

There is no reference counterpart (rllab ships the family as CEM / CMA-ES and no script of the reference uses it): the torch statements in this
module are the specification, the kernels of csrc/tu_es.hip (and, for the 128 x 128 policy's step, csrc/tu_es_wide.hip; for both widths at Cassie3d's
shape, 45 observations and 10 actions, csrc/tu_es3d.hip) evaluate them.

  parameters  theta = flat_params(policy.mean_net), the row [W1 | b1 | W2 | b2 | W3 | b3] (policy._MEAN_ORDER, the actor row of csrc/mlp32_tiles.h),
              P entries: 2118 for the shape (26, 6), 2151 for (26, 7), 1863 for (17, 7) at 32 x 32 hidden units; 20 742, 20 871 and 19 719 at
              128 x 128 (19 590 for (17, 6)); 2858 and 23 690 for Cassie3d's (45, 10).  log_std is never touched, so a TRPO run can load an ES snapshot and continue from it.
  noise       table = randn(table_size) float32 on the device from a generator seeded by table_seed (default 1 << 24 entries, 64 MB): regenerated
              from the seed on load, never written to a snapshot.
  population  n_envs (even) per rank; local environment i evaluates direction d = i >> 1 with sign s = +1 (i even) or -1 (i odd), direction d is
              eps_d = table[off_d : off_d + P].  The offsets of ALL ranks are drawn once per iteration, randint(0, table_size - P + 1, (M_global,)),
              from a generator seeded identically on every rank; a rank keeps its shard (TRPO's rule for the exploration noise: a run does not
              depend on how the environments are sharded).
  action      (es_actions_torch; CassieEsPolicyStep, CassieEsWidePolicyStep at width 128, CassieEs3dPolicyStep / CassieEs3dWidePolicyStep at 45 x 10)  w_i = theta + (s_i sigma) eps_(i >> 1);  mean_i = W3 tanh(W2 tanh(W1 obs_i + b1) + b2) + b3
              with the layers cut out of w_i;  act_i = alive_i ? mean_i : 0;  env_action_i = NormalizedActions(act_i): a dead environment gets
              the middle of the box.
  rollout     reset every environment, then up to max_path_length steps with (es_book_torch; CassieEsBook)
                fitness += alive ? rew : 0;  length += alive;  alive &= !done,
              stopped early when no environment is alive (polled every 50 steps with one scalar read-back, as sim_policy.py does).  Environments
              that finished keep being stepped (auto-reset is on) and are ignored.
  update      all fitness values gathered (rollout.gather_returns) and shaped -- centered ranks in [-0.5, 0.5] over all 2 M_global values
              (argsort(stable=True): ties by position), or fitness_shaping="zscore" --, per direction w_d = u(2d) - u(2d + 1),
                g = (1 / (2 M_global sigma)) sum_d w_d eps_d   (es_grad_torch; CassieEsGrad: each rank sums its shard, then all_sum_),
              descent direction -g + l2_coeff theta, one Lasagne Adam step (adam.adam_step_ / CassiePgAdam).

Defaults are OpenAI's: sigma 0.02, learning_rate 0.01, l2_coeff 0.005; max_path_length 1000.  The snapshot machinery and the gather are sampler.Sampler's,
shared with every other algorithm.  The 32 x 32 and the 128 x 128 policy in float32 on the GPU have kernels (the policy step is one kernel per width;
the bookkeeping, the gradient and Adam do not see the width); other hidden sizes, CPU tensors, float64 or a library without the symbols -- one
without the CassieEsWide* symbols at width 128 only, or the CassieEs3d* ones at 45 x 10 only -- take the torch statements.  On Cassie3d
(make_cassie_es(env="cassie3d")) nothing else changes: the perturbation is in the parameters, once per episode, and no noise is put on the actions.
"""
import ctypes as ct
import time

import torch

from ._lib import Kernels, available, ptr
from .adam import FlatAdam
from .comm import _world, all_sum_
from .policy import NormalizedActions, _two_layer_tanh, flat_params, set_flat_params
from .sampler import Sampler, broadcast_initial_policy, gaussian_policy_nets, make_cassie_algo


# --------------------------------------------------------------------------------------------- the torch statements
def param_count(obs_dim, hidden_sizes, act_dim):
    h1, h2 = hidden_sizes
    return h1 * obs_dim + h1 + h2 * h1 + h2 + act_dim * h2 + act_dim


def directions(table, offsets, n_params, dtype=None):
    """eps [M, n_params]: row d is table[offsets[d] : offsets[d] + n_params]."""
    eps = table[offsets.unsqueeze(1) + torch.arange(n_params, device=offsets.device)]
    return eps if dtype is None else eps.to(dtype)


def es_actions_torch(theta, table, offsets, sigma, obs, alive, act_map, hidden_sizes=(32, 32)):
    """The perturbed actions of the population (the torch statement of CassieEsPolicyStep): obs [n, D], offsets [n / 2], alive [n] (bool / uint8) or
    None.  Materialises the [n, P] weight matrix."""
    n, D = obs.shape
    h1, h2 = hidden_sizes
    A = (theta.numel() - (h1 * D + h1 + h2 * h1 + h2)) // (h2 + 1)
    dt = theta.dtype
    eps = directions(table, offsets, theta.numel(), dt).repeat_interleave(2, dim=0)
    sign = torch.tensor([1.0, -1.0], dtype=dt, device=theta.device).repeat(n // 2)
    w = theta + (sign * sigma).unsqueeze(1) * eps
    W1, b1, W2, b2, W3, b3 = torch.split(w, [h1 * D, h1, h2 * h1, h2, A * h2, A], dim=1)
    x = obs.to(dt).unsqueeze(2)
    x = torch.tanh(torch.baddbmm(b1.unsqueeze(2), W1.reshape(n, h1, D), x))
    x = torch.tanh(torch.baddbmm(b2.unsqueeze(2), W2.reshape(n, h2, h1), x))
    mean = torch.baddbmm(b3.unsqueeze(2), W3.reshape(n, A, h2), x).squeeze(2)
    if alive is not None:
        mean = torch.where(alive.bool().unsqueeze(1), mean, torch.zeros_like(mean))
    return act_map(mean)


def es_book_torch(rew, done, alive, fitness, length):
    """Bookkeeping of one Env.step, in place (the torch statement of CassieEsBook); alive is bool or uint8."""
    up = alive.bool()
    fitness += torch.where(up, rew, torch.zeros_like(rew))
    length += up.to(length.dtype)
    alive.copy_((up & ~done.bool()).to(alive.dtype))


def es_grad_torch(table, offsets, w, n_params, chunk=4096):
    """sum_d w_d eps_d in w's dtype (the torch statement of CassieEsGrad and of the caller's sum over its rows), `chunk` directions at a time."""
    g = torch.zeros(n_params, dtype=w.dtype, device=w.device)
    for i in range(0, offsets.numel(), chunk):
        g += w[i:i + chunk] @ directions(table, offsets[i:i + chunk], n_params, w.dtype)
    return g


def centered_ranks(f):
    """Ranks of f scaled to [-0.5, 0.5] (float64); equal values are ranked by position."""
    n = f.numel()
    order = torch.argsort(f, stable=True)
    ranks = torch.empty(n, dtype=torch.float64, device=f.device)
    ranks[order] = torch.arange(n, dtype=torch.float64, device=f.device)
    return ranks / (n - 1) - 0.5


def shape_fitness(f, how="centered_rank"):
    if how == "centered_rank":
        return centered_ranks(f)
    if how == "zscore":
        f = f.double()
        return (f - f.mean()) / (f.std(unbiased=False) + 1e-8)
    raise ValueError("fitness_shaping must be 'centered_rank' or 'zscore', got %r" % (how,))


def pair_weights(u):
    """w_d = u(2d) - u(2d + 1)."""
    return u[0::2] - u[1::2]


# --------------------------------------------------------------------------------------------- the kernel-call layer
class EsKernels(Kernels):
    """The library calls of ES on one noise table (csrc/tu_es.hip, csrc/tu_es_wide.hip, csrc/tu_es3d.hip).  ENTRY names the exported functions; every call goes through
    the dict `fn` (key -> function, looked up at call time, so a test can wrap its entries).  `hidden` = (128, 128) puts the Wide* functions under
    the keys ParamCount, PairsPerWorkgroup and PolicyStep, the shape (45, 10) the 3d* / 3dWide* ones (entry_for); an object looks up the symbols of
    its own width and shape only.  The kernels do not
    check offsets: set_directions does, on the host, with one read-back, and raises before anything is launched.  ValueError for an unsupported
    shape or width, or a table that is not a contiguous float32 vector."""

    ENTRY = {"ParamCount": "CassieEsParamCount", "PairsPerWorkgroup": "CassieEsPairsPerWorkgroup", "PolicyStep": "CassieEsPolicyStep", "Book": "CassieEsBook",
             "GradRows": "CassieEsGradRows", "Grad": "CassieEsGrad",
             "WideParamCount": "CassieEsWideParamCount", "WidePairsPerWorkgroup": "CassieEsWidePairsPerWorkgroup", "WidePolicyStep": "CassieEsWidePolicyStep",
             "3dParamCount": "CassieEs3dParamCount", "3dPairsPerWorkgroup": "CassieEs3dPairsPerWorkgroup", "3dPolicyStep": "CassieEs3dPolicyStep",
             "3dWideParamCount": "CassieEs3dWideParamCount", "3dWidePairsPerWorkgroup": "CassieEs3dWidePairsPerWorkgroup",
             "3dWidePolicyStep": "CassieEs3dWidePolicyStep"}
    SHAPE3D = (45, 10)   # Cassie3d's observations and actions: the shape of the 3d* entries

    @classmethod
    def entry_for(cls, hidden, shape=None):
        """key -> exported name for the policy width `hidden`, (32, 32) or (128, 128), and the shape (obs_dim, act_dim): (45, 10) takes the
        kernels of csrc/tu_es3d.hip, any other shape (or none) those of tu_es.hip / tu_es_wide.hip."""
        hidden = tuple(int(x) for x in hidden)
        if hidden not in ((32, 32), (128, 128)):
            raise ValueError("EsKernels: hidden sizes %r have no kernels (32 x 32 and 128 x 128 do)" % (hidden,))
        entry = {k: v for k, v in cls.ENTRY.items() if not k.startswith(("Wide", "3d"))}
        prefix = ("3d" if shape is not None and tuple(int(x) for x in shape) == cls.SHAPE3D else "") + ("Wide" if hidden == (128, 128) else "")
        if prefix:
            entry.update({k: cls.ENTRY[prefix + k] for k in ("ParamCount", "PairsPerWorkgroup", "PolicyStep")})
        return entry

    def __init__(self, table, n_envs, obs_dim, act_dim, low=None, high=None, hidden=(32, 32)):
        super().__init__(table.device, entry=self.entry_for(hidden, (obs_dim, act_dim)))
        self.hidden = tuple(int(x) for x in hidden)
        self.D, self.A, self.n = int(obs_dim), int(act_dim), int(n_envs)
        self.step_kind = ("es3d" if (self.D, self.A) == self.SHAPE3D else "es") + ("_wide_step" if self.hidden == (128, 128) else "_step")
        self.P = self.fn["ParamCount"](self.D, self.A)
        if self.P == 0:
            raise ValueError("EsKernels: unsupported policy shape %d -> %d" % (self.D, self.A))
        if self.n <= 0 or self.n % 2:
            raise ValueError("EsKernels: the number of environments must be positive and even, got %d" % self.n)
        if table.dtype != torch.float32 or table.dim() != 1 or not table.is_contiguous() or table.numel() < self.P:
            raise ValueError("EsKernels: the table must be a contiguous float32 vector of at least %d entries" % self.P)
        self.table = table
        self.low, self.high = low, high
        self.offsets, self._dir_np = None, 0
        self._partial = {}
        self.env_actions = None

    def set_directions(self, offsets, n_params=None):
        """The directions of the calls that follow: offsets [n_envs / 2] int64, contiguous, on the table's device, every one in
        [0, table_len - n_params] (n_params: P by default; grad() takes any width).  One read-back; ValueError before anything is launched."""
        n_params = self.P if n_params is None else int(n_params)
        if n_params < 1 or n_params > self.table.numel():
            raise ValueError("EsKernels: n_params %d outside [1, %d]" % (n_params, self.table.numel()))
        if not torch.is_tensor(offsets) or offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous():
            raise ValueError("EsKernels: the offsets must be a contiguous int64 vector")
        if offsets.numel() != self.n // 2:
            raise ValueError("EsKernels: %d offsets for %d environments (one per pair: %d)" % (offsets.numel(), self.n, self.n // 2))
        if offsets.device != self.dev:
            raise ValueError("EsKernels: the offsets are on %s, the table on %s" % (offsets.device, self.dev))
        lo, hi = torch.stack([offsets.min(), offsets.max()]).tolist()
        top = self.table.numel() - n_params
        if lo < 0 or hi > top:
            raise ValueError("EsKernels: offsets must lie in [0, %d], got [%d, %d]" % (top, lo, hi))
        self.offsets, self._dir_np = offsets, n_params

    def policy_step(self, obs, theta, sigma, alive=None, out=None):
        """env_actions [n, act_dim] float64 of the population at obs [n, obs_dim] float64 (CassieEsPolicyStep or CassieEsWidePolicyStep); alive
        uint8 [n] or None.  (At 45 x 10: CassieEs3dPolicyStep or CassieEs3dWidePolicyStep.)"""
        if self.offsets is None or self._dir_np != self.P:
            raise ValueError("EsKernels.policy_step: set_directions first")
        if obs.dtype != torch.float64 or not obs.is_contiguous() or obs.shape != (self.n, self.D) or obs.device != self.dev:
            raise TypeError("CassieEsPolicyStep: observations must be a contiguous float64 tensor [%d, %d] on %s" % (self.n, self.D, self.dev))
        if theta.dtype != torch.float32 or not theta.is_contiguous() or theta.numel() != self.P or theta.device != self.dev:
            raise TypeError("CassieEsPolicyStep: theta must be a contiguous float32 vector of %d entries" % self.P)
        if alive is not None and (alive.dtype != torch.uint8 or not alive.is_contiguous() or alive.numel() != self.n):
            raise TypeError("CassieEsPolicyStep: alive must be a contiguous uint8 vector of %d entries" % self.n)
        for b in (self.low, self.high):
            if b is None or b.dtype != torch.float64 or not b.is_contiguous() or b.numel() != self.A or b.device != self.dev:
                raise TypeError("CassieEsPolicyStep: the action bounds must be contiguous float64 vectors of %d entries" % self.A)
        if out is None:
            if self.env_actions is None:
                self.env_actions = torch.empty((self.n, self.A), dtype=torch.float64, device=self.dev)
            out = self.env_actions
        assert out.dtype == torch.float64 and out.is_contiguous() and out.shape == (self.n, self.A)
        P = ptr
        self._call("PolicyStep", P(obs), self.n, self.D, self.A, P(theta), P(self.table), ct.c_longlong(self.table.numel()), P(self.offsets), ct.c_float(sigma),
                   P(alive), P(self.low), P(self.high), P(out))
        return out

    def book(self, rew, done, alive, fitness, length):
        """es_book_torch in one launch (CassieEsBook), on as many environments as rew has."""
        n = rew.numel()
        for t, dt in ((rew, torch.float64), (done, torch.uint8), (alive, torch.uint8), (fitness, torch.float64), (length, torch.int64)):
            if t.dtype != dt or not t.is_contiguous() or t.numel() != n or t.device != self.dev:
                raise TypeError("CassieEsBook: contiguous rew / fitness float64, done / alive uint8, length int64 of %d entries on %s" % (n, self.dev))
        P = ptr
        self._call("Book", P(rew), P(done), n, P(alive), P(fitness), P(length))

    def grad(self, w):
        """sum_d w_d table[off_d : off_d + n_params] as float32 [n_params] (CassieEsGrad + the sum over its rows), n_params as given to set_directions."""
        if self.offsets is None:
            raise ValueError("EsKernels.grad: set_directions first")
        m, k = self.offsets.numel(), self._dir_np
        if w.dtype != torch.float32 or not w.is_contiguous() or w.numel() != m or w.device != self.dev:
            raise TypeError("CassieEsGrad: the weights must be a contiguous float32 vector of %d entries" % m)
        if (m, k) not in self._partial:
            self._partial[m, k] = torch.empty((self.fn["GradRows"](m), k), dtype=torch.float32, device=self.dev)
        partial = self._partial[m, k]
        P = ptr
        self._call("Grad", P(self.table), ct.c_longlong(self.table.numel()), P(self.offsets), P(w), m, k, P(partial))
        return partial.sum(0)


def make_table(size, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return torch.randn(int(size), dtype=torch.float32, device=device, generator=g)


# --------------------------------------------------------------------------------------------- ES
class ES(FlatAdam, Sampler):
    """ES on Sampler's snapshot machinery and gather; the baseline the constructor takes (the on-policy family's signature) is unused.  Switches (attributes, default True) that tests set to force the torch
    statements: fused_policy_step (CassieEsPolicyStep), fused_book (CassieEsBook), fused_grad (CassieEsGrad), fused_adam (CassiePgAdam).
    last_policy_step_kind ("es_step" / "es_wide_step" at width 128, "es3d_step" / "es3d_wide_step" on Cassie3d, or "torch"), last_book_fused, last_grad_kind ("es_grad" / "torch") and last_adam_fused say what ran."""
    ALGO = "es"
    CASSIE3D = True   # make_cassie_es(env="cassie3d"): csrc/tu_es3d.hip

    def __init__(self, env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, sigma=0.02, learning_rate=0.01, l2_coeff=0.005, max_path_length=1000,
                 table_size=1 << 24, table_seed=None, fitness_shaping="centered_rank", beta1=0.9, beta2=0.999, epsilon=1e-8, seed=1, env_reset_masked=None,
                 env_id0=None):
        if n_envs <= 0 or n_envs % 2:
            raise ValueError("ES: n_envs must be positive and even (two environments per direction), got %d" % n_envs)
        super().__init__(env_step, env_reset, policy, n_envs, obs_dim, act_map, batch_size=n_envs * _world(), max_path_length=max_path_length, seed=seed,
                         env_reset_masked=env_reset_masked, env_id0=env_id0)
        self.baseline = baseline   # (never fitted, never written: the snapshot's "baseline" entry is None)
        if self.env_id0 % 2:
            raise ValueError("ES: a shard must start on an even environment id, got %d" % self.env_id0)
        shape_fitness(torch.zeros(2), fitness_shaping)
        self._adam_init(float(learning_rate), beta1, beta2, epsilon)
        self.sigma, self.l2_coeff, self.fitness_shaping = float(sigma), float(l2_coeff), fitness_shaping
        self.n_params = sum(p.numel() for p in policy.mean_net.parameters())
        self.table_size, self.table_seed = int(table_size), int(seed * 1000003 + 15485863 if table_seed is None else table_seed)
        if self.table_size < self.n_params:
            raise ValueError("ES: table_size %d is smaller than the %d parameters" % (self.table_size, self.n_params))
        dev = next(policy.parameters()).device
        self.table = make_table(self.table_size, self.table_seed, dev)
        self.gen_off = torch.Generator(device=dev)   # the offsets of ALL ranks: the same seed on every rank
        self.gen_off.manual_seed(seed * 1000003 + 32452843)
        self.offsets = None
        self._ek = None
        self.last_policy_step_kind = self.last_grad_kind = self.last_book_fused = None

    def _kernels(self):
        """EsKernels for this run when they apply -- CUDA, a float32 two-layer tanh policy with 32 x 32 or 128 x 128 hidden units of a supported shape,
        rllab's normalize() action map with float64 bounds -- else None (the torch statements)."""
        if self._ek is not None:
            return self._ek or None
        self._ek = False
        p = next(self.policy.parameters())
        lin = _two_layer_tanh(self.policy)
        if p.device.type != "cuda" or p.dtype != torch.float32 or lin is None or self.hidden_sizes not in ((32, 32), (128, 128)) or not isinstance(self.act_map, NormalizedActions):
            return None
        low, high = self.act_map.low, self.act_map.high
        A = lin[2].out_features
        if lin[0].in_features != self.obs_dim or not all(t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == A for t in (low, high)):
            return None
        # no library, one without the symbols or an unsupported shape: the torch statements.  Anything else EsKernels objects to is a mistake and raises.
        entry = EsKernels.entry_for(self.hidden_sizes, (self.obs_dim, A))   # (the symbols of this width and shape only: a library without the wide ones still serves 32 x 32)
        if not available(*entry.values()) or Kernels(p.device, entry={"ParamCount": entry["ParamCount"]}).fn["ParamCount"](self.obs_dim, A) == 0:
            return None
        self._ek = None   # (a refusal below is raised again by the next call, not remembered as 'torch')
        self._ek = EsKernels(self.table, self.n_envs, self.obs_dim, A, low, high, hidden=self.hidden_sizes)
        return self._ek

    def draw_directions(self):
        """This iteration's offsets: all M_global drawn on every rank, this rank's shard kept (and checked: one read-back)."""
        m_global, m = self.n_envs_global // 2, self.n_envs // 2
        dev = self.table.device
        off = torch.randint(0, self.table_size - self.n_params + 1, (m_global,), generator=self.gen_off, device=dev, dtype=torch.int64)
        d0 = self.env_id0 // 2
        self.offsets = off[d0:d0 + m].contiguous()
        ek = self._kernels()
        if ek is not None:
            ek.set_directions(self.offsets)
        return self.offsets

    # ---- one episode of every environment; nothing is stored per step
    @torch.no_grad()
    def collect(self):
        if self.offsets is None:
            self.draw_directions()
        theta = flat_params(self.policy.mean_net).contiguous()
        dev, n = theta.device, self.n_envs
        ek = self._kernels()
        obs = self.env_reset()
        fitness = torch.zeros(n, dtype=torch.float64, device=dev)
        length = torch.zeros(n, dtype=torch.int64, device=dev)
        alive = torch.ones(n, dtype=torch.uint8, device=dev)
        step_fused = ek is not None and getattr(self, "fused_policy_step", True)
        book_fused = ek is not None and getattr(self, "fused_book", True)
        self.last_policy_step_kind, self.last_book_fused = ek.step_kind if step_fused else "torch", False
        for t in range(self.max_path_length):
            if step_fused:
                actions = ek.policy_step(obs, theta, self.sigma, alive)
            else:
                actions = es_actions_torch(theta, self.table, self.offsets, self.sigma, obs, alive, self.act_map, self.hidden_sizes)
            obs, rew, done = self.env_step(actions)
            if book_fused and rew.dtype == torch.float64 and done.dtype == torch.uint8:
                ek.book(rew, done, alive, fitness, length)
                self.last_book_fused = True
            else:
                es_book_torch(rew, done, alive, fitness, length)
            if t % 50 == 49 and not bool(alive.any()):   # the one scalar read-back per 50 steps
                break
        return dict(fitness=fitness, length=length, alive=alive)

    def local_gradient_sum(self, w):
        """sum over this rank's directions of w_d eps_d, in theta's dtype."""
        ek = self._kernels()
        dt = next(self.policy.parameters()).dtype
        if ek is not None and getattr(self, "fused_grad", True):
            self.last_grad_kind = "es_grad"
            return ek.grad(w.to(torch.float32).contiguous())
        self.last_grad_kind = "torch"
        return es_grad_torch(self.table, self.offsets, w.to(dt), self.n_params)

    @torch.no_grad()
    def update(self, all_fitness):
        """One ES step from the fitness of ALL environments of the job, in global environment order.  Returns (gradient norm, step norm) on the device."""
        net = self.policy.mean_net
        theta = flat_params(net).contiguous()
        m_global, d0, m = self.n_envs_global // 2, self.env_id0 // 2, self.n_envs // 2
        w = pair_weights(shape_fitness(all_fitness, self.fitness_shaping))[d0:d0 + m]
        g = all_sum_(self.local_gradient_sum(w).contiguous(), "gradient_all_reduce") * (1.0 / (2.0 * m_global * self.sigma))
        descent = self.l2_coeff * theta - g
        before = theta.clone()
        self.adam_step(theta, descent.contiguous())
        set_flat_params(net, theta)
        return g.double().norm(), (theta - before).double().norm()

    def train_iteration(self):
        timing = getattr(self, "timing", False)
        sync = torch.cuda.synchronize if next(self.policy.parameters()).is_cuda else (lambda: None)
        self.draw_directions()
        if timing:
            sync(); t0 = time.perf_counter()
        roll = self.collect()
        if timing:
            sync(); t1 = time.perf_counter()
        f = self._gather_returns(roll["fitness"])
        gnorm, snorm = self.update(f)
        steps = all_sum_(roll["length"].sum().double().reshape(1), "stats_all_reduce")[0]
        vals = torch.stack([steps, f.mean(), f.max(), f.min(), gnorm, snorm]).tolist()   # one read-back
        stats = dict(itr=self.itr, env_steps=int(vals[0]), episodes=int(f.numel()), avg_return=vals[1], max_return=vals[2], min_return=vals[3],
                     avg_path_length=vals[0] / f.numel(), grad_norm=vals[4], step_norm=vals[5], gathered=int(f.numel()))
        if timing:
            sync(); t2 = time.perf_counter()
            stats.update(seconds_rollout=t1 - t0, seconds_update=t2 - t1)
        self.itr += 1
        return stats

    # ---- snapshot: Sampler's, plus the algorithm, the policy shape, the hyper-parameters, the Adam state, the table's seed and size (never the
    # table) and the offset generator
    def _snapshot_fields(self):
        return dict(super()._snapshot_fields(), sigma=self.sigma, learning_rate=self.learning_rate, l2_coeff=self.l2_coeff, fitness_shaping=self.fitness_shaping,
                    max_path_length=int(self.max_path_length), **self._adam_snapshot(), table_seed=int(self.table_seed), table_size=int(self.table_size),
                    gen_off_state=self.gen_off.get_state())

    def _load_fields(self, ck):
        super()._load_fields(ck)
        self._adam_load(ck)
        dev = next(self.policy.parameters()).device
        seed, size = int(ck.get("table_seed", self.table_seed)), int(ck.get("table_size", self.table_size))
        if (seed, size) != (self.table_seed, self.table_size):   # the table is part of the run: regenerated from the snapshot's seed
            self.table_seed, self.table_size = seed, size
            self.table = make_table(size, seed, dev)
            self._ek = None
        if ck.get("gen_off_state") is not None:
            self.gen_off.set_state(ck["gen_off_state"])
        self.offsets = None


def make_cassie_es(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, hidden_sizes=(32, 32), terrain=None, sync_policy=True, **kw):
    """ES on the batched MI355X environment; the counterpart of ppo.make_cassie_ppo (same env and sync_policy rules; env="cassie3d", control_mode
    "PD" / "Torque", kp, kd: Cassie3dVecEnv, sampler.make_cassie_algo).  With a terrain library both
    environments of a pair stand on the same field (ids drawn over env_ids // 2): otherwise the antithetic difference would measure the ground,
    not the perturbation."""
    return make_cassie_algo(ES, gaussian_policy_nets(hidden_sizes, 1.0), broadcast_initial_policy, n_envs, kind, control_mode, device, trajectory, seed, terrain,
                            sync_policy, terrain_ids=lambda ids: ids // 2, **kw)
