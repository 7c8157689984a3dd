"""PPO over the batched environment: the clipped surrogate, GAE(lambda) advantages and several epochs of minibatch Adam steps per rollout.

There is no reference counterpart (rllab's own PPO is the KL-penalised L-BFGS variant and no script of the reference uses it): the torch
statements in this module are the specification, the kernels of csrc/tu_ppo.hip evaluate them.

  advantages  per environment column of the [T][N] batch, backwards, float64 (gae_advantages; CassieTrpoGae):
                live = 1 - cut;  delta = r + gamma live V(s') - V(s);  adv = delta + gamma lambda live adv';  returns as TRPO's.
              V is the LinearFeatureBaseline; a path cut at max_path_length is terminal, as for TRPO and VPG.  Centring and the baseline
              fit are OnPolicy.process's.  With a value.MLPValueFunction in the baseline slot (make_cassie_ppo(value="mlp")) V is that network,
              nothing is fitted in process(), and every minibatch step is followed by one Adam step of the value network: value.py.
  loss        of one minibatch of M samples (all ranks together), ratio = exp(ll_new(a) - ll_old(a))  (ppo_loss):
                L = -(1/M) sum min(ratio adv, clip(ratio, 1 - eps, 1 + eps) adv) - entropy_coeff sum_a (log_std_a + 0.5 log(2 pi e))
  gradient    in closed form (clipped_grad_closed_form; CassieTrpoClipGrad / CassiePgClipGrad evaluate it in one launch):
                clipped = (adv > 0 and ratio > 1 + eps) or (adv < 0 and ratio < 1 - eps);  w = clipped ? 0 : ratio adv;  z = (a - mean) / std
                dL/dmean = -(1/M) w z / std;   dL/dlog_std = -(1/M) sum_s w (z^2 - 1) - entropy_coeff
  update      `epochs` passes over the rollout; per pass a fresh device permutation, minibatch j = rows perm[j m : (j + 1) m] with
              m = minibatch_size / world; per minibatch: gradient -> mean over ranks -> one Lasagne Adam step (adam.adam_step_ / CassiePgAdam),
              the Adam state kept across minibatches and iterations.  Nothing is read back inside the loop.  As for DDPG, the result depends
              on the number of ranks unless minibatch_size equals the batch (each rank permutes its own shard).

The sampler, exploration noise, baseline kernels and snapshot machinery are sampler.OnPolicy's, shared with TRPO and VPG.
"""
import ctypes as ct
import math

import torch
import torch.distributed as dist

from ._lib import Kernels, available, ptr
from .adam import FlatAdam, adam_step_, fused_adam_step_
from .comm import _world, all_mean_, all_sum_
from .fisher import AnalyticFisher
from .policy import GaussianMLPPolicy, _MEAN_ORDER, _two_layer_tanh, add_to_log_std_slot_, flat_grad, flat_params, hidden_sizes_of, set_flat_params
from .sampler import OnPolicy, broadcast_initial_policy, gaussian_policy_nets, make_cassie_algo
from .value import MLPValueFunction, ValueKernels, aligned_value_params


# --------------------------------------------------------------------------------------------- the torch statements
def gae_advantages(rew, cut, values, last_value, gamma, lam):
    """rew, cut, values: [T, N] (values = V of every sample of the batch); last_value [N] = V of the observation after the last step.
    Returns (returns, adv), both [T, N]: the torch statement of CassieTrpoGae."""
    T = rew.shape[0]
    returns, adv = torch.zeros_like(rew), torch.zeros_like(rew)
    run, v_next, a_next = last_value.clone(), last_value, torch.zeros_like(rew[0])
    for t in range(T - 1, -1, -1):
        live = (~cut[t].bool()).to(rew.dtype)
        run = rew[t] + gamma * run * live
        delta = rew[t] + gamma * live * v_next - values[t]
        a_next = delta + gamma * lam * live * a_next
        returns[t], adv[t] = run, a_next
        v_next = values[t]
    return returns, adv


def _old_ls_vector(old_log_std):
    return old_log_std if old_log_std.dim() == 1 else old_log_std[0]


def surrogate_terms(mean, log_std, act, adv, old_mean, old_log_std, clip):
    """Per sample: (min(ratio adv, clip(ratio) adv), ratio, clipped flag) of the Gaussian (mean, log_std [A]) against the old one."""
    ll_new = GaussianMLPPolicy.log_likelihood(act, mean, log_std)
    ll_old = GaussianMLPPolicy.log_likelihood(act, old_mean, old_log_std)
    ratio = (ll_new - ll_old).exp()
    sur = torch.minimum(ratio * adv, ratio.clamp(1.0 - clip, 1.0 + clip) * adv)
    clipped = ((adv > 0) & (ratio > 1.0 + clip)) | ((adv < 0) & (ratio < 1.0 - clip))
    return sur, ratio, clipped


def ppo_loss(policy, obs, act, adv, old_mean, old_log_std, clip, entropy_coeff):
    """The loss of one minibatch (its rows are the M samples) through autograd: any dtype, any device."""
    mean = policy.mean_net(obs)
    sur, _, _ = surrogate_terms(mean, policy.log_std, act, adv, old_mean, _old_ls_vector(old_log_std), clip)
    entropy = (policy.log_std + 0.5 * math.log(2.0 * math.pi * math.e)).sum()
    return -sur.mean() - entropy_coeff * entropy


def minibatch_stats(policy, obs, act, adv, old_mean, old_log_std, clip):
    """[3] float64 sums over the rows: -min(..) (the loss without the entropy term), KL(old || new), clipped samples."""
    with torch.no_grad():
        mean, ls_old = policy.mean_net(obs), _old_ls_vector(old_log_std)
        sur, _, clipped = surrogate_terms(mean, policy.log_std, act, adv, old_mean, ls_old, clip)
        kl = GaussianMLPPolicy.kl(old_mean, ls_old, mean, policy.log_std)
        return torch.stack([-sur.double().sum(), kl.double().sum(), clipped.double().sum()])


def clipped_grad_closed_form(policy, obs, act, adv, old_mean, old_log_std, clip, entropy_coeff, scale=None):
    """The gradient of ppo_loss in closed form (what the kernels evaluate), flat in parameter order; scale = 1 / M (default: the rows given).
    The mean network's part J' (dL/dmean) comes from AnalyticFisher's reverse pass at the policy's CURRENT parameters."""
    with torch.no_grad():
        scale = 1.0 / obs.shape[0] if scale is None else scale
        fisher = AnalyticFisher(policy, obs)
        mean = policy.mean_net(obs)
        _, ratio, clipped = surrogate_terms(mean, policy.log_std, act, adv, old_mean, _old_ls_vector(old_log_std), clip)
        w = torch.where(clipped, torch.zeros_like(ratio), ratio * adv).unsqueeze(-1)
        std = policy.log_std.detach().exp()
        z = (act - mean) / std
        g = fisher.vjp(-scale * w * z / std)
        return add_to_log_std_slot_(policy, g, -scale * (w * (z * z - 1.0)).sum(0) - entropy_coeff)


def aligned_flat_params(policy):
    """flat_params(policy) in a buffer whose mean-network part starts on a 16-byte boundary (the width-128 kernels read b1, W2, b2, W3 as
    float4, and log_std -- 6, 7 or, for Cassie3d, 10 floats -- sits in front of them in the flat vector): pointers into it reach the kernels as they are."""
    theta = flat_params(policy)
    first = 0
    for nm, p in policy.named_parameters():
        if nm == _MEAN_ORDER[0]:
            break
        first += p.numel()
    pad = (-first) % 4
    buf = torch.empty(pad + theta.numel(), dtype=theta.dtype, device=theta.device)
    out = buf[pad:]
    out.copy_(theta)
    return out


class ClipGradKernels(Kernels):
    """The gradient of ppo_loss on minibatches of one batch, at the parameters in `theta` (a flat vector in parameter order that the caller
    updates in place: aligned_flat_params): width 32 -> CassieTrpoClipGrad, width 128 -> CassiePgClipGrad (Cassie3d's 45 x 10: CassiePg3dClipGrad), one
    launch each; CPU tensors, other shapes, fused=False or a library without the symbols -> autograd of ppo_loss.  `kind`: "trpo_clip", "pg_clip",
    "pg3d_clip" or "autograd"."""

    def __init__(self, policy, theta, obs, act, adv, old_mean, old_log_std, clip, entropy_coeff, fused=True):
        self.policy, self.theta, self.clip, self.entropy_coeff = policy, theta, float(clip), float(entropy_coeff)
        self.obs, self.act, self.adv, self.old_mean = obs, act, adv, old_mean
        self.old_ls = _old_ls_vector(old_log_std).detach().clone().contiguous()
        self.kind = "autograd"
        lin = _two_layer_tanh(policy)
        if not fused or lin is None or not obs.is_cuda or obs.dtype != torch.float32 or theta.dtype != torch.float32:
            return
        hs = hidden_sizes_of(policy)
        D, A, H = lin[0].in_features, lin[2].out_features, hs[0]
        prefix = {(32, 32): "CassieTrpo", (128, 128): "CassiePg3d" if (D, A) == (45, 10) else "CassiePg"}.get(hs)   # (45 x 10: csrc/tu_pg3d.hip)
        if prefix is None or not available(prefix + "ClipGrad"):
            return
        super().__init__(obs.device, entry={k: prefix + k for k in ("ClipGrad", "ClipGradRows", "ParamCount")})
        NP = self.fn["ParamCount"](D, A)
        if NP == 0:
            return
        self.D, self.A, self.NP = D, A, NP
        self.obs, self.act, self.adv, self.old_mean = obs.contiguous(), act.contiguous(), adv.to(torch.float32).contiguous(), old_mean.contiguous()
        # where every parameter sits in theta, and the permutation from a partial row [gW1 | gb1 | gW2 | gb2 | gW3 | gb3 | g_log_std] to it
        sizes = dict(zip(_MEAN_ORDER, [H * D, H, H * H, H, A * H, A]))
        sizes["log_std"] = A
        korder, koff, o = _MEAN_ORDER + ["log_std"], {}, 0
        for nm in korder:
            koff[nm] = o
            o += sizes[nm]
        self.off, gather, o = {}, [], 0
        for nm, p in policy.named_parameters():
            if nm not in sizes or p.numel() != sizes[nm]:
                return
            self.off[nm] = o
            gather.append(torch.arange(koff[nm], koff[nm] + sizes[nm]))
            o += p.numel()
        if len(self.off) != len(korder):
            return
        dev = obs.device
        self.gather = torch.cat(gather).to(dev)
        self.ent = None
        if self.entropy_coeff != 0.0:
            self.ent = torch.zeros(o, dtype=torch.float32, device=dev)
            self.ent[self.off["log_std"]:self.off["log_std"] + A] = -self.entropy_coeff
        self._bufs = {}
        self.kind = {"CassieTrpo": "trpo_clip", "CassiePg": "pg_clip", "CassiePg3d": "pg3d_clip"}[prefix]

    def _rows(self, m):
        return self.fn["ClipGradRows"](m)

    def _fused(self, idx, m, scale, stats_out):
        n = self.obs.shape[0]
        rows = self._rows(m)
        if rows not in self._bufs:
            self._bufs[rows] = (torch.empty((rows, self.NP + self.A), dtype=torch.float32, device=self.obs.device),
                                torch.empty((rows, 3), dtype=torch.float64, device=self.obs.device))
        partial, stats = self._bufs[rows]
        P = ptr
        base = self.theta.data_ptr()
        W = [ct.c_void_p(base + 4 * self.off[k]) for k in _MEAN_ORDER]
        if idx is not None:
            assert idx.dtype == torch.int64 and idx.is_contiguous() and idx.numel() == m
        self._call("ClipGrad", P(self.obs), n, self.D, self.A, *W, P(idx), m, P(self.act), P(self.adv), P(self.old_mean), P(self.old_ls),
                   ct.c_void_p(base + 4 * self.off["log_std"]), ct.c_float(self.clip), ct.c_float(scale), P(partial), P(stats))
        g = partial.sum(0)[self.gather]
        if self.ent is not None:
            g += self.ent
        if stats_out is None:
            return g, stats.sum(0)
        torch.sum(stats, 0, out=stats_out)
        return g, stats_out

    def grad(self, idx=None, m=None, stats_out=None):
        """(gradient of the minibatch's loss with 1/M = 1/m, flat in parameter order; [3] float64 sums of minibatch_stats) for the rows
        idx [m] of the batch (None: rows 0 .. m - 1, m = the batch by default) at the parameters in theta."""
        m = (self.obs.shape[0] if idx is None else idx.numel()) if m is None else m
        if self.kind != "autograd":
            return self._fused(idx, m, 1.0 / m, stats_out)
        pol = self.policy
        set_flat_params(pol, self.theta)
        sl = slice(0, m) if idx is None else idx
        rows = [x[sl] for x in (self.obs, self.act, self.adv, self.old_mean)]
        g = flat_grad(ppo_loss(pol, *rows, self.old_ls, self.clip, self.entropy_coeff), pol).detach()
        st = minibatch_stats(pol, *rows, self.old_ls, self.clip)
        if stats_out is not None:
            stats_out.copy_(st)
            st = stats_out
        return g, st


# --------------------------------------------------------------------------------------------- PPO
class PPO(FlatAdam, OnPolicy):
    """PPO on OnPolicy's sampler and baseline.  Switches (attributes, default True) that tests set to force the torch path: fused_policy_step,
    fused_gae (CassieTrpoGae), fused_grad (ClipGradKernels), fused_adam (CassiePgAdam).  last_grad_kind says which gradient ran.
    baseline: a LinearFeatureBaseline, or a value.MLPValueFunction (recognised by type) -- then fused_value (ValueKernels) is one more switch, fused_gae
    and fused_adam cover CassieVfGae and the value network's Adam step, last_value_kind says which value path ran, and the value network has its own
    Adam state (value_adam_t, value_adam_m, value_adam_v) and step size value_learning_rate."""
    ALGO = "ppo"
    CASSIE3D = True   # make_cassie_ppo(..., env="cassie3d"): the 45 x 10 policy on csrc/tu_pg3d.hip and the baseline kernels at 45

    def __init__(self, env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size=10000, max_path_length=1000, discount=0.99,
                 learning_rate=3e-4, clip_range=0.2, gae_lambda=0.95, epochs=4, minibatch_size=None, entropy_coeff=0.0, beta1=0.9, beta2=0.999,
                 epsilon=1e-8, seed=1, env_reset_masked=None, env_id0=None, value_learning_rate=1e-3):
        super().__init__(env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size=batch_size, max_path_length=max_path_length,
                         discount=discount, seed=seed, env_reset_masked=env_reset_masked, env_id0=env_id0)
        self._adam_init(learning_rate, beta1, beta2, epsilon)
        self.value_learning_rate = value_learning_rate
        self.value_adam_t, self.value_adam_m, self.value_adam_v = 0, None, None
        self.last_value_kind = None
        self.clip_range, self.gae_lambda, self.epochs, self.entropy_coeff = clip_range, gae_lambda, int(epochs), entropy_coeff
        world, n_local = _world(), self.horizon * n_envs
        self.minibatch_size = n_local * world // 4 if minibatch_size is None else int(minibatch_size)
        self._check_minibatch(n_local)
        self.last_grad_kind = None
        dev = next(policy.parameters()).device
        rank = dist.get_rank() if dist.is_initialized() else 0
        self.gen_mb = torch.Generator(device=dev)   # the minibatch permutations of this rank's shard
        self.gen_mb.manual_seed(seed * 1000003 + 7919 * (rank + 1))

    def _check_minibatch(self, n_local):
        world = _world()
        if self.epochs < 1 or self.minibatch_size < 1 or self.minibatch_size % world != 0:
            raise ValueError("PPO: minibatch_size %d must be a positive multiple of the %d ranks (epochs %d >= 1)" % (self.minibatch_size, world, self.epochs))
        m = self.minibatch_size // world
        if n_local % m != 0:
            raise ValueError("PPO: a rank's %d samples per iteration are not a multiple of its minibatch of %d (minibatch_size %d over %d ranks)"
                             % (n_local, m, self.minibatch_size, world))
        return m

    def _advantages(self, bk, batch, obs, tt):
        """OnPolicy.process's hook with GAE(lambda) advantages: CassieTrpoGae, or gae_advantages on the values of the kernels or of the baseline."""
        T, N = batch["rew"].shape
        if self.value_kind == "mlp":
            return self._value_advantages(batch, obs)
        coeffs = self.baseline.coeffs
        self.last_gae_fused = bk is not None and getattr(self, "fused_gae", True)
        if self.last_gae_fused:
            last_v = None if coeffs is None else bk.predict(self.obs.to(obs.dtype), self.path_t, coeffs)
            return bk.gae(batch["obs"], batch["t"], batch["rew"], batch["done"], coeffs, last_v, self.discount, self.gae_lambda)
        if bk is not None and coeffs is not None:
            last_v, values = bk.predict(self.obs.to(obs.dtype), self.path_t, coeffs), bk.predict(obs, tt, coeffs).view(T, N)
        else:
            last_v, values = self.baseline.predict(self.obs.to(obs.dtype), self.path_t), self.baseline.predict(obs, tt).view(T, N)
        return (*gae_advantages(batch["rew"], batch["done"], values, last_v, self.discount, self.gae_lambda), None)

    @property
    def value_kind(self):
        return "mlp" if isinstance(self.baseline, MLPValueFunction) else "linear"

    def _load_baseline_coeffs(self, coeffs, dev):
        if self.value_kind == "linear":   # (the value network has no coefficients: its snapshot entry is None)
            super()._load_baseline_coeffs(coeffs, dev)

    def _value_advantages(self, batch, obs):
        """_advantages with the value network: V of every sample and of self.obs (ValueKernels.predict), GAE and the value target y = adv + V
        (ValueKernels.gae).  V_old and y go into process()'s dictionary for optimize()."""
        T, N = batch["rew"].shape
        vf = self.baseline
        vk = ValueKernels(vf, aligned_value_params(vf), fused=getattr(self, "fused_value", True))
        self.last_value_kind = vk.kind
        values = vk.predict(obs).view(T, N)
        last_v = vk.predict(self.obs.to(obs.dtype).contiguous())
        self.last_gae_fused = vk.kind == "vf_grad" and getattr(self, "fused_gae", True)
        returns, adv, y, sums = vk.gae(values, last_v, batch["rew"], batch["done"], self.discount, self.gae_lambda, fused=self.last_gae_fused)
        self._value_batch = dict(v_old=values.reshape(-1), vtarget=y.reshape(-1))
        return returns, adv, sums

    def _processed_extras(self):
        if self.value_kind != "mlp":
            return {}
        extras, self._value_batch = self._value_batch, None
        return extras

    def _value_adam_step(self, theta, g):
        """One Lasagne Adam step of the value network's flat vector: FlatAdam.adam_step's rule on the second state."""
        if self.value_adam_m is None:
            self.value_adam_m, self.value_adam_v = torch.zeros_like(theta), torch.zeros_like(theta)
        self.value_adam_t += 1
        fused = getattr(self, "fused_adam", True) and theta.is_cuda and theta.dtype == torch.float32
        (fused_adam_step_ if fused else adam_step_)(theta, g, self.value_adam_m, self.value_adam_v, self.value_adam_t, self.value_learning_rate, self.beta1,
                                                    self.beta2, self.epsilon)

    def optimize(self, d):
        pol = self.policy
        obs, act, adv, old_mean, old_lstd = d["obs"], d["act"], d["adv"], d["mean"], d["log_std"]
        n_local, world = obs.shape[0], _world()
        m = self._check_minibatch(n_local)
        nmb = n_local // m
        theta = aligned_flat_params(pol)
        ck = ClipGradKernels(pol, theta, obs, act, adv, old_mean, old_lstd, self.clip_range, self.entropy_coeff, fused=getattr(self, "fused_grad", True))
        self.last_grad_kind = ck.kind
        # per minibatch step (loss sum, KL sum, clipped samples, gradient norm), kept on the device and read once behind the loop
        acc = torch.zeros((self.epochs * nmb, 4), dtype=torch.float64, device=obs.device)
        vk = None
        if self.value_kind == "mlp":   # the value network's flat vector, updated in place beside the policy's
            vk = ValueKernels(self.baseline, aligned_value_params(self.baseline), fused=getattr(self, "fused_value", True))
            vk.set_batch(obs, d["vtarget"])
            self.last_value_kind = vk.kind
        vacc = None if vk is None else torch.zeros(self.epochs * nmb, dtype=torch.float64, device=obs.device)   # per minibatch step: sum (V - y)^2 / 2
        self.last_perms = []
        k = 0
        for _ in range(self.epochs):
            perm = torch.randperm(n_local, generator=self.gen_mb, device=obs.device)
            if getattr(self, "keep_perms", False):
                self.last_perms.append(perm)
            for j in range(nmb):
                idx = perm[j * m:(j + 1) * m]
                g, _ = ck.grad(idx, stats_out=acc[k, :3])
                g = all_mean_(g.contiguous(), "gradient_all_reduce")
                acc[k, 3] = torch.linalg.vector_norm(g, dtype=torch.float64)
                self.adam_step(theta, g.to(theta.dtype))
                if vk is not None:   # the value network's step on the same rows
                    gv, _ = vk.grad(idx, stats_out=vacc[k])
                    gv = all_mean_(gv.contiguous(), "gradient_all_reduce")
                    self._value_adam_step(vk.theta, gv.to(vk.theta.dtype))
                k += 1
        set_flat_params(pol, theta)
        M = float(m * world)
        ent = self.entropy_coeff * float(pol.log_std.numel()) * 0.5 * math.log(2.0 * math.pi * math.e)   # (the log_std part of the bonus is not logged)
        sums = all_sum_(acc[:, :3].contiguous(), "stats_all_reduce")
        if vk is not None:
            return self._stats_with_value(vk, d, sums, acc, vacc, M, ent)
        rows = torch.cat([sums, acc[:, 3:]], dim=1).tolist()   # the one read-back
        return self._policy_stats(rows, M, ent)

    @staticmethod
    def _policy_stats(rows, M, ent):
        return dict(loss_first=rows[0][0] / M - ent, loss_last=rows[-1][0] / M - ent, mean_kl=sum(r[1] for r in rows) / (M * len(rows)),
                    clip_frac=sum(r[2] for r in rows) / (M * len(rows)), grad_norm=sum(r[3] for r in rows) / len(rows), minibatch_steps=len(rows))

    def _stats_with_value(self, vk, d, sums, acc, vacc, M, ent):
        """optimize()'s statistics with the value network's: its parameters go back into the module, and the value losses and the sums of the
        explained variance 1 - Var(y - V_old) / Var(y) (over the batch, all ranks) join the one read-back."""
        set_flat_params(self.baseline, vk.theta)
        y = d["vtarget"].double()
        dv = y - d["v_old"].double()
        ev = torch.stack([dv.sum(), (dv * dv).sum(), y.sum(), (y * y).sum(), torch.tensor(float(y.numel()), dtype=torch.float64, device=y.device)])
        extra = all_sum_(torch.cat([vacc, ev]), "stats_all_reduce")
        K = acc.shape[0]
        flat = torch.cat([torch.cat([sums, acc[:, 3:]], dim=1).reshape(-1), extra]).tolist()   # the one read-back
        rows, vl, (s1, s2, t1, t2, cnt) = [flat[4 * i:4 * i + 4] for i in range(K)], flat[4 * K:5 * K], flat[5 * K:]
        var_d, var_y = s2 / cnt - (s1 / cnt) ** 2, t2 / cnt - (t1 / cnt) ** 2
        return dict(self._policy_stats(rows, M, ent), value_loss_first=vl[0] / M, value_loss_last=vl[-1] / M,
                    explained_variance=1.0 - var_d / var_y if var_y > 0.0 else float("nan"))

    # ---- snapshot: Sampler's, plus the algorithm, the policy shape, the hyper-parameters, the Adam state and the permutation generator
    def _snapshot_fields(self):
        f = dict(super()._snapshot_fields(), learning_rate=float(self.learning_rate), clip_range=float(self.clip_range), gae_lambda=float(self.gae_lambda),
                 epochs=int(self.epochs), minibatch_size=int(self.minibatch_size), entropy_coeff=float(self.entropy_coeff), **self._adam_snapshot(),
                 gen_mb_state=self.gen_mb.get_state())
        if self.value_kind == "mlp":   # (a snapshot without value_kind is a linear-baseline run's: its entries are what they were)
            cpu = lambda x: None if x is None else x.detach().cpu()
            f.update(value_kind="mlp", value_hidden=list(self.baseline.hidden_sizes), value_net=flat_params(self.baseline).detach().cpu(),
                     value_adam_t=int(self.value_adam_t), value_adam_m=cpu(self.value_adam_m), value_adam_v=cpu(self.value_adam_v),
                     value_learning_rate=float(self.value_learning_rate))
        return f

    def _load_fields(self, ck):
        super()._load_fields(ck)
        theirs, mine = ck.get("value_kind", "linear"), self.value_kind
        if theirs != mine:
            raise ValueError("PPO.load: the snapshot's value function is %r, this run's is %r" % (theirs, mine))
        if mine == "mlp" and tuple(ck["value_hidden"]) != self.baseline.hidden_sizes:
            raise ValueError("PPO.load: the snapshot's value network has hidden sizes %r, this run's has %r" % (tuple(ck["value_hidden"]), self.baseline.hidden_sizes))
        if mine == "mlp" and ck["value_net"].numel() != sum(p.numel() for p in self.baseline.parameters()):   # (another observation width: the other robot's)
            raise ValueError("PPO.load: the snapshot's value network has %d parameters, this run's has %d"
                             % (ck["value_net"].numel(), sum(p.numel() for p in self.baseline.parameters())))
        self._adam_load(ck)
        if ck.get("gen_mb_state") is not None:
            self.gen_mb.set_state(ck["gen_mb_state"])
        if mine == "mlp":
            dev = next(self.baseline.parameters()).device
            back = lambda x: None if x is None else x.to(dev)
            set_flat_params(self.baseline, ck["value_net"].to(dev))
            self.value_adam_t, self.value_adam_m, self.value_adam_v = int(ck["value_adam_t"]), back(ck["value_adam_m"]), back(ck["value_adam_v"])
            self.value_learning_rate = float(ck.get("value_learning_rate", self.value_learning_rate))


def broadcast_initial_networks(algo):
    """sampler.broadcast_initial_policy, and rank 0's value network is authoritative too (a collective: every rank must call it)."""
    broadcast_initial_policy(algo)
    if algo.value_kind == "mlp" and dist.is_initialized() and dist.get_world_size() > 1:
        theta = flat_params(algo.baseline)
        dist.broadcast(theta, 0)
        set_flat_params(algo.baseline, theta)


def policy_and_value_nets(hidden_sizes, init_std, value_hidden):
    """make_nets with a learned value function: the GaussianMLPPolicy, then -- right after it, so that the seed fixes both -- the MLPValueFunction."""
    def make(obs_dim, act_dim, dev):
        pol = GaussianMLPPolicy(obs_dim, act_dim, tuple(hidden_sizes), init_std=init_std).to(dev)
        return pol, MLPValueFunction(obs_dim, tuple(value_hidden)).to(dev)
    return make


def make_cassie_ppo(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, hidden_sizes=(128, 128), init_std=1.0, terrain=None,
                    sync_policy=True, value="linear", value_hidden=(128, 128), value_learning_rate=1e-3, **kw):
    """PPO on the batched MI355X environment; the counterpart of vpg.make_cassie_vpg (same env, terrain and sync_policy rules).  env="cassie3d"
    (with control_mode and, through **kw, kp / kd) runs it on Cassie3dVecEnv: sampler.make_cassie_algo.  value: "linear" (the LinearFeatureBaseline)
    or "mlp" (value.MLPValueFunction(obs_dim, value_hidden), trained with value_learning_rate)."""
    if value not in ("linear", "mlp"):   # (checked before any device is touched)
        raise ValueError("make_cassie_ppo: value must be 'linear' or 'mlp', got %r" % (value,))
    nets = gaussian_policy_nets(hidden_sizes, init_std) if value == "linear" else policy_and_value_nets(hidden_sizes, init_std, value_hidden)
    return make_cassie_algo(PPO, nets, broadcast_initial_networks, n_envs, kind, control_mode, device, trajectory, seed, terrain, sync_policy,
                            value_learning_rate=value_learning_rate, **kw)
