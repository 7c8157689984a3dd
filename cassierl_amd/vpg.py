"""Vanilla policy gradient over the batched environment: counterpart of rllab/envs/vpg_cassie.py:15-48.

  policy     GaussianMLPPolicy(hidden_sizes=(128, 128), init_std=1.0)            vpg_cassie.py
             (tanh hidden units, state-independent learned log-std)
  baseline   LinearFeatureBaseline                                               vpg_cassie.py
  algorithm  VPG: batch_size=10000, max_path_length=1000, n_itr=1000, discount=0.99   vpg_cassie.py
  env        normalize(Cassie2dEnv())                                            vpg_cassie.py

What rllab's VPG does with these [external: rllab's published source, not on this machine]:
  * the loss is -mean(logli(a | theta) * adv), with center_adv=True and gae_lambda=1 (BatchPolopt's defaults, as for TRPO);
  * the optimiser is FirstOrderOptimizer(batch_size=None, max_epochs=1) with lasagne.updates.adam and learning_rate=1e-3: ONE
    full-batch Adam step per iteration, the Adam state (m, v, t) kept across iterations;
  * Lasagne's Adam: t += 1; a = lr sqrt(1 - beta2^t) / (1 - beta1^t); m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2;
    theta -= a m / (sqrt(v) + eps), beta1 = 0.9, beta2 = 0.999, eps = 1e-8 -- eps outside the bias correction, which is NOT what
    torch.optim.Adam does (it adds eps to the bias-corrected sqrt(v_hat));
  * vpg_cassie.py's step_size=0.005 and use_gpu=True are swallowed by BatchPolopt's **kwargs: rllab's VPG never reads them.

The sampler, the exploration noise keyed by the global env id, the baseline kernels, advantage centring and the snapshot machinery
are TRPO's (cassierl_amd/trpo.py), unchanged.  The hot paths of the width-128 policy are HIP kernels (csrc/tu_pg.hip): the policy
step of the sampler, the policy gradient J' w, and the Adam step.
"""
import math

import torch
import torch.distributed as dist
from torch import nn

from . import terrain as terrain_lib
from .trpo import (TRPO, FusedFisher, GaussianMLPPolicy, LinearFeatureBaseline, NormalizedActions, _world, all_mean_, broadcast_initial_policy,
                   flat_grad, flat_params, hidden_sizes_of, set_flat_params)

_MEAN_ORDER = ["mean_net.0.weight", "mean_net.0.bias", "mean_net.2.weight", "mean_net.2.bias", "mean_net.4.weight", "mean_net.4.bias"]


def _two_layer_tanh(policy):
    lin = [m for m in policy.mean_net if isinstance(m, nn.Linear)]
    ok = len(lin) == 3 and all(isinstance(m, (nn.Linear, nn.Tanh)) for m in policy.mean_net)
    return lin if ok else None


def adam_step_(theta, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """Lasagne's Adam on flat tensors, in place; t is the step count after its increment (the torch statement of CassiePgAdam).  The betas
    are taken in the parameters' precision, as a float32 Lasagne graph holds them: for float32, 1 - 0.999f = 0.00099998713, not 0.001."""
    beta1, beta2 = (torch.tensor([beta1, beta2], dtype=theta.dtype).tolist())
    a = lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    m.mul_(beta1).add_(g, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
    theta.sub_(a * m / (v.sqrt() + eps))


def fused_adam_step_(theta, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """adam_step_ as one launch of CassiePgAdam (contiguous float32 CUDA tensors)."""
    import ctypes as ct
    from . import _lib
    L = _lib.load()
    for x in (theta, g, m, v):
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("CassiePgAdam needs contiguous float32 CUDA tensors")
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = L.CassiePgAdam(theta.numel(), P(g), P(m), P(v), P(theta), int(t), ct.c_float(lr), ct.c_float(beta1), ct.c_float(beta2), ct.c_float(eps),
                        ct.c_void_p(torch.cuda.current_stream(theta.device).cuda_stream))
    if rc != 0:
        raise RuntimeError("CassiePgAdam failed (%d)" % rc)


def closed_form_grad(policy, vjp, act, old_mean, old_lstd, adv):
    """Gradient of -mean(logli(a | theta) adv) at theta = theta_old in closed form (the sampler's batch is on-policy): with z = (a - mean) / std,
        d loss / d mean = -adv z / std / N,   d loss / d log_std = -sum_s adv (z^2 - 1) / N,
    and the mean network's part J' (d loss / d mean) from `vjp` (a flat vector in parameter order with a zero log_std slot)."""
    with torch.no_grad():
        std = old_lstd.exp()
        z = (act - old_mean) / std
        n_inv = 1.0 / act.shape[0]
        g = vjp(-(adv.unsqueeze(-1) * z / std) * n_inv)
        g_ls = -((adv.unsqueeze(-1) * (z * z - 1.0)).sum(0)) * n_inv
        i0 = 0
        for nm, p in policy.named_parameters():
            if nm == "log_std":
                g[i0:i0 + p.numel()] += g_ls.to(g.dtype)
            i0 += p.numel()
    return g


class PolicyGradKernels:
    """The policy gradient of one batch: width 32 -> CassieTrpoVjp (FusedFisher.vjp), width 128 -> CassiePgVjp, each in closed form;
    CPU, other shapes or fused=False -> autograd of the surrogate.  `kind` says which ("trpo_vjp", "pg_vjp" or "autograd")."""

    def __init__(self, policy, obs, fused=True):
        self.policy, self.obs = policy, obs
        self.kind, self._vjp = "autograd", None
        lin = _two_layer_tanh(policy)
        if not fused or lin is None or not obs.is_cuda or obs.dtype != torch.float32:
            return
        hs = hidden_sizes_of(policy)
        if hs == (32, 32):
            try:
                self._vjp = FusedFisher(policy, obs).vjp
                self.kind = "trpo_vjp"
            except (ValueError, OSError):
                pass
        elif hs == (128, 128):
            import ctypes as ct
            from . import _lib
            L = _lib.load()
            D, A = lin[0].in_features, lin[2].out_features
            NP = L.CassiePgParamCount(D, A)
            if NP == 0:
                return
            self.L, self.ct, self.D, self.A, self.NP = L, ct, D, A, NP
            self.obs = obs.contiguous()
            self.sizes = [128 * D, 128, 128 * 128, 128, A * 128, A]
            self._vjp = self._pg_vjp
            self.kind = "pg_vjp"

    def _pg_vjp(self, w):
        pol, ct = self.policy, self.ct
        w = w.to(torch.float32).contiguous()
        n = self.obs.shape[0]
        partial = torch.empty((self.L.CassiePgPartialRows(n), self.NP), dtype=torch.float32, device=self.obs.device)
        live = dict(pol.named_parameters())
        P = lambda t: ct.c_void_p(t.data_ptr())
        rc = self.L.CassiePgVjp(P(self.obs), n, self.D, self.A, *[P(live[k].detach()) for k in _MEAN_ORDER], P(w), P(partial),
                                ct.c_void_p(torch.cuda.current_stream(self.obs.device).cuda_stream))
        if rc != 0:
            raise RuntimeError("CassiePgVjp failed (%d)" % rc)
        pieces = dict(zip(_MEAN_ORDER, torch.split(partial.sum(0), self.sizes)))
        pieces["log_std"] = torch.zeros_like(pol.log_std.detach())
        return torch.cat([pieces[nm].reshape(-1) for nm, _ in pol.named_parameters()])

    def grad(self, act, old_mean, old_lstd, adv):
        """This rank's gradient of -mean(logli adv) (flat, parameter order)."""
        if self._vjp is not None:
            return closed_form_grad(self.policy, self._vjp, act, old_mean, old_lstd, adv)
        mean, log_std = self.policy.dist_info(self.obs)
        loss = -(self.policy.log_likelihood(act, mean, log_std) * adv).mean()
        return flat_grad(loss, self.policy).detach()


class VPG(TRPO):
    """rllab's VPG on TRPO's sampler and baseline.  Switches (attributes, default True) that tests set to force the torch path:
    fused_policy_step (the sampler's policy step), fused_grad (PolicyGradKernels), fused_adam (CassiePgAdam)."""

    def __init__(self, env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size=10000, max_path_length=1000, discount=0.99,
                 learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, log_kl=False, seed=1, env_reset_masked=None, env_id0=None):
        super().__init__(env_step, env_reset, policy, baseline, n_envs, obs_dim, act_map, batch_size=batch_size, max_path_length=max_path_length,
                         discount=discount, seed=seed, env_reset_masked=env_reset_masked, env_id0=env_id0)
        self.learning_rate, self.beta1, self.beta2, self.epsilon, self.log_kl = learning_rate, beta1, beta2, epsilon, log_kl
        self.adam_t, self.adam_m, self.adam_v = 0, None, None
        self.last_grad_kind = None

    @property
    def hidden_sizes(self):
        return hidden_sizes_of(self.policy)

    # the sampler's policy step (CassiePgPolicyStep for a 128-128 policy, CassieTrpoPolicyStep for 32 x 32) is TRPO._fused_policy_step

    def optimize(self, d):
        pol = self.policy
        obs, act, adv, old_mean, old_lstd = d["obs"], d["act"], d["adv"], d["mean"], d["log_std"]
        pk = PolicyGradKernels(pol, obs, fused=getattr(self, "fused_grad", True))
        self.last_grad_kind = pk.kind
        g = all_mean_(pk.grad(act, old_mean, old_lstd, adv).contiguous(), "gradient_all_reduce")
        theta = flat_params(pol).contiguous()
        if self.adam_m is None:
            self.adam_m, self.adam_v = torch.zeros_like(theta), torch.zeros_like(theta)
        before = theta.clone()
        self.adam_t += 1
        fused = getattr(self, "fused_adam", True) and theta.is_cuda and theta.dtype == torch.float32
        (fused_adam_step_ if fused else adam_step_)(theta, g.to(theta.dtype), self.adam_m, self.adam_v, self.adam_t, self.learning_rate,
                                                    self.beta1, self.beta2, self.epsilon)
        self.last_adam_fused = fused
        set_flat_params(pol, theta)
        vals = [g.double().norm(), (theta - before).double().norm()]
        if self.log_kl:   # rllab's logged MeanKL / MaxKL / LossAfter: one more forward pass over the batch
            with torch.no_grad():
                mean, log_std = pol.dist_info(obs)
                kl = pol.kl(old_mean, old_lstd, mean, log_std)
                loss_after = -(pol.log_likelihood(act, mean, log_std) * adv).mean()
                mk = kl.max().double().reshape(1).clone()
                if _world() > 1:
                    dist.all_reduce(mk, op=dist.ReduceOp.MAX)
                vals += [all_mean_(kl.mean().double().reshape(1).clone(), "stats_all_reduce")[0], mk[0],
                         all_mean_(loss_after.double().reshape(1).clone(), "stats_all_reduce")[0]]
        vals = torch.stack(vals).tolist()   # one read-back
        st = dict(grad_norm=vals[0], step_norm=vals[1])
        if self.log_kl:
            st.update(mean_kl=vals[2], max_kl=vals[3], loss_after=vals[4])
        return st

    # ---- snapshot: TRPO's, plus the algorithm, the policy shape, the learning rate and the Adam state
    def _snapshot_fields(self):
        return dict(algo="vpg", hidden_sizes=list(self.hidden_sizes), learning_rate=float(self.learning_rate), adam_t=int(self.adam_t),
                    adam_m=None if self.adam_m is None else self.adam_m.detach().cpu(), adam_v=None if self.adam_v is None else self.adam_v.detach().cpu())

    def _load_fields(self, ck):
        algo = ck.get("algo", "trpo")
        if algo != "vpg":
            raise ValueError("VPG.load: the snapshot was written by %s, this run is vpg" % algo)
        theirs, mine = tuple(ck.get("hidden_sizes", (32, 32))), self.hidden_sizes
        if theirs != mine:
            raise ValueError("VPG.load: the snapshot's policy has hidden sizes %r, this run's has %r" % (theirs, mine))
        dev = next(self.policy.parameters()).device
        self.adam_t = int(ck.get("adam_t", 0))
        self.adam_m = None if ck.get("adam_m") is None else ck["adam_m"].to(dev)
        self.adam_v = None if ck.get("adam_v") is None else ck["adam_v"].to(dev)


def make_cassie_vpg(n_envs, kind="walk", control_mode="PD", device=0, trajectory=None, seed=1, hidden_sizes=(128, 128), init_std=1.0,
                    learning_rate=1e-3, terrain=None, sync_policy=True, **kw):
    """vpg_cassie.py:15-48 on the batched MI355X environment; the counterpart of trpo.make_cassie_trpo (same env, terrain and sync_policy rules)."""
    from .vec_env import CassieVecEnv
    env = CassieVecEnv(n_envs, kind=kind, control_mode=control_mode, n_substeps=10, auto_reset=True, device=device, trajectory=trajectory)
    env.use_torch_stream()
    dev = "cuda:%d" % device
    bufs = env.alloc()
    torch.manual_seed(seed)
    obs_w = env.observation_space.shape[0]
    policy = GaussianMLPPolicy(obs_w, env.adim, tuple(hidden_sizes), init_std=init_std).to(dev)
    act_map = NormalizedActions(env.action_space.low, env.action_space.high, dev)
    algo = VPG(lambda a: env.step(a, bufs), lambda: env.reset(bufs), policy, LinearFeatureBaseline(), n_envs, obs_w, act_map, seed=seed,
               learning_rate=learning_rate, env_reset_masked=lambda m: env.reset(bufs, mask=m), **kw)
    algo.env = env
    algo.terrain_spec = terrain
    if terrain is not None:
        env.set_terrain_library(terrain_lib.library_of_spec(terrain), terrain_lib.DEFAULT_SIZE[:2])
        env.set_terrain_ids(terrain_lib.assign_terrains(terrain["seed"], algo.env_ids, len(terrain["files"])).to(dev))
    if sync_policy:
        broadcast_initial_policy(algo)
    return algo
