"""The Gaussian tanh-MLP policy of the on-policy family, rllab's normalize() action map, and the flat views of a module's parameters and gradients
that every optimiser here works on."""
import math

import torch
from torch import nn


class GaussianMLPPolicy(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_sizes=(32, 32), init_std=2.0, dtype=torch.float32):
        super().__init__()
        layers, d = [], obs_dim
        for h in hidden_sizes:
            layers += [nn.Linear(d, h), nn.Tanh()]
            d = h
        layers.append(nn.Linear(d, act_dim))
        self.mean_net = nn.Sequential(*layers)
        self.log_std = nn.Parameter(torch.full((act_dim,), math.log(init_std)))
        for m in self.mean_net:
            if isinstance(m, nn.Linear):  # rllab: Xavier-uniform weights, zero bias [external]
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)
        self.to(dtype)

    def dist_info(self, obs):
        return self.mean_net(obs), self.log_std.expand(obs.shape[0], -1)

    @torch.no_grad()
    def get_actions(self, obs, generator=None, noise=None):
        mean, log_std = self.dist_info(obs)
        if noise is None:
            noise = torch.randn(mean.shape, dtype=mean.dtype, device=mean.device, generator=generator)
        return mean + noise.to(mean.dtype) * log_std.exp(), mean, log_std

    @staticmethod
    def log_likelihood(actions, mean, log_std):
        z = (actions - mean) / log_std.exp()
        return -(log_std.sum(-1) + 0.5 * (z * z).sum(-1) + 0.5 * mean.shape[-1] * math.log(2 * math.pi))

    @staticmethod
    def kl(old_mean, old_log_std, new_mean, new_log_std):
        old_std, new_std = old_log_std.exp(), new_log_std.exp()
        num = (old_mean - new_mean) ** 2 + old_std ** 2 - new_std ** 2
        return (num / (2 * new_std ** 2 + 1e-8) + new_log_std - old_log_std).sum(-1)


def hidden_sizes_of(policy):
    """Hidden layer widths of a GaussianMLPPolicy, e.g. (128, 128)."""
    return tuple(m.out_features for m in policy.mean_net if isinstance(m, nn.Linear))[:-1]


class NormalizedActions:
    """rllab.envs.normalized_env.normalize (actions only): [-1, 1] -> [lb, ub], then clip."""

    def __init__(self, low, high, device, dtype=torch.float64):
        self.low = torch.as_tensor(low, dtype=dtype, device=device)
        self.high = torch.as_tensor(high, dtype=dtype, device=device)

    def __call__(self, a):
        a = a.to(self.low.dtype)
        scaled = self.low + (a + 1.0) * 0.5 * (self.high - self.low)
        return torch.minimum(torch.maximum(scaled, self.low), self.high).contiguous()


def flat_params(module):
    return torch.cat([p.data.reshape(-1) for p in module.parameters()])


def set_flat_params(module, flat):
    i = 0
    for p in module.parameters():
        n = p.numel()
        p.data.copy_(flat[i:i + n].view_as(p))
        i += n


def flat_grad(y, module, retain_graph=False, create_graph=False):
    g = torch.autograd.grad(y, list(module.parameters()), retain_graph=retain_graph, create_graph=create_graph)
    return torch.cat([x.reshape(-1) for x in g])


_MEAN_ORDER = ["mean_net.0.weight", "mean_net.0.bias", "mean_net.2.weight", "mean_net.2.bias", "mean_net.4.weight", "mean_net.4.bias"]   # the kernels' row order


def _two_layer_tanh(policy):
    """The three Linear layers of a two-hidden-layer tanh policy (what every policy kernel covers), else None."""
    lin = [m for m in policy.mean_net if isinstance(m, nn.Linear)]
    ok = len(lin) == 3 and all(isinstance(m, (nn.Linear, nn.Tanh)) for m in policy.mean_net)
    return lin if ok else None


def add_to_log_std_slot_(policy, g, g_ls):
    """g (flat, parameter order) += g_ls in the log_std slot."""
    i0 = 0
    for nm, p in policy.named_parameters():
        if nm == "log_std":
            g[i0:i0 + p.numel()] += g_ls.to(g.dtype)
        i0 += p.numel()
    return g


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
        return add_to_log_std_slot_(policy, g, g_ls)
