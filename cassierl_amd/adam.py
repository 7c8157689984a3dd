"""Lasagne's Adam on flat tensors: the torch statement, its kernel (CassiePgAdam, csrc/tu_pg.hip) and the state VPG, PPO and ES keep of it."""
import ctypes as ct
import math

import torch

from ._lib import Kernels, ptr


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
    k = Kernels(theta.device, entry={"Adam": "CassiePgAdam"})
    for x in (theta, g, m, v):
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("CassiePgAdam needs contiguous float32 CUDA tensors")
    P = ptr
    k._call("Adam", theta.numel(), P(g), P(m), P(v), P(theta), int(t), ct.c_float(lr), ct.c_float(beta1), ct.c_float(beta2), ct.c_float(eps))


class FlatAdam:
    """Lasagne's Adam on the algorithm's flat parameter vector, for VPG, PPO and ES: the state (adam_t, adam_m, adam_v, attributes of the
    algorithm and entries of its snapshot under these names), the step -- CassiePgAdam for float32 CUDA parameters unless the switch
    `fused_adam` is off, else adam_step_; last_adam_fused says which -- and the state's way into and out of a snapshot."""

    def _adam_init(self, learning_rate, beta1, beta2, epsilon):
        self.learning_rate, self.beta1, self.beta2, self.epsilon = learning_rate, beta1, beta2, epsilon
        self.adam_t, self.adam_m, self.adam_v = 0, None, None
        self.last_adam_fused = None

    def adam_step(self, theta, g):
        """One step of theta (flat, contiguous, updated in place) along g."""
        if self.adam_m is None:
            self.adam_m, self.adam_v = torch.zeros_like(theta), torch.zeros_like(theta)
        self.adam_t += 1
        fused = self.last_adam_fused = getattr(self, "fused_adam", True) and theta.is_cuda and theta.dtype == torch.float32
        (fused_adam_step_ if fused else adam_step_)(theta, g, self.adam_m, self.adam_v, self.adam_t, self.learning_rate, self.beta1, self.beta2, self.epsilon)

    def _adam_snapshot(self):
        return dict(adam_t=int(self.adam_t), adam_m=None if self.adam_m is None else self.adam_m.detach().cpu(),
                    adam_v=None if self.adam_v is None else self.adam_v.detach().cpu())

    def _adam_load(self, ck):
        dev = next(self.policy.parameters()).device
        self.adam_t = int(ck.get("adam_t", 0))
        self.adam_m = None if ck.get("adam_m") is None else ck["adam_m"].to(dev)
        self.adam_v = None if ck.get("adam_v") is None else ck["adam_v"].to(dev)
