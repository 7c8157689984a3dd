"""Batched Cassie3d physics (model/cassie3d_stiff.xml) over include/cassie3d_vec.h -- BASELINE.json configs[4].

The reference has no Cassie3d environment class (only the MJCF), so this mirrors the torque-mode surface of
`Cassie2d` (src/Cassie2d/Cassie2d.cpp:78-94: Reset, Step, GetGeneralState) with a leading n_envs axis.
No CPU fallback: constructing it loads libcassie2d.so and needs a HIP device.
"""
import ctypes as ct

import numpy as np

from . import _lib

NQ, NV, NU, STATE_STRIDE, DEBUG_STRIDE = 21, 20, 10, 80, 1869
OFF = dict(qpos=0, qvel=21, warmstart=41, ctrl=61, time=71, niter=72, nefc=73, overflow=74)
CTRL_RANGE = np.array([4.5, 4.5, 12.2, 12.2, 0.9] * 2)  # cassie3d_stiff.xml:184-195


class Cassie3dVec:
    def __init__(self, n_envs, device=0):
        self.L = _lib.load()
        self.n_envs, self.device = n_envs, device
        h = ct.c_void_p()
        rc = self.L.Cassie3dVecCreate(ct.byref(h), n_envs, device)
        if rc != 0:
            raise RuntimeError("Cassie3dVecCreate failed (%d): no HIP device / allocation failure; there is no CPU path" % rc)
        self.h = h

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError("libcassie2d error %d: %s" % (rc, self.L.Cassie3dVecLastError(self.h).decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.Cassie3dVecFree(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._chk(self.L.Cassie3dVecSynchronize(self.h))

    def counters(self):
        """env-substeps requested / done by the 64-row kernel / with the 64-row cap leaving contacts out / handed down by the lane-per-leg kernel."""
        out = (ct.c_uint64 * 4)()
        self._chk(self.L.Cassie3dVecGetCounters(self.h, out))
        req, gen, cap, leg = int(out[0]), int(out[1]), int(out[2]), int(out[3])
        return dict(substeps=req, general_kernel_substeps=gen, capped_substeps=cap, general_frac=(gen / req if req else 0.0),
                    leg_handover_substeps=leg, leg_handover_frac=(leg / req if req else 0.0))

    def reset_counters(self):
        self._chk(self.L.Cassie3dVecResetCounters(self.h))

    # ---- device API (torch tensors are only the allocator here)
    def reset(self, qpos=None, qvel=None):
        self._chk(self.L.Cassie3dVecReset(self.h, None if qpos is None else qpos.data_ptr(), None if qvel is None else qvel.data_ptr()))

    def step(self, torques, n_sub=10):
        assert torques.is_cuda and torques.element_size() == 8 and torques.is_contiguous() and torques.shape == (self.n_envs, NU)
        self._chk(self.L.Cassie3dVecStep(self.h, torques.data_ptr(), n_sub))

    def time_steps(self, torques, n_sub, steps):
        ms = ct.c_float()
        self._chk(self.L.Cassie3dVecTimeSteps(self.h, torques.data_ptr(), n_sub, steps, ct.byref(ms)))
        return ms.value

    # ---- host API (tests)
    def step_host(self, torques, n_sub=1):
        a = np.ascontiguousarray(torques, dtype=np.float64).reshape(self.n_envs, NU)
        self._chk(self.L.Cassie3dVecStepHost(self.h, a.ctypes.data, n_sub))

    def get_state_host(self):
        s = np.empty((self.n_envs, STATE_STRIDE))
        self._chk(self.L.Cassie3dVecGetStateHost(self.h, s.ctypes.data))
        return s

    def set_state_host(self, s):
        s = np.ascontiguousarray(s, dtype=np.float64).reshape(self.n_envs, STATE_STRIDE)
        self._chk(self.L.Cassie3dVecSetStateHost(self.h, s.ctypes.data))

    def debug_forward_host(self, torques):
        a = np.ascontiguousarray(torques, dtype=np.float64).reshape(self.n_envs, NU)
        dbg = np.zeros((self.n_envs, DEBUG_STRIDE))
        self._chk(self.L.Cassie3dVecDebugForwardHost(self.h, a.ctypes.data, dbg.ctypes.data))
        return dbg


def state_record(qpos, qvel, warmstart=None, ctrl=None, time=0.0):
    s = np.zeros(STATE_STRIDE)
    s[0:21], s[21:41] = qpos, qvel
    if warmstart is not None:
        s[41:61] = warmstart
    if ctrl is not None:
        s[61:71] = ctrl
    s[71] = time
    return s


NOBS = 45
CONTROL_MODES = {"Torque": 0, "PD": 1}   # CASSIE3D_CTRL_TORQUE / CASSIE3D_CTRL_PD
# joint ranges of the ten actuated hinges (abduction, yaw, hip, knee, toe per leg; cassie3d_stiff.xml:67-93), degrees
PD_RANGE_DEG = np.array([[-15.0, 22.5], [-22.5, 22.5], [-50.0, 80.0], [-164.0, -37.0], [-140.0, -30.0]] * 2)


def action_space(control_mode):
    from .vec_env import Box
    if control_mode == "Torque":
        return Box(-CTRL_RANGE, CTRL_RANGE)
    r = np.radians(PD_RANGE_DEG)
    return Box(r[:, 0], r[:, 1])


class Cassie3dVecEnv(Cassie3dVec):
    """N Cassie3d environments with the vocabulary of CassieVecEnv: one call per Env.step returns observation [n, 45], reward and done,
    with auto-reset.  PD actions are targets of the ten actuated hinges; the law kp (target - q) - kd v is applied inside the physics
    kernels at EVERY substep (include/cassie3d_vec.h).  step / step_host / reset are the environment's here; the record access of
    Cassie3dVec (get_state_host, set_state_host, synchronize, reset_counters) is inherited, and substep_pd_host runs the bare PD physics."""

    def __init__(self, n_envs, control_mode="PD", n_substeps=10, auto_reset=True, kp=10.0, kd=5.0, device=0):
        assert control_mode in CONTROL_MODES, "Invalid Control Mode"
        super().__init__(n_envs, device)
        self.control_mode, self.n_substeps, self.auto_reset = control_mode, n_substeps, bool(auto_reset)
        cfg = _lib.Cassie3dEnvConfig(CONTROL_MODES[control_mode], n_substeps, int(bool(auto_reset)))
        cfg.kp[:] = np.broadcast_to(np.asarray(kp, dtype=np.float64), (NU,)).tolist()
        cfg.kd[:] = np.broadcast_to(np.asarray(kd, dtype=np.float64), (NU,)).tolist()
        rc = self.L.Cassie3dVecEnvConfigure(self.h, ct.byref(cfg))
        if rc != 0:
            msg = self.L.Cassie3dVecLastError(self.h).decode()
            self.close()
            raise ValueError("Cassie3dVecEnvConfigure failed (%d): %s" % (rc, msg))

    # the snapshot hooks of the learning code (sampler.Sampler.save / load): the whole record of every environment
    FULL_STATE_WIDTH = STATE_STRIDE

    def get_full_state_host(self):
        return self.get_state_host()

    def set_full_state_host(self, s):
        self.set_state_host(s)

    @property
    def observation_space(self):
        from .vec_env import Box
        high = np.full((NOBS,), 1e20)
        return Box(-high, high)

    @property
    def action_space(self):
        return action_space(self.control_mode)

    def counters(self):
        """The physics counters of Cassie3dVec plus done flags raised and, of those, by the failure guard."""
        c = super().counters()
        out = (ct.c_uint64 * 2)()
        self._chk(self.L.Cassie3dVecEnvGetCounters(self.h, out))
        c.update(done=int(out[0]), guard=int(out[1]))
        return c

    # ---- host API (tests)
    def step_host(self, actions, terminal_obs=False):
        """One Env.step from numpy actions [n, 10]: (obs, reward, done) or, with terminal_obs, (obs, reward, done, terminal_obs)."""
        a = np.ascontiguousarray(actions, dtype=np.float64).reshape(self.n_envs, NU)
        obs, rew, done = np.empty((self.n_envs, NOBS)), np.empty(self.n_envs), np.empty(self.n_envs, dtype=np.uint8)
        tobs = np.empty((self.n_envs, NOBS)) if terminal_obs else None
        self._chk(self.L.Cassie3dVecEnvStepHost(self.h, a.ctypes.data, obs.ctypes.data, rew.ctypes.data, done.ctypes.data,
                                                None if tobs is None else tobs.ctypes.data))
        return (obs, rew, done.astype(bool), tobs) if terminal_obs else (obs, rew, done.astype(bool))

    def substep_pd_host(self, targets, n_sub=1):
        """n_sub raw PD substeps towards numpy targets [n, 10] with the configured gains: no observation, reward or reset."""
        import torch
        t = torch.as_tensor(np.ascontiguousarray(targets, dtype=np.float64).reshape(self.n_envs, NU), device="cuda:%d" % self.device)
        self._chk(self.L.Cassie3dVecSubstepPd(self.h, t.data_ptr(), n_sub))
        self.synchronize()

    def reset_host(self, mask=None):
        import torch
        dev = "cuda:%d" % self.device
        out = self.alloc()
        m = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.n_envs), device=dev)
        obs = self.reset(out, m)
        self.synchronize()
        return obs.cpu().numpy()

    # ---- device API (torch tensors are only the allocator here)
    def alloc(self):
        import torch
        dev = "cuda:%d" % self.device
        return dict(obs=torch.empty((self.n_envs, NOBS), dtype=torch.float64, device=dev),
                    reward=torch.empty(self.n_envs, dtype=torch.float64, device=dev),
                    done=torch.empty(self.n_envs, dtype=torch.uint8, device=dev))

    def use_torch_stream(self):
        import torch
        self._chk(self.L.Cassie3dVecSetStream(self.h, ct.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def reset(self, out=None, mask=None):
        """Standing pose for the environments of `mask` (uint8 CUDA tensor [n]; None: all); returns every environment's observation."""
        out = out or self.alloc()
        self._chk(self.L.Cassie3dVecEnvReset(self.h, None if mask is None else mask.data_ptr(), out["obs"].data_ptr()))
        return out["obs"]

    def step(self, actions, out=None, terminal_obs=None):
        """actions: float64 CUDA tensor [n_envs, 10].  Returns (obs, reward, done) tensors (views of `out`)."""
        out = out or self.alloc()
        assert actions.is_cuda and actions.element_size() == 8 and actions.is_contiguous() and actions.shape == (self.n_envs, NU)
        self._chk(self.L.Cassie3dVecEnvStep(self.h, actions.data_ptr(), out["obs"].data_ptr(), out["reward"].data_ptr(),
                                            out["done"].data_ptr(), None if terminal_obs is None else terminal_obs.data_ptr()))
        return out["obs"], out["reward"], out["done"]
