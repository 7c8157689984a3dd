"""ctypes binding of libcassie2d.so (the HIP extension).  No fallback: if the library is
missing or no HIP device is present the import / create call raises."""
import ctypes as ct
import os

from . import build as _build

_LIB = None


class CassieVecConfig(ct.Structure):
    _fields_ = [("env_kind", ct.c_int), ("control_mode", ct.c_int), ("n_substeps", ct.c_int),
                ("flags", ct.c_int), ("auto_reset", ct.c_int)]


class Cassie3dEnvConfig(ct.Structure):
    _fields_ = [("control_mode", ct.c_int), ("n_substeps", ct.c_int), ("auto_reset", ct.c_int),
                ("kp", ct.c_double * 10), ("kd", ct.c_double * 10)]


EXPORTS = [
    # legacy ABI (include/cassie2d.h)
    "Cassie2dInit", "Reset", "StepOsc", "StepTorque", "StepJacobian", "StepPd", "GetGeneralState",
    "GetOperationalSpaceState", "Display", "Render",
    # batched ABI (include/cassie_vec.h)
    "CassieVecCreate", "CassieVecFree", "CassieVecLastError", "CassieVecNumEnvs", "CassieVecActionDim",
    "CassieVecSetStream", "CassieVecSynchronize", "CassieVecGetCounters", "CassieVecResetCounters", "CassieVecTierInfo", "CassieVecQpIterations", "CassieVecSetTrajectory", "CassieVecSetHeightField", "CassieVecSetTerrainLibrary", "CassieVecSetTerrainIds", "CassieVecGetTerrainIds", "CassieVecReset", "CassieVecResetTo",
    "CassieVecStep", "CassieVecSubstep", "CassieVecStandingStep", "CassieVecAccumulate", "CassieVecGetState", "CassieVecGetOpState", "CassieVecStatePtr",
    "CassieVecStepHost", "CassieVecGetStateHost", "CassieVecSetStateHost", "CassieVecGetFullStateHost",
    "CassieVecDebugSubstepHost", "CassieVecDebugWorkspaceHost", "CassieVecTimeSteps",
    # batched Cassie3d physics (include/cassie3d_vec.h)
    "Cassie3dVecCreate", "Cassie3dVecFree", "Cassie3dVecLastError", "Cassie3dVecSetStream", "Cassie3dVecSynchronize",
    "Cassie3dVecReset", "Cassie3dVecStep", "Cassie3dVecStatePtr", "Cassie3dVecGetCounters", "Cassie3dVecResetCounters", "Cassie3dVecStepHost", "Cassie3dVecGetStateHost",
    "Cassie3dVecSetStateHost", "Cassie3dVecDebugForwardHost", "Cassie3dVecTimeSteps",
    "Cassie3dVecEnvConfigure", "Cassie3dVecSubstepPd", "Cassie3dVecEnvReset", "Cassie3dVecEnvStep", "Cassie3dVecEnvStepHost", "Cassie3dVecEnvGetCounters",
    # fused policy kernels of the TRPO outer loop (include/cassie_trpo.h)
    "CassieTrpoParamCount", "CassieTrpoPartialRows", "CassieTrpoFvp", "CassieTrpoVjp", "CassieTrpoSurrogate", "CassieTrpoCgUpdate", "CassieTrpoPolicyStep", "CassieTrpoSamplerRows", "CassieTrpoSamplerStep",
    "CassieTrpoBaselineFeatures", "CassieTrpoBaselinePredict", "CassieTrpoReturnsAdvantages", "CassieTrpoGramRows", "CassieTrpoGramRowSize", "CassieTrpoBaselineGram", "CassieTrpoRidgeSolve",
    # width-128 policy (include/cassie_trpo.h)
    "CassiePgParamCount", "CassiePgPolicyStep", "CassiePgPartialRows", "CassiePgVjp", "CassiePgAdam",
    "CassiePgFvp", "CassiePgSurrogateRows", "CassiePgSurrogate", "CassiePgCgUpdate",
    # DDPG (include/cassie_trpo.h)
    "CassieDdpgParamCount", "CassieDdpgPartialRows", "CassieDdpgPolicyStep", "CassieDdpgPoolCommit", "CassieDdpgCriticGrad", "CassieDdpgActorGrad", "CassieDdpgApply",
    # SAC (include/cassie_trpo.h)
    "CassieSacParamCount", "CassieSacPolicyStep", "CassieSacCriticGrad", "CassieSacActorGrad", "CassieSacApply",
    # SAC at the Cassie3d shape, 45 x 10 (include/cassie_trpo.h)
    "CassieSac3dParamCount", "CassieSac3dPolicyStep", "CassieSac3dCriticGrad", "CassieSac3dActorGrad", "CassieSac3dCriticApply", "CassieSac3dActorApply",
    # TD3 (include/cassie_trpo.h)
    "CassieTd3PolicyStep", "CassieTd3CriticGrad", "CassieTd3CriticApply",
    # PPO (include/cassie_trpo.h)
    "CassieTrpoGae", "CassieTrpoClipGradRows", "CassieTrpoClipGrad", "CassiePgClipGradRows", "CassiePgClipGrad",
    # PPO at the Cassie3d shape, 45 x 10 (include/cassie_trpo.h)
    "CassiePg3dParamCount", "CassiePg3dPolicyStep", "CassiePg3dClipGradRows", "CassiePg3dClipGrad",
    # PPO's value network, 26 and 45 observations (include/cassie_trpo.h)
    "CassieVfParamCount", "CassieVfPredict", "CassieVfGae", "CassieVfGradRows", "CassieVfGrad",
    # ES (include/cassie_trpo.h)
    "CassieEsParamCount", "CassieEsPairsPerWorkgroup", "CassieEsPolicyStep", "CassieEsBook", "CassieEsGradRows", "CassieEsGrad",
    "CassieEsWideParamCount", "CassieEsWidePairsPerWorkgroup", "CassieEsWidePolicyStep",
    # ES at the Cassie3d shape, 45 x 10 (include/cassie_trpo.h)
    "CassieEs3dParamCount", "CassieEs3dPairsPerWorkgroup", "CassieEs3dPolicyStep",
    "CassieEs3dWideParamCount", "CassieEs3dWidePairsPerWorkgroup", "CassieEs3dWidePolicyStep",
]


def lib_path():
    # CASSIE2D_LIB lets experiments (A/B kernel builds) point at another build of the same HIP extension
    return os.environ.get("CASSIE2D_LIB", _build.LIB)


def load():
    """dlopen the HIP extension; raises OSError if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise OSError("HIP extension %s is missing: run `python -m cassierl_amd.build` (needs hipcc); "
                      "cassierl_amd has no CPU fallback" % path)
    # torch bundles its own libamdhip64.so.7; two HIP runtimes in one process cannot both own the GPU.
    # Importing torch first makes the dynamic loader bind libcassie2d.so to the runtime torch already loaded
    # (same SONAME), so tensors, streams and our kernels share one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ct.CDLL(path)
    vp, dp, u8p = ct.c_void_p, ct.c_void_p, ct.c_void_p
    L.CassieVecCreate.argtypes = [ct.POINTER(ct.c_void_p), ct.c_int, ct.c_int, ct.POINTER(CassieVecConfig)]
    L.CassieVecFree.argtypes = [vp]
    L.CassieVecFree.restype = None
    L.CassieVecLastError.argtypes = [vp]
    L.CassieVecLastError.restype = ct.c_char_p
    L.CassieVecNumEnvs.argtypes = [vp]
    L.CassieVecActionDim.argtypes = [vp]
    L.CassieVecSetStream.argtypes = [vp, vp]
    L.CassieVecSynchronize.argtypes = [vp]
    L.CassieVecGetCounters.argtypes = [vp, ct.POINTER(ct.c_uint64)]
    L.CassieVecResetCounters.argtypes = [vp]
    if hasattr(L, "CassieVecQpIterations"):
        L.CassieVecQpIterations.argtypes = [vp, ct.POINTER(ct.c_double)]
    if hasattr(L, "CassieVecTierInfo"):   # (absent from A/B libraries built from earlier rounds' sources: CASSIE2D_LIB)
        L.CassieVecTierInfo.argtypes = [vp, ct.POINTER(ct.c_uint64)]
    L.CassieVecSetTrajectory.argtypes = [vp, dp, dp, ct.c_int]
    L.CassieVecSetHeightField.argtypes = [vp, dp, ct.c_int, ct.c_int, ct.c_double, ct.c_double]
    if hasattr(L, "CassieVecSetTerrainLibrary"):   # (absent from A/B libraries built from earlier sources: CASSIE2D_LIB)
        L.CassieVecSetTerrainLibrary.argtypes = [vp, ct.c_int, vp, vp, vp, dp]
        L.CassieVecSetTerrainIds.argtypes = [vp, u8p, vp]
        L.CassieVecGetTerrainIds.argtypes = [vp, vp]
    L.CassieVecReset.argtypes = [vp, u8p, dp]
    L.CassieVecResetTo.argtypes = [vp, u8p, dp, dp, dp]
    L.CassieVecStep.argtypes = [vp, dp, dp, dp, u8p, dp]
    L.CassieVecSubstep.argtypes = [vp, ct.c_int, dp, ct.c_int]
    L.CassieVecStandingStep.argtypes = [vp, ct.c_int, dp, dp, ct.c_int]
    if hasattr(L, "CassieVecAccumulate"):   # (absent from A/B libraries built from earlier sources: CASSIE2D_LIB)
        L.CassieVecAccumulate.argtypes = [vp, dp, u8p, dp, vp]
    L.CassieVecGetState.argtypes = [vp, dp, dp]
    L.CassieVecGetOpState.argtypes = [vp, dp]
    L.CassieVecStatePtr.argtypes = [vp]
    L.CassieVecStatePtr.restype = ct.c_void_p
    L.CassieVecStepHost.argtypes = [vp, dp, dp, dp, u8p]
    L.CassieVecGetStateHost.argtypes = [vp, dp, dp]
    L.CassieVecSetStateHost.argtypes = [vp, dp]
    L.CassieVecGetFullStateHost.argtypes = [vp, dp]
    L.CassieVecDebugSubstepHost.argtypes = [vp, ct.c_int, dp, dp]
    if hasattr(L, "CassieVecDebugWorkspaceHost"):
        L.CassieVecDebugWorkspaceHost.argtypes = [vp, dp, ct.c_uint64, ct.POINTER(ct.c_uint64)]
    L.CassieVecTimeSteps.argtypes = [vp, dp, ct.c_int, dp, dp, u8p, ct.POINTER(ct.c_float)]
    L.Cassie3dVecCreate.argtypes = [ct.POINTER(ct.c_void_p), ct.c_int, ct.c_int]
    L.Cassie3dVecFree.argtypes = [vp]
    L.Cassie3dVecFree.restype = None
    L.Cassie3dVecLastError.argtypes = [vp]
    L.Cassie3dVecLastError.restype = ct.c_char_p
    L.Cassie3dVecSetStream.argtypes = [vp, vp]
    L.Cassie3dVecSynchronize.argtypes = [vp]
    L.Cassie3dVecReset.argtypes = [vp, dp, dp]
    L.Cassie3dVecStep.argtypes = [vp, dp, ct.c_int]
    L.Cassie3dVecStatePtr.argtypes = [vp]
    L.Cassie3dVecStatePtr.restype = ct.c_void_p
    L.Cassie3dVecGetCounters.argtypes = [vp, ct.POINTER(ct.c_uint64)]
    L.Cassie3dVecResetCounters.argtypes = [vp]
    L.Cassie3dVecStepHost.argtypes = [vp, dp, ct.c_int]
    L.Cassie3dVecGetStateHost.argtypes = [vp, dp]
    L.Cassie3dVecSetStateHost.argtypes = [vp, dp]
    L.Cassie3dVecDebugForwardHost.argtypes = [vp, dp, dp]
    L.Cassie3dVecTimeSteps.argtypes = [vp, dp, ct.c_int, ct.c_int, ct.POINTER(ct.c_float)]
    if hasattr(L, "Cassie3dVecEnvStep"):   # (absent from A/B libraries built from earlier sources: CASSIE2D_LIB)
        L.Cassie3dVecEnvConfigure.argtypes = [vp, ct.POINTER(Cassie3dEnvConfig)]
        L.Cassie3dVecSubstepPd.argtypes = [vp, dp, ct.c_int]
        L.Cassie3dVecEnvReset.argtypes = [vp, u8p, dp]
        L.Cassie3dVecEnvStep.argtypes = [vp, dp, dp, dp, u8p, dp]
        L.Cassie3dVecEnvStepHost.argtypes = [vp, dp, dp, dp, u8p, dp]
        L.Cassie3dVecEnvGetCounters.argtypes = [vp, ct.POINTER(ct.c_uint64)]
    L.Cassie2dInit.restype = ct.c_void_p
    _LIB = L
    return L


def available(*symbols):
    """Whether the HIP extension is there and exports every one of `symbols`: the one answer to "kernels or the torch statements"."""
    try:
        L = load()
    except OSError:
        return False
    return all(hasattr(L, s) for s in symbols)


def ptr(t):
    """A tensor's device pointer as a library argument (None stays a null pointer)."""
    return None if t is None else ct.c_void_p(t.data_ptr())


class Kernels:
    """Base of every kernel-call class (trpo.py, ppo.py, es.py, offpolicy.py): ENTRY names the exported functions, every call goes through the
    dict `fn` (key -> function, filled from ENTRY and looked up at call time, so a test can wrap or count its entries), and a non-zero return
    code raises RuntimeError("<symbol> failed (%d)").  `entry`: this object's own ENTRY (a launcher whose symbol depends on the policy's width);
    `fn`: a dict shared with another object."""

    ENTRY = {}           # key in `fn` -> exported name
    STREAM_LAST = True   # _call appends the current stream of `dev` as the last argument

    def __init__(self, dev, fn=None, entry=None):
        if entry is not None:
            self.ENTRY = entry
        self.L, self.dev = load(), dev
        self.fn = {} if fn is None else fn
        self.fn.update({k: getattr(self.L, name) for k, name in self.ENTRY.items()})

    _p = staticmethod(ptr)

    def _stream(self):
        import torch
        return ct.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _call(self, key, *args):
        rc = self.fn[key](*args, self._stream()) if self.STREAM_LAST else self.fn[key](*args)
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (self.ENTRY[key], rc))
