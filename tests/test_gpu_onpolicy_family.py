"""The library calls of one on-policy iteration, per exported symbol, counted through the kernel-call base (cassierl_amd/_lib.py: Kernels.fn): the
numbers are the ones the modules made when every call site was written out by hand -- no launch more, none less -- together with which path ran."""
import collections

import pytest

pytestmark = pytest.mark.gpu

_BASELINE = {"CassieTrpoBaselineFeatures": 1, "CassieTrpoGramRows": 1, "CassieTrpoGramRowSize": 1, "CassieTrpoBaselineGram": 1, "CassieTrpoRidgeSolve": 1}
_SAMPLER = {"CassieTrpoSamplerRows": 1, "CassieTrpoSamplerStep": 2}
# 64 environments x 2 steps = 128 samples: a full tile at width 32, a partial group of four tiles at width 128; the first iteration of a run
CASES = {
    "trpo32": (dict(hidden_sizes=(32, 32)),
               dict(_BASELINE, **_SAMPLER, CassieTrpoPolicyStep=2, CassieTrpoReturnsAdvantages=1, CassieTrpoParamCount=1, CassieTrpoPartialRows=2, CassieTrpoVjp=1,
                    CassieTrpoFvp=11, CassieTrpoCgUpdate=10, CassieTrpoSurrogate=2),
               dict(last_fisher_kind="trpo_fvp", policy_step_entry="CassieTrpoPolicyStep")),
    "trpo128": (dict(hidden_sizes=(128, 128), init_std=1.0),
                dict(_BASELINE, **_SAMPLER, CassiePgPolicyStep=2, CassieTrpoReturnsAdvantages=1, CassiePgParamCount=1, CassiePgPartialRows=1, CassiePgSurrogateRows=1,
                     CassiePgVjp=1, CassiePgFvp=11, CassiePgCgUpdate=10, CassiePgSurrogate=2),
                dict(last_fisher_kind="pg_fvp", policy_step_entry="CassiePgPolicyStep")),
    "vpg": (dict(),
            dict(_BASELINE, **_SAMPLER, CassiePgPolicyStep=2, CassieTrpoReturnsAdvantages=1, CassiePgParamCount=1, CassiePgPartialRows=1, CassiePgVjp=1, CassiePgAdam=1),
            dict(last_grad_kind="pg_vjp", policy_step_entry="CassiePgPolicyStep", last_adam_fused=True)),
    "ppo": (dict(epochs=2, minibatch_size=64),
            dict(_BASELINE, **_SAMPLER, CassiePgPolicyStep=2, CassieTrpoGae=1, CassiePgParamCount=1, CassiePgClipGradRows=4, CassiePgClipGrad=4, CassiePgAdam=4),
            dict(last_grad_kind="pg_clip", policy_step_entry="CassiePgPolicyStep", last_gae_fused=True, last_adam_fused=True)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_library_calls_of_one_iteration(name, monkeypatch):
    from cassierl_amd import _lib
    from cassierl_amd import ppo as P
    from cassierl_amd import trpo as T
    from cassierl_amd import vpg as V
    from cassierl_amd.trajectory import default_gait
    kw, expected, kinds = CASES[name]
    make = {"trpo32": T.make_cassie_trpo, "trpo128": T.make_cassie_trpo, "vpg": V.make_cassie_vpg, "ppo": P.make_cassie_ppo}[name]
    algo = make(64, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, batch_size=128, **kw)
    counts = collections.Counter()
    init = _lib.Kernels.__init__

    def counting_init(self, *a, **k):
        init(self, *a, **k)
        for key, f in list(self.fn.items()):
            def counted(*args, _f=f, _symbol=self.ENTRY[key]):
                counts[_symbol] += 1
                return _f(*args)
            self.fn[key] = counted

    monkeypatch.setattr(_lib.Kernels, "__init__", counting_init)
    try:
        algo.train_iteration()
    finally:
        algo.env.close()
    print(name, dict(sorted(counts.items())))
    assert dict(counts) == expected
    for attr, want in kinds.items():
        assert getattr(algo, attr) == want, attr
    for attr in {"last_fisher_kind", "last_grad_kind", "last_gae_fused", "last_adam_fused"} - set(kinds):
        assert getattr(algo, attr, None) is None, attr   # TRPO has no gradient kind and no Adam, VPG / PPO no Fisher object, only PPO a GAE switch
