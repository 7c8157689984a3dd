#!/usr/bin/env python3
"""Bit-for-bit A/B of the off-policy units (csrc/tu_ddpg.hip, tu_sac.hip, tu_sac3d.hip, tu_td3.hip) between two builds of the library (not a test), in the manner
of tools/ab_onpolicy_bits.py, whose helpers it uses: every entry point of the four units is called with fixed-seed inputs and one line
`<case> <buffer> <sha256 of the buffer's bytes>` is printed per output buffer.  Run once per library, each in its own process (CASSIE2D_LIB selects
the library), and diff the outputs:
    python tools/ab_offpolicy_bits.py > a.txt;  CASSIE2D_LIB=/path/to/other/libcassie2d.so python tools/ab_offpolicy_bits.py > b.txt;  diff a.txt b.txt
Batches: 1, 31, 33, 129, 1000, and 32 768 + 33 for the gradients (past the grid cap of 256 workgroups: the tile loop takes a second trip), 65 536 + 33
for the policy steps and the pool commit; all four (obs_dim, act_dim) pairs where the entry point has them.  The batch's index holds entries out of the
pool's range (clamped), outputs are pre-filled with NaN, and every apply kernel takes the partial rows of the gradient call before it (1, 2, 8 and 256
rows).  CassieSacApply runs with and without a temperature state.  The six CassieSac3d* entry points run at (45, 10) in the same manner: both
critics' CassieSac3dCriticApply on their blocks of the gradient call's rows, CassieSac3dActorApply with and without a temperature state.
    python tools/ab_offpolicy_bits.py --time [reps]
times the four policy steps instead (65 536 rows, median of `reps` synchronised calls): one JSON line per entry point."""
import ctypes as ct
import json
import os
import sys
import time

import torch

from ab_onpolicy_bits import DEV, GEN, L, SHAPES, SIZES, F, P, _lib, call, emit, nan_like, net, rnd

GRAD_CAP, STEP_CAP, CALLS = 32768 + 33, 65536 + 33, 20   # CALLS: launches between two synchronisations of --time
ACTOR, CRITIC = 0, 1   # CASSIE_DDPG_ACTOR, CASSIE_DDPG_CRITIC
ADAM = (F(1e-3), F(0.9), F(0.999), F(1e-8))


def critic(D, A):
    return [rnd(32, D, scale=0.3), rnd(32, scale=0.3), rnd(32, 32 + A, scale=0.15), rnd(32, scale=0.3), rnd(1, 32, scale=0.3), rnd(1, scale=0.3)]


def N(ps):   # a network as the C ABI takes it
    return (ct.c_void_p * 6)(*[p.data_ptr() for p in ps])


def flat(ps):
    return torch.cat([p.flatten() for p in ps])


def copies(ps):
    return [p.clone() for p in ps]


def ddpg_apply(tag, D, A, which, rows, part, live, ns):
    """CassieDdpgApply on copies of `live` and a target, Adam state and statistics that hold something already."""
    live, targ = copies(live), net(D, A, 32) if which == ACTOR else critic(D, A)
    np_ = L.CassieDdpgParamCount(D, A, which)
    m, v, stats = rnd(np_, scale=0.01), rnd(np_, scale=0.01).abs(), rnd(ns, dtype=torch.float64)
    call("CassieDdpgApply", rows, D, A, which, P(part), F(1.0 / 7), N(live), N(targ), P(m), P(v), 3, *ADAM, F(5e-3), P(stats))
    emit(tag, live=flat(live), target=flat(targ), m=m, v=v, stats=stats)


def run_updates():
    for D, A in SHAPES:
        NPA, NPQ, NPS = L.CassieDdpgParamCount(D, A, ACTOR), L.CassieDdpgParamCount(D, A, CRITIC), L.CassieSacParamCount(D, A)
        for n in SIZES + [GRAD_CAP]:
            GEN.manual_seed(7000 * D + 70 * A + n % 997)
            tag = "D%d A%d n%d" % (D, A, n)
            cap = n + 77
            obs, nobs, act = rnd(cap, D, scale=0.7), rnd(cap, D, scale=0.7), rnd(cap, A).tanh()
            rew, term = rnd(cap, scale=0.1), (torch.rand(cap, generator=GEN) < 0.1).float().to(DEV)
            idx = torch.randint(-2, cap + 2, (n,), generator=GEN, dtype=torch.int64).to(DEV)
            pool = (P(obs), P(act), P(rew), P(term), P(nobs), ct.c_longlong(cap), P(idx), n, D, A)
            pool_obs = (P(obs), ct.c_longlong(cap), P(idx), n, D, A)
            eps, eps_next, log_alpha = rnd(n, A), rnd(n, A), rnd(1, scale=0.5)
            pi, pi2, tpi = net(D, A, 32), net(D, 2 * A, 32), net(D, A, 32)
            q1, q2, tq1, tq2 = critic(D, A), critic(D, A), critic(D, A), critic(D, A)
            rows = L.CassieDdpgPartialRows(n)
            # DDPG: critic gradient, its apply, actor gradient, its apply
            part = nan_like(rows, NPQ + 2)
            call("CassieDdpgCriticGrad", *pool, N(tpi), N(tq1), N(q1), F(0.99), P(part))
            emit(tag + " ddpg criticgrad", partial=part)
            ddpg_apply(tag + " ddpg apply critic", D, A, CRITIC, rows, part, q1, 2)
            part = nan_like(rows, NPA + 1)
            call("CassieDdpgActorGrad", *pool_obs, N(pi), N(q1), P(part))
            emit(tag + " ddpg actorgrad", partial=part)
            ddpg_apply(tag + " ddpg apply actor", D, A, ACTOR, rows, part, pi, 1)
            # SAC: both critics' gradient, actor gradient, its apply with and without a temperature state
            part = nan_like(2, rows, NPQ + 2)
            call("CassieSacCriticGrad", *pool, N(pi2), N(tq1), N(tq2), N(q1), N(q2), P(eps_next), P(log_alpha), F(0.99), P(part))
            emit(tag + " sac criticgrad", partial=part)
            part = nan_like(rows, NPS + 2)
            call("CassieSacActorGrad", *pool_obs, N(pi2), N(q1), N(q2), P(eps), P(log_alpha), P(part))
            emit(tag + " sac actorgrad", partial=part)
            for label, tuned in (("alpha", True), ("fixed", False)):
                live, la = copies(pi2), log_alpha.clone()
                m, v, stats = rnd(NPS, scale=0.01), rnd(NPS, scale=0.01).abs(), rnd(3, dtype=torch.float64)
                am, av = (rnd(1, scale=0.01), rnd(1, scale=0.01).abs()) if tuned else (None, None)
                call("CassieSacApply", rows, D, A, P(part), F(1.0 / 7), N(live), P(m), P(v), 3, *ADAM, P(la), P(am), P(av), 2 if tuned else 0, F(3e-4), F(-float(A)),
                     P(stats))
                bufs = dict(live=flat(live), m=m, v=v, log_alpha=la, stats=stats)
                if tuned:
                    bufs.update(alpha_m=am, alpha_v=av)
                emit(tag + " sac apply " + label, **bufs)
            # TD3: both critics' gradient and their apply
            part = nan_like(2, rows, NPQ + 2)
            call("CassieTd3CriticGrad", *pool, N(tpi), N(tq1), N(tq2), N(q1), N(q2), P(eps_next), F(0.2), F(0.5), F(0.99), P(part))
            emit(tag + " td3 criticgrad", partial=part)
            l1, l2, t1, t2 = copies(q1), copies(q2), copies(tq1), copies(tq2)
            ms = [rnd(NPQ, scale=0.01) for _ in range(2)]
            vs = [rnd(NPQ, scale=0.01).abs() for _ in range(2)]
            stats = rnd(4, dtype=torch.float64)
            call("CassieTd3CriticApply", rows, D, A, P(part), F(1.0 / 7), N(l1), N(l2), N(t1), N(t2), P(ms[0]), P(vs[0]), P(ms[1]), P(vs[1]), 3, *ADAM, F(5e-3), P(stats))
            emit(tag + " td3 criticapply", qf1=flat(l1), qf2=flat(l2), target1=flat(t1), target2=flat(t2), m1=ms[0], v1=vs[0], m2=ms[1], v2=vs[1], stats=stats)


def run_sac3d():
    D, A = 45, 10
    NPA, NPQ = L.CassieSac3dParamCount(D, A, ACTOR), L.CassieSac3dParamCount(D, A, CRITIC)
    for n in SIZES + [GRAD_CAP]:
        GEN.manual_seed(7000 * D + 70 * A + n % 997)
        tag = "D%d A%d n%d" % (D, A, n)
        cap = n + 77
        obs, nobs, act = rnd(cap, D, scale=0.7), rnd(cap, D, scale=0.7), rnd(cap, A).tanh()
        rew, term = rnd(cap, scale=0.1), (torch.rand(cap, generator=GEN) < 0.1).float().to(DEV)
        idx = torch.randint(-2, cap + 2, (n,), generator=GEN, dtype=torch.int64).to(DEV)
        eps, eps_next, log_alpha = rnd(n, A), rnd(n, A), rnd(1, scale=0.5)
        pi2 = net(D, 2 * A, 32)
        q1, q2, tq1, tq2 = critic(D, A), critic(D, A), critic(D, A), critic(D, A)
        rows = L.CassieDdpgPartialRows(n)
        # both critics' gradient, each critic's apply on its block of the rows
        part = nan_like(2, rows, NPQ + 2)
        call("CassieSac3dCriticGrad", P(obs), P(act), P(rew), P(term), P(nobs), ct.c_longlong(cap), P(idx), n, D, A, N(pi2), N(tq1), N(tq2), N(q1), N(q2), P(eps_next),
             P(log_alpha), F(0.99), P(part))
        emit(tag + " sac3d criticgrad", partial=part)
        for k, (q, tq) in enumerate(((q1, tq1), (q2, tq2))):
            live, targ = copies(q), copies(tq)
            m, v, stats = rnd(NPQ, scale=0.01), rnd(NPQ, scale=0.01).abs(), rnd(2, dtype=torch.float64)
            call("CassieSac3dCriticApply", rows, D, A, P(part[k]), F(1.0 / 7), N(live), N(targ), P(m), P(v), 3, *ADAM, F(5e-3), P(stats))
            emit(tag + " sac3d criticapply %d" % (k + 1), live=flat(live), target=flat(targ), m=m, v=v, stats=stats)
        # actor gradient, its apply with and without a temperature state
        part = nan_like(rows, NPA + 2)
        call("CassieSac3dActorGrad", P(obs), ct.c_longlong(cap), P(idx), n, D, A, N(pi2), N(q1), N(q2), P(eps), P(log_alpha), P(part))
        emit(tag + " sac3d actorgrad", partial=part)
        for label, tuned in (("alpha", True), ("fixed", False)):
            live, la = copies(pi2), log_alpha.clone()
            m, v, stats = rnd(NPA, scale=0.01), rnd(NPA, scale=0.01).abs(), rnd(3, dtype=torch.float64)
            am, av = (rnd(1, scale=0.01), rnd(1, scale=0.01).abs()) if tuned else (None, None)
            call("CassieSac3dActorApply", rows, D, A, P(part), F(1.0 / 7), N(live), P(m), P(v), 3, *ADAM, P(la), P(am), P(av), 2 if tuned else 0, F(3e-4), F(-float(A)),
                 P(stats))
            bufs = dict(live=flat(live), m=m, v=v, log_alpha=la, stats=stats)
            if tuned:
                bufs.update(alpha_m=am, alpha_v=av)
            emit(tag + " sac3d actorapply " + label, **bufs)
    for n in SIZES + [STEP_CAP]:
        GEN.manual_seed(4510 + n % 997)
        th2, ins = net(D, 2 * A, 32), step_inputs(A, n, D)
        args, bufs = sac3d_step(n, th2, ins)
        call("CassieSac3dPolicyStep", *args)
        emit("CassieSac3dPolicyStep n%d" % n, **bufs)


def sac3d_step(n, th2, ins):
    """CassieSac3dPolicyStep's call and its output buffers."""
    D, A = 45, 10
    obs64, noise, low, high = ins[:4]
    o32, a32, env = nan_like(n, D), nan_like(n, A), nan_like(n, A, dtype=torch.float64)
    return (P(obs64), n, D, A, N(th2), P(noise), P(low), P(high), P(o32), P(a32), P(env)), dict(obs32=o32, act=a32, env_act=env)


def step_inputs(A, n, D=26):
    obs64, noise = rnd(n, D, dtype=torch.float64), rnd(n, A)
    low, high = -rnd(A, dtype=torch.float64).abs() - 0.5, rnd(A, dtype=torch.float64).abs() + 0.5
    path_t = torch.randint(0, 3, (n,), generator=GEN, dtype=torch.int64).to(DEV)   # a third of the paths are fresh
    return obs64, noise, low, high, path_t, rnd(n, A, scale=0.3)


def policy_steps(A, n, th, th2, ins):
    """The three policy steps on the same inputs: {entry point: (its call, its output buffers)}."""
    D = 26
    obs64, noise, low, high, path_t, ou = ins
    out = {}
    for name in ("CassieDdpgPolicyStep", "CassieSacPolicyStep", "CassieTd3PolicyStep"):
        o32, a32, env = nan_like(n, D), nan_like(n, A), nan_like(n, A, dtype=torch.float64)
        tail = (P(low), P(high), P(o32), P(a32), P(env))
        bufs = dict(obs32=o32, act=a32, env_act=env)
        if name == "CassieDdpgPolicyStep":
            args = (P(obs64), n, D, A, *map(P, th), P(noise), P(path_t), F(0.15), F(0.3), F(0.1), P(ou)) + tail
            bufs["ou"] = ou
        elif name == "CassieSacPolicyStep":
            args = (P(obs64), n, D, A, N(th2), P(noise)) + tail
        else:
            args = (P(obs64), n, D, A, N(th), P(noise), F(0.1)) + tail
        out[name] = (args, bufs)
    return out


def run_steps():
    for A in (6, 7):
        for n in SIZES + [STEP_CAP]:
            GEN.manual_seed(41 * A + n % 997)
            th, th2 = net(26, A, 32), net(26, 2 * A, 32)
            for name, (args, bufs) in policy_steps(A, n, th, th2, step_inputs(A, n)).items():
                call(name, *args)
                emit("%s A%d n%d" % (name, A, n), **bufs)
    for D in (26, 17):
        for n in SIZES + [STEP_CAP]:
            GEN.manual_seed(300 + D + n % 997)
            rew, done, nobs = rnd(n, dtype=torch.float64), (torch.rand(n, generator=GEN) < 0.1).to(torch.uint8).to(DEV), rnd(n, D, dtype=torch.float64)
            prew, pterm, pnobs = nan_like(n), nan_like(n), nan_like(n, D)
            call("CassieDdpgPoolCommit", P(rew), P(done), P(nobs), n, D, ct.c_double(0.01), P(prew), P(pterm), P(pnobs))
            emit("CassieDdpgPoolCommit D%d n%d" % (D, n), rew=prew, term=pterm, nobs=pnobs)


def time_steps(reps):
    A, n = 6, 65536
    GEN.manual_seed(9)
    th, th2 = net(26, A, 32), net(26, 2 * A, 32)
    ins, th3d, ins3d = step_inputs(A, n), net(45, 20, 32), step_inputs(10, n, 45)   # named: the calls below hold raw pointers into them
    steps = policy_steps(A, n, th, th2, ins)
    steps["CassieSac3dPolicyStep"] = sac3d_step(n, th3d, ins3d)
    for name, (args, _) in steps.items():
        ts = []
        for r in range(reps + 3):   # three warm-up rounds
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(CALLS):
                call(name, *args)
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) / CALLS)
        ts = sorted(ts[3:])
        print(json.dumps(dict(entry=name, rows=n, reps=reps, calls=CALLS, median_us=ts[len(ts) // 2] * 1e6, min_us=ts[0] * 1e6)), flush=True)


if __name__ == "__main__":
    print("# library %s" % os.path.dirname(_lib.lib_path()), file=sys.stderr)
    if sys.argv[1:2] == ["--time"]:
        time_steps(int(sys.argv[2]) if len(sys.argv) > 2 else 30)
        sys.exit(0)
    run_updates()
    run_steps()
    run_sac3d()
