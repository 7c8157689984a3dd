#!/usr/bin/env python3
"""Bit-for-bit A/B of the on-policy units (csrc/tu_trpo.hip, tu_ppo.hip, tu_pg.hip, tu_pg_trpo.hip) between two builds of the library (not a test):
every entry point of the four units is called with fixed-seed inputs and one line `<case> <buffer> <sha256 of the buffer's bytes>` is printed per
output buffer.  The kernels sum in a fixed order, so two builds that keep the order print the same lines.  Run once per library, each in its own
process (CASSIE2D_LIB selects the library, as tools/ab_bench.py does), and diff the outputs:
    python tools/ab_onpolicy_bits.py > a.txt;  CASSIE2D_LIB=/path/to/other/libcassie2d.so python tools/ab_onpolicy_bits.py > b.txt;  diff a.txt b.txt
Sizes: 1, 31, 33, 129 (one group of four tiles plus one sample), 1000, and one past each grid cap so that the tile / group loop takes a second trip
(65 536 + 33 for the width-32 kernels, 32 768 + 33 for the width-128 VJP and clip-gradient kernels); all four (obs_dim, act_dim) pairs where the
entry point has them; the clip-gradient kernels with and without a minibatch index; the CG step at 13, 3072 and 21 504 entries.
CassieTrpoPolicyStep chooses its one-lane-per-environment kernel once per process, by CASSIE_TRPO_POLICY_VALU=1: with that variable set the tool
runs the width-32 policy-step cases alone (lines tagged `valu`), so a full comparison is two processes per library."""
import ctypes as ct
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cassierl_amd import _lib  # noqa: E402

L = _lib.load()
DEV = torch.device("cuda")
GEN = torch.Generator(device="cpu")
SHAPES = [(26, 6), (26, 7), (17, 6), (17, 7)]
SIZES = [1, 31, 33, 129, 1000]
CAP32, CAP128 = 65536 + 33, 32768 + 33


def rnd(*shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=GEN, dtype=torch.float64) * scale).to(dtype).to(DEV)


def P(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def F(x):
    return ct.c_float(x)


def call(name, *args):
    rc = getattr(L, name)(*args, None)   # the null stream
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (name, rc))


def emit(case, **bufs):
    torch.cuda.synchronize()
    for k, t in bufs.items():
        print("%s %s %s" % (case, k, hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()), flush=True)


def net(D, A, H, scale=0.3):
    return [rnd(H, D, scale=scale), rnd(H, scale=scale), rnd(H, H, scale=scale / 2), rnd(H, scale=scale), rnd(A, H, scale=scale), rnd(A, scale=scale)]


def nan_like(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def policy_rows(pre, n):   # rows of partial sums of the VJP kernels
    return getattr(L, pre + "PartialRows")(n)


def run_width(pre, H, cap):
    """The entry points both widths have: Fvp, Vjp, Surrogate, PolicyStep, ClipGrad (pre: CassieTrpo / CassiePg)."""
    for D, A in SHAPES:
        NP = getattr(L, pre + "ParamCount")(D, A)
        for n in SIZES + [cap]:
            GEN.manual_seed(1000 * D + 10 * A + n % 997)
            tag = "%s D%d A%d n%d" % (pre, D, A, n)
            th, dr = net(D, A, H), net(D, A, H)
            obs, w = rnd(n, D), rnd(n, A, scale=1.0 / max(n, 1))
            prec, ls_new, ls_old = rnd(A).exp(), rnd(A, scale=0.2), rnd(A, scale=0.2)
            old_mean, adv = rnd(n, A, scale=0.5), rnd(n)
            act = old_mean + rnd(n, A, scale=0.7)
            rows = policy_rows(pre, n)
            # J' w
            part = nan_like(rows, NP)
            call(pre + "Vjp", P(obs), n, D, A, *map(P, th), P(w), P(part))
            emit(tag + " vjp", partial=part)
            # Fisher-vector product
            part = nan_like(rows, NP)
            if pre == "CassieTrpo":
                call(pre + "Fvp", P(obs), n, D, A, *map(P, th), *map(P, dr), P(prec), F(1.0 / n), P(part))
                emit(tag + " fvp", partial=part)
            else:
                work = nan_like(n, A)
                call(pre + "Fvp", P(obs), n, D, A, *map(P, th), *map(P, dr), P(prec), F(1.0 / n), P(work), P(part))
                emit(tag + " fvp", work=work, partial=part)
            # line search
            srows = rows if pre == "CassieTrpo" else L.CassiePgSurrogateRows(n)
            sur = nan_like(srows, 2, dtype=torch.float64)
            call(pre + "Surrogate", P(obs), n, D, A, *map(P, th), P(ls_new), P(ls_old), P(act), P(adv), P(old_mean), P(sur))
            emit(tag + " surrogate", partial=sur)
            # clipped-surrogate gradient on a minibatch of m = n positions of a batch of n + 77 rows, through an index (some entries out of range:
            # clamped) and without one (rows 0 .. m - 1)
            nb = n + 77
            bobs, bact_mean, badv = rnd(nb, D), rnd(nb, A, scale=0.5), rnd(nb)
            bact = bact_mean + rnd(nb, A, scale=0.7)
            idx = torch.randint(-2, nb + 2, (n,), generator=GEN, dtype=torch.int64).to(DEV)
            crows = getattr(L, pre + "ClipGradRows")(n)
            for label, ix in (("idx", idx), ("noidx", None)):
                part, stats = nan_like(crows, NP + A), nan_like(crows, 3, dtype=torch.float64)
                call(pre + "ClipGrad", P(bobs), nb, D, A, *map(P, th), P(ix), n, P(bact), P(badv), P(bact_mean), P(ls_old), P(ls_new), F(0.2), F(1.0 / n), P(part), P(stats))
                emit(tag + " clipgrad " + label, partial=part, stats=stats)
            # sampler's policy step (the environment's 26-wide rows only)
            if D == 26:
                obs64, noise = rnd(n, D, dtype=torch.float64), rnd(n, A)
                low, high = -rnd(A, dtype=torch.float64).abs() - 0.5, rnd(A, dtype=torch.float64).abs() + 0.5
                o32, mean, a32, env = nan_like(n, D), nan_like(n, A), nan_like(n, A), nan_like(n, A, dtype=torch.float64)
                call(pre + "PolicyStep", P(obs64), n, D, A, *map(P, th), P(ls_new), P(noise), P(low), P(high), P(o32), P(mean), P(a32), P(env))
                emit(tag + " policystep", obs32=o32, mean=mean, act=a32, env_act=env)


def run_policy_step(pre, H, cap, suffix):
    """The sampler's policy step alone (the environment's 26-wide rows), for the second process that selects the other kernel."""
    for D, A in SHAPES[:2]:
        for n in SIZES + [cap]:
            GEN.manual_seed(31 * A + n % 997)
            th, ls = net(D, A, H), rnd(A, scale=0.2)
            obs64, noise = rnd(n, D, dtype=torch.float64), rnd(n, A)
            low, high = -rnd(A, dtype=torch.float64).abs() - 0.5, rnd(A, dtype=torch.float64).abs() + 0.5
            o32, mean, a32, env = nan_like(n, D), nan_like(n, A), nan_like(n, A), nan_like(n, A, dtype=torch.float64)
            call(pre + "PolicyStep", P(obs64), n, D, A, *map(P, th), P(ls), P(noise), P(low), P(high), P(o32), P(mean), P(a32), P(env))
            emit("%s D%d A%d n%d policystep%s" % (pre, D, A, n, suffix), obs32=o32, mean=mean, act=a32, env_act=env)


def run_cg(name, sizes):
    for n in sizes:
        GEN.manual_seed(77 + n)
        n_ls = min(6, n - 1)
        ls_off = n - n_ls
        apm, hls = rnd(n - n_ls), rnd(n_ls).abs()
        x, r, p = rnd(n), rnd(n), rnd(n)
        scal = torch.tensor([float((r * r).sum()), 1.0], dtype=torch.float32, device=DEV)
        for it in range(2):   # the second call runs on the first one's outputs
            call(name, n, ls_off, n_ls, P(apm), P(hls), F(0.1), F(1e-10), P(x), P(r), P(p), P(scal))
            emit("%s n%d call%d" % (name, n, it), x=x, r=r, p=p, scal=scal)


def run_rest():
    for n in SIZES + [CAP32]:
        GEN.manual_seed(5 + n)
        # CassieTrpoSamplerStep
        rew, done = rnd(n, dtype=torch.float64), (torch.rand(n, generator=GEN) < 0.1).to(torch.uint8).to(DEV)
        path_t = torch.randint(0, 12, (n,), generator=GEN, dtype=torch.int64).to(DEV)
        path_ret = rnd(n, dtype=torch.float64)
        rows = L.CassieTrpoSamplerRows(n)
        rew_row, t_row, cut_row = nan_like(n, dtype=torch.float64), torch.full((n,), -1, dtype=torch.int64, device=DEV), torch.full((n,), 7, dtype=torch.uint8, device=DEV)
        part = nan_like(rows, 2, dtype=torch.float64)
        call("CassieTrpoSamplerStep", P(rew), P(done), n, ct.c_longlong(10), P(path_t), P(path_ret), P(rew_row), P(t_row), P(cut_row), P(part))
        emit("CassieTrpoSamplerStep n%d" % n, path_t=path_t, path_ret=path_ret, rew_row=rew_row, t_row=t_row, cut_row=cut_row, partial=part)
        # CassiePgAdam
        g, m, v, theta = rnd(n), rnd(n, scale=0.1), rnd(n, scale=0.1).abs(), rnd(n)
        call("CassiePgAdam", n, P(g), P(m), P(v), P(theta), 3, F(1e-3), F(0.9), F(0.999), F(1e-8))
        emit("CassiePgAdam n%d" % n, m=m, v=v, theta=theta)
    # CassieTrpoGae: [T][n] batch
    for D in (26, 17):
        for n, T in ((1, 3), (33, 5), (1000, 8)):
            GEN.manual_seed(900 + D + n)
            obs, t = rnd(T * n, D, scale=4.0), torch.randint(0, 300, (T * n,), generator=GEN, dtype=torch.int64).to(DEV)
            rew, cut = rnd(T * n, dtype=torch.float64), (torch.rand(T * n, generator=GEN) < 0.1).to(torch.uint8).to(DEV)
            coeffs, last = rnd(2 * D + 4, scale=0.1, dtype=torch.float64), rnd(n, dtype=torch.float64)
            for label, cf, lv in (("fit", coeffs, last), ("nofit", None, None)):
                ret, adv = nan_like(T * n, dtype=torch.float64), nan_like(T * n, dtype=torch.float64)
                part = nan_like((n + 255) // 256, 2, dtype=torch.float64)
                call("CassieTrpoGae", P(obs), P(t), P(rew), P(cut), T, n, D, P(cf), P(lv), ct.c_double(0.99), ct.c_double(0.95), P(ret), P(adv), P(part))
                emit("CassieTrpoGae D%d n%d T%d %s" % (D, n, T, label), returns=ret, adv=adv, partial=part)


if __name__ == "__main__":
    print("# library %s" % os.path.basename(os.path.dirname(_lib.lib_path())), file=sys.stderr)
    if os.environ.get("CASSIE_TRPO_POLICY_VALU") == "1":
        run_policy_step("CassieTrpo", 32, CAP32, " valu")
        sys.exit(0)
    run_width("CassieTrpo", 32, CAP32)
    run_width("CassiePg", 128, CAP128)
    run_cg("CassieTrpoCgUpdate", [13, 3072])
    run_cg("CassiePgCgUpdate", [13, 3072, 21504])
    run_rest()
