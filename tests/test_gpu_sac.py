"""SAC's kernels (csrc/tu_sac.hip) against the torch statements of cassierl_amd/sac.py, and train_sac.py / sim_policy.py on the GPU.  -m gpu only.

Test for test as tests/test_gpu_ddpg.py, with its float32 rounding bounds."""
import copy
import os
import sys
import time

import numpy as np
import pytest

from test_gpu_ddpg import _free_port, _run, _small

pytestmark = pytest.mark.gpu


def _nets(D, A, seed, ls_width=0.05, ls_bias=-1.0, mean_bias=None):
    """Actor, two critics and their targets with test_gpu_ddpg._nets' scaling (HeUniform hidden weights, biases N(0, 0.1), output weights +-0.3, the
    critics' output bias 0.5); the actor's log_std head is scaled down (weights +-0.05, bias -1) so that it stays away from the clamp's bounds and
    |u| stays moderate; the targets are other draws.  ls_width, ls_bias: another log_std head (tests/test_gpu_offpolicy_edges.py: one that crosses the
    clamp's bounds); mean_bias [A]: replaces the mean head's bias after every draw, so that the other parameters are those of the default."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import sac as S
    torch.manual_seed(seed)
    pol = S.SquashedGaussianMLPPolicy(D, A)
    qfs = [G.ContinuousMLPQFunction(D, A) for _ in range(4)]
    with torch.no_grad():
        for net in [pol] + qfs:
            for lin in (net.l1, net.l2, net.l3):
                lin.bias.copy_(0.1 * torch.randn_like(lin.bias))
            net.l3.weight.uniform_(-0.3, 0.3)
        for qf in qfs:
            qf.l3.bias.fill_(0.5)
        pol.l3.weight[A:].uniform_(-ls_width, ls_width)
        pol.l3.bias[A:].fill_(ls_bias)
        if mean_bias is not None:
            pol.l3.bias[:A].copy_(torch.as_tensor(mean_bias, dtype=torch.float32))
    return [pol.cuda()] + [q.cuda() for q in qfs]   # actor, qf1, qf2, target_qf1, target_qf2


def _margin_ok(pol, qf1, qf2, obs, act, noise, eps=1e-4, inside=True, untied=True):
    """Rows (float64 reference) whose gradient-carrying hidden pre-activations all keep |z| >= eps (the actor at s, each live critic at (s, a) and at
    (s, a~)), whose two critics are not tied at (s, a~), and whose log_std keeps eps from both bounds of the clamp and lies between them.
    inside=False keeps the rows whose raw log_std lies outside the bounds (still eps away from them); untied=False keeps the ties."""
    import torch
    p, q1, q2 = (copy.deepcopy(m).double() for m in (pol, qf1, qf2))
    o, a, e = obs.double(), act.double(), noise.double()
    A = pol.act_dim
    with torch.no_grad():
        z1 = p.l1(o); z2 = p.l2(z1.relu())
        out = p.l3(z2.relu())
        ls = out[:, A:]   # the raw head: where inside is required, the clamp changes nothing on the rows that are kept
        at = torch.tanh(out[:, :A] + ls.clamp(-20.0, 2.0).exp() * e)
        conds, qs = [z1, z2], []
        for q in (q1, q2):
            y1 = q.l1(o)
            y2 = q.l2(torch.cat([y1.relu(), a], 1)); y2m = q.l2(torch.cat([y1.relu(), at], 1))
            conds += [y1, y2, y2m]
            qs.append(q.l3(y2m.relu()).squeeze(-1))
        ok = torch.stack([(z.abs() >= eps).all(1) for z in conds]).all(0)
        if untied:
            ok &= (qs[0] - qs[1]).abs() >= eps
        ok &= ((ls - 2.0).abs() >= eps).all(1) & ((ls + 20.0).abs() >= eps).all(1)
        if inside:
            ok &= (ls < 2.0).all(1) & (ls > -20.0).all(1)
        return ok


def _pool_with_margin(pol, qf1, qf2, D, A, candidates=40000, seed=11, inside=True, untied=True):
    """test_gpu_ddpg._pool_with_margin with SAC's conditions.  The actor's noise belongs to the batch position, not to the pool row, so a row is
    kept only if it meets the conditions with the noise it will meet: the test draws batch position b's noise as noise_of_row[idx[b]]."""
    import torch
    from cassierl_amd import ddpg as G
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = 0.7 * torch.randn(candidates, D, device="cuda", generator=g)
    act = torch.rand(candidates, A, device="cuda", generator=g) * 2 - 1
    noise = torch.randn(candidates, A, device="cuda", generator=g)
    keep = _margin_ok(pol, qf1, qf2, obs, act, noise, inside=inside, untied=untied)
    dropped = 1.0 - keep.float().mean().item()
    obs, act, noise = obs[keep], act[keep], noise[keep]
    m = obs.shape[0]
    pool = G.ReplayPool(m, 1, D, A, "cuda")
    pool.obs.copy_(obs); pool.act.copy_(act)
    pool.rew.copy_(torch.randn(m, device="cuda", generator=g) * 0.1)
    pool.term.copy_((torch.rand(m, device="cuda", generator=g) < 0.2).float())
    pool.nobs.copy_(0.7 * torch.randn(m, D, device="cuda", generator=g))
    pool.size = m
    return pool, noise, dropped


def _log_alpha(v=0.3):
    import torch
    return torch.full((1,), float(np.log(v)), device="cuda")


@pytest.mark.parametrize("n", [5000, 65536])
@pytest.mark.parametrize("control_mode,adim", [("PD", 6), ("OSC", 7)])
def test_sac_policy_step_matches_the_torch_statement(control_mode, adim, n):
    import torch
    from cassierl_amd import sac as S
    from cassierl_amd import trpo as T
    from cassierl_amd.vec_env import action_space
    pol, qf1, qf2, _, _ = _nets(26, adim, 7)
    box = action_space(control_mode)
    amap = T.NormalizedActions(box.low, box.high, "cuda")
    algo = S.SAC(None, None, pol, qf1, qf2, n, 26, amap, replay_pool_size=3 * n)
    fused = algo._fused_step(torch.device("cuda:0"))
    assert fused is not None
    step = fused[0]
    pool = algo.pool
    lo, hi = torch.as_tensor(box.low, device="cuda"), torch.as_tensor(box.high, device="cuda")
    for top in (n, 2 * n, 0):   # the middle of the ring, an append that ends exactly at capacity, the next one at 0
        for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs):
            t.copy_(torch.randn_like(t))
        before = [t.clone() for t in (pool.obs, pool.act, pool.rew, pool.term, pool.nobs)]
        obs = torch.randn(n, 26, dtype=torch.float64, device="cuda")
        noise = torch.randn(n, adim, device="cuda")
        with torch.no_grad():
            a_ref = algo._explore(obs.float(), noise)
        step(obs, noise, top)
        act = pool.act[top:top + n]
        assert torch.equal(pool.obs[top:top + n], obs.float())
        err = (act - a_ref).abs().max().item()
        print("policy step n %d A %d top %d: max action error %.3g" % (n, adim, top, err))
        assert err < 5e-6 * (1 + a_ref.abs().max().item())
        assert act.min().item() >= -1.0 and act.max().item() <= 1.0
        assert (algo._env_actions - amap(act)).abs().max().item() < 1e-12
        assert (algo._env_actions >= lo).all() and (algo._env_actions <= hi).all()
        rest = torch.ones(pool.capacity, dtype=torch.bool, device="cuda")
        rest[top:top + n] = False
        for now, was in zip((pool.obs, pool.act), before[:2]):
            assert torch.equal(now[rest], was[rest])
        for now, was in zip((pool.rew, pool.term, pool.nobs), before[2:]):   # the policy step opens the rows; the commit fills these
            assert torch.equal(now, was)


@pytest.mark.parametrize("batch,obs_dim,act_dim", [(1000, 26, 6), (65536, 26, 6), (4099, 26, 7), (777, 17, 6)])
def test_sac_gradients_match_autograd(batch, obs_dim, act_dim):
    """CassieSacCriticGrad and CassieSacActorGrad against float32 autograd on the gathered batch; indices with repeats; 4099 and 777 end in a tile
    that is not a multiple of 32.  The pool is built by rejection (_margin_ok); at most 3 % of the candidates may be dropped.

    The actor's gradient goes through exp, tanh and softplus: where 2e-4 max|g| does not hold for it, the kernel's error against float64 autograd
    must be at most four times that of torch's float32 autograd against float64 on the same batch (a different summation order over up to 65 536
    samples); both errors are printed."""
    import torch
    from cassierl_amd import sac as S
    pol, qf1, qf2, tq1, tq2 = _nets(obs_dim, act_dim, 3)
    pool, row_noise, dropped = _pool_with_margin(pol, qf1, qf2, obs_dim, act_dim)
    print("margins: %.2f %% of the candidate rows dropped" % (100 * dropped))
    assert dropped <= 0.03
    la = _log_alpha()
    alpha = la.exp()
    k = S.SacKernels(pol, qf1, qf2, tq1, tq2, la)
    g = torch.Generator(device="cuda").manual_seed(5)
    idx = torch.randint(0, pool.size, (batch,), device="cuda", generator=g)
    idx[1] = idx[0]
    assert idx.unique().numel() < batch
    eps_s = row_noise[idx].contiguous()
    eps_s2 = torch.randn(batch, act_dim, device="cuda", generator=g)
    s, a, r, term, s2 = pool.sample(idx)
    gamma = 0.99
    rows = k.L.CassieDdpgPartialRows(batch)
    # ---- critics
    with torch.no_grad():
        a2, lp2 = pol.sample(s2, eps_s2)
        y = r + (1 - term) * gamma * (torch.min(tq1(s2, a2), tq2(s2, a2)) - alpha * lp2)
    part = k.critic_grad(pool, idx, eps_s2, gamma).clone()
    for i, qf in enumerate((qf1, qf2)):
        q = qf(s, a)
        loss = ((q - y) ** 2).mean()
        gref = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(qf.parameters()))])
        NP = gref.numel()
        assert part.shape == (2, rows, NP + 2)
        tot = part[i].double().sum(0)
        err = ((tot[:NP] / batch).float() - gref).abs().max().item()
        print("critic %d gradient: max error %.3g of max %.3g; loss %.8g / %.8g; mean Q %.8g / %.8g" %
              (i + 1, err, gref.abs().max().item(), tot[NP].item() / batch, loss.item(), tot[NP + 1].item() / batch, q.double().mean().item()))
        assert err < 2e-4 * gref.abs().max().item()
        assert abs(tot[NP].item() / batch - loss.double().item()) < 1e-5 * abs(loss.item())
        assert abs(tot[NP + 1].item() / batch - q.double().mean().item()) < 1e-5 * abs(q.double().mean().item())
    assert torch.equal(part, k.critic_grad(pool, idx, eps_s2, gamma))   # fixed-order sums: the same bits twice
    # ---- actor
    def actor_loss(p, c1, c2, s_, e_, al):
        at, lp = p.sample(s_, e_)
        qm = torch.min(c1(s_, at), c2(s_, at))
        return (al * lp - qm).mean(), lp, qm
    loss, lp, qm = actor_loss(pol, qf1, qf2, s, eps_s, alpha)
    gref = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, list(pol.parameters()))])
    p64, c64a, c64b = (copy.deepcopy(m).double() for m in (pol, qf1, qf2))
    loss64 = actor_loss(p64, c64a, c64b, s.double(), eps_s.double(), alpha.double())[0]
    g64 = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss64, list(p64.parameters()))])
    part = k.actor_grad(pool, idx, eps_s).clone()
    NP = gref.numel()
    assert part.shape == (rows, NP + 2)
    tot = part.double().sum(0)
    gf = (tot[:NP] / batch).float()
    err = (gf - gref).abs().max().item()
    err_kernel64, err_torch64 = (gf.double() - g64).abs().max().item(), (gref.double() - g64).abs().max().item()
    print("actor gradient: max error %.3g of max %.3g; against float64: kernel %.3g, torch float32 %.3g; mean log pi %.8g / %.8g; mean min Q %.8g / %.8g" %
          (err, gref.abs().max().item(), err_kernel64, err_torch64, tot[NP].item() / batch, lp.double().mean().item(), tot[NP + 1].item() / batch,
           qm.double().mean().item()))
    assert err < 2e-4 * gref.abs().max().item() or err_kernel64 <= 4 * err_torch64
    assert abs(tot[NP].item() / batch - lp.double().mean().item()) < 1e-5 * abs(lp.double().mean().item())
    assert abs(tot[NP + 1].item() / batch - qm.double().mean().item()) < 1e-5 * abs(qm.double().mean().item())
    assert torch.equal(part, k.actor_grad(pool, idx, eps_s))


@pytest.mark.parametrize("rows", [1, 64])
@pytest.mark.parametrize("learn_alpha", [True, False])
def test_sac_apply_matches_adam_and_the_log_alpha_step(learn_alpha, rows):
    """Five steps with gradients spanning 1e-4 .. 1: CassieSacApply (actor, log_alpha) and CassieDdpgApply on a SAC critic block (Adam + soft update)."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import sac as S
    from cassierl_amd import trpo as T
    from cassierl_amd.vpg import adam_step_
    pol, qf1, qf2, tq1, tq2 = _nets(26, 6, 4)
    la = _log_alpha(0.7)
    k = S.SacKernels(pol, qf1, qf2, tq1, tq2, la)
    pol_r, qf_r, tq_r, la_r = copy.deepcopy(pol), copy.deepcopy(qf2), copy.deepcopy(tq2), la.clone()
    adam_pi, adam_pi_r, adam_q, adam_q_r = G.new_adam(pol), G.new_adam(pol_r), G.new_adam(qf2), G.new_adam(qf_r)
    adam_a, adam_a_r = S.new_alpha_adam(la), S.new_alpha_adam(la_r)
    NP, NQ = T.flat_params(pol).numel(), T.flat_params(qf2).numel()
    stats, want = torch.zeros(5, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda")
    lr, alr, tau, scale, tent = 1e-3, 3e-3, 5e-3, 1.0 / 37, -6.0
    torch.manual_seed(5)
    for t in range(1, 6):
        mag = lambda n: 10.0 ** torch.randint(-4, 1, (n,), device="cuda").float()   # gradients spanning 1e-4 .. 1
        part = torch.randn(rows, NP + 2, device="cuda") * mag(NP + 2)
        partq = torch.randn(2, rows, NQ + 2, device="cuda") * mag(NQ + 2)
        alpha_before = la.double().exp().item()   # the temperature the kernel holds before its step (la and la_r agree to float32 rounding only)
        k.actor_apply(part, scale, adam_pi, lr, 0.9, 0.999, 1e-8, adam_a if learn_alpha else None, alr, tent, stats[2:])
        k.critic_apply(1, partq[1], scale, adam_q, lr, 0.9, 0.999, 1e-8, tau, stats)
        G._adam_on(pol_r, part[:, :NP].sum(0) * scale, adam_pi_r, lr, 0.9, 0.999, 1e-8)
        if learn_alpha:
            adam_a_r["t"] += 1
            adam_step_(la_r, -(part[:, NP].sum(0, keepdim=True) * scale + tent), adam_a_r["m"], adam_a_r["v"], adam_a_r["t"], alr)
        G._adam_on(qf_r, partq[1, :, :NQ].sum(0) * scale, adam_q_r, lr, 0.9, 0.999, 1e-8)
        G.soft_update_(tq_r, qf_r, tau)
        sums = part[:, NP:].double().sum(0)
        want += torch.cat([partq[1, :, NQ:].double().sum(0), sums, (alpha_before * sums[0] - sums[1]).reshape(1)])
        assert adam_pi["t"] == adam_q["t"] == t and adam_a["t"] == (t if learn_alpha else 0)
    pairs = [(T.flat_params(pol), T.flat_params(pol_r)), (adam_pi["m"], adam_pi_r["m"]), (adam_pi["v"], adam_pi_r["v"]), (T.flat_params(qf2), T.flat_params(qf_r)),
             (T.flat_params(tq2), T.flat_params(tq_r)), (adam_q["m"], adam_q_r["m"]), (adam_q["v"], adam_q_r["v"]), (la, la_r)]
    if learn_alpha:
        pairs += [(adam_a["m"], adam_a_r["m"]), (adam_a["v"], adam_a_r["v"])]
        assert la.item() != float(np.float32(np.log(0.7)))
    else:
        assert la.item() == float(np.float32(np.log(0.7))) and adam_a["m"].item() == 0
    for a, b in pairs:
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item(), ((a - b).abs().max().item(), b.abs().max().item())
    # the four sums are float64 sums of the float32 columns; the actor-loss column is exp(log_alpha) sum log pi - sum min Q in float64
    print("apply statistics: %s / %s" % (stats.tolist(), want.tolist()))
    assert (stats[:4] - want[:4]).abs().max().item() <= 1e-12 * want[:4].abs().max().item()
    assert abs(stats[4].item() - want[4].item()) <= 1e-12 * abs(want[4].item())


def test_fused_update_equals_the_torch_update_on_stand_data():
    """4096 stand environments, Torque mode, 8 vector steps into the pool, then three updates of batch 4096 with fused_update True and False from
    the same state, the same indices and the same noises."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import sac as S
    from cassierl_amd import trpo as T
    from cassierl_amd.trajectory import default_gait
    algo = S.make_cassie_sac(4096, kind="stand", control_mode="Torque", trajectory=default_gait(), seed=1, replay_pool_size=4096 * 8, batch_size=4096,
                             min_pool_size=10 ** 9)
    for _ in range(8):
        assert algo.train_step() == 0
    assert algo.last_policy_step_fused and algo.pool.size == 4096 * 8 and algo.pool.top == 0
    assert torch.isfinite(algo.pool.obs).all() and torch.isfinite(algo.pool.nobs).all() and torch.isfinite(algo.pool.rew).all()
    assert algo.pool.act.abs().max().item() <= 1.0 and algo.pool.act.std().item() > 0.1
    nets = (algo.policy, algo.qf1, algo.qf2, algo.target_qf1, algo.target_qf2)
    state0 = [copy.deepcopy(n.state_dict()) for n in nets]
    theta0 = [T.flat_params(n).clone() for n in nets] + [algo.log_alpha.clone()]
    draws = [(algo.sample_indices(), algo.sample_noise()) for _ in range(3)]
    res = {}
    for fused in (True, False):
        for n, sd in zip(nets, state0):
            n.load_state_dict(sd)
        algo.log_alpha.copy_(theta0[-1])
        algo.adam_pi, algo.adam_q1, algo.adam_q2 = G.new_adam(algo.policy), G.new_adam(algo.qf1), G.new_adam(algo.qf2)
        algo.adam_alpha = S.new_alpha_adam(algo.log_alpha)
        algo.fused_update = fused
        for idx, noise in draws:
            algo.update(idx, noise)
            assert algo.last_update_kind == ("sac_kernels" if fused else "torch")
        res[fused] = [T.flat_params(n).clone() for n in nets] + [algo.log_alpha.clone()]
    rels = [((a - b).norm() / b.norm()).item() for a, b in zip(res[True], res[False])]
    moved = [(a - t0).norm().item() for a, t0 in zip(res[False], theta0)]
    print("fused vs torch update, relative difference (actor, qf1, qf2, target_qf1, target_qf2, log_alpha): %s; moved by %s" % (rels, moved))
    assert all(m > 0 for m in moved)
    assert all(r < 1e-5 for r in rels), rels
    algo.env.close()


NP_ALL = 2316 + 4 * 2145 + 1   # actor, four critics, log_alpha


def test_gpu_resume_equals_the_uninterrupted_run(tmp_path):
    """train_sac.py: two epochs, snapshot, one more epoch in a fresh process == three epochs uninterrupted, bit for bit (the ring wraps at 8 steps,
    paths are truncated at 10)."""
    from conftest import ROOT
    script = os.path.join(ROOT, "train_sac.py")
    small = _small(1024)
    snap, b, c = str(tmp_path / "snap.pt"), str(tmp_path / "b.npy"), str(tmp_path / "c.npy")
    _run([sys.executable, script, "--n-epochs", "2", "--snapshot", snap] + small)
    sb = _run([sys.executable, script, "--n-epochs", "1", "--load-policy", snap, "--dump-params", b] + small)
    sc = _run([sys.executable, script, "--n-epochs", "3", "--dump-params", c] + small)
    assert sb[0]["sampler_restored"] and sb[0]["pool_restored"] and sb[0]["pool_size"] == 1024 * 8
    last_b, last_c = sb[-1], sc[-1]
    assert last_b["itr"] == last_c["itr"] == 2 and last_b["updates"] == last_c["updates"] == 6 and last_c["update_kind"] == "sac_kernels"
    for key in ("avg_reward", "qf1_loss", "qf2_loss", "policy_loss", "avg_log_pi", "alpha", "avg_q", "episodes"):
        assert last_b[key] == last_c[key], (key, last_b[key], last_c[key])
    tb, tc = np.load(b), np.load(c)
    assert tb.size == NP_ALL and np.isfinite(tc).all() and tc[-1] != 0.0
    assert np.array_equal(tb, tc)


def test_two_rank_sac_keeps_identical_parameters(tmp_path):
    """train_sac.py on two ranks with 1024 envs each (both on device 0, gloo): finite, identical parameters on both ranks."""
    from conftest import ROOT
    script = os.path.join(ROOT, "train_sac.py")
    out = str(tmp_path / "two.npy")
    env = dict(os.environ, CASSIE_DEVICE_MAP="0,0", CASSIE_BACKEND="gloo")
    args = _small(2048)   # the batch is counted over the two ranks
    st = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
               script, "--n-epochs", "2", "--dump-params", out] + args, timeout=900, env=env)
    assert len(st) == 2 and st[-1]["updates"] == 6 and st[-1]["env_steps"] == 2 * 1024 * 6 and st[-1]["update_kind"] == "sac_kernels"
    t0, t1 = np.load(out), np.load(out + ".rank1.npy")
    assert t0.size == NP_ALL and np.isfinite(t0).all() and np.isfinite(t1).all()
    assert np.array_equal(t0, t1)


def test_sim_policy_rolls_out_a_sac_snapshot(tmp_path):
    from conftest import ROOT
    snap = str(tmp_path / "snap.pt")
    _run([sys.executable, os.path.join(ROOT, "train_sac.py"), "--envs-per-gpu", "512", "--batch-size", "512", "--pool-size", "4096", "--min-pool-size", "1024",
          "--epoch-length", "4", "--n-epochs", "2", "--kind", "stand", "--control-mode", "Torque", "--snapshot", snap])
    assert os.path.exists(snap)
    base = [sys.executable, os.path.join(ROOT, "sim_policy.py"), snap, "--envs", "256", "--max-path-length", "60", "--kind", "stand", "--control-mode", "Torque"]
    det, smp = _run(base + ["--deterministic"])[-1], _run(base)[-1]
    for r, d in ((det, True), (smp, False)):
        assert r["itr"] == 2 and r["envs"] == 256 and r["deterministic"] == d and 0 < r["avg_path_length"] <= 60 and np.isfinite(r["avg_return"])
        assert np.isfinite(r["min_return"]) and np.isfinite(r["max_return"])
    assert det["avg_return"] != smp["avg_return"]


def test_sac_update_timing_batch_65536():
    """One fused update at batch 65 536 against the torch statement, alternated, median of 20 synchronised repeats after warm-up.  A guard, not the
    measurement (tools/ab_sac_update.py): the kernels replace well over a hundred launches with five, so losing to torch means a broken kernel."""
    import torch
    from cassierl_amd import ddpg as G
    from cassierl_amd import sac as S
    pol, qf1, qf2, tq1, tq2 = _nets(26, 6, 9)
    pool, _, _ = _pool_with_margin(pol, qf1, qf2, 26, 6, candidates=200000)
    las = {True: _log_alpha(), False: _log_alpha()}
    k = S.SacKernels(pol, qf1, qf2, tq1, tq2, las[True])
    idx = torch.randint(0, pool.size, (65536,), device="cuda")
    noise = torch.randn(2, 65536, 6, device="cuda")
    adam = {f: (G.new_adam(pol), G.new_adam(qf1), G.new_adam(qf2), S.new_alpha_adam(las[f])) for f in (True, False)}

    def fused():
        k.update(pool, idx, noise[0], noise[1], 0.99, 3e-4, 3e-4, 3e-4, 5e-3, -6.0, *adam[True])

    def torch_update():
        S.sac_update_torch_(pol, qf1, qf2, tq1, tq2, las[False], *adam[False], pool.sample(idx), noise[0], noise[1], 0.99, 3e-4, 3e-4, 3e-4, 5e-3, -6.0)

    out = {}
    for name, fn in (("fused", fused), ("torch", torch_update)) * 2:   # alternated, the second round kept
        for _ in range(5):
            fn()
        ts = []
        for _ in range(20):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        out[name] = float(np.median(ts)) * 1e3
    print("SAC update ms at batch 65536: %s" % out)
    assert out["fused"] < out["torch"]
