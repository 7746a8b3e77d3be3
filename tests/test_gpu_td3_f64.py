"""cn_td3_update (csrc/crowdnav_td3.hip) against a float64 statement of the same TD3 update (tests/td3_f64.py), with the
gradients themselves observed rather than only the weights after Adam.

Adam with beta1 = beta2 = 0 steps w' = w - lr g / (|g| + eps); the tests invert that per element and compare the recovered
gradient of every tensor of Q1, Q2 and the actor with float64 at LAMBDA x the float32 rounding error propagated through the
networks' signed Jacobians (td3_f64.propagated_bounds).  The critics' gradients come from
a call with lr_actor = 0, the actor's from a call with lr_critic = 0, so the steps do not mix.  Every ReLU mask is made
unambiguous by construction (td3_f64.establish_margins) and dead units are planted, whose weights must come back bit for bit.
`-s` prints the worst error / bound of every tensor."""
import copy
import ctypes as C

import pytest
import torch

import adam_series as A
import td3_f64 as R
from learner_handle import LearnerHandle, batch_struct, lib, mlp_struct, ring_fields

pytestmark = pytest.mark.gpu

CFG = dict(gamma=0.99, tau=2.0 ** -4, max_v=0.22, max_w=2.0, noise_std=0.25, noise_clip=0.5)
LR = 1024.0       # the step dominates |w| for all but the smallest gradients: the inversion's absolute error ~ u |w| eps / LR

# (obs_dim, hidden, batch) and the kernel constant each probes (launch_gemm's tiles: F 16 x 16, G 16 x 32, H 32 x 32; the
# critics' q partial sums qnt = (H + 15) / 16, the action gradient's dant = (H + 31) / 32; F reduces Dc = obs_dim + 2 in blocks
# of 16 = 4 wavefronts x 4-wide steps, TD3_FKB = 8 blocks in flight; H splits the batch over 4 wavefronts in steps of 4)
SHAPES = [
    (398, 256, 128),                                   # the product
    (46, 32, 16),                                      # the reference's learn() goldens
] + [(45, h, 40) for h in (1, 4, 15, 16, 17, 31, 32, 33, 257)] + [   # hidden around the 16 / 32 tiles, qnt and dant
    (dc - 2, 40, 24) for dc in (3, 31, 32, 33)] + [                 # Dc: a lone ragged block, and around 2 full blocks of 16
    (20, 48, b) for b in (1, 3, 33, 127, 129)] + [                  # batch around the 32-row weight-gradient tile and its 4-row steps
    (398, 256, 4096),                                  # the batch limit
    (398, 4096, 64),                                   # the hidden limit
]
ALL_DONE = (45, 17, 40)                                # y = r in every row
DISCRIMINATE = ((398, 256, 128), (45, 33, 40))         # the wrong-variant checks
SCALE_ERR = 1e-3                                      # the uniform gradient scale error the DISCRIMINATE shapes must reject


def make_case(shape, seed=0, margins=True):
    obs_dim, hidden, B = shape
    g = torch.Generator().manual_seed(seed + 1000 * hidden + B)
    P = R.new_params(obs_dim, hidden, g, dtype=torch.float32, device="cuda")
    s = torch.randn((B, obs_dim), generator=g) * 0.5
    a = torch.stack([torch.rand(B, generator=g) * 0.22, torch.rand(B, generator=g) * 4 - 2], 1)
    r = 2 + 0.5 * torch.randn(B, generator=g)
    s2 = torch.randn((B, obs_dim), generator=g) * 0.5
    d = (torch.rand(B, generator=g) < 0.3).float()
    if shape == ALL_DONE:
        d[:] = 1
    elif B >= 2:
        d[0], d[1] = 0, 1
    nz = torch.randn((B, 2), generator=g)
    nz[0::5, 0] = 2.0; nz[1::5, 1] = -2.0; nz[2::7] = 10.0         # exactly +-noise_clip (2 x 0.25 = 0.5), and beyond it
    batch = tuple(x.float().cuda().contiguous() for x in (s, a, r, s2, d, nz))
    dead = R.plant_dead_units(P, hidden) if margins else {}
    N = R.chain_length(*shape)
    rep = R.establish_margins(P, batch, CFG, N) if margins else {}
    return P, batch, N, dead, rep


class Fused(LearnerHandle):
    """One cn_td3 handle on its own float32 copies of the parameters."""

    def __init__(self, P, shape, lr_c, lr_a, eps, beta1=0.0, beta2=0.0, tau=CFG["tau"], replay=None, noise_std=CFG["noise_std"]):
        self.P = {n: {k: v.detach().clone().contiguous() for k, v in p.items()} for n, p in P.items()}
        cfg = lib()[0].CnTd3Config(obs_dim=shape[0], hidden=shape[1], batch=shape[2], policy_delay=2, gamma=CFG["gamma"], tau=tau,
                                   lr_actor=lr_a, lr_critic=lr_c, beta1=beta1, beta2=beta2, eps=eps, noise_std=noise_std,
                                   noise_clip=CFG["noise_clip"], max_v=CFG["max_v"], max_w=CFG["max_w"], reserved=0.0, seed=7,
                                   **{n: mlp_struct(self.P[n], R.NAMES) for n in R.NETS}, **ring_fields(replay))
        super().__init__("td3", cfg, (self.P, replay))

    def update(self, batch, do_actor):
        super().update(int(do_actor), batch=batch_struct(batch))

    def loss(self):
        return float(super().loss())


def _check_soft(P0, P1, tgt, src, tau, report, label):
    """targets = t (1 - tau) + (the local network's weights AFTER its step) tau; from the pre-step weights it would fail."""
    worst = wrong = 0.0
    for k in R.NAMES:
        t0 = P0[tgt][k].double()
        want = R.soft_update(t0, P1[src][k].double(), tau)
        bnd = R.soft_bound(t0, P1[src][k].double(), tau)
        worst = max(worst, R.worst_ratio(P1[tgt][k], want, bnd))
        wrong = max(wrong, R.worst_ratio(P1[tgt][k], R.soft_update(t0, P0[src][k].double(), tau), bnd))
    report.append("%-18s soft %-7s worst/bound %.3g  (from the pre-step weights: %.3g)" % (label, tgt, worst, wrong))
    assert worst <= 1.0, (label, tgt, worst)
    return wrong


def _tightness(ref):
    """sum of the bound over sum of |g|, worst tensor: how wide the tolerance is relative to the gradient"""
    return max([float(ref["bound"][k].sum() / ref["g"][k].abs().sum()) for k in R.NAMES if bool((ref["g"][k] != 0).any())] or [0.0])


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_fused_td3_gradients_losses_and_soft_updates_match_float64(shape):
    report = []
    try:
        _gradients_losses_and_soft_updates(shape, report)
    finally:
        print("\n".join(report))


def _gradients_losses_and_soft_updates(shape, report):
    obs_dim, hidden, B = shape
    P0, batch, N, dead, rep = make_case(shape)
    worst_margin, _, _ = R.margin_report(P0, batch, CFG, N)
    mixed = sum(v["mixed"] for v in rep.values()); units = sum(v["units"] for v in rep.values())
    assert worst_margin >= 1.0, ("no ReLU margin", worst_margin)
    P64, b64 = R.to64(P0), R.batch_double(batch)
    ref = R.critic_grads(P64, b64, CFG)
    report.append("%s: strict chain %d, margins >= %.3g bounds, %d of %d hidden units with a mixed mask" % (
        shape, N, worst_margin, mixed, units))
    t = ref["t"]
    if B >= 5:
        frac = float((t["q1t"] < t["q2t"]).double().mean())
        assert 0.2 <= frac <= 0.8, frac
    if B >= 2 and shape != ALL_DONE:
        assert 0 < float(b64[4].mean()) < 1
    if shape == ALL_DONE:
        assert torch.equal(t["y"], b64[2])
    lg = R.actor_fwd(P64["actor"], b64[0], CFG)["logits"]
    assert float(lg.abs().max()) >= 7.0
    eps_c = A.pow2_at_least(max(float(ref[n]["g"][k].abs().max()) for n in ("q1", "q2") for k in R.NAMES))
    for do_actor in (0, 1):
        k_ = Fused(P0, shape, LR, 0.0, eps_c)
        k_.update(batch, do_actor)
        P1 = k_.P
        loss = k_.loss()
        k_.close()
        l1 = float(ref["l1"])
        report.append("loss %.9g float64 %.9g (relative %.2g)" % (loss, l1, abs(loss - l1) / abs(l1)))
        assert abs(loss - l1) <= 1e-5 * abs(l1), (loss, l1)
        assert R.same(P0, P1, "actor")
        for net in ("q1", "q2"):
            g, extra = R.recover(P0, P1, net, LR, eps_c)
            ratios = R.compare_grads(g, ref[net]["g"], ref[net]["bound"], extra)
            report.append("critic do_actor=%d %-7s worst/bound " % (do_actor, net) + " ".join("%s %.3g" % kv for kv in ratios.items())
                          + "   bound/|g| %.2g" % _tightness(ref[net]))
            assert R.accept(ratios), (net, ratios)
            R.check_dead(P0, P1, net, dead)
            R.rejects_gross(g, ref[net], extra, net)
            if shape in DISCRIMINATE and do_actor == 0:
                scaled = {kk: v * (1 + SCALE_ERR) for kk, v in ref[net]["g"].items()}
                tiled = dict(ref[net]["g"], w2=R.zero_tile(ref[net]["g"]["w2"]))
                assert not R.accept(R.compare_grads(g, scaled, ref[net]["bound"], extra)), "x (1 + %g) accepted" % SCALE_ERR
                assert not R.accept(R.compare_grads(g, tiled, ref[net]["bound"], extra)), "zeroed tile accepted"
                if net == "q1":
                    wy = R.critic_grads(P64, b64, CFG, y_from="q1t")
                    assert not R.accept(R.compare_grads(g, wy["q1"]["g"], wy["q1"]["bound"], extra)), "y from Q1_t alone accepted"
        if do_actor:
            wrong = [_check_soft(P0, P1, tg, src, CFG["tau"], report, "critic call")
                     for tg, src in (("q1_t", "q1"), ("q2_t", "q2"), ("actor_t", "actor"))]
            assert min(wrong[:2]) > 100.0              # the pre-step soft update fails by orders of magnitude
        else:
            assert all(R.same(P0, P1, n) for n in ("q1_t", "q2_t", "actor_t"))
    # the actor's gradient: lr_critic = 0, so Q1 is the critic the actor loss runs through
    refa = R.actor_grads(P64, b64[0], CFG, N_mask=N)
    assert refa["flip_rows"] == 0
    eps_a = A.pow2_at_least(max(float(refa["g"][k].abs().max()) for k in R.NAMES))
    k_ = Fused(P0, shape, 0.0, LR, eps_a)
    k_.update(batch, 1)
    P1 = k_.P
    k_.close()
    assert R.same(P0, P1, "q1") and R.same(P0, P1, "q2")
    g, extra = R.recover(P0, P1, "actor", LR, eps_a)
    ratios = R.compare_grads(g, refa["g"], refa["bound"], extra)
    report.append("actor             worst/bound " + " ".join("%s %.3g" % kv for kv in ratios.items())
                  + "   bound/|g| %.2g" % _tightness(refa))
    assert R.accept(ratios), ratios
    R.check_dead(P0, P1, "actor", dead)
    R.rejects_gross(g, refa, extra, "actor")
    if hidden >= 4:    # (hidden 1: the lone Q1 unit can be inactive on every (s, pi(s)) row, and the actor's gradient exactly 0)
        assert any(bool((v != 0).any()) for v in refa["g"].values())
    if shape in DISCRIMINATE:
        scaled = {kk: v * (1 + SCALE_ERR) for kk, v in refa["g"].items()}
        assert not R.accept(R.compare_grads(g, scaled, refa["bound"], extra)), "actor x (1 + %g) accepted" % SCALE_ERR
        assert not R.accept(R.compare_grads(g, dict(refa["g"], w2=R.zero_tile(refa["g"]["w2"])), refa["bound"], extra))
    for tg, src in (("q1_t", "q1"), ("q2_t", "q2"), ("actor_t", "actor")):
        _check_soft(P0, P1, tg, src, CFG["tau"], report, "actor call")


@pytest.mark.parametrize("shape", DISCRIMINATE, ids=["%dx%dx%d" % s for s in DISCRIMINATE])
def test_fused_td3_adam_across_four_updates_matches_float64(shape):
    """Four updates with policy_delay 2 (the actor on the 1st and 3rd: its step count 1, 2 where the critics' is 1, 3), betas
    0.5 / 0.75, eps >= max |g|.  Before each update the margins are re-established on the kernel's current weights and the float64
    gradients computed there; float64 Adam carries the moments and each optimizer's own bias corrections.  The actor's gradient
    runs through the Q1 the kernel stepped in the same update (read back); the actor through the pre-update Q1 and, on the 3rd
    update, the actor's bias correction with the critics' step count are rejected.  The soft updates follow the post-step weights."""
    P0, batch, N, dead, _ = make_case(shape, seed=5)
    b64 = R.batch_double(batch)
    ref0 = R.critic_grads(R.to64(P0), b64, CFG)
    eps = 2 * A.pow2_at_least(max(float(ref0[n]["g"][k].abs().max()) for n in ("q1", "q2") for k in R.NAMES))
    lr_c, lr_a, b1, b2 = 2.0 ** -2, 2.0 ** -8, 0.5, 0.75
    k_ = Fused(P0, shape, lr_c, lr_a, eps, beta1=b1, beta2=b2)
    oc = {n: R.Adam64(lr_c, b1, b2, eps) for n in ("q1", "q2")}
    oa = R.Adam64(lr_a, b1, b2, eps)
    gerr = {}
    report = []
    try:
        for step in range(4):
            do_actor = step % 2 == 0
            if step:
                R.establish_margins(k_.P, batch, CFG, N, rescale=False)
            assert R.margin_report(k_.P, batch, CFG, N)[0] >= 1.0
            pre = R.to64(k_.P)
            c = R.critic_grads(pre, b64, CFG)
            assert max(float(c[n]["g"][kk].abs().max()) for n in ("q1", "q2") for kk in R.NAMES) <= eps
            k_.update(batch, do_actor)
            post = R.to64(k_.P)
            worst = 0.0
            for n in ("q1", "q2"):
                oc[n].t += 1
                for kk in R.NAMES:
                    w_pred, sb = A.tensor_step(oc[n], gerr, n, kk, pre[n][kk], c[n]["g"][kk], c[n]["bound"][kk], eps)
                    worst = max(worst, R.worst_ratio(post[n][kk], w_pred, sb))
            report.append("update %d critics worst/bound %.3g" % (step, worst))
            assert worst <= 1.0
            if do_actor:
                a_ok = R.actor_grads(pre, b64[0], CFG, q1=post["q1"], N_mask=N)
                a_pre = R.actor_grads(pre, b64[0], CFG)
                oa.t += 1
                res = {}
                before = copy.deepcopy(oa)                 # the variants start from the moments before this step
                for name, ag, tt in (("right", a_ok, None), ("pre-update Q1", a_pre, None), ("critics' step count", a_ok, oc["q1"].t)):
                    o = copy.deepcopy(before) if name != "right" else oa
                    w = 0.0
                    ge = gerr if name == "right" else dict(gerr)      # only the right series' bounds are carried on
                    for kk in R.NAMES:
                        w_pred, sb = A.tensor_step(o, ge, "actor", kk, pre["actor"][kk], ag["g"][kk], ag["bound"][kk], eps, t=tt)
                        w = max(w, R.worst_ratio(post["actor"][kk], w_pred, sb))
                    res[name] = w
                report.append("update %d actor worst/bound %.3g (ambiguous rows %d); pre-update Q1 %.3g; critics' step count %.3g" % (
                    step, res["right"], a_ok["flip_rows"], res["pre-update Q1"], res["critics' step count"]))
                assert res["right"] <= 1.0 and res["pre-update Q1"] > 1.0
                if oa.t != oc["q1"].t:
                    assert res["critics' step count"] > 1.0
                for tg, src in (("q1_t", "q1"), ("q2_t", "q2"), ("actor_t", "actor")):
                    for kk in R.NAMES:
                        want = R.soft_update(pre[tg][kk], post[src][kk], CFG["tau"])
                        assert R.worst_ratio(post[tg][kk], want, R.soft_bound(pre[tg][kk], post[src][kk], CFG["tau"])) <= 1.0
    finally:
        k_.close()
    print("\n".join(["%s:" % (shape,)] + report))


def test_cn_td3_create_rejects_shapes_out_of_range():
    _abi, L = lib()
    z = torch.zeros(16, device="cuda")
    m = _abi.CnTd3Mlp(*([z.data_ptr()] * 6))
    for obs_dim, hidden, batch in ((8, 16, 0), (8, 16, 4097), (8, 0, 16), (8, 4097, 16), (0, 16, 16)):
        cfg = _abi.CnTd3Config(obs_dim=obs_dim, hidden=hidden, batch=batch, policy_delay=2, actor=m, actor_t=m, q1=m, q1_t=m, q2=m, q2_t=m)
        h = C.c_void_p()
        assert L.cn_td3_create(C.byref(cfg), 0, C.byref(h)) == -2            # CN_ERR_CONFIG
        assert b"out of range" in L.cn_td3_last_error()
        assert not h.value


def test_two_handles_on_identical_parameters_end_bit_identical():
    shape = (45, 33, 40)
    P0, batch, _, _, _ = make_case(shape, margins=False)
    a = Fused(P0, shape, 3e-4, 3e-4, 1e-8, beta1=0.9, beta2=0.999, tau=0.005)
    b = Fused(P0, shape, 3e-4, 3e-4, 1e-8, beta1=0.9, beta2=0.999, tau=0.005)
    try:
        for step in range(4):
            a.update(batch, step % 2 == 0)
            b.update(batch, step % 2 == 0)
        assert all(R.same(a.P, b.P, n) for n in R.NETS)
        assert a.loss() == b.loss()
    finally:
        a.close(); b.close()


def _ring(shape, cap, size, fill=float("nan"), seed=3):
    obs_dim, _, _ = shape
    g = torch.Generator().manual_seed(seed)
    ring = dict(s=torch.randn((cap, obs_dim), generator=g) * 0.5, a=torch.rand((cap, 2), generator=g),
                r=torch.randn(cap, generator=g), s2=torch.randn((cap, obs_dim), generator=g) * 0.5, d=(torch.rand(cap, generator=g) < 0.3).float())
    if fill is not None:
        for k in ring:
            ring[k][size:] = fill
    ring = {k: v.float().cuda().contiguous() for k, v in ring.items()}
    ring["size"] = torch.tensor([size], dtype=torch.int64, device="cuda")
    return ring


def test_replay_path_samples_only_live_rows():
    """batch == NULL: indices drawn on the device from [0, *size_dev), *size_dev <= 0 taken as 1.  (a) With noise_std 0 a ring
    of live size 1 equals an explicit batch of B copies of row 0, bit for bit; (b) *size_dev = 0 equals size 1; (c) rows
    [size, capacity) full of NaN or of a finite sentinel 1e30 never reach the weights or the loss, at sizes 1, 37 (not a power of
    two), 63 and 64."""
    shape = (45, 33, 40)
    B = shape[2]
    P0, _, _, _, _ = make_case(shape, margins=False)
    args = dict(lr_c=3e-4, lr_a=3e-4, eps=1e-8, beta1=0.9, beta2=0.999, tau=0.005, noise_std=0.0)
    ring1 = _ring(shape, 64, 1)
    ring0 = _ring(shape, 64, 1)
    ring0["size"].zero_()
    ringx = _ring(shape, 64, 1)
    batch = tuple(ringx[k][:1].expand((B,) + ringx[k].shape[1:]).contiguous() for k in ("s", "a", "r", "s2", "d")) + (
        torch.zeros((B, 2), device="cuda"),)
    hs = [Fused(P0, shape, replay=ring1, **args), Fused(P0, shape, replay=ring0, **args), Fused(P0, shape, **args)]
    try:
        for step in range(3):
            hs[0].update(None, step % 2 == 0)
            hs[1].update(None, step % 2 == 0)
            hs[2].update(batch, step % 2 == 0)
        assert all(R.same(hs[0].P, hs[2].P, n) for n in R.NETS)
        assert all(R.same(hs[0].P, hs[1].P, n) for n in R.NETS)
    finally:
        for h in hs:
            h.close()
    # (d) a finite sentinel 1e30 in rows [size, capacity): a sampled dead row (an off-by-one in the index) would make y and the
    # loss ~1e60 -- every update's loss stays of the order of the live rows' (|r| < 5, |q| < 10)
    for fill in (float("nan"), 1e30):
        for size in (1, 37, 63, 64):
            ring = _ring(shape, 64, size, fill=fill)
            h = Fused(P0, shape, replay=ring, **dict(args, noise_std=0.2))
            try:
                for step in range(4):
                    h.update(None, step % 2 == 0)
                    assert h.loss() < 1e3, (fill, size, step, h.loss())
                assert all(bool(torch.isfinite(v).all()) for p in h.P.values() for v in p.values()), (fill, size)
                assert not R.same(P0, h.P, "q1")
            finally:
                h.close()
