"""cn_sac_update and cn_sac_act (csrc/crowdnav_sac.hip) on the device: the reference's learn() goldens (tests/golden/sac.npz), a
float64 statement of the per-row arithmetic (tests/sac_f64.py) at shapes around the tile edges, wrong variants that must be
rejected, argument checks, determinism, the replay path, a hipGraph capture, the act kernel, and the trainer end to end.
`-s` prints the worst error / bound of every quantity."""
import csv
import ctypes as C
import functools
import glob
import math
import os

import numpy as np
import pytest
import torch

import adam_series as A
import sac_f64 as S
import td3_f64 as R
from learner_handle import LearnerHandle, batch_struct, lib
from replay_distinct_ref import _mix_int

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "sac.npz"))
SHAPES = [                                             # (obs_dim, hidden, hidden_v, batch)
    (363, 256, 2, 64), (398, 256, 2, 64), (363, 256, 256, 64),      # the product: both layouts, value net as written / intended
    (46, 32, 2, 16),
] + [(45, h, 2, 40) for h in (15, 16, 17, 31, 32, 33)] + [(45, 24, hv, 40) for hv in (1, 2, 3, 16, 17, 256)] + [
    (20, 48, 2, b) for b in (3, 31, 32, 33, 127, 128, 129)] + [(398, 256, 2, 4096), (64, 4096, 2, 16), (64, 256, 4096, 16)]
DISCRIMINATE = ((46, 32, 2, 16), (45, 33, 3, 40), (363, 256, 2, 64))


class Fused(LearnerHandle):
    """One cn_sac handle on its own float32 copies of the parameters (a dict as tests/sac_f64.py's)."""

    def __init__(self, P, shape, lr=3e-4, replay=None, soft_update=0, tau=5e-3, seed=7, **over):
        self.shape = shape
        self.P = {n: {k: v.detach().clone().float().cuda().contiguous() for k, v in p.items()} for n, p in P.items()}
        super().__init__("sac", S.handle_config(self.P, shape, lr, replay, soft_update, tau, seed, **over), (self.P, replay))

    def update(self, batch, eps=None, sync=True):
        super().update(batch=None if batch is None else batch_struct(tuple(batch) + (eps,)), sync=sync)

    def dev(self, what, shape):
        return self.batch_dev(what, shape).cpu().double()

    def loss(self):
        return super().loss((3,)).cpu().double()

    def rows(self):
        B = self.shape[3]
        rec = self.dev(5, (B, 12))
        return dict(mean=rec[:, 0:2], log_std=rec[:, 2:4], raw=rec[:, 4:6], z=rec[:, 6:8], logp=rec[:, 8], qn=rec[:, 9], a_new=rec[:, 10:12],
                    dl=self.dev(6, (B, 4)), dq=self.dev(7, (B,)), dv=self.dev(8, (B,)), loss=self.loss())


_cuda, _reference = S.cuda, functools.partial(S.reference, device="cuda")


def _same(Pa, Pb):
    return all(torch.equal(Pa[n][k], Pb[n][k]) for n in Pa for k in Pa[n])


def _golden_params(prefix):
    names = dict(actor=dict(w1="linear1.weight", b1="linear1.bias", w2="linear2.weight", b2="linear2.bias", mean_w="mean_linear.weight",
                            mean_b="mean_linear.bias", ls_w="log_std_linear.weight", ls_b="log_std_linear.bias"))
    for n in ("q", "v", "v_t"):
        names[n] = {k: "linear%s.%s" % (k[1], "weight" if k[0] == "w" else "bias") for k in S.NAMES}
    return {n: {k: torch.from_numpy(G["%s.%s.%s" % (prefix, n, f)]) for k, f in m.items()} for n, m in names.items()}


def test_fused_sac_update_on_the_reference_learn_goldens():
    """Four cn_sac_update calls on the reference's batch and eps against sac.Agent.learn's parameters and losses, at the DDPG golden
    test's tolerances: rtol 5e-4, atol 2e-6 on parameters, 1e-5 (relative) on losses.  soft_update = 0: sac.py:290 as committed."""
    shape = (46, 32, 2, 16)
    f = Fused(_golden_params("init"), shape, soft_update=0)
    batch = _cuda([torch.from_numpy(G[k]) for k in ("upd_s", "upd_a", "upd_r", "upd_s2", "upd_d")])
    try:
        for step in range(4):
            f.update(batch, torch.from_numpy(G["eps"][step]).cuda().contiguous())
            want = _golden_params("step%d" % step)
            worst = 0.0
            for n in want:
                for k in want[n]:
                    got, w = f.P[n][k].cpu().double(), want[n][k].double()
                    worst = max(worst, float(((got - w).abs() / (2e-6 + 5e-4 * w.abs())).max()))
            ls = f.loss().numpy()
            print("step %d: worst parameter error / tolerance %.3g, losses %s (golden %s)" % (step, worst, ls, G["loss"][step]))
            assert worst <= 1.0, (step, worst)
            np.testing.assert_allclose(ls, G["loss"][step], rtol=1e-5, atol=0)
    finally:
        f.close()


def _run_case(shape):
    """One update with beta1 = beta2 = 0 (w' = w - lr g / (|g| + eps): invertible per element), eps = a power of two >= every
    gradient element, each optimiser's lr as large against its own gradients as Q's.  -> the case, the float64 reference and its
    bounds, the kernel's rows, its recovered weight gradients {(net, name): g} and their inversion bounds, V_t before, P after."""
    P, batch, eps, eps1, chain = S.make_case(*shape)
    want, Bd = _reference(P, batch, eps)
    top = {n: A.pow2_at_least(max(float(want[k].abs().max()) for k in S.GRADS if k[0] == n)) for n in ("q", "v", "actor")}
    e_ = max(top.values())
    lr = {n: LR * e_ / top[n] for n in top}
    f = Fused(P, shape, soft_update=1, tau=2.0 ** -4, lr_q=lr["q"], lr_v=lr["v"], lr_actor=lr["actor"], eps=e_, beta1=0.0, beta2=0.0)
    try:
        f.update(_cuda(batch), eps.cuda().contiguous())
        got = f.rows()
        P1 = {n: {k: v.cpu() for k, v in p.items()} for n, p in f.P.items()}
    finally:
        f.close()
    g, extra = {}, {}
    for n, k in S.GRADS:
        g[(n, k)] = R.invert_step(P[n][k], P1[n][k], lr[n], e_)
        extra[(n, k)] = R.inversion_bound(g[(n, k)], P[n][k], P1[n][k], lr[n], e_)
    got.update(g)
    return dict(P=P, batch=batch, eps=eps, eps1=eps1, want=want, Bd=Bd, got=got, extra=extra, P1=P1)


def _ratios(got, want, Bd, extra, keys=None):
    """worst |got - want| / bound per quantity: the rows' quantities and the three losses at the propagated bound, a weight
    gradient at that plus what the inversion of its Adam step leaves"""
    return {k: R.worst_ratio(got[k], want[k], Bd[k] + (extra[k] if k in extra else 0.0)) for k in (keys or S.KEYS + S.GRADS)}


LR = 2.0 ** -10
_CASES = {}


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = _run_case(shape)
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_sac_rows_losses_and_gradients_match_float64(shape):
    """Per row: the action, the loss gradients at Q, V and the two heads; the three losses; and EVERY weight gradient of Q, V and
    the actor (trunk and both heads), recovered by inverting the Adam step with beta1 = beta2 = 0 -- each element against float64
    within sac_f64.reference's propagated bound, on inputs with margins: no ReLU mask and no clamp decision differs, and elements
    clamped at -20, clamped at 2 and inside all occur.  The log_std gradient is exactly zero on every clamped element and
    non-zero on every other; V_t follows the stepped V (soft_update = 1).

    What the input choices of sac_f64.make_case leave out: the coef eps / std and coef (eps^2 - 1) terms of the heads' gradients
    are held to float64 only on elements with log_std in [-4, 2] (eps is zero below -4, where float32 keeps no digit of
    z - mean), and never with a saturated tanh (|z - mean| <= 2).  The scaled-gradient rejection of
    test_wrong_variants_are_rejected is per network (its worst tensor), not per tensor."""
    c = _case(shape)
    want, got, P, P1 = c["want"], c["got"], c["P"], c["P1"]
    ratios = _ratios(got, want, c["Bd"], c["extra"])
    print(shape, {str(k): "%.3g" % v for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    raw = want["raw"]
    ins = (raw >= -20) & (raw <= 2)
    if shape[3] >= 3:
        assert bool((raw < -20).any()) and bool((raw > 2).any()) and bool(ins.any())
    g_ls = got["dl"][:, 2:]
    assert bool((g_ls[~ins] == 0).all()) and bool((g_ls[ins] != 0).all())
    for n in ("q", "v", "actor"):                          # no gradient is trivially zero, and zero / twice the gradient is rejected
        keys = [k for k in S.GRADS if k[0] == n]
        assert all(bool((want[k] != 0).any()) for k in keys), n
        for wrong in (0.0, 2.0):
            assert max(_ratios(got, {k: want[k] * wrong for k in keys}, c["Bd"], c["extra"], keys).values()) > 1.0, (n, wrong)
    for k in S.NAMES:                                      # the soft update from the STEPPED V: two roundings (tau a power of two)
        t0, v1 = P["v_t"][k].double(), P1["v"][k].double()
        assert R.worst_ratio(P1["v_t"][k], R.soft_update(t0, v1, 2.0 ** -4), R.soft_bound(t0, v1, 2.0 ** -4)) <= 1.0, k
    assert all(bool(torch.isfinite(v).all()) for p in P1.values() for v in p.values())


SCALE_ERR = S.SCALE_ERR
SCALED = ("dl", "dq", "dv", "loss") + S.GRADS


@pytest.mark.parametrize("shape", DISCRIMINATE, ids=lambda s: "x".join(map(str, s)))
def test_wrong_variants_are_rejected(shape):
    """The acceptance rule above rejects: rsample's gradient, a single squash, the first sample, an unclamped regulariser; and, one
    quantity at a time, each per-row gradient, each loss and each network's weight gradients scaled by 1 + 1e-3.  (V's target
    from a post-update Q: see test_value_target_uses_the_pre_update_q.)"""
    c = _case(shape)
    got, want, Bd, extra = c["got"], c["want"], c["Bd"], c["extra"]
    assert max(_ratios(got, want, Bd, extra).values()) <= 1.0
    for var in ("rsample", "single_squash", "first_sample", "unclamped_regulariser"):
        wrong, wb = _reference(c["P"], c["batch"], c["eps"], variant=var, eps_first=c["eps1"])
        worst = max(_ratios(got, wrong, wb, extra).values())
        print(shape, var, "%.3g" % worst)
        assert worst > 1.0, (var, worst)
    for k in ("dl", "dq", "dv"):
        assert R.worst_ratio(got[k], want[k] * (1 + SCALE_ERR), Bd[k]) > 1.0, k
    for i in range(3):
        assert float((got["loss"][i] - want["loss"][i] * (1 + SCALE_ERR)).abs() / Bd["loss"][i]) > 1.0, ("loss", i)
    for n in ("q", "v", "actor"):
        keys = [k for k in S.GRADS if k[0] == n]
        r = _ratios(got, {k: want[k] * (1 + SCALE_ERR) for k in keys}, Bd, extra, keys)
        print(shape, n, "x (1 + 1e-3):", {k[1]: "%.3g" % v for k, v in r.items()})
        assert max(r.values()) > 1.0, (n, r)


def test_value_target_uses_the_pre_update_q():
    """Q(s, a_new) of the record is the PRE-update Q's: with a huge Q learning rate the stepped Q gives another value."""
    shape = (45, 33, 3, 40)
    P, batch, eps, eps1, chain = S.make_case(*shape)
    want, Bd = _reference(P, batch, eps)
    f = Fused(P, shape, lr_q=0.5)
    try:
        f.update(_cuda(batch), eps.cuda().contiguous())
        got = f.rows()
        assert R.worst_ratio(got["dv"], want["dv"], Bd["dv"]) <= 1.0
        post, pb = _reference({**P, "q": {k: v.cpu() for k, v in f.P["q"].items()}}, batch, eps)
        assert R.worst_ratio(got["dv"], post["dv"], pb["dv"]) > 1.0
    finally:
        f.close()


@pytest.mark.parametrize("shape", [(363, 256, 2, 64), (363, 256, 256, 64), (45, 24, 17, 40), (20, 48, 3, 129)], ids=lambda s: "x".join(map(str, s)))
def test_soft_update_as_written_pulls_the_stepped_v_and_leaves_the_target(shape):
    """soft_update = 0 (sac.py:290 as committed; sac_pull_kernel): V ends as (1 - tau) V' + tau V_t, V' the stepped V that a
    second handle on the same parameters with soft_update = 1 leaves in V; V_t keeps every bit; Q and the actor are the same
    in both.  tau a power of two: two roundings."""
    P, batch, eps, _, _ = S.make_case(*shape)
    tau = 2.0 ** -4
    a, b = Fused(P, shape, soft_update=0, tau=tau), Fused(P, shape, soft_update=1, tau=tau)
    try:
        for h in (a, b):
            h.update(_cuda(batch), eps.cuda().contiguous())
        for k in S.NAMES:
            v1, vt0 = b.P["v"][k].cpu().double(), P["v_t"][k].double()
            assert torch.equal(a.P["v_t"][k].cpu(), P["v_t"][k]), k
            assert not torch.equal(b.P["v"][k].cpu(), P["v"][k]), k
            assert R.worst_ratio(a.P["v"][k].cpu(), R.soft_update(v1, vt0, tau), R.soft_bound(v1, vt0, tau)) <= 1.0, k
            assert R.worst_ratio(a.P["v"][k].cpu(), v1, R.soft_bound(v1, vt0, tau)) > 1.0, k          # the pull happened
        assert all(torch.equal(a.P[n][k], b.P[n][k]) for n in ("actor", "q") for k in a.P[n])
    finally:
        a.close(); b.close()


def test_cn_sac_create_update_and_act_reject_bad_arguments():
    _abi, L = lib()
    shape = (20, 16, 2, 8)
    P, batch, eps, _, _ = S.make_case(*shape)
    err = lambda: L.cn_td3_last_error().decode()
    for over, text in ((dict(hidden=0), "out of range"), (dict(hidden_v=4097), "out of range"), (dict(batch=4097), "out of range"),
                       (dict(soft_update=2), "soft_update"), (dict(log_std_min=3.0), "log_std_min")):
        with pytest.raises(AssertionError):
            Fused(P, shape, **over)
        assert text in err(), (over, err())
    f = Fused(P, shape)
    try:
        assert L.cn_sac_update(None, None, None) != 0 and "null handle" in err()
        assert L.cn_sac_update(f.h, None, None) != 0 and "no explicit batch and no replay ring" in err()
        b = _cuda(batch)
        bad = _abi.CnTd3Batch(b[0].data_ptr(), None, b[2].data_ptr(), b[3].data_ptr(), b[4].data_ptr(), None)
        assert L.cn_sac_update(f.h, C.byref(bad), None) != 0 and "null batch pointer" in err()
        assert L.cn_sac_batch_dev(f.h, 9) is None and L.cn_sac_batch_dev(None, 0) is None
    finally:
        f.close()
    obs, out = torch.zeros((4, 20), device="cuda"), torch.zeros((4, 2), device="cuda")
    act = _abi.CnSacActor(*[f.P["actor"][k].data_ptr() for k in S.ACTOR_NAMES])
    io = dict(obs=obs.data_ptr(), obs_ld=20, n=4, obs_dim=20, hidden=16, deterministic=0, actor=act, max_v=0.22, max_w=2.0, log_std_min=-20.0,
              log_std_max=2.0, eps=None, seed=1, counter=0, twist=out.data_ptr(), mean=None, log_std=None, z=None)
    for over, text in ((dict(hidden=481), "hidden <= 480"), (dict(obs_ld=19), "out of range"), (dict(n=0), "out of range"), (dict(twist=None), "null argument")):
        assert L.cn_sac_act(C.byref(_abi.CnSacActIO(**{**io, **over})), 0, None) != 0 and text in err(), (over, err())


def _ring(shape, cap, size, fill=None, seed=3):
    D, B = shape[0], shape[3]
    g = torch.Generator().manual_seed(seed)
    ring = dict(s=torch.randn((cap, D), generator=g) * 0.5, a=torch.rand((cap, 2), generator=g), r=torch.randn(cap, generator=g),
                s2=torch.randn((cap, D), generator=g) * 0.5, d=(torch.rand(cap, generator=g) < 0.3).float())
    if fill is not None:
        for k in ring:
            ring[k][size:] = fill
    ring = {k: v.cuda().contiguous() for k, v in ring.items()}
    ring["size"] = torch.tensor(size, dtype=torch.int64, device="cuda")
    return ring


def test_two_handles_on_identical_parameters_end_bit_identical():
    shape = (363, 256, 2, 64)
    g = torch.Generator().manual_seed(1)
    P = S.new_params(shape[0], shape[1], shape[2], g)
    ring = _ring(shape, 512, 300)
    a, b = Fused(P, shape, replay=ring), Fused(P, shape, replay=ring)
    try:
        for _ in range(5):
            a.update(None); b.update(None)
        assert _same(a.P, b.P) and torch.equal(a.loss(), b.loss()) and not _same(a.P, {n: {k: v.cuda() for k, v in p.items()} for n, p in P.items()})
    finally:
        a.close(); b.close()


_mix64 = _mix_int           # cn_mix64 on Python ints: stated once, in tests/actor_f64.py


def test_replay_path_samples_only_live_rows_and_its_eps_is_the_documented_draw():
    """batch == NULL: rows [size, capacity) full of NaN never reach the weights or the losses; row m of update c is ring row
    mix64(mix64(seed ^ mix64(c)) ^ m) % size and its eps Box-Muller on the same hash with c ^ 0x5bd1e995."""
    shape = (45, 33, 2, 40)
    g = torch.Generator().manual_seed(2)
    P = S.new_params(shape[0], shape[1], shape[2], g)
    for size in (1, 37, 64):
        ring = _ring(shape, 64, size, fill=float("nan"))
        f = Fused(P, shape, replay=ring, seed=7)
        try:
            for c in range(3):
                f.update(None)
                assert bool(torch.isfinite(f.loss()).all()), (size, c)
                xs, e = f.dev(0, (40, 47)), f.dev(4, (40, 2))
                for m in (0, 1, 39):
                    row = _mix64(_mix64(7 ^ _mix64(c)) ^ m) % size
                    assert torch.equal(xs[m, :45].float(), ring["s"][row].cpu())
                    h = _mix64(_mix64(7 ^ _mix64(c ^ 0x5bd1e995)) ^ m)
                    u1 = (np.float32(h >> 40) + np.float32(1)) * np.float32(1.0 / 16777217.0)
                    u2 = np.float32((h >> 8) & 0xffffff) * np.float32(1.0 / 16777216.0)
                    rr = math.sqrt(-2.0 * math.log(float(u1)))
                    want = (rr * math.cos(6.28318530718 * float(u2)), rr * math.sin(6.28318530718 * float(u2)))
                    np.testing.assert_allclose(e[m].numpy(), want, rtol=2e-5, atol=2e-6)
            assert all(bool(torch.isfinite(v).all()) for p in f.P.values() for v in p.values()), size
        finally:
            f.close()


def test_replay_of_live_size_one_equals_the_explicit_batch_and_size_zero():
    """batch == NULL on a ring of live size 1 equals, bit for bit, an explicit batch of B copies of row 0 with the eps the
    replay handle drew (cn_sac_batch_dev 4); *size_dev = 0 equals size 1."""
    shape = (45, 33, 2, 40)
    B = shape[3]
    P = S.new_params(shape[0], shape[1], shape[2], torch.Generator().manual_seed(5))
    ring1, ring0, ringx = _ring(shape, 64, 1), _ring(shape, 64, 1), _ring(shape, 64, 1)
    ring0["size"].zero_()
    batch = tuple(ringx[k][:1].expand((B,) + ringx[k].shape[1:]).contiguous() for k in ("s", "a", "r", "s2", "d"))
    hs = [Fused(P, shape, replay=ring1, seed=7), Fused(P, shape, replay=ring0, seed=7), Fused(P, shape, seed=7)]
    try:
        for _ in range(3):
            hs[0].update(None); hs[1].update(None)
            hs[2].update(batch, hs[0].dev(4, (B, 2)).float().cuda().contiguous())
        assert _same(hs[0].P, hs[2].P) and _same(hs[0].P, hs[1].P)
        assert torch.equal(hs[0].loss(), hs[2].loss()) and torch.equal(hs[0].loss(), hs[1].loss())
        assert not _same(hs[0].P, {n: {k: v.cuda() for k, v in p.items()} for n, p in P.items()})
    finally:
        for h in hs:
            h.close()


def test_graph_capture_of_the_update_replays_bit_for_bit():
    """One stream, a straight chain of launches: a captured update replayed three times equals three eager updates."""
    shape = (363, 256, 2, 64)
    g = torch.Generator().manual_seed(4)
    P = S.new_params(shape[0], shape[1], shape[2], g)
    ring = _ring(shape, 512, 300)
    eager, graphed = Fused(P, shape, replay=ring), Fused(P, shape, replay=ring)
    try:
        for _ in range(3):
            eager.update(None)
        P0 = {n: {k: v.clone() for k, v in p.items()} for n, p in graphed.P.items()}
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            graphed.update(None, sync=False)
        torch.cuda.synchronize()
        assert _same(P0, graphed.P)                              # capturing ran nothing
        for _ in range(3):
            gr.replay()
        torch.cuda.synchronize()
        assert _same(eager.P, graphed.P) and torch.equal(eager.loss(), graphed.loss())
    finally:
        eager.close(); graphed.close()


@pytest.mark.parametrize("n", [1, 16, 4096])
def test_cn_sac_act_matches_float64(n):
    """Supplied eps and deterministic, a row stride larger than obs_dim (mean, log_std, z and the twist; the tile edges, the clamp
    and the documented draw: tests/test_gpu_sac_act_f64.py); drawn eps: mean and variance of 2n unit normals within
    5 standard errors (|mean| <= 5 / sqrt(2n), |var - 1| <= 5 sqrt(2 / (2n)))."""
    from crowdnav.sac import Agent
    ag = Agent(obs_dim=363, hidden=256, device="cuda:0", seed=5, memory_size=16)
    with torch.no_grad():
        ag.actor.log_std_linear.weight.mul_(100); ag.actor.mean_linear.weight.mul_(30)
    g = torch.Generator().manual_seed(n)
    buf = (torch.rand((n, 370), generator=g) * 3.5).cuda()
    obs = buf[:, :363]
    eps = torch.randn((n, 2), generator=g).cuda()
    p = {k: v.detach().double().cpu() for k, v in zip(S.ACTOR_NAMES, [ag.actor.linear1.weight, ag.actor.linear1.bias, ag.actor.linear2.weight,
         ag.actor.linear2.bias, ag.actor.mean_linear.weight, ag.actor.mean_linear.bias, ag.actor.log_std_linear.weight, ag.actor.log_std_linear.bias])}
    mean, raw, _, _ = S.trunk(p, obs.double().cpu())
    ls = raw.clamp(-20, 2)
    for det in (False, True):
        z = mean if det else eps.double().cpu() * ls.exp() + mean
        t = torch.tanh(z)
        want = torch.stack([torch.sigmoid(t[:, 0]) * 0.22, torch.tanh(t[:, 1]) * 2.0], 1)
        m_, l_, z_ = (torch.empty((n, 2), device="cuda") for _ in range(3))
        got = ag.act_fused(obs, eps=None if det else eps, deterministic=det, mean=m_, log_std=l_, z=z_)
        torch.cuda.synchronize()
        # forward error of the trunk: chain x 2^-24 x magnitudes; the heads are 1-Lipschitz in z up to max_w
        chain = 363 / 16 + 2 * 256 / 16 + 64
        h1a = obs.double().cpu().abs() @ p["w1"].abs().T + p["b1"].abs()
        h2a = h1a @ p["w2"].abs().T + p["b2"].abs()
        e_mean = chain * S.EPS32 * (h2a @ p["mean_w"].abs().T + 1)
        e_raw = chain * S.EPS32 * (h2a @ p["ls_w"].abs().T + 1)
        e_z = e_mean + (0 if det else eps.double().cpu().abs() * ls.exp() * (e_raw + 8 * S.EPS32)) + 8 * S.EPS32 * (z.abs() + 1)
        assert bool(((m_.cpu().double() - mean).abs() <= e_mean).all())
        assert bool(((z_.cpu().double() - z).abs() <= e_z).all())
        # the clamp is 1-Lipschitz: every element within e_raw; exactly the edge where float64 is past it by more than e_raw
        ld = l_.cpu().double()
        assert bool(((ld - ls).abs() <= e_raw).all())
        assert bool((ld[raw < -20 - e_raw] == -20.0).all()) and bool((ld[raw > 2 + e_raw] == 2.0).all())
        assert bool(((got.cpu().double() - want).abs() <= 2.0 * e_z + 8 * S.EPS32).all())
        np.testing.assert_allclose(got.cpu().numpy(), ag.act(obs, eps=eps, deterministic=det).cpu().numpy(), rtol=0, atol=float(2 * e_z.max() + 1e-6))
    if n == 4096:
        with torch.no_grad():
            ag.actor.log_std_linear.weight.zero_(); ag.actor.log_std_linear.bias.zero_()       # std = 1: z - mean = eps
        m_, z_ = torch.empty((n, 2), device="cuda"), torch.empty((n, 2), device="cuda")
        ag.act_fused(obs, mean=m_, z=z_)
        e = (z_ - m_).double().cpu().reshape(-1)
        k = e.numel()
        assert abs(float(e.mean())) <= 5 / math.sqrt(k) and abs(float(e.var()) - 1) <= 5 * math.sqrt(2.0 / k)
        z2 = torch.empty((n, 2), device="cuda")
        ag.act_fused(obs, z=z2)
        assert not torch.equal(z_, z2)                            # the call counter keys the draw


@pytest.mark.parametrize("learner", ["fused", "torch"])
def test_trainer_runs_sac_end_to_end_and_evaluates_its_checkpoint(tmp_path, learner):
    """python -m crowdnav.train --algo sac --envs 16 --updates 16: the three checkpoints under the reference's names, the CSV,
    finite losses; --evaluate --load reads them back."""
    from crowdnav import train as T
    from crowdnav.sac import Agent
    out = str(tmp_path / "run")
    agent, episodes = T.main(["--algo", "sac", "--scenario", "bench", "--envs", "16", "--updates", "16", "--launches", "120", "--max-steps", "25",
                              "--memory", "20000", "--log-every", "40", "--checkpoint-every", "50", "--seed", "3", "--csv", "--out", out,
                              "--learner", learner])
    assert isinstance(agent, Agent) and agent.batch_size == 64 and agent.obs_dim == 363 and agent.hidden_v == 2 and episodes > 16
    assert bool(getattr(agent, "_fused", None)) == (learner == "fused")
    latest = int(open(os.path.join(out, "latest_checkpoint.txt")).read().split()[0])
    assert latest == episodes
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, "sac_*_model_ep%d.pt" % latest)))
    assert names == sorted("sac_%s_model_ep%d.pt" % (k, latest) for k in ("actor", "critic_v", "critic_soft_q"))
    rows = list(csv.reader(open(os.path.join(out, "sac_training.csv"))))
    assert len(rows) - 1 == episodes and all(len(r) == 8 for r in rows)
    sd = torch.load(os.path.join(out, "sac_critic_v_model_ep%d.pt" % latest), map_location="cuda")
    for k, v in agent.v_t.state_dict().items():
        assert torch.equal(sd[k], v)
    loss = agent.learn()
    assert loss is not None and loss.shape == (3,) and bool(torch.isfinite(loss).all())
    assert all(bool(torch.isfinite(p).all()) for m in (agent.actor, agent.q, agent.v, agent.v_t) for p in m.parameters())
    st = T.main(["--algo", "sac", "--evaluate", "--load", out, "--scenario", "bench", "--envs", "32", "--max-steps", "20", "--seed", "4", "--out", out])
    assert len(st.rows) == 32 and os.path.exists(os.path.join(out, "sac_training_test_bench.csv"))
