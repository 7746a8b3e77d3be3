"""cn_dqn_act and cn_dqn_update (csrc/crowdnav_dqn.hip) held to the float64 statement of tests/dqn_f64.py at the tile edges of the
GEMMs only DQN instantiates (GATE = true, td3_wgrad_kernel<true> with the RMSprop epilogue, the I = 3 weight-gradient job, R = 2B
stacked rows) and at the limits hidden = 4096 and batch = 4096.  Raw cn_dqn handles through crowdnav._abi, so hidden sizes above
cn_dqn_act's 480 can be updated.  Every tolerance is a bound derived from the arithmetic (dqn_f64.bounded: float32 unit roundoff
propagated through the signed Jacobians, times td3_f64.LAMBDA); integers -- actions, chunk marks, flags, counters, replay rows --
are compared exactly.  `-s` prints the worst error / bound of every tensor and shape, and the counts of integers compared.

RMSprop with rho = 0 steps w' = w - lr g / (|g| + eps); with lr and eps powers of two the tests invert that per element
(td3_f64.invert_step) and so read the gradient the kernel used."""
import ctypes as C

import numpy as np
import pytest
import torch

import dqn_f64 as Q
import td3_f64 as R
from learner_handle import LearnerHandle, batch_struct, lib, mlp_struct, ring_fields, stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
GAMMA = 0.99
CN_ERR_CONFIG = -2
SHAPE_IDS = ["%d|%dx%dx%d" % s for s in Q.UPDATE_SHAPES]


def _mlp(p):
    return mlp_struct(p, R.NAMES)


class Fused(LearnerHandle):
    """One cn_dqn handle on its own float32 copies of the online and target parameters."""

    def __init__(self, p, pt, shape, lr, rho, eps, target_every=1 << 30, learn_start=0, seed=7, replay=None):
        self.shape = shape
        self.p = {k: v.detach().clone().contiguous() for k, v in p.items()}
        self.pt = {k: v.detach().clone().contiguous() for k, v in pt.items()}
        D, ld, H, B = shape
        cfg = lib()[0].CnDqnConfig(obs_dim=D, obs_ld=ld, hidden=H, batch=B, gamma=GAMMA, lr=lr, rho=rho, eps=eps, target_every=target_every,
                                    learn_start=learn_start, q=_mlp(self.p), q_t=_mlp(self.pt), seed=seed, **ring_fields(replay))
        super().__init__("dqn", cfg, (self.p, self.pt, replay))

    def update(self, batch=None, perm=None, sync=True):
        if batch is not None:
            pm = None if perm is None else (perm if torch.is_tensor(perm) else torch.as_tensor(np.asarray(perm), dtype=torch.int32).to(DEV))
            batch = batch_struct(tuple(batch) + (pm,), "CnDqnBatch")
        super().update(batch=batch, sync=sync)

    def view(self, what, shape, dtype=torch.float32):
        return self.batch_dev(what, shape, {torch.float32: "<f4", torch.int32: "<i4", torch.int64: "<i8"}[dtype])

    def loss(self):
        return super().loss((2,)).double().cpu().numpy()

    def flags(self):
        return self.view(5, (8,), torch.int32).cpu().numpy()[:5]

    def counter(self):
        return int(self.view(8, (1,), torch.int64)[0])


def _same(p0, p1):
    return all(torch.equal(p0[k], p1[k]) for k in R.NAMES)


def _fmt(r):
    return " ".join("%s %.3g" % kv for kv in r.items())


# ---- cn_dqn_act --------------------------------------------------------------------------------------------------------------
def _act(p, x, D, H, n):
    _abi, L = lib()
    q = torch.full((n, 3), float("nan"), device=DEV)
    act = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    tw = torch.zeros((n, 2), device=DEV)
    io = _abi.CnDqnActIO(obs=x.data_ptr(), obs_ld=x.stride(0), n=n, obs_dim=D, hidden=H, reserved=0, q=_mlp(p), epsilon=0.0,
                         epsilon_discount=0.995, epsilon_min=0.05, episodes_dev=None, seed=1, counter=0, action=act.data_ptr(),
                         twist=tw.data_ptr(), q_out=q.data_ptr())
    rc = L.cn_dqn_act(C.byref(io), 0, stream())
    torch.cuda.synchronize()
    return rc, q, act, tw


@pytest.mark.parametrize("H", Q.ACT_HIDDEN)
def test_act_q_within_the_forward_bound_and_argmax_of_its_own_q(H):
    """Every row of every (hidden, D, ld, n): q_out within the forward bound of float64, action = the lowest-index argmax of the
    device's OWN q_out, the twist of that action; NaN in the padding columns changes no bit; the argmax equals float64's on every
    row whose float64 gap exceeds twice the bound, and at most 2 % of the rows are left out of that last comparison."""
    worst, rows = 0.0, 0
    for D in Q.ACT_D:
        for n in Q.ACT_N:
            out = {}
            for ld in (D, D + 3):
                p, x = Q.act_case(H, D, ld, n, device=DEV)
                rc, q, act, tw = _act(p, x, D, H, n)
                assert rc == 0, (H, D, ld, n)
                out[ld] = (q, act, tw)
            q, act, tw = out[D]
            assert all(torch.equal(a_, b_) for a_, b_ in zip(out[D], out[D + 3])), ("padding columns were read", H, D, n)
            exact, bound, _ = Q.bounded(lambda ps: Q.act_pass(ps, Q.to64(p), x[:, :D].double()))
            ratio = R.worst_ratio(q, exact["q"], bound["q"])
            assert ratio <= 1.0, (H, D, n, ratio)
            q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
            own = torch.where(q1 > q0, 1, 0)
            own = torch.where(q2 > torch.maximum(q0, q1), 2, own)
            assert torch.equal(act.long(), own), (H, D, n)
            assert torch.equal(tw, torch.tensor(Q.TWISTS, dtype=torch.float32, device=DEV)[act.long()])
            clear = ~Q.unclear_rows(exact["q"], bound["q"])
            assert float(clear.double().mean()) >= 0.98, (H, D, n, float(clear.double().mean()))
            assert torch.equal(act.long()[clear], exact["q"].argmax(1)[clear]), (H, D, n)
            worst, rows = max(worst, ratio), rows + n
    print("act hidden %d: worst |q - float64| / bound %.3g over %d rows x 2 strides" % (H, worst, rows))


def test_act_refuses_hidden_481():
    p, x = Q.act_case(481, 16, 16, 4, device=DEV)
    rc, q, act, _ = _act(p, x, 16, 481, 4)
    _, L = lib()
    assert rc == CN_ERR_CONFIG and b"hidden" in L.cn_td3_last_error()
    assert bool(torch.isnan(q).all()) and bool((act == -1).all())          # nothing was enqueued


# ---- cn_dqn_update: gradients through rho = 0 -----------------------------------------------------------------------------------
def _recovered(p0, p1, lr, eps):
    g = {k: R.invert_step(p0[k], p1[k], lr, eps) for k in R.NAMES}
    return g, {k: R.inversion_bound(g[k], p0[k], p1[k], lr, eps) for k in R.NAMES}


def _check_chunk(tag, g, extra, exact, bound, grp, report):
    """The six recovered gradients within their bounds; a zero, a doubled and a tile-zeroed reference are rejected."""
    want, bnd = Q.part(exact, grp), Q.part(bound, grp)
    ratios = R.compare_grads(g, want, bnd, extra)
    report.append("%s %s worst/bound %s" % (tag, grp, _fmt(ratios)))
    assert Q.within(ratios), (tag, grp, ratios)
    assert max(R.compare_grads(g, {k: torch.zeros_like(v) for k, v in want.items()}, bnd, extra).values()) > 1.0, tag
    assert max(R.compare_grads(g, {k: 2 * v for k, v in want.items()}, bnd, extra).values()) > 1.0, tag
    tiles, skipped = 0, []
    for k in ("w1", "w2", "w3", "b3"):
        cut = R.zero_tile(want[k])
        if bool(((want[k] - cut).abs() > 2 * (bnd[k] + extra[k])).any()):       # the tile holds something the bound can see
            tiles += 1
            assert R.worst_ratio(g[k], cut, bnd[k] + extra[k]) > 1.0, (tag, grp, k, "a zeroed 16 x 16 tile was accepted")
        else:                                  # (a tile of units that are off on every row: its gradient is zero either way)
            skipped.append(k)
    report.append("%s %s zeroed tile rejected in %d of 4 tensors%s" % (tag, grp, tiles, ", nothing to see in " + " ".join(skipped) if skipped else ""))
    assert tiles >= 1 and "b3" not in skipped, (tag, grp, skipped)
    return max(ratios.values())


def _dead_unchanged(p0, p1, dead, tag):
    for a_, b_ in zip(Q.dead_slices(p0, dead), Q.dead_slices(p1, dead)):
        assert torch.equal(a_, b_), (tag, "a dead unit moved")


@pytest.mark.parametrize("shape", Q.UPDATE_SHAPES, ids=SHAPE_IDS)
def test_update_gradients_of_both_chunks_match_float64(shape):
    """F = 0: one step; all six gradients of chunk 1, loss[0], loss[1] == 0, the target net and the dead units untouched.
    F = B: every sample final, r[m] := the device's own pre-step q[m][a_m] (read from the first handle, what = 7: the same weights,
    the same rows and a deterministic kernel give the second handle the same bits), the shuffle puts the B s rows in chunk 1 and the
    B extra rows in chunk 2.  Chunk 1's targets then equal its outputs bit for bit (the unchosen columns of Y are q itself, the
    chosen one is r = q), so its error, its loss, every dq, every gradient sum and the RMSprop step (lr 0 / (0 + eps)) are exactly
    zero: step 1 leaves all six tensors bit-identical -- observed as loss[0] == 0 exactly, and through chunk 2, whose gradients are
    therefore taken at the ORIGINAL weights and are recovered and bounded exactly as chunk 1's are (a step of lr = 1024 on any
    nonzero gradient would throw them far outside).  This is the only construction that sees chunk 2's gradients themselves."""
    report = []
    try:
        _gradients(shape, report)
    finally:
        print("\n".join(report))


def _gradients(shape, report):
    D, ld, H, B = shape
    tag = "%d|%dx%dx%d" % shape
    p0, pt0, batch, dead, N = Q.make_case(shape, device=DEV)
    assert ld == D or bool(torch.isnan(batch[0][:, D:]).all() and torch.isnan(batch[3][:, D:]).all())
    assert Q.margin_ratio(p0, Q.stacked(batch, D), N) >= 1.0
    p64, pt64, b64 = Q.to64(p0), Q.to64(pt0), Q.batch64(batch, D)
    lr = Q.LR_RECOVER
    # F = 0
    pl = Q.plan(np.zeros(B), 0, 1 << 30, perm=np.random.default_rng(B).permutation(B))
    mark = torch.from_numpy(pl["chunk"]).to(DEV)
    run = lambda ps, hp: Q.update_pass(ps, p64, pt64, Q.acc0(p0), b64, mark, hp, False)
    g_ = Q.part(run(R._Pass(), Q.hyper(GAMMA, 1, 0, 1)), "g1")
    eps = Q.pow2_at_least(max(float(v.abs().max()) for v in g_.values()))
    hp = Q.hyper(GAMMA, lr, 0.0, eps)
    exact, bound, _ = Q.bounded(lambda ps: run(ps, hp))
    h = Fused(p0, pt0, shape, lr, 0.0, eps)
    try:
        h.update(batch, pl["perm"])
        q_dev, loss, fl = h.view(7, (2 * B, 3)), h.loss(), h.flags()
        assert h.view(4, (2 * B,), torch.int32).cpu().numpy().tolist() == pl["chunk"].tolist() and fl.tolist() == pl["flags"].tolist()
        assert h.counter() == 1
    finally:
        h.close()
    g, extra = _recovered(p0, h.p, lr, eps)
    _check_chunk(tag, g, extra, exact, bound, "g1", report)
    rl = abs(loss[0] - float(exact["loss1"])) / float(bound["loss1"])
    report.append("%s F=0 loss %.9g float64 %.9g error/bound %.3g; q error/bound %.3g" % (
        tag, loss[0], float(exact["loss1"]), rl, R.worst_ratio(q_dev, exact["q"], bound["q"])))
    assert rl <= 1.0 and loss[1] == 0.0
    assert R.worst_ratio(q_dev, exact["q"], bound["q"]) <= 1.0
    assert _same(pt0, h.pt)
    _dead_unchanged(p0, h.p, dead, tag)
    # F = B
    s, a, r, s2, d = batch
    r2 = q_dev[:B].gather(1, a.long()[:, None])[:, 0].contiguous()
    batch2 = (s, a, r2, s2, torch.ones_like(d))
    pl2 = Q.plan(np.ones(B), 0, 1 << 30, perm=Q.final_perm(B, np.random.default_rng(B + 1)))
    assert (pl2["chunk"][:B] == 1).all() and (pl2["chunk"][B:] == 2).all()
    mark2 = torch.from_numpy(pl2["chunk"]).to(DEV)
    b64_2 = Q.batch64(batch2, D)
    run2 = lambda ps, hp: Q.update_pass(ps, p64, pt64, Q.acc0(p0), b64_2, mark2, hp, False, only=2)
    g_ = Q.part(run2(R._Pass(), Q.hyper(GAMMA, 1, 0, 1)), "g2")
    eps2 = Q.pow2_at_least(max(float(v.abs().max()) for v in g_.values()))
    hp2 = Q.hyper(GAMMA, lr, 0.0, eps2)
    exact2, bound2, _ = Q.bounded(lambda ps: run2(ps, hp2))
    h2 = Fused(p0, pt0, shape, lr, 0.0, eps2)
    try:
        h2.update(batch2, pl2["perm"])
        loss2, fl2, Y = h2.loss(), h2.flags(), h2.view(6, (2 * B, 3))
        assert torch.equal(h2.view(7, (2 * B, 3)), q_dev)
        assert h2.view(4, (2 * B,), torch.int32).cpu().numpy().tolist() == pl2["chunk"].tolist() and fl2.tolist() == pl2["flags"].tolist()
    finally:
        h2.close()
    assert torch.equal(Y[:B], q_dev[:B]) and torch.equal(Y[B:], r2[:, None].expand(B, 3))
    assert loss2[0] == 0.0, (tag, "chunk 1's error is not exactly zero", loss2)
    g2, extra2 = _recovered(p0, h2.p, lr, eps2)
    _check_chunk(tag, g2, extra2, exact2, bound2, "g2", report)
    rl2 = abs(loss2[1] - float(exact2["loss2"])) / float(bound2["loss2"])
    report.append("%s F=B loss2 %.9g float64 %.9g error/bound %.3g" % (tag, loss2[1], float(exact2["loss2"]), rl2))
    assert rl2 <= 1.0
    assert _same(pt0, h2.pt)
    _dead_unchanged(p0, h2.p, dead, tag)


# ---- two chunks, wrong variants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", Q.DISCRIMINATE, ids=["product", "ragged"])
@pytest.mark.parametrize("nf", [1, -1], ids=["F=1", "F=B-1"])
def test_two_step_update_matches_float64_and_rejects_every_wrong_variant(shape, nf):
    """rho = 0, lr = 2^-5, eps = the power of two above the largest gradient: Y, the chunk marks, both losses and the final weights
    against the float64 two-step update.  The allowance of the final weights is the chunk gradients' rounding carried through both
    steps by the same propagation (the pass runs step 1, the forward on the stepped weights, step 2); where a pre-activation of
    that second forward lies within its own bound of zero, the effect of the other mask is added (dqn_f64.bounded).  No second,
    measured allowance is used."""
    D, ld, H, B = shape
    nf = nf if nf > 0 else B - 1
    p0, pt0, batch, dead, N = Q.make_case(shape, n_final=nf, device=DEV)
    p64, pt64, b64 = Q.to64(p0), Q.to64(pt0), Q.batch64(batch, D)
    pl = Q.plan(batch[4].cpu().numpy(), 0, 1 << 30, perm=np.random.default_rng(1).permutation(B + nf))
    mark = torch.from_numpy(pl["chunk"]).to(DEV)
    run = lambda ps, hp, v=None: Q.update_pass(ps, p64, pt64, Q.acc0(p0), b64, mark, hp, False, v)
    g_ = Q.part(run(R._Pass(), Q.hyper(GAMMA, 1, 0, 1)), "g1")
    lr, eps = 2.0 ** -5, Q.pow2_at_least(max(float(v.abs().max()) for v in g_.values()))
    hp = Q.hyper(GAMMA, lr, 0.0, eps)
    exact, bound, flips = Q.bounded(lambda ps: run(ps, hp))
    h = Fused(p0, pt0, shape, lr, 0.0, eps)
    try:
        h.update(batch, pl["perm"])
        Y, loss = h.view(6, (2 * B, 3)), h.loss()
        assert h.view(4, (2 * B,), torch.int32).cpu().numpy().tolist() == pl["chunk"].tolist()
        assert h.flags().tolist() == pl["flags"].tolist()
    finally:
        h.close()
    rows = torch.from_numpy(pl["chunk"] > 0).to(DEV)
    ratios = R.compare_grads(h.p, Q.part(exact, "p2"), Q.part(bound, "p2"))
    ry = R.worst_ratio(Y[rows], exact["Y"][rows], bound["Y"][rows])
    rl = [abs(loss[i] - float(exact["loss%d" % (i + 1)])) / float(bound["loss%d" % (i + 1)]) for i in (0, 1)]
    print("%s F=%d final weights worst/bound %s; Y %.3g; losses %.3g %.3g; %d ambiguous masks" % (shape, nf, _fmt(ratios), ry, rl[0], rl[1], flips))
    assert Q.within(ratios) and ry <= 1.0 and all(x <= 1.0 for x in rl)
    assert _same(pt0, h.pt)
    _dead_unchanged(p0, h.p, dead, shape)
    least = float("inf")
    for v in Q.VARIANTS:
        if v == "max_online":                          # the first update reads the online net anyway: the series test has it
            continue
        wrong = run(R._Pass(), hp, v)
        assert all(bool(torch.isfinite(t).all()) for t in h.p.values())
        f = max(R.compare_grads(h.p, Q.part(wrong, "p2"), Q.part(bound, "p2")).values())
        least = min(least, f)
        assert f > 1.0, (v, "accepted")
    print("%s F=%d smallest factor by which a wrong variant exceeded its bound: %.3g" % (shape, nf, least))


# ---- a series with the product's optimiser, eager and as a hipGraph ---------------------------------------------------------------
def test_series_with_the_products_optimiser_eager_and_graph():
    """Eight updates on one handle, F = 3, 0, 0, B, 0, 1, 0, 0, target_every = 3, crowdnav.dqn.Agent's lr / rho / eps: after every
    update the weights, both losses, flags 0-4, the counter and the target net against the float64 series (its bounds carry every
    earlier update's error forward).  Then the same series with the update captured ONCE into a hipGraph (every update enqueues the
    same sixteen launches on one stream; the batch lives in fixed buffers that are refilled between replays) and replayed: bit for
    bit the eager series.  The default queue count, no parallel branches."""
    import inspect
    from crowdnav.dqn import Agent
    dflt = {k: v.default for k, v in inspect.signature(Agent.__init__).parameters.items()}
    shape, te = Q.PRODUCT, 3
    D, ld, H, B = shape
    hp = Q.hyper(GAMMA, dflt["lr"], dflt["rho"], dflt["eps"])
    p0, pt0, _, dead, N = Q.make_case(shape, seed=0, device=DEV)
    batches, plans = [], []
    for u, F in enumerate(Q.SERIES_F):
        batch = Q.make_case(shape, n_final=B if F is None else F, seed=u, device=DEV, margins=False)[2]
        batches.append(batch)
        plans.append(Q.plan(batch[4].cpu().numpy(), u, te, seed=5))
    b64 = [Q.batch64(b, D) for b in batches]
    marks = [torch.from_numpy(pl["chunk"]).to(DEV) for pl in plans]
    run = lambda ps, v=None: Q.series_pass(ps, Q.to64(p0), Q.to64(pt0), hp, te, b64, marks, v)
    exact, bound, flips = Q.bounded(run)
    eager = Fused(p0, pt0, shape, dflt["lr"], dflt["rho"], dflt["eps"], target_every=te, seed=5)
    seen, worst, worst_l = [], 0.0, 0.0
    try:
        for u, batch in enumerate(batches):
            eager.update(batch, None)                                # the shuffle is drawn on the device (seed 5, counter u)
            pre = "u%d." % u
            ratios = R.compare_grads(eager.p, Q.part(exact, pre + "p2"), Q.part(bound, pre + "p2"))
            loss = eager.loss()
            rl = [abs(loss[i] - float(exact[pre + "loss%d" % (i + 1)])) / max(float(bound[pre + "loss%d" % (i + 1)]), 1e-300)
                  if (loss[i] != 0 or float(exact[pre + "loss%d" % (i + 1)]) != 0) else 0.0 for i in (0, 1)]
            print("series update %d: weights worst/bound %s; losses %.3g %.3g" % (u, _fmt(ratios), rl[0], rl[1]))
            assert Q.within(ratios) and all(x <= 1.0 for x in rl), u
            assert eager.flags().tolist() == plans[u]["flags"].tolist() and eager.counter() == u + 1
            assert eager.view(4, (2 * B,), torch.int32).cpu().numpy().tolist() == plans[u]["chunk"].tolist()
            if (u + 1) % te == 0:
                assert _same(eager.p, eager.pt), u
            tr = R.compare_grads(eager.pt, Q.part(exact, pre + "t"), Q.part(bound, pre + "t"))
            assert Q.within(tr), u
            if u + 1 < te:
                assert _same(eager.pt, pt0)
            worst, worst_l = max(worst, max(ratios.values())), max(worst_l, max(rl))
            seen.append(({k: v.clone() for k, v in eager.p.items()}, {k: v.clone() for k, v in eager.pt.items()}, loss))
        _dead_unchanged(p0, eager.p, dead, "series")
        last = "u%d.p2" % (len(batches) - 1)
        least = float("inf")
        for v in ("max_online", "phantom", "eps_in_sqrt"):
            wrong = run(R._Pass(), v)
            f = max(R.compare_grads(eager.p, Q.part(wrong, last), Q.part(bound, last)).values())
            least = min(least, f)
            assert f > 1.0, (v, "accepted")
        print("series: worst weights %.3g, worst loss %.3g, %d ambiguous masks, smallest wrong-variant factor %.3g" % (worst, worst_l, flips, least))
    finally:
        eager.close()
    graphed = Fused(p0, pt0, shape, dflt["lr"], dflt["rho"], dflt["eps"], target_every=te, seed=5)
    try:
        static = tuple(t.clone() for t in batches[0])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed.update(static, None, sync=False)
        torch.cuda.synchronize()
        assert _same(graphed.p, p0) and graphed.counter() == 0          # capturing ran nothing
        for u, batch in enumerate(batches):
            for dst, src in zip(static, batch):
                dst.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            assert _same(graphed.p, seen[u][0]) and _same(graphed.pt, seen[u][1]), u
            assert np.array_equal(graphed.loss(), seen[u][2]) and graphed.counter() == u + 1, u
    finally:
        graphed.close()


# ---- the drawn shuffle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 17, 64, 4096])
def test_drawn_shuffle_marks_and_flags_equal_the_cpu_statement(B):
    """Explicit batches, perm = NULL: the chunk array and flags of updates 0-5 of one handle, three seeds, F in {0, 1, B}, equal
    dqn_f64.plan exactly (lr = 0: the weights stay).  The marks of the two wrong shuffles (ascending swaps, counter + 1) differ."""
    shape, te = (4, 4, 8, B), 4
    compared, told = 0, {v: False for v in Q.SHUFFLE_VARIANTS}
    for seed in (0, (1 << 64) - 1, 0x6A09E667F3BCC908):
        for F in sorted({0, 1, B}):
            p0, pt0, batch, _, _ = Q.make_case(shape, n_final=F, seed=F, device=DEV, margins=False)
            d = batch[4].cpu().numpy()
            h = Fused(p0, pt0, shape, 0.0, 0.9, 1e-6, target_every=te, seed=seed)
            try:
                for c in range(6):
                    h.update(batch, None)
                    pl = Q.plan(d, c, te, seed=seed)
                    chunk = h.view(4, (2 * B,), torch.int32).cpu().numpy()
                    assert np.array_equal(chunk, pl["chunk"]), (seed, F, c)
                    assert h.flags().tolist() == pl["flags"].tolist() and h.counter() == c + 1, (seed, F, c)
                    compared += 2 * B
                    for v in Q.SHUFFLE_VARIANTS:
                        told[v] |= not np.array_equal(chunk, Q.plan(d, c, te, seed=seed, variant=v)["chunk"])
            finally:
                h.close()
    assert B < 17 or all(told.values()), told
    print("shuffle B %d: %d chunk marks compared exactly" % (B, compared))


# ---- replay rows -----------------------------------------------------------------------------------------------------------------
RING_CAP = (1 << 24) + 1
LIVE = (1, 2, 3, 255, 256, 257, 10 ** 6, (1 << 24) + 1)


@pytest.fixture(scope="module")
def ring():
    row = torch.arange(RING_CAP, device=DEV)
    rg = dict(s=row.float().contiguous(), s2=(-row).float().contiguous(), r=row.float().contiguous(), d=torch.zeros(RING_CAP, device=DEV),
              size=torch.zeros(1, dtype=torch.int64, device=DEV))
    rg["a"] = torch.stack([(row % 3).float(), torch.zeros(RING_CAP, device=DEV)], 1).contiguous()
    return rg


@pytest.mark.parametrize("B", [1, 64, 4096])
def test_replay_rows_equal_the_cpu_statement(ring, B):
    """A ring with r[row] = s[row] = row, s2[row] = -row, a[row] = row mod 3 (D = ld = 1; rows up to 2^24 are exact in float32):
    the gathered r, a and both halves of x equal dqn_f64.replay_row at every live size, update after update (lr = 0)."""
    shape, seed = (1, 1, 4, B), 0xBB67AE8584CAA73B
    p0, pt0, _, _, _ = Q.make_case(shape, device=DEV, margins=False)
    h = Fused(p0, pt0, shape, 0.0, 0.9, 1e-6, seed=seed, replay=ring)
    compared = 0
    try:
        for c, size in enumerate(LIVE):
            ring["size"].fill_(size)
            h.update(None)
            want = Q.replay_row(seed, c, np.arange(B), size)
            assert want.max() < size
            assert np.array_equal(h.view(1, (B,)).double().cpu().numpy(), want.astype(np.float64)), (B, size)
            assert np.array_equal(h.view(3, (B,), torch.int32).cpu().numpy(), want % 3), (B, size)
            x = h.view(0, (2 * B, 1)).double().cpu().numpy()[:, 0]
            assert np.array_equal(x[:B], want.astype(np.float64)) and np.array_equal(x[B:], -want.astype(np.float64)), (B, size)
            assert h.counter() == c + 1 and h.flags()[0] == 1
            compared += 4 * B
    finally:
        h.close()
    print("replay B %d: %d indices compared exactly" % (B, compared))


def test_replay_waits_for_learn_start(ring):
    """While size <= learn_start nothing moves and the counter stays; the first larger size steps."""
    shape = (1, 1, 4, 8)
    p0, pt0, _, _, _ = Q.make_case(shape, device=DEV, margins=False)
    h = Fused(p0, pt0, shape, 1e-2, 0.9, 1e-6, learn_start=256, target_every=1, seed=3, replay=ring)
    try:
        for size in (1, 2, 3, 255, 256):
            ring["size"].fill_(size)
            h.update(None)
            assert _same(h.p, p0) and _same(h.pt, pt0) and h.counter() == 0, size
            assert h.flags()[[0, 1, 4]].tolist() == [0, 0, 0] and not h.view(4, (16,), torch.int32).any()
        ring["size"].fill_(257)
        h.update(None)
        assert not _same(h.p, p0) and h.counter() == 1 and h.flags()[0] == 1 and _same(h.p, h.pt)
    finally:
        h.close()
