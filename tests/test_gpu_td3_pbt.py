"""cn_td3_pop_exploit (include/crowdnav.h: population-based training on a cn_td3_pop handle) against its statement, bit for bit -- no
tolerance anywhere in this file.  The plan and the state against the NumPy restatement (tests/pbt_ref.py); what the replaced members
take over by running on (a missed moment, step counter or bias-correction slot diverges at the first update: Adam's state has no
accessor, so it is held through the updates it drives); the rewritten tables against a population created with the perturbed values;
the log-fed fitness and its skip rule; the survivors against a population that never exploited; capture; the refusals.
Shapes: obs_dim 5, hidden 17, batch 8, rings of 64 rows -- odd sizes, so the copy's heads and tails and the GEMM tile edges are all
exercised (the bias tensors hold 17, 2 and 1 floats)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import pbt_ref as R
from learner_handle import alias, err, lib, stream
from test_gpu_td3_population import Member, Pop

pytestmark = pytest.mark.gpu

D, H, B, RING = 5, 17, 8, 64
CN_ERR_ARG, CN_ERR_CONFIG = -1, -2
NAN = float("nan")
LO, HI = [1e-5, 1e-5, 0.8, 0.05, 0.1], [1e-2, 1e-2, 0.999, 1.0, 1.0]
MEMBER_DTYPE = np.dtype([("src", "<i4"), ("generation", "<i4"), ("fitness", "<u4"), ("hyper", "<u4", (5,))])


def member(p, **kw):
    """Member p of a sweep: every hyper-parameter PBT knows differs between members, inside [LO, HI]."""
    f = dict(lr_actor=3e-4 * (1 + p % 4), lr_critic=1e-3 / (1 + p % 3), gamma=0.99 - 0.002 * p, noise_std=0.2 + 0.001 * p,
             noise_clip=0.5 - 0.001 * p, live=RING)
    f.update(kw)
    return Member(D, H, B, key=p, **f)


def hypers_of(m):
    return [m.hyper[k] for k in R.HYPERS]


def c_config(cfg):
    _abi, _ = lib()
    return _abi.CnTd3PbtConfig(n_replace=cfg["n_replace"], min_episodes=cfg["min_episodes"], explore_mask=cfg["explore_mask"], reserved=0,
                               factor=tuple(float(x) for x in cfg["factor"]), lo=tuple(float(x) for x in cfg["lo"]),
                               hi=tuple(float(x) for x in cfg["hi"]), seed=cfg["seed"])


class PbtPop(Pop):
    """A population with its PBT binding; tot [P][5] float64 on the device when the fitness comes from logs."""

    def bind(self, cfg, logs=False):
        _abi, L = lib()
        self.pbt_cfg, arr = c_config(cfg), None
        if logs:
            self.tot = torch.zeros((self.P, 5), dtype=torch.float64, device="cuda")
            self.rows, self.n = torch.zeros((self.P, 4, 8), device="cuda"), torch.zeros(self.P, dtype=torch.int64, device="cuda")
            arr = (_abi.CnEpisodeLog * self.P)(*[_abi.CnEpisodeLog(rows=self.rows[p].data_ptr(), max_rows=4, n_dev=self.n[p:].data_ptr(),
                                                                  tot_dev=self.tot[p].data_ptr()) for p in range(self.P)])
        assert L.cn_td3_pop_pbt_bind(self.h, C.byref(self.pbt_cfg), arr) == 0, err()
        return self

    def exploit(self, fitness=None):
        self.fit = None if fitness is None else torch.tensor(fitness, dtype=torch.float32, device="cuda")
        assert self.L.cn_td3_pop_exploit(self.h, None if self.fit is None else C.c_void_p(self.fit.data_ptr()), stream()) == 0, err()

    def state(self):
        """(calls, applied, the members as a structured array [P]) after a synchronisation."""
        _abi, L = lib()
        torch.cuda.synchronize()
        raw = alias(L.cn_td3_pop_pbt_state_dev(self.h), (C.sizeof(_abi.CnTd3PbtState),), "|u1").cpu().numpy().tobytes()
        calls, applied = np.frombuffer(raw, "<u8", 2)
        return int(calls), int(applied), np.frombuffer(raw, MEMBER_DTYPE, 64, 16)[:self.P].copy()

    def params(self):
        torch.cuda.synchronize()
        return [inst.params() for inst in self.insts]


def same_state(got, ref):
    calls, applied, mem = got
    assert (calls, applied) == (ref["calls"], ref["applied"])
    assert mem["src"].tolist() == ref["src"].tolist() and mem["generation"].tolist() == ref["generation"].tolist()
    assert mem["fitness"].tolist() == ref["fitness"].view(np.uint32).tolist()
    assert mem["hyper"].tolist() == ref["hyper"].view(np.uint32).tolist()


def same_tensors(got, want, where):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), (where, j)


def fitness_for(P, call):
    """Ties (five distinct values), a NaN, a -0.0 next to a 0.0; another arrangement in every call."""
    f = [float((7 * p + 3 * call) % 5) for p in range(P)]
    f[(1 + call) % P], f[(2 + call) % P], f[(3 + call) % P] = NAN, -0.0, 0.0
    return f


@pytest.mark.parametrize("P,n", [(5, 2), (64, 32)])
def test_plan_and_state_equal_the_restatement_over_three_calls(P, n):
    members = [member(p) for p in range(P)]
    cfg = R.make_config(n, explore=("lr_actor", "lr_critic", "noise_std"), factor=(0.8, 1.2), lo=LO, hi=HI, seed=0xC0FFEE + P)
    ref = R.make_state([hypers_of(m) for m in members])
    pop = PbtPop(members)
    try:
        pop.bind(cfg)
        same_state(pop.state(), ref)                       # what the bind leaves
        for a in (0, 1):
            pop.update(a)
        for call in range(3):
            pop.update(call % 2)                            # (members that were equal after a copy differ again: other seeds, other rings)
            before = pop.params()
            f = fitness_for(P, call)
            pop.exploit(f)
            pairs = R.exploit(ref, cfg, fitness=f)
            same_state(pop.state(), ref)
            after = pop.params()
            replaced = dict(pairs)
            assert len(replaced) == n
            for p in range(P):
                same_tensors(after[p], before[replaced.get(p, p)], (call, p))      # a survivor: untouched; a replaced member: its source's
            for dst, src in pairs:
                assert not torch.equal(before[dst][12], before[src][12]), (call, dst, src)     # (q1's w1: every update moves it)
        assert ref["generation"].max() >= 1 and (ref["hyper"] != np.asarray([hypers_of(m) for m in members], np.float32)).any()
        pop.update(0)                                       # the rewritten tables still name valid jobs
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for ps in pop.params() for t in ps)
    finally:
        pop.close()


def test_a_replaced_member_runs_on_as_its_source():
    """Members 0 and 3: one seed, byte-equal rings, other initial weights.  After 5 updates 3 copies 0 with factor (1, 1); from then on the
    two have one seed, one counter, one ring, so every update must leave them equal -- networks, loss, gathered batch -- which it does only
    if Adam's moments, both step counters, the bias corrections and the running beta products all came along."""
    S = 0x1234ABCD5678
    ms = [member(0, seed=S, lr_actor=3e-4, lr_critic=3e-4), member(1), member(2), member(3, seed=S, lr_actor=3e-4, lr_critic=3e-4)]
    ms[3].ring = {k: t.clone() for k, t in ms[0].ring.items()}
    for k in ("gamma", "noise_std", "noise_clip"):
        ms[3].hyper[k] = ms[0].hyper[k]
    cfg = R.make_config(1, explore=R.HYPERS, factor=(1.0, 1.0), lo=LO, hi=HI, seed=9)
    pop = PbtPop(ms).bind(cfg)
    try:
        for a in (0, 1, 0, 1, 0):
            pop.update(a)
        snap = pop.snapshot()
        assert not torch.equal(snap[3][0], snap[0][0])
        pop.exploit([3.0, 2.0, 1.0, 0.0])
        _, applied, mem = pop.state()
        assert applied == 1 and mem["src"].tolist() == [0, 1, 2, 0] and mem["hyper"][3].tolist() == mem["hyper"][0].tolist()
        for u, a in enumerate((1, 0, 1, 0, 1, 0)):
            pop.update(a)
            snap = pop.snapshot()
            same_tensors(snap[3], snap[0], "update %d after the exploit" % u)
            assert not torch.equal(snap[1][0], snap[0][0])
    finally:
        pop.close()


@pytest.mark.parametrize("mode", (0, 1))
def test_the_tables_were_rewritten(mode):
    """X exploits while fresh (Adam's state is zero, so weights and hyper-parameters are all a member is); Y is created with what X's
    state says member 1 now has.  Four updates later every member of X equals its twin in Y, the noise after scale and clip included."""
    ms = [member(p) for p in range(3)]
    cfg = R.make_config(1, explore=R.HYPERS, factor=(0.5, 3.0), lo=[1e-5, 1e-5, 0.8, 0.15, 0.1], hi=[1e-2, 1e-2, 0.999, 0.5, 1.0], seed=21)
    ref = R.make_state([hypers_of(m) for m in ms])
    assert R.exploit(ref, cfg, fitness=[2.0, 0.0, 1.0]) == [(1, 0)]
    h0, h1 = np.asarray(hypers_of(ms[0]), np.float32), ref["hyper"][1]
    clamped = [k for k in range(5) if h1[k] in (cfg["lo"][k], cfg["hi"][k])]
    free = [k for k in range(5) if h1[k] in (np.float32(h0[k] * np.float32(0.5)), np.float32(h0[k] * np.float32(3.0))) and k not in clamped]
    assert clamped and free and all(h1[k] != h0[k] for k in range(5)), (clamped, free, h1, h0)      # the mix the test is about
    x = PbtPop(ms, mode).bind(cfg)
    try:
        x.exploit([2.0, 0.0, 1.0])
        same_state(x.state(), ref)
        twin = copy.copy(ms[1])
        twin.nets = {k: [t.clone() for t in ts] for k, ts in ms[0].nets.items()}
        twin.hyper = dict(ms[1].hyper, **dict(zip(R.HYPERS, x.state()[2]["hyper"][1].view(np.float32).tolist())))
        y = Pop([ms[0], twin, ms[2]], mode)
        try:
            for u, a in enumerate((0, 1, 0, 1)):
                x.update(a); y.update(a)
                sx, sy = x.snapshot(), y.snapshot()
                for p in range(3):
                    same_tensors(sx[p], sy[p], (mode, "update %d" % u, "member %d" % p))
        finally:
            y.close()
    finally:
        x.close()


def test_fitness_from_the_logs_and_the_skip_rule():
    ms = [member(p) for p in range(3)]
    cfg = R.make_config(1, min_episodes=2, explore=("lr_critic",), factor=(0.8, 1.2), lo=LO, hi=HI, seed=5)
    ref = R.make_state([hypers_of(m) for m in ms])
    pop = PbtPop(ms).bind(cfg, logs=True)
    try:
        pop.update(0)
        tot = np.zeros((3, 5))
        tot[:, 0], tot[:, 2] = (2, 1, 2), (20.0, 10.0, -7.0)
        pop.tot.copy_(torch.from_numpy(tot))
        before, state0 = pop.params(), pop.state()
        pop.exploit()                                       # member 1 is one episode short
        assert R.exploit(ref, cfg, tot=tot) is None
        got = pop.state()
        same_state(got, ref)
        assert got[0] == 1 and got[1] == 0 and got[2].tobytes() == state0[2].tobytes()
        for p in range(3):
            same_tensors(pop.params()[p], before[p], "skipped, member %d" % p)
        tot[1, 0], tot[1, 2] = 3, 10.0
        pop.tot.copy_(torch.from_numpy(tot))
        pop.exploit()
        pairs = R.exploit(ref, cfg, tot=tot)
        assert pairs == [(2, 0)] and ref["fitness"].tolist() == [10.0, np.float32(10.0 / 3.0), -3.5]
        same_state(pop.state(), ref)
        same_tensors(pop.params()[2], before[0], "member 2 <- member 0")
        pop.exploit()                                       # `last` has advanced: no new episodes, skipped
        assert R.exploit(ref, cfg, tot=tot) is None
        same_state(pop.state(), ref)
        assert pop.state()[:2] == (3, 1)
        tot[:, 0] += (2, 4, 2)
        tot[:, 2] += (1.0, 8.0, 6.0)                        # the NEW episodes alone rank: 0.5, 2, 3
        pop.tot.copy_(torch.from_numpy(tot))
        pop.exploit()
        assert R.exploit(ref, cfg, tot=tot) == [(0, 2)] and ref["fitness"].tolist() == [0.5, 2.0, 3.0]
        same_state(pop.state(), ref)
        assert pop.state()[:2] == (4, 2)
    finally:
        pop.close()


def test_survivors_do_not_notice_an_exploit():
    ms = [member(p) for p in range(4)]
    cfg = R.make_config(1, explore=R.HYPERS, factor=(0.8, 1.2), lo=LO, hi=HI, seed=77)
    x, y = PbtPop(ms).bind(cfg), Pop(ms)
    try:
        for a in (0, 1, 0):
            x.update(a); y.update(a)
        x.exploit([1.0, 4.0, 3.0, 2.0])
        _, _, mem = x.state()
        assert mem["generation"].tolist() == [1, 0, 0, 0] and mem["src"][0] == 1
        for a in (1, 0, 1, 0):
            x.update(a); y.update(a)
        sx, sy = x.snapshot(), y.snapshot()
        for p in (1, 2, 3):
            same_tensors(sx[p], sy[p], "survivor %d" % p)
        assert not torch.equal(sx[0][0], sy[0][0])
    finally:
        x.close(); y.close()


def test_a_captured_exploit_and_update_equal_the_eager_ones():
    ms = [member(p) for p in range(4)]
    cfg = R.make_config(2, explore=("lr_actor", "gamma"), factor=(0.8, 1.2), lo=LO, hi=HI, seed=3)
    f = [0.5, NAN, 2.0, 1.0]
    eager = PbtPop(ms).bind(cfg)
    try:
        eager.update(0); eager.exploit(f); eager.update(1)
        want, want_state = eager.snapshot(), eager.state()
    finally:
        eager.close()
    pop = PbtPop(ms).bind(cfg)
    try:
        pop.update(0)
        fit = torch.tensor(f, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert pop.L.cn_td3_pop_exploit(pop.h, C.c_void_p(fit.data_ptr()), stream()) == 0, err()
            pop.update(1)
        assert pop.state()[0] == 0                          # capturing ran nothing
        g.replay()
        got, got_state = pop.snapshot(), pop.state()
        assert got_state[:2] == want_state[:2] == (1, 1) and got_state[2].tobytes() == want_state[2].tobytes()
        for p in range(4):
            same_tensors(got[p], want[p], "graph, member %d" % p)
        del g
    finally:
        pop.close()


def test_refusals_with_a_live_handle():
    _abi, L = lib()
    ms = [member(p) for p in range(5)]
    good = R.make_config(2, explore=R.HYPERS, lo=LO, hi=HI)
    pop = PbtPop(ms)
    one = PbtPop(ms[:1])
    try:
        def bind(h, want, *texts, logs=None, **kw):
            cfg = c_config(dict(good, **{k: v for k, v in kw.items() if k in good}))
            for k, v in kw.items():
                if k not in good:
                    setattr(cfg, k, v)
            rc = L.cn_td3_pop_pbt_bind(h, C.byref(cfg), logs)
            assert rc == want and "cn_td3_pop_pbt_bind" in err() and all(t in err() for t in texts), (kw, rc, err())
            assert not L.cn_td3_pop_pbt_state_dev(h)       # a refused bind binds nothing

        fit = torch.zeros(5, device="cuda")
        assert L.cn_td3_pop_exploit(pop.h, C.c_void_p(fit.data_ptr()), stream()) == CN_ERR_ARG and "cn_td3_pop_pbt_bind first" in err()
        assert L.cn_td3_pop_pbt_bind(pop.h, None, None) == CN_ERR_ARG and "null cfg" in err()
        for n in (0, -1, 3, 64):
            bind(pop.h, CN_ERR_ARG, "n_replace", n_replace=n)
        bind(one.h, CN_ERR_ARG, "n_replace", n_replace=1)   # a population of one has nobody to copy from
        for m in (0, -3):
            bind(pop.h, CN_ERR_ARG, "min_episodes", min_episodes=m)
        for bad in ((0.0, 1.2), (0.8, -1.0), (NAN, 1.2), (0.8, float("inf"))):
            bind(pop.h, CN_ERR_ARG, "factor", factor=bad)
        for k in range(5):
            lo, hi = list(LO), list(HI)
            lo[k], hi[k] = HI[k], LO[k]
            bind(pop.h, CN_ERR_ARG, R.HYPERS[k], "lo <= hi", lo=lo, hi=hi)
            bind(pop.h, CN_ERR_ARG, R.HYPERS[k], lo=[NAN if j == k else x for j, x in enumerate(LO)])
            bind(pop.h, CN_ERR_ARG, R.HYPERS[k], hi=[float("inf") if j == k else x for j, x in enumerate(HI)])
        for mask in (1 << 5, 0x80000000, 0x3F):
            bind(pop.h, CN_ERR_ARG, "explore_mask", explore_mask=mask)
        t = torch.zeros(64, dtype=torch.float64, device="cuda")
        full = dict(rows=t.data_ptr(), max_rows=1, n_dev=t.data_ptr(), tot_dev=t.data_ptr())
        for field, val in (("rows", None), ("n_dev", None), ("tot_dev", None), ("max_rows", -1)):
            logs = (_abi.CnEpisodeLog * 5)(*[_abi.CnEpisodeLog(**dict(full, **({field: val} if p == 3 else {}))) for p in range(5)])
            bind(pop.h, CN_ERR_ARG, "member 3", "incomplete log", logs=logs)
        # a member that starts outside the bounds: member 4's gamma is 0.982
        bind(pop.h, CN_ERR_CONFIG, "member 4", "gamma", "outside", lo=[LO[0], LO[1], 0.983, LO[3], LO[4]])
        bind(pop.h, CN_ERR_CONFIG, "member 0", "noise_std", "outside", hi=[HI[0], HI[1], HI[2], 0.19, HI[4]])
        pop.bind(good)                                      # and a good one binds: without logs a fitness is needed
        assert L.cn_td3_pop_exploit(pop.h, None, stream()) == CN_ERR_ARG and "no logs were bound" in err()
        assert pop.state()[:2] == (0, 0)
    finally:
        pop.close(); one.close()
