"""A population's shared replay source (include/crowdnav.h: cn_td3_pop_set_replay_source, CN_REPLAY_SHARED) against its statement, bit
for bit -- no tolerance anywhere in this file.
Sampling: cn_replay_sample_shared against the restatement (tests/replay_shared_ref.py) on that file's plan, which reaches both sides
of every seam between two rings.
The update: after every one of four updates (do_actor 0, 1, 0, 1) member p's {ring, row} pairs equal the restatement, its gathered
batch equals the rows indexed from the members' rings on the host, and its networks, loss, batch and noise equal a solo cn_td3_update
handle made from cfgs[p] and fed those rows as an explicit batch.  Then P = 1, the switch back, capture, twins, cn_td3_pop_exploit,
the state round trip, the refusals, and the Python classes.
Shapes (obs_dim, hidden, batch, P): two small ones off every tile of the GEMM launches and the product shape at P = 2; live sizes
with an empty ring and a ring smaller than the batch, and equal ones (64 rows each: at (398, 256, 128, 2) the batch is the whole
union, a permutation of it in CN_SAMPLE_DISTINCT)."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_shared_ref as S
from learner_handle import LearnerHandle, alias, batch_struct, err, lib, stream
from test_gpu_td3_population import DO_ACTOR, Member, Pop, _same, _snapshot, run_pop

pytestmark = pytest.mark.gpu

CN_ERR_ARG = -1
OWN, SHARED = 0, 1
SHAPES = [(45, 33, 40, 3), (1, 17, 33, 2), (398, 256, 128, 2)]
RING = ("s", "a", "r", "s2", "d")


# ---- sampling ---------------------------------------------------------------------------------------------------------------------
def _size_table(sizes):
    """(the sizes on the device, the device table of P pointers to them)"""
    t = torch.tensor([int(s) for s in sizes], dtype=torch.int64, device="cuda")
    return t, torch.tensor([t.data_ptr() + 8 * q for q in range(len(sizes))], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("which", range(len(S.SIZE_TUPLES)))
def test_sample_shared_equals_the_restatement(which):
    _, L = lib()
    sizes = S.SIZE_TUPLES[which]
    cases = [c for c in S.sample_plan() if c[0] == sizes]
    assert cases
    sizes_dev, table = _size_table(sizes)
    out = torch.full((sum(c[1] for c in cases), 2), -7, dtype=torch.int64, device="cuda")
    at = 0
    for _, B, member, seed, counter, mode in cases:                   # every launch enqueued, one synchronisation
        rc = L.cn_replay_sample_shared(seed, counter, B, C.c_void_p(table.data_ptr()), len(sizes), member, mode, C.c_void_p(out[at:].data_ptr()), 0, stream())
        assert rc == 0, err()
        at += B
    got = out.cpu().numpy()
    at = 0
    for _, B, member, seed, counter, mode in cases:
        want = S.pairs(seed, counter, B, sizes, member, mode)
        assert np.array_equal(got[at:at + B], want), (sizes[:8], B, member, seed, counter, mode)
        at += B
    del sizes_dev


# ---- the update -------------------------------------------------------------------------------------------------------------------
def _members(D, H, B, sizes, seeds=None):
    """Members that differ in everything a member may differ in; rings a little larger than what they hold."""
    return [Member(D, H, B, key=p, lr_actor=3e-4 * (1 + p), lr_critic=1e-3 / (1 + p), gamma=0.99 - 0.02 * p, noise_std=0.2 + 0.05 * p,
                   noise_clip=0.5 - 0.05 * p, live=live, cap=live + 3, **({} if seeds is None else dict(seed=seeds[p])))
            for p, live in enumerate(sizes)]


class SharedPop(Pop):
    def __init__(self, members, mode=0, source=SHARED):
        super().__init__(members, mode)
        self.members, self.mode = members, mode
        self.set_source(source)

    def set_source(self, source):
        assert self.L.cn_td3_pop_set_replay_source(self.h, source) == 0, err()

    def src(self, p):
        ptr = self.L.cn_td3_pop_batch_src_dev(self.h, p)
        assert ptr, p
        torch.cuda.synchronize()
        return alias(ptr, (self.members[0].B, 2), "<i8").cpu().numpy().copy()


def _explicit_batch(members, pr):
    """The rows `pr` [B, 2] = {ring, row} indexed from the members' rings on the host -> five device tensors."""
    q, row = torch.from_numpy(pr[:, 0]), torch.from_numpy(pr[:, 1])
    out = []
    for k in RING:
        stack = [m.ring[k] for m in members]
        out.append(torch.stack([stack[int(a)][int(b)] for a, b in zip(q, row)]).cuda().contiguous())
    return tuple(out)


class Solos:
    """One solo cn_td3 handle per member, on fresh instances, driven beside a population."""

    def __init__(self, members, mode):
        self.members, self.mode = members, mode
        self.insts = [m.instance() for m in members]
        self.hs = [LearnerHandle("td3", i.cfg, i) for i in self.insts]
        for h in self.hs:
            assert h.set_replay_sample(mode) == 0, err()
        self.c = 0

    def update(self, do_actor, source):
        """-> (the restatement's pairs per member or None, the members' snapshots)"""
        sizes = [m.live for m in self.members]
        pairs, snaps = [], []
        for p, (h, inst) in enumerate(zip(self.hs, self.insts)):
            if source == SHARED:
                pr = S.pairs([m.seed for m in self.members], self.c, inst.m.B, sizes, p, self.mode)
                h.update(do_actor, batch=batch_struct(_explicit_batch(self.members, pr) + (None,)))
            else:
                pr = None
                h.update(do_actor)
            pairs.append(pr)
            snaps.append(_snapshot(inst, alias(h.L.cn_td3_loss_dev(h.h), ()), lambda what, h=h: h.L.cn_td3_batch_dev(h.h, what)))
        self.c += 1
        return pairs, snaps

    def close(self):
        for h in self.hs:
            h.close()


def _hold(pop, solos, do_actor, source, where):
    """One update of both; the population's members against the statement."""
    pop.update(do_actor)
    got = pop.snapshot()
    pairs, want = solos.update(do_actor, source)
    D = pop.members[0].D
    for p in range(pop.P):
        _same(got[p], want[p], where + ("member %d" % p,))
        if source == SHARED:
            assert np.array_equal(pop.src(p), pairs[p]), where + (p,)
            s, a, r, s2, d = _explicit_batch(pop.members, pairs[p])
            xs, x2 = got[p][37], got[p][38]
            assert torch.equal(xs[:, :D], s) and torch.equal(xs[:, D:], a) and torch.equal(x2[:, :D], s2), where + (p,)
            assert torch.equal(got[p][39], r) and torch.equal(got[p][40], d), where + (p,)
    return pairs


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("equal_sizes", (False, True))
@pytest.mark.parametrize("D,H,B,P", SHAPES)
def test_every_member_equals_a_solo_handle_fed_the_rows_of_the_statement(D, H, B, P, equal_sizes, mode):
    sizes = (64,) * P if equal_sizes else {3: (300, 0, 7), 2: (300, 7)}[P]
    members = _members(D, H, B, sizes)
    assert [m.seed for m in members] == list(S.UPDATE_SEEDS[:P])
    pop, solos = SharedPop(members, mode), Solos(members, mode)
    try:
        rings = set()
        for u, a in enumerate(DO_ACTOR):
            pairs = _hold(pop, solos, a, SHARED, (D, H, B, P, sizes, mode, "update %d" % u))
            rings |= {int(q) for pr in pairs for q in pr[:, 0]}
            if mode == S.DISTINCT and B <= sum(sizes):
                for pr in pairs:
                    assert len({tuple(x) for x in pr.tolist()}) == B
        assert rings == {q for q, n in enumerate(sizes) if n > 0}      # every member drew from every ring that holds rows
    finally:
        pop.close()
        solos.close()


@pytest.mark.parametrize("mode", S.MODES)
def test_one_member_shared_is_own(mode):
    m = Member(45, 33, 40, key=7, live=77, cap=80)
    pop = SharedPop([m], mode)
    try:
        want = run_pop([m], mode)
        for u, a in enumerate(DO_ACTOR):
            pop.update(a)
            _same(pop.snapshot()[0], want[u][0], (mode, u))
            pr = pop.src(0)
            assert not pr[:, 0].any() and np.array_equal(pr, S.pairs(m.seed, u, 40, (77,), 0, mode))
    finally:
        pop.close()


def test_switching_back_to_own_gives_the_own_source_from_that_update_on():
    D, H, B = 45, 33, 40
    members = _members(D, H, B, (300, 50, 7))
    pop, solos = SharedPop(members, 1), Solos(members, 1)
    try:
        for u, (a, source) in enumerate(zip(DO_ACTOR + DO_ACTOR, (SHARED, SHARED, OWN, OWN, SHARED, OWN, SHARED, SHARED))):
            pop.set_source(source)
            _hold(pop, solos, a, source, ("switch", u))
    finally:
        pop.close()
        solos.close()


def test_captured_pair_replayed_twice_equals_four_eager_updates():
    D, H, B = 45, 33, 40
    members = _members(D, H, B, (300, 0, 7))
    eager = SharedPop(members)
    pop = SharedPop(members)
    try:
        for a in DO_ACTOR:                                            # (also loads the kernels before anything is captured)
            eager.update(a)
        want, want_src = eager.snapshot(), [eager.src(p) for p in range(3)]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pop.update(0)
            pop.update(1)
        pop.set_source(OWN)                                           # a captured update keeps the source it was captured with
        for _ in range(2):
            g.replay()
        got = pop.snapshot()
        for p in range(3):
            _same(got[p], want[p], "graph, member %d" % p)
            assert np.array_equal(pop.src(p), want_src[p]) and np.array_equal(want_src[p], S.pairs([m.seed for m in members], 3, B, (300, 0, 7), p, 0))
        del g
    finally:
        pop.close()
        eager.close()


def test_twins_stay_twins():
    D, H, B = 30, 16, 17
    a, b = Member(D, H, B, key=1, live=50, cap=53), Member(D, H, B, key=2, live=9, cap=12)
    twin = Member(D, H, B, key=1, live=50, cap=53)
    pop = SharedPop([a, b, twin])
    try:
        for x in DO_ACTOR:
            pop.update(x)
        last = pop.snapshot()
        _same(last[2], last[0], "twins")
        assert np.array_equal(pop.src(0), pop.src(2)) and not np.array_equal(pop.src(0), pop.src(1))
        for j in range(36):
            assert not torch.equal(last[0][j], last[1][j]), j
    finally:
        pop.close()


def _pbt_bind(pop, n_replace, seed):
    import pbt_ref as R
    from test_gpu_td3_pbt import c_config
    cfg = R.make_config(n_replace, explore=("lr_actor", "lr_critic", "noise_std"), factor=(0.8, 1.2), lo=[1e-5, 1e-5, 0.8, 0.05, 0.1],
                        hi=[1e-2, 1e-2, 0.999, 1.0, 1.0], seed=seed)
    pop.pbt_cfg = c_config(cfg)
    assert pop.L.cn_td3_pop_pbt_bind(pop.h, C.byref(pop.pbt_cfg), None) == 0, err()


def test_after_an_exploit_the_shared_update_still_follows_the_statement():
    """cn_td3_pop_exploit rewrites noise_std in the prep tables in place, and the shared launch reads those tables: after it the pairs
    and the gathered rows are the statement's (the counters are never copied), and the noise is what an own-source population that
    went through the same exploit draws -- the noise depends on (seed, counter, row, noise_std, noise_clip) alone."""
    D, H, B, sizes = 5, 17, 8, (40, 0, 21, 64)
    members = _members(D, H, B, sizes)
    pops = [SharedPop(members, 1, SHARED), SharedPop(members, 1, OWN), SharedPop(members, 1, SHARED)]
    try:
        for pop in pops:
            _pbt_bind(pop, 2, 0xC0FFEE)
            pop.update(0)
            pop.update(1)
            if pop is not pops[2]:                                    # (the third never exploits: what the noise would have been)
                fit = torch.tensor([3.0, 0.0, 1.0, 2.0], device="cuda")
                assert pop.L.cn_td3_pop_exploit(pop.h, C.c_void_p(fit.data_ptr()), stream()) == 0, err()
            pop.update(0)
        shared, own, never = pops[0].snapshot(), pops[1].snapshot(), pops[2].snapshot()
        moved = 0
        for p in range(4):
            pr = S.pairs([m.seed for m in members], 2, B, sizes, p, 1)
            assert np.array_equal(pops[0].src(p), pr), p
            s, a, r, s2, d = _explicit_batch(members, pr)
            assert torch.equal(shared[p][37][:, :D], s) and torch.equal(shared[p][37][:, D:], a) and torch.equal(shared[p][38][:, :D], s2)
            assert torch.equal(shared[p][39], r) and torch.equal(shared[p][40], d)
            assert torch.equal(shared[p][41], own[p][41]), p          # the noise, with the rewritten noise_std
            moved += not torch.equal(shared[p][41], never[p][41])
            assert all(torch.isfinite(t).all() for t in shared[p])
        assert moved == 2                                             # the two replaced members' noise_std was perturbed
    finally:
        for pop in pops:
            pop.close()


def test_after_a_state_round_trip_the_shared_update_still_follows_the_statement():
    """Two shared updates, save; two more.  A fresh population of the same members that loads the blob and runs those two equals it:
    networks, loss, batch, pairs.  (The first population is held to the statement by the test above all others.)"""
    D, H, B, sizes = 45, 33, 40, (300, 0, 7)
    members = _members(D, H, B, sizes)
    first, second = SharedPop(members, 1), SharedPop(members, 1)
    try:
        L = first.L
        for a in (0, 1):
            first.update(a)
        n = L.cn_td3_pop_state_size(first.h)
        assert n and n == L.cn_td3_pop_state_size(second.h), err()
        blob = torch.zeros(n, dtype=torch.uint8, device="cuda")
        assert L.cn_td3_pop_state_save(first.h, C.c_void_p(blob.data_ptr()), n, stream()) == 0, err()
        for a in (0, 1):
            first.update(a)
        want, want_src = first.snapshot(), [first.src(p) for p in range(3)]
        assert L.cn_td3_pop_state_load(second.h, C.c_void_p(blob.data_ptr()), n, stream()) == 0, err()
        for inst, src in zip(second.insts, first.insts):              # (the rings are the caller's: these two hold the same rows)
            assert all(torch.equal(inst.ring[k], src.ring[k]) for k in RING)
        for a in (0, 1):
            second.update(a)
        got = second.snapshot()
        for p in range(3):
            _same(got[p], want[p], "state, member %d" % p)
            assert np.array_equal(second.src(p), want_src[p])
            assert np.array_equal(want_src[p], S.pairs([m.seed for m in members], 3, B, sizes, p, 1))
    finally:
        first.close()
        second.close()


def test_refusals():
    _, L = lib()
    assert L.cn_td3_pop_set_replay_source(None, SHARED) == CN_ERR_ARG and "null handle" in err()
    assert not L.cn_td3_pop_batch_src_dev(None, 0)
    members = _members(20, 16, 8, (30, 5))
    pop = Pop(members)
    try:
        assert not L.cn_td3_pop_batch_src_dev(pop.h, 0)               # a fresh handle: the own source, no shared update yet
        pop.update(0)
        assert not L.cn_td3_pop_batch_src_dev(pop.h, 0)
        assert L.cn_td3_pop_set_replay_source(pop.h, SHARED) == 0, err()
        for bad in (2, -1):
            assert L.cn_td3_pop_set_replay_source(pop.h, bad) == CN_ERR_ARG and "cn_td3_pop_set_replay_source" in err() and "source" in err()
        pop.update(0)                                                 # still shared: the handle kept its source
        torch.cuda.synchronize()
        for member in (-1, 2):
            assert not L.cn_td3_pop_batch_src_dev(pop.h, member), member
        for p in range(2):
            got = alias(L.cn_td3_pop_batch_src_dev(pop.h, p), (8, 2), "<i8").cpu().numpy()
            assert np.array_equal(got, S.pairs([m.seed for m in members], 1, 8, (30, 5), p, 0)), p
    finally:
        pop.close()
    sizes_dev, table = _size_table((3, 4))
    rows = torch.zeros((4, 2), dtype=torch.int64, device="cuda")
    t, r = C.c_void_p(table.data_ptr()), C.c_void_p(rows.data_ptr())
    for args, word in (((1, 2, 0, t, 2, 0, 0, r), "B < 1"), ((1, 2, -1, t, 2, 0, 0, r), "B < 1"), ((1, 2, 4, t, 0, 0, 0, r), "P must be"),
                       ((1, 2, 4, t, 65, 0, 0, r), "P must be"), ((1, 2, 4, t, 2, -1, 0, r), "self"), ((1, 2, 4, t, 2, 2, 0, r), "self"),
                       ((1, 2, 4, t, 2, 0, 2, r), "mode"), ((1, 2, 4, t, 2, 0, -1, r), "mode"), ((1, 2, 4, None, 2, 0, 0, r), "null"),
                       ((1, 2, 4, t, 2, 0, 0, None), "null")):
        assert L.cn_replay_sample_shared(*args, 0, stream()) == CN_ERR_ARG and "cn_replay_sample_shared" in err() and word in err(), (args, err())
    torch.cuda.synchronize()
    assert not rows.any()
    del sizes_dev


def test_python_population_shares_and_starts_on_the_sum_of_the_rings():
    """crowdnav.td3.Population(replay_source="shared"): ready() is DeviceReplay.ready's inequality on the sum of the live sizes; learn
    gathers what the statement names; set_replay_source switches back."""
    from crowdnav import td3

    def agents(n):
        out = []
        for p in range(2):
            a = td3.Agent(obs_dim=20, hidden=32, batch_size=16, memory_size=64, device="cuda:0", seed=3 + p)
            g = torch.Generator().manual_seed(p)
            if n[p]:
                a.memory.add(torch.randn((n[p], 20), generator=g).cuda(), torch.rand((n[p], 2), generator=g).cuda(), torch.randn(n[p], generator=g).cuda(),
                             torch.randn((n[p], 20), generator=g).cuda(), (torch.rand(n[p], generator=g) < 0.1).cuda())
            out.append(a)
        return out
    with pytest.raises(ValueError):
        td3.Population(agents((1, 1)), replay_source="pooled")
    assert not td3.Population(agents((10, 6)), replay_source="shared").ready()      # 16 rows: not more than a batch
    assert not td3.Population(agents((17, 0))).ready()                             # own: member 1 has nothing
    ag = agents((17, 0))
    pop = td3.Population(ag, replay_source="shared")
    assert pop.replay_source == "shared" and pop.ready()
    masked = agents((10, 0))                        # bounds that straddle the inequality: one host read settles it
    masked[1].memory.add_masked(torch.randn(7, 20).cuda(), torch.rand(7, 2).cuda(), torch.randn(7).cuda(), torch.randn(7, 20).cuda(),
                                torch.zeros(7, dtype=torch.bool).cuda(), torch.ones(7, dtype=torch.bool).cuda())
    assert td3.Population(masked, replay_source="shared").ready()
    with pytest.raises(Exception):
        pop.batch_src(0)                            # no shared update yet
    loss = pop.learn(1)
    torch.cuda.synchronize()
    assert loss.shape == (2,) and torch.isfinite(loss).all()
    seeds = [int(a.fused_config().seed) for a in ag]
    for p in range(2):
        pr = pop.batch_src(p)
        assert pr.shape == (16, 2) and pr.dtype == torch.int64
        assert np.array_equal(pr.cpu().numpy(), S.pairs(seeds, 0, 16, (17, 0), p, 0))
        rows = pr[:, 1]
        assert torch.equal(pop.batch_dev(p, 0, (16, 22))[:, :20], ag[0].memory.s[rows])
    pop.set_replay_source("own")
    assert pop.replay_source == "own" and not pop.ready()
    with pytest.raises(ValueError):
        pop.set_replay_source("pooled")
