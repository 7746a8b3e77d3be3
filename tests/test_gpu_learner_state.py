"""cn_td3_state_* / cn_td3_pop_state_* (include/crowdnav.h: a learner's whole state as one blob, out and in by one launch each)
against their statement -- bytes only, no tolerance anywhere in this file.  The raw handles of tests/learner_handle.py; the blob
against the NumPy restatement (tests/state_ref.py) packed from direct reads of the live tensors; a load against running on.
A solo handle's parameter tensors are carved from one buffer at word offsets 0, 1, 2, 3 past a 16-byte boundary, so the copy's
16-byte path, its heads and tails and its word-by-word path all run; the shapes give segments of 1, 2, 3, 5, 15, ... words and, at
(398, 256), tensors that span several 4096-word pieces."""
import ctypes as C

import numpy as np
import pytest
import torch

import pbt_ref as R
import state_ref as S
from learner_handle import LearnerHandle, alias, err, lib, ring_fields, stream
from test_gpu_td3_pbt import HI, LO, PbtPop, fitness_for, member
from test_gpu_td3_population import NETS, Member

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 2), (17, 33, 16), (398, 256, 128)]
CN_ERR_ARG, CN_ERR_CONFIG = -1, -2
GUARD = 256


class Carved:
    """A member's state on the device with the 36 parameter tensors carved from ONE buffer: tensor j starts (j + shift) % 4 words past
    a 16-byte boundary."""

    def __init__(self, m, shift=0):
        _abi, _ = lib()
        self.m = m
        flat = [(k, t) for k in NETS for t in m.nets[k]]
        self.buf = torch.zeros(sum((t.numel() + 3) // 4 * 4 + 8 for _, t in flat) + 8, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.nets, at = {k: [] for k in NETS}, 0
        for j, (k, t) in enumerate(flat):
            at = (at + 3) // 4 * 4 + (j + shift) % 4
            view = self.buf[at:at + t.numel()].view(t.shape)
            assert view.data_ptr() % 16 == 4 * ((j + shift) % 4)
            view.copy_(t)
            self.nets[k].append(view)
            at += t.numel()
        self.ring = {k: t.cuda().contiguous() for k, t in m.ring.items()}
        self.size = torch.tensor([m.live], dtype=torch.int64, device="cuda")
        mlps = {k: _abi.CnTd3Mlp(*[t.data_ptr() for t in ts]) for k, ts in self.nets.items()}
        self.cfg = _abi.CnTd3Config(obs_dim=m.D, hidden=m.H, batch=m.B, reserved=0.0, seed=m.seed, **ring_fields(dict(self.ring, size=self.size)),
                                    **m.hyper, **mlps)


def segments(L, h, pop):
    """[(cn_state_segment fields, live address)] of a handle, from the library's accessor."""
    _abi, _ = lib()
    f = L.cn_td3_pop_state_segment_dev if pop else L.cn_td3_state_segment_dev
    out, seg = [], _abi.CnStateSegment()
    while len(out) < 100000:
        seg.kind = -1                              # past the end the entry is left alone; a hyper-parameter segment is filled in, address NULL
        ptr = f(h, len(out), C.byref(seg))
        if ptr is None and seg.kind == -1:
            return out
        assert (ptr is None) == (seg.kind == S.HYPER)
        out.append(((seg.member, seg.kind, seg.index, seg.offset, seg.bytes), ptr))
    raise AssertionError("the directory does not end")


def live(L, h, pop):
    """Every state tensor's bytes as they stand (None for the hyper-parameter segments, which have no one address)."""
    torch.cuda.synchronize()
    return [None if ptr is None else alias(ptr, (row[4],), "|u1").cpu().numpy().copy() for row, ptr in segments(L, h, pop)]


def same(got, want, where):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None) and (g is None or (g.shape == w.shape and (g == w).all())), (where, i)


class Blob:
    """A device buffer for a handle's blob between two guards of 0xA5; shift: bytes past a 16-byte boundary (a multiple of 4)."""

    def __init__(self, L, h, pop, shift=0):
        self.L, self.h, self.pop = L, h, pop
        self.n = (L.cn_td3_pop_state_size if pop else L.cn_td3_state_size)(h)
        assert self.n > 0, err()
        self.buf = torch.full((GUARD + shift + self.n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.at = GUARD + shift
        self.ptr = self.buf.data_ptr() + self.at

    def save(self, expect=0, ptr="own", n=None):
        f = self.L.cn_td3_pop_state_save if self.pop else self.L.cn_td3_state_save
        rc = f(self.h, C.c_void_p(self.ptr) if ptr == "own" else ptr, self.n if n is None else n, stream())
        assert rc == expect, (rc, err())
        return self

    def load(self, into=None, expect=0, ptr="own", n=None):
        f = self.L.cn_td3_pop_state_load if self.pop else self.L.cn_td3_state_load
        rc = f(self.h if into is None else into, C.c_void_p(self.ptr) if ptr == "own" else ptr, self.n if n is None else n, stream())
        assert rc == expect, (rc, err())
        return self

    def bytes(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[:self.at] == 0xA5).all() and (b[self.at + self.n:] == 0xA5).all(), "a guard byte was written"
        return b[self.at:self.at + self.n].copy()


def solo(D, H, B, key=0, shift=0, like=None):
    m = Member(D, H, B, key=key, live=max(2 * B, 8), seed=None if like is None else like.seed)
    if like is not None:
        m.ring = {k: t.clone() for k, t in like.ring.items()}
    inst = Carved(m, shift)
    return m, inst, LearnerHandle("td3", inst.cfg, inst)


def step(h, k):
    h.update(int(k % 2 == 0), sync=False)          # policy_delay 2, as Agent.learn(step) decides


def expected_blob(L, h, pop, P, D, H, B, pbt, hypers=None):
    """The restatement packed from direct reads of the live tensors; hypers[p]: float32[5], what the tables hold for member p."""
    tensors = live(L, h, pop)
    rows = [r for r, _ in segments(L, h, pop)]
    for i, r in enumerate(rows):
        if r[1] == S.HYPER:
            tensors[i] = np.asarray(hypers[r[0]], dtype=np.float32).view(np.uint8)
    assert rows == S.directory(P, D, H, B, pbt, pop)[1]
    return S.pack(P, D, H, B, tensors, pbt, pop)


@pytest.mark.parametrize("D,H,B", SHAPES)
def test_solo_blob_equals_the_restatement_and_a_load_continues_bit_for_bit(D, H, B):
    _, L = lib()
    m, inst, h = solo(D, H, B, key=1)
    m2, inst2, h2 = solo(D, H, B, key=2, shift=1, like=m)          # other initial weights, another alignment of every tensor
    try:
        for k in range(3):
            step(h, k)
        blob = Blob(L, h.h, False, shift=0 if B != 2 else 4)       # one shape with the blob itself off the 16-byte boundary
        assert blob.n == S.total_bytes(1, D, H)
        saved = blob.save().bytes()
        at_save = live(L, h.h, False)
        assert (saved == expected_blob(L, h.h, False, 1, D, H, B, False)).all()
        counter = [t for (r, _), t in zip(segments(L, h.h, False), at_save) if r[1] == S.COUNTER][0]
        assert int(counter.view(np.uint64)[0]) == 3
        # round trip: three more updates, back, the same three
        first = []
        for k in range(3, 6):
            step(h, k)
            first.append(live(L, h.h, False))
        assert any((a != b).any() for a, b in zip(first[-1], at_save))
        blob.load()
        same(live(L, h.h, False), at_save, "after the load")
        for k in range(3, 6):
            step(h, k)
            same(live(L, h.h, False), first[k - 3], ("round trip", k))
        # a fresh handle, initialised differently, continues as the original did
        assert any((a != b).any() for a, b in zip(live(L, h2.h, False)[:36], at_save[:36]))
        blob.load(into=h2.h)
        same(live(L, h2.h, False), at_save, "fresh handle after the load")
        for k in range(3, 6):
            step(h2, k)
            same(live(L, h2.h, False), first[k - 3], ("fresh handle", k))
        assert (Blob(L, h2.h, False).save().bytes() == Blob(L, h.h, False).save().bytes()).all()      # equal states give equal blobs
    finally:
        h.close(); h2.close()


def pbt_members(P):
    return [member(p) for p in range(P)]


def pop_hypers(pop, members):
    if pop.bound:
        return pop.state()[2]["hyper"].view(np.float32)
    return np.asarray([[m.hyper[k] for k in R.HYPERS] for m in members], dtype=np.float32)


def make_pop(members, cfg):
    pop = PbtPop(members)
    pop.bound = cfg is not None
    if cfg is not None:
        pop.bind(cfg)
    return pop


@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_population_load_into_a_fresh_population_continues_bit_for_bit(P):
    """P = 1 cannot bind PBT (n_replace is 1 ... P / 2): it runs without; the others with PBT bound and exploits applied before the save."""
    _, L = lib()
    D, H, B = 5, 17, 8
    members = pbt_members(P)
    cfg = R.make_config(max(1, P // 2), explore=("lr_actor", "lr_critic", "gamma", "noise_std", "noise_clip"), factor=(0.8, 1.2), lo=LO, hi=HI,
                        seed=0xBEEF + P) if P > 1 else None
    fit = lambda call: [float((5 * p + 3 * call) % 7) for p in range(P)]
    a, b = make_pop(members, cfg), make_pop(members, cfg)
    try:
        for k in range(2):
            a.update(int(k % 2 == 0))
        if cfg:
            a.exploit(fit(0)); a.update(0); a.exploit(fit(1))
            calls, applied, mem = a.state()
            assert applied > 0 and mem["generation"].max() >= 1
            start = np.asarray([[m.hyper[k] for k in R.HYPERS] for m in members], dtype=np.float32)
            assert (mem["hyper"].view(np.float32) != start).any()          # the tables differ from the configurations
        blob = Blob(L, a.h, True)
        assert blob.n == S.total_bytes(P, D, H, bool(cfg), True)
        saved = blob.save().bytes()
        assert (saved == expected_blob(L, a.h, True, P, D, H, B, bool(cfg), pop_hypers(a, members))).all()
        at_save, state_at_save = live(L, a.h, True), a.state() if cfg else None

        def go_on(pop):
            out = []
            for k in range(3, 6):
                pop.update(int(k % 2 == 0))
                out.append(live(L, pop.h, True) + [t.cpu().numpy().view(np.uint8) for ps in pop.params() for t in ps])
            if cfg:
                pop.exploit(fit(2))
                calls, applied, mem = pop.state()
                out.append([np.asarray([calls, applied], dtype=np.uint64).view(np.uint8), mem.view(np.uint8)] + live(L, pop.h, True))
                pop.update(1)                                              # ... with the hyper-parameters that exploit wrote
                out.append(live(L, pop.h, True) + [t.cpu().numpy().view(np.uint8) for ps in pop.params() for t in ps])
            return out
        want = go_on(a)
        blob.load(into=b.h)
        same(live(L, b.h, True), at_save, "fresh population after the load")
        if cfg:
            sa, sb = state_at_save, b.state()
            assert sa[:2] == sb[:2] and (sa[2].view(np.uint8) == sb[2].view(np.uint8)).all()
        assert (Blob(L, b.h, True).save().bytes() == saved).all()          # the hyper-parameter tables too
        got = go_on(b)
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, ("fresh population", i))
    finally:
        a.close(); b.close()


def test_python_owners_round_trip_and_show_the_loaded_hyper_parameters():
    """FusedPopulation.save_state / load_state through crowdnav.td3.Population: pbt_state() of the loading side shows the loaded values
    on its agents."""
    from crowdnav.td3 import Agent, Population

    def population():
        agents = [Agent(obs_dim=5, hidden=17, batch_size=8, memory_size=64, seed=10 + p, actor_lr=3e-4 * (1 + p), critic_lr=1e-3 / (1 + p),
                        noise_std=0.2 + 0.01 * p) for p in range(4)]
        g = torch.Generator().manual_seed(3)
        for a in agents:
            a.memory.add(torch.randn((40, 5), generator=g).cuda(), torch.rand((40, 2), generator=g).cuda(), torch.randn(40, generator=g).cuda(),
                         torch.randn((40, 5), generator=g).cuda(), (torch.rand(40, generator=g) < 0.1).cuda())
        return Population(agents).bind_pbt(2, explore=("lr_actor", "lr_critic", "noise_std"), min_episodes=1, seed=7)
    a, b = population(), population()
    fitness = torch.tensor([3.0, 1.0, 0.0, 2.0], device="cuda")
    for k in range(4):
        a.learn(k)
    a.exploit(fitness)
    blob = a._fused.save_state().clone()
    assert blob.numel() == a._fused.state_size() == S.total_bytes(4, 5, 17, True, True)
    want = a.pbt_state()
    assert want["applied"] == 1
    b._fused.load_state(blob)
    got = b.pbt_state()
    assert got == want
    for x, y in zip(a.agents, b.agents):
        assert (x.actor_lr, x.critic_lr, x.noise_std) == (y.actor_lr, y.critic_lr, y.noise_std) and y.opt_a.param_groups[0]["lr"] == y.actor_lr
    for k in range(4, 7):
        la, lb = a.learn(k), b.learn(k)
        assert torch.equal(la, lb)
    for x, y in zip(a.agents, b.agents):
        assert all(torch.equal(p, q) for p, q in zip(x.actor.parameters(), y.actor.parameters()))
        assert all(torch.equal(p, q) for p, q in zip(x.q2_t.parameters(), y.q2_t.parameters()))


def header_with(saved, **fields):
    """The blob `saved` with header fields replaced."""
    _abi, _ = lib()
    hdr = _abi.CnStateHeader.from_buffer_copy(saved[:C.sizeof(_abi.CnStateHeader)].tobytes())
    for k, v in fields.items():
        setattr(hdr, k, v)
    out = saved.copy()
    out[:C.sizeof(_abi.CnStateHeader)] = np.frombuffer(bytes(hdr), dtype=np.uint8)
    return out


def test_refusals_write_nothing():
    _, L = lib()
    D, H, B = 3, 5, 2
    m, inst, h = solo(D, H, B, key=3)
    members = pbt_members(2)
    pop = make_pop(members, R.make_config(1, explore=("lr_actor",), factor=(0.8, 1.2), lo=LO, hi=HI, seed=5))
    try:
        for handle, is_pop, name in ((h.h, False, "cn_td3_state_"), (pop.h, True, "cn_td3_pop_state_")):
            (h if not is_pop else pop).update(0)
            blob = Blob(L, handle, is_pop)
            before = live(L, handle, is_pop)
            # save: nothing of the buffer is written
            blob.save(CN_ERR_ARG, ptr=None); assert name + "save: null blob_dev" in err()
            blob.save(CN_ERR_ARG, n=blob.n - 16); assert "bytes" in err()
            blob.save(CN_ERR_ARG, n=blob.n + 16); assert "bytes" in err()
            blob.save(CN_ERR_ARG, ptr=C.c_void_p(blob.ptr + 1)); assert "4-byte aligned" in err()
            torch.cuda.synchronize()
            assert (blob.buf == 0xA5).all()
            saved = blob.save().bytes()
            (h if not is_pop else pop).update(1)                           # the live state now differs from the blob
            before = live(L, handle, is_pop)
            blob.load(expect=CN_ERR_ARG, ptr=None); assert name + "load: null blob_dev" in err()
            blob.load(expect=CN_ERR_ARG, n=blob.n - 16); assert "bytes" in err()
            blob.load(expect=CN_ERR_ARG, ptr=C.c_void_p(blob.ptr + 2)); assert "4-byte aligned" in err()
            bad = [(CN_ERR_ARG, "magic", dict(magic=S.MAGIC ^ 1)), (CN_ERR_ARG, "version", dict(version=2)), (CN_ERR_CONFIG, "family", dict(family=2)),
                   (CN_ERR_CONFIG, "n_members", dict(n_members=3)), (CN_ERR_CONFIG, "obs_dim", dict(obs_dim=D + 1)), (CN_ERR_CONFIG, "hidden", dict(hidden=H + 1)),
                   (CN_ERR_CONFIG, "batch", dict(batch=B + 1 if not is_pop else 9)), (CN_ERR_CONFIG, "pbt_bound", dict(pbt_bound=0 if is_pop else 1)),
                   (CN_ERR_CONFIG, "n_segments", dict(n_segments=1)), (CN_ERR_CONFIG, "total_bytes", dict(total_bytes=16))]
            for rc, word, fields in bad:
                blob.buf[blob.at:blob.at + blob.n] = torch.from_numpy(header_with(saved, **fields)).cuda()
                blob.load(expect=rc)
                assert word in err(), (word, err())
                same(live(L, handle, is_pop), before, ("refused load", word))
            wrong = saved.copy()
            wrong[48 + 32 + 8] ^= 1                                        # the second directory entry's index
            blob.buf[blob.at:blob.at + blob.n] = torch.from_numpy(wrong).cuda()
            blob.load(expect=CN_ERR_CONFIG); assert "directory" in err()
            same(live(L, handle, is_pop), before, "refused load: directory")
            blob.buf[blob.at:blob.at + blob.n] = torch.from_numpy(saved).cuda()
            blob.load()                                                    # and the blob as it was saved is taken
            assert any((x != y).any() for x, y in zip(live(L, handle, is_pop), before) if x is not None)
        # a population that never bound PBT has another size: the bound population's blob is refused by its byte count
        plain = make_pop(members, None)
        try:
            before = live(L, plain.h, True)
            big = Blob(L, pop.h, True).save()
            assert Blob(L, plain.h, True).n < big.n
            big.load(into=plain.h, expect=CN_ERR_ARG); assert "bytes" in err()
            same(live(L, plain.h, True), before, "refused load: size")
        finally:
            plain.close()
    finally:
        h.close(); pop.close()


def test_a_captured_save_replays_to_the_same_blob():
    _, L = lib()
    D, H, B = 17, 33, 16
    m, inst, h = solo(D, H, B, key=4)
    try:
        h.update(0)
        blob = Blob(L, h.h, False)                 # (the size call built the job table: the capture only enqueues)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            blob.save()
        torch.cuda.current_stream().wait_stream(side)
        h.update(1)
        g.replay()
        first = blob.bytes()
        assert (first == expected_blob(L, h.h, False, 1, D, H, B, False)).all()
        assert (first == Blob(L, h.h, False).save().bytes()).all()         # ... which is what an eager save gives
        h.update(0)
        g.replay()
        second = blob.bytes()
        assert (second != first).any() and (second == expected_blob(L, h.h, False, 1, D, H, B, False)).all()
    finally:
        h.close()
