"""cn_nstep_record (include/crowdnav.h) on the GPU against its NumPy restatement (tests/nstep_ref.py, which
tests/test_nstep_ref_helpers.py holds to hand-written episodes and a derived rounding bound): members with explicit counters /
last_return on synthetic arrays with scripted `done`, every buffer compared byte for byte after EVERY call -- the five ring arrays
with their sentinel rows, pos, size, the log rows, n, tot, prev, resetting and the five pending tensors.  With W = 1 the twin is
cn_pop_record itself."""
import ctypes as C

import numpy as np
import pytest
import torch

import nstep_ref as N
import pop_record_ref as R
from learner_handle import lib, stream

pytestmark = pytest.mark.gpu

CN_ERR_ARG, CN_ERR_CONFIG = -1, -2
INPUTS = ("obs", "action", "reward", "done", "counters", "last_return")
STATE = tuple(k for k in R.ARRAYS if k not in INPUTS + ("resetting",))     # what a call writes in the caller's buffers


def _dev(m):
    """Member m's caller-owned buffers on the device, sentinel rows included; the three counters as int64."""
    t = {k: torch.from_numpy(np.ascontiguousarray(m[k])).cuda() for k in R.ARRAYS if k != "resetting"}
    for k in R.SCALARS:
        t[k] = torch.tensor(m[k], dtype=torch.int64, device="cuda")
    return t


def _rec_struct(_abi, t, m):
    p = (lambda k: t[k].data_ptr()) if m["n"] else (lambda k: None)
    ring = _abi.CnReplayRing(s=t["s"].data_ptr(), a=t["a"].data_ptr(), r=t["r"].data_ptr(), s2=t["s2"].data_ptr(), d=t["d"].data_ptr(),
                             capacity=m["cap"], pos_dev=t["pos"].data_ptr(), size_dev=t["size"].data_ptr(), obs_dim=m["D"], reserved=0)
    log = _abi.CnEpisodeLog(rows=t["rows"].data_ptr(), max_rows=m["max_rows"], n_dev=t["n_log"].data_ptr(), tot_dev=t["tot"].data_ptr())
    return _abi.CnPopRecordMember(env=None, counters=p("counters"), last_return=p("last_return"), prev=p("prev"), obs=p("obs"),
                                  action=p("action"), reward=p("reward"), done=p("done"), ring=ring, log=log, n=m["n"], reserved=0)


class Handle:
    """An n-step handle over members ms (NumPy, with N.add_pending's fields) and their device buffers ts."""

    def __init__(self, ms, ts, W):
        from crowdnav._fused import FusedNStepRecorder
        _abi, _ = lib()
        self.ms, self.ts = ms, ts
        members = [_abi.CnNstepMember(rec=_rec_struct(_abi, t, m), gamma=float(m["gamma"]), reserved_f=0.0) for m, t in zip(ms, ts)]
        self.rec = FusedNStepRecorder(members, W, ms[0]["D"], torch.device("cuda:0"), 0, keep=ts)
        assert lib()[1].cn_nstep_record_members(self.rec.h) == len(ms)

    def upload_inputs(self, p):
        m, t = self.ms[p], self.ts[p]
        for k in INPUTS:
            t[k].copy_(torch.from_numpy(np.ascontiguousarray(m[k])))

    def download(self, p):
        """Member p as the device holds it, in the restatement's form."""
        m, t = self.ms[p], self.ts[p]
        got = {k: v for k, v in m.items() if not isinstance(v, np.ndarray) and k not in R.SCALARS}
        for k in R.ARRAYS:
            if k != "resetting":
                got[k] = t[k].cpu().numpy()
        for k in R.SCALARS:
            got[k] = int(t[k])
        got["resetting"] = np.concatenate([self.rec.resetting(p).cpu().numpy(), m["resetting"][m["n"]:]])
        for k, v in zip(N.PENDING, self.rec.pending(p)):
            got[k] = v.cpu().numpy()
        return got

    def close(self):
        torch.cuda.synchronize()
        self.rec.__del__()


def _member(rng, n, D, W, gamma=0.99, cap=None, **kw):
    return N.add_pending(R.make_member(rng, n, D, cap=max(n * W, 1) if cap is None else cap, done="none", resetting="none", **kw), W, gamma)


def _scripted(ms, W, calls, seed, handle=None, check=True, first_call=0):
    """The 20-call script of nstep_ref.scripted_call through one handle and through the restatement, compared after every call."""
    ts = [_dev(m) for m in ms] if handle is None else handle.ts
    h = Handle(ms, ts, W) if handle is None else handle
    rngs = [np.random.default_rng(seed + 100 * p) for p in range(len(ms))] if first_call == 0 else h.rngs
    h.rngs = rngs
    for call in range(first_call, first_call + calls):
        for p, m in enumerate(ms):
            if m["n"] == 0:
                continue
            for e in N.scripted_call(rngs[p], m, call, W):
                m["resetting"][e] = 1
                h.rec.resetting(p)[e] = 1
            h.upload_inputs(p)
        h.rec.record(call + 1)
        for p, m in enumerate(ms):
            N.record(m, call + 1)
            if check:
                N.assert_members_equal(h.download(p), m, "call %d member %d" % (call, p))
    return h


def test_window_one_is_cn_pop_record_byte_for_byte():
    """Twin buffers, P = 3 with n = (5, 0, 1025) (the third crosses the 1024-thread scan), D = 7, 12 calls: one side through
    cn_nstep_record with W = 1, the other through cn_pop_record; ring, log, prev and resetting after every call, and the restatement."""
    from crowdnav._fused import FusedPopulationRecorder
    _abi, _ = lib()
    rng = np.random.default_rng(1)
    ms = [_member(rng, n, 7, 1, cap=max(n, 1) + 3, pos=2, size=1) for n in (5, 0, 1025)]
    ts, twins = [_dev(m) for m in ms], [_dev(m) for m in ms]
    h = Handle(ms, ts, 1)
    plain = FusedPopulationRecorder([_rec_struct(_abi, t, m) for t, m in zip(twins, ms)], 7, torch.device("cuda:0"), 0, keep=twins)
    rngs = [np.random.default_rng(10 + p) for p in range(3)]
    for call in range(12):
        for p, m in enumerate(ms):
            if m["n"]:
                N.scripted_call(rngs[p], m, call, 1)
                h.upload_inputs(p)
                for k in INPUTS:
                    twins[p][k].copy_(ts[p][k])
        h.rec.record(call + 1); plain.record(call + 1)
        for p, m in enumerate(ms):
            N.record(m, call + 1)
            N.assert_members_equal(h.download(p), m, "call %d member %d" % (call, p))
            for k in STATE + R.SCALARS:
                a, b = ts[p][k], twins[p][k]
                assert torch.equal(a.view(torch.int64) if k == "tot" else a, b.view(torch.int64) if k == "tot" else b), (call, p, k)
            assert torch.equal(h.rec.resetting(p), plain.resetting(p)), (call, p)
            pend = h.rec.pending(p)
            assert not pend[0].any() and not pend[1].any() and not pend[2].any() and not pend[3].any()      # W = 1: nothing ever pends
    assert int(ts[2]["n_log"]) > 1025 and 0 < int(ts[0]["size"])
    h.close()


@pytest.mark.parametrize("D", (1, 7, 398))
@pytest.mark.parametrize("W", (2, 3, 5, 16))
def test_twenty_scripted_calls_equal_the_restatement(W, D):
    """n = 7 environments, capacity == n W exactly, 20 calls of nstep_ref.scripted_call: an environment done on consecutive calls, one
    done at its first step, all done in one call (the ring wraps inside it), a flag set by the caller, rewards -0.0f, +-200 and
    inexact products."""
    m = _member(np.random.default_rng(W * 1000 + D), 7, D, W, pos=3, size=2)
    h = _scripted([m], W, 20, seed=W + D)
    assert m["size"] == m["cap"] == 7 * W and m["n_log"] >= 10
    assert (m["d"][:m["cap"]] == 0).any() and (m["d"][:m["cap"]] == 1).any()          # rows of both kinds are in the ring
    h.close()


def test_a_fused_multiply_add_would_show():
    """The script's rewards make at least one pending return differ between separate rounding and a float64 fused evaluation."""
    rng = np.random.default_rng(5)
    w = N.discount(0.99, 1)
    r = rng.standard_normal(64).astype(np.float32) * 50
    base = rng.standard_normal(64).astype(np.float32)
    separate = (base + (w * r).astype(np.float32)).astype(np.float32)
    fused = (base.astype(np.float64) + np.float64(w) * r.astype(np.float64)).astype(np.float32)
    assert (separate != fused).any()


def test_a_member_is_independent_of_its_position_and_of_the_others():
    """P = 4 with n = (3, 0, 70, 1030), W = 3, 8 calls: every member with rows equals a handle of its own on the same inputs."""
    W, rows = 3, (3, 0, 70, 1030)
    mk = lambda: [_member(np.random.default_rng(40 + p), n, 4, W, gamma=(0.99, 0.9, 1.0, 0.97)[p], cap=n * W + 5, pos=1) for p, n in enumerate(rows)]
    together = mk()
    h = _scripted(together, W, 8, seed=7)
    for p, n in enumerate(rows):
        if n == 0:
            continue
        alone = mk()[p]
        ts = [_dev(alone)]
        h1 = Handle([alone], ts, W)
        rng = np.random.default_rng(7 + 100 * p)
        for call in range(8):
            for e in N.scripted_call(rng, alone, call, W):
                alone["resetting"][e] = 1
                h1.rec.resetting(0)[e] = 1
            h1.upload_inputs(0)
            h1.rec.record(call + 1)
        N.assert_members_equal(h1.download(0), h.download(p), "member %d alone" % p)
        h1.close()
    empty = h.download(1)
    assert empty["pos"] == 1 and empty["size"] == 0 and empty["n_log"] == 0 and all(v.numel() == 0 for v in h.rec.pending(1))
    h.close()


def test_state_round_trip_into_a_fresh_handle():
    """7 calls, then the pending tensors and the flags are copied into a fresh handle over copies of the buffers; both stay byte-equal
    (and equal to the restatement) for 7 more calls."""
    W = 5
    m = _member(np.random.default_rng(9), 9, 7, W, cap=9 * W + 4)
    h = _scripted([m], W, 7, seed=3)
    assert m["count"].any() and m["pret"].any()
    m2 = N.copy_member(m)
    t2 = {k: v.clone() for k, v in h.ts[0].items()}
    h2 = Handle([m2], [t2], W)
    assert not any(v.any() for v in h2.rec.pending(0)) and not h2.rec.resetting(0).any()         # zero at create
    for dst, src in zip(h2.rec.pending(0), h.rec.pending(0)):
        dst.copy_(src)
    h2.rec.resetting(0).copy_(h.rec.resetting(0))
    h2.rngs = [np.random.default_rng(77)]
    h.rngs = [np.random.default_rng(77)]
    _scripted([m], W, 7, seed=0, handle=h, first_call=7)
    _scripted([m2], W, 7, seed=0, handle=h2, first_call=7)
    N.assert_members_equal(h2.download(0), h.download(0), "restored")
    h.close(); h2.close()


def test_every_refusal_carries_its_message_and_writes_nothing():
    _abi, L = lib()
    m = _member(np.random.default_rng(2), 4, 3, 2, cap=8)
    t = _dev(m)
    before = {k: v.clone() for k, v in t.items()}

    def refused(code, *texts, W=2, gamma=0.99, n_members=1, obs_dim=3, **kw):
        rec = _rec_struct(_abi, t, m)
        for k, v in kw.items():
            if k.startswith("ring_"):
                setattr(rec.ring, k[5:], v)
            else:
                setattr(rec, k, v)
        arr = (_abi.CnNstepMember * 1)(_abi.CnNstepMember(rec=rec, gamma=gamma, reserved_f=0.0))
        h = C.c_void_p()
        rc = L.cn_nstep_record_create(arr, n_members, W, obs_dim, 0, C.byref(h))
        msg = L.cn_last_error().decode()
        assert rc == code and not h.value and "cn_nstep_record_create" in msg, (rc, msg)
        for x in texts:
            assert x in msg, (x, msg)

    for W in (0, -1, 17, 1 << 20):
        refused(CN_ERR_ARG, "n_step", "1 ... 16", W=W)
    for g in (float("nan"), float("inf"), 0.0, -0.5, 1.0000001, 2.0):
        refused(CN_ERR_ARG, "member 0", "gamma", "(0, 1]", gamma=g)
    refused(CN_ERR_ARG, "member 0", "n * n_step", "ring.capacity", W=3)                       # 4 * 3 > 8
    refused(CN_ERR_ARG, "member 0", "n exceeds ring.capacity", W=1, ring_capacity=3)          # cn_pop_record_create's words
    # carried over from cn_pop_record_create, the entry point named anew
    refused(CN_ERR_ARG, "n_members", "1 ... 64", n_members=0)
    refused(CN_ERR_ARG, "n_members", "1 ... 64", n_members=65)
    refused(CN_ERR_CONFIG, "obs_dim", obs_dim=0)
    refused(CN_ERR_ARG, "member 0", "prev is null", prev=None)
    refused(CN_ERR_ARG, "member 0", "n is negative", n=-1)
    refused(CN_ERR_ARG, "member 0", "env", "counters", "last_return", counters=None)
    refused(CN_ERR_ARG, "member 0", "incomplete ring", ring_s2=None)
    refused(CN_ERR_CONFIG, "member 0", "ring.obs_dim", obs_dim=4)
    assert L.cn_nstep_record(None, 1.0, stream()) == CN_ERR_ARG and b"cn_nstep_record: null handle" in L.cn_last_error()
    ok = Handle([m], [t], 2)
    pd = _abi.CnNstepPending()
    for p in (-1, 1, 64):
        assert L.cn_nstep_record_resetting(ok.rec.h, p) is None and ("member %d out of range" % p) in L.cn_last_error().decode()
        assert L.cn_nstep_record_pending(ok.rec.h, p, C.byref(pd)) == CN_ERR_ARG and "cn_nstep_record_pending" in L.cn_last_error().decode()
    assert L.cn_nstep_record_pending(ok.rec.h, 0, None) == CN_ERR_ARG and "out is null" in L.cn_last_error().decode()
    ok.close()
    torch.cuda.synchronize()
    for k, v in t.items():
        assert torch.equal(v.view(torch.int64) if v.dtype == torch.float64 else v, before[k].view(torch.int64) if v.dtype == torch.float64 else before[k]), k
