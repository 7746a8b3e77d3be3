"""The population recorder of include/crowdnav.h (cn_pop_record_*) without a GPU: cn_pop_record_member against its ctypes mirror as gcc
lays it out, the five exports, every refusal that can be reached without a handle (the argument checks come before any device work;
FAKE pointers are compared and never dereferenced; the two refusals that need a live handle are in tests/test_gpu_pop_record.py),
crowdnav.train's --population-record switch, and the NumPy restatement of the statement (tests/pop_record_ref.py) against the PyTorch
formulations DeviceReplay(fused=False) / DeviceEpisodeLog(fused=False) on CPU tensors."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import pop_record_ref as R
from conftest import ROOT
from learner_handle import lib

CN_ERR_ARG, CN_ERR_CONFIG = -1, -2
NAMES = ("cn_pop_record_create", "cn_pop_record_destroy", "cn_pop_record_members", "cn_pop_record_resetting", "cn_pop_record")
FAKE = 0x1000        # a non-null "device pointer"
FIELDS = ["env", "counters", "last_return", "prev", "obs", "action", "reward", "done", "ring", "log", "n", "reserved"]


def test_member_struct_matches_its_mirror_field_by_field(tmp_path):
    _abi, _ = lib()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _abi.CnPopRecordMember
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(cn_pop_record_member));', 'printf("max %d\\n", CN_POP_RECORD_MAX);',
             'printf("abi %d\\n", CN_ABI_VERSION);', 'printf("cols %d\\n", CN_COUNTER_COLS);']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(cn_pop_record_member, %s));' % (f[0], f[0]))
    lines += ["{ int (*f)(const cn_pop_record_member*, int, int, int, cn_pop_record_handle*) = cn_pop_record_create; (void)f; }",
              "{ void (*f)(cn_pop_record_handle) = cn_pop_record_destroy; (void)f; }",
              "{ int (*f)(cn_pop_record_handle) = cn_pop_record_members; (void)f; }",
              "{ uint8_t* (*f)(cn_pop_record_handle, int) = cn_pop_record_resetting; (void)f; }",
              "{ int (*f)(cn_pop_record_handle, float, void*) = cn_pop_record; (void)f; }",
              "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    obj = tmp_path / "layout.o"
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"),
                    "-o", str(obj), str(src)], check=True)
    stubs = tmp_path / "stubs.c"
    stubs.write_text("\n".join("void %s(void) {}" % n for n in NAMES))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(obj), str(stubs)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls) == 64 + C.sizeof(_abi.CnReplayRing) + C.sizeof(_abi.CnEpisodeLog) + 8 == 176
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]
    assert [f[0] for f in cls._fields_] == FIELDS
    assert int(got["max"]) == _abi.CN_POP_RECORD_MAX == 64
    assert int(got["cols"]) == _abi.CN_COUNTER_COLS == 14
    assert int(got["abi"]) == _abi.EXPECTED_ABI == 7              # additive: the version stays


def test_the_five_names_are_exported_with_prototypes():
    _abi, L = lib()
    for name in NAMES:
        assert name in _abi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.cn_pop_record_create.argtypes[0] is C.POINTER(_abi.CnPopRecordMember)
    assert L.cn_pop_record.argtypes == [C.c_void_p, C.c_float, C.c_void_p]
    assert L.cn_pop_record_resetting.restype is C.c_void_p
    assert L.cn_pop_record_destroy.restype is None


def _ring(_abi, base=FAKE, **kw):
    f = dict(s=base, a=base + 8, r=base + 16, s2=base + 24, d=base + 32, capacity=64, pos_dev=base + 40, size_dev=base + 48, obs_dim=398, reserved=0)
    f.update(kw)
    return _abi.CnReplayRing(**f)


def _log(_abi, base=FAKE, **kw):
    f = dict(rows=base + 56, max_rows=100, n_dev=base + 64, tot_dev=base + 72)
    f.update(kw)
    return _abi.CnEpisodeLog(**f)


def _member(_abi, base, ring=None, log=None, **kw):
    """A valid explicit-array member whose eleven written pointers are base + 0, 8, ..., 80 (distinct between bases 0x100 apart)."""
    f = dict(env=None, counters=FAKE, last_return=FAKE, prev=base + 80, obs=FAKE, action=FAKE, reward=FAKE, done=FAKE,
             ring=_ring(_abi, base, **(ring or {})), log=_log(_abi, base, **(log or {})), n=16, reserved=0)
    f.update(kw)
    return _abi.CnPopRecordMember(**f)


def _create(L, members, n_members, obs_dim, want_rc, *texts, out="fresh"):
    h = C.c_void_p()
    rc = L.cn_pop_record_create(members, n_members, obs_dim, 0, C.byref(h) if out == "fresh" else out)
    msg = L.cn_last_error().decode()
    assert rc == want_rc, (rc, msg)
    for t in texts:
        assert t in msg, (t, msg)
    assert "cn_pop_record_create" in msg
    assert not h.value                       # *out stays NULL


def test_create_refusals_name_the_field_and_the_member():
    _abi, L = lib()
    arr = lambda *ms: (_abi.CnPopRecordMember * len(ms))(*ms)
    A, B, Cc = 0x10000, 0x20000, 0x30000
    good = lambda base=A, **kw: _member(_abi, base, **kw)
    _create(L, None, 1, 398, CN_ERR_ARG, "members")
    _create(L, arr(good()), 1, 398, CN_ERR_ARG, "out", out=None)
    big = arr(*[good()] * 65)
    for n in (0, -1, 65, 1 << 20):
        _create(L, big, n, 398, CN_ERR_ARG, "n_members", "1 ... 64")
    for D in (0, -1, -398):
        _create(L, arr(good()), 1, D, CN_ERR_CONFIG, "obs_dim")
    _create(L, arr(good(), good(B, n=-1)), 2, 398, CN_ERR_ARG, "member 1", "n is negative")
    _create(L, arr(good(n=-(1 << 31))), 1, 398, CN_ERR_ARG, "member 0", "n is negative")
    # a NULL row pointer in a member with rows; none of them is looked at in a member without
    for field in ("prev", "obs", "action", "reward", "done"):
        _create(L, arr(good(), good(B), good(Cc, **{field: None})), 3, 398, CN_ERR_ARG, "member 2", field + " is null")
    # neither an environment nor both explicit arrays
    for kw in (dict(counters=None), dict(last_return=None), dict(counters=None, last_return=None)):
        _create(L, arr(good(), good(B, **kw)), 2, 398, CN_ERR_ARG, "member 1", "env", "counters", "last_return")
    # an incomplete ring or log
    for field in ("s", "a", "r", "s2", "d", "pos_dev", "size_dev"):
        _create(L, arr(good(), good(B, ring={field: None})), 2, 398, CN_ERR_ARG, "member 1", "incomplete ring")
    for kw in (dict(capacity=0), dict(capacity=-5), dict(obs_dim=0)):
        _create(L, arr(good(ring=kw)), 1, 398, CN_ERR_ARG, "member 0", "incomplete ring")
    for field in ("rows", "n_dev", "tot_dev"):
        _create(L, arr(good(), good(B, log={field: None})), 2, 398, CN_ERR_ARG, "member 1", "incomplete log")
    _create(L, arr(good(log=dict(max_rows=-1))), 1, 398, CN_ERR_ARG, "member 0", "max_rows")
    _create(L, arr(good(), good(B, n=65)), 2, 398, CN_ERR_ARG, "member 1", "capacity")
    _create(L, arr(good(n=17, ring=dict(capacity=16))), 1, 398, CN_ERR_ARG, "member 0", "capacity")
    # one observation width for all
    _create(L, arr(good(), good(B, ring=dict(obs_dim=397))), 2, 398, CN_ERR_CONFIG, "member 1", "ring.obs_dim")
    _create(L, arr(good()), 1, 363, CN_ERR_CONFIG, "member 0", "ring.obs_dim")
    # two members naming the same written array: each of the eleven, named on both sides
    for field in ("s", "a", "r", "s2", "d", "pos_dev", "size_dev"):
        shared = getattr(_ring(_abi, A), field)
        _create(L, arr(good(), good(B), good(Cc, ring={field: shared})), 3, 398, CN_ERR_CONFIG, "member 2", "member 0", "ring." + field)
    for field in ("rows", "n_dev", "tot_dev"):
        shared = getattr(_log(_abi, B), field)
        _create(L, arr(good(), good(B), good(Cc, log={field: shared})), 3, 398, CN_ERR_CONFIG, "member 2", "member 1", "log." + field)
    _create(L, arr(good(), good(B, prev=A + 80)), 2, 398, CN_ERR_CONFIG, "member 1", "member 0", "prev")
    _create(L, arr(good(), good()), 2, 398, CN_ERR_CONFIG, "member 1", "member 0", "race")
    # the first failing check wins in member order
    _create(L, arr(good(n=-1), good(B, obs=None)), 2, 398, CN_ERR_ARG, "member 0")


def test_null_handles_are_refused_everywhere():
    _abi, L = lib()
    assert L.cn_pop_record(None, 1.0, None) == CN_ERR_ARG and b"cn_pop_record: null handle" in L.cn_last_error()
    assert L.cn_pop_record_resetting(None, 0) is None and b"cn_pop_record_resetting: null handle" in L.cn_last_error()
    assert L.cn_pop_record_members(None) == 0
    L.cn_pop_record_destroy(None)                                # a no-op, as free(NULL)


def test_population_record_switch():
    from crowdnav import train
    base = ["--algo", "td3", "--learner", "fused"]
    assert train.parse_args(base + ["--population", "2"]).population_record == "one-call"          # the default
    for v in ("one-call", "per-member"):
        a = train.parse_args(base + ["--population", "2", "--population-record", v])
        assert a.population_record == v and a.population == 2 and a.population_act == "one-launch"


@pytest.mark.parametrize("argv,text", [
    (["--population-record", "per-member"], "--population"),                                     # not without a population
    (["--algo", "td3", "--learner", "fused", "--population-record", "one-call"], "--population"),
    (["--algo", "td3", "--learner", "fused", "--population", "2", "--population-record", "both"], "invalid choice"),
])
def test_population_record_refusals(argv, text, capsys):
    from crowdnav import train
    with pytest.raises(SystemExit) as ex:
        train.parse_args(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "--population-record" in err and text in err, err


# ---- the restatement against the PyTorch formulations, on the CPU ---------------------------------------------------------------------
def _torch_side(m):
    """DeviceReplay(fused=False) / DeviceEpisodeLog(fused=False) on CPU tensors, loaded with member m's state."""
    import torch
    from crowdnav.td3 import DeviceReplay
    from crowdnav.train import DeviceEpisodeLog
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    cap, mr = m["cap"], m["max_rows"]
    rep = DeviceReplay(cap, m["D"], "cpu", fused=False)
    for k in ("s", "s2", "a"):
        getattr(rep, k)[:cap] = t(m[k][:cap])
    rep.r[:cap, 0] = t(m["r"][:cap]); rep.d[:cap, 0] = t(m["d"][:cap])
    rep.pos_dev.fill_(m["pos"]); rep.size_dev.fill_(m["size"])
    log = DeviceEpisodeLog("cpu", mr, fused=False)
    log.rows[:mr] = t(m["rows"][:mr]); log.n.fill_(m["n_log"]); log.tot.copy_(t(m["tot"]))
    return rep, log


def _torch_record(m, rep, log, launch):
    import torch
    n = m["n"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:n]))
    keep = t(m["resetting"]) == 0
    rep.add_masked(t(m["prev"]), t(m["action"]), t(m["reward"]), t(m["obs"]), t(m["done"]), keep)
    log.add(t(m["done"]), t(m["counters"]), t(m["last_return"]), launch, keep)


CPU_CASES = [
    # n, D, patterns of done / resetting, ring (cap, pos, size), log (max_rows, n_log)
    dict(n=1, D=1, done="all", resetting="none"),
    dict(n=63, D=5, done="alternating", resetting="last"),
    dict(n=64, D=3, done="last", resetting="alternating"),
    dict(n=65, D=7, done="none", resetting="all"),
    dict(n=65, D=7, done="all", resetting="none", cap=65, pos=63, size=60),          # capacity == n, the write wraps, size saturates
    dict(n=1023, D=2, done="alternating", resetting="alternating", cap=1100, pos=1098, size=1000),
    dict(n=1025, D=2, done="row1024", resetting="row1024"),
    dict(n=2049, D=1, done="all", resetting="row1024", max_rows=2000, n_log=1997),   # rows are dropped, the count goes on
    dict(n=17, D=4, done="all", resetting="none", max_rows=0),
]


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: "n%d-%s-%s" % (c["n"], c["done"], c["resetting"]))
def test_restatement_equals_the_pytorch_formulations(case):
    """Two consecutive calls (the second sees resetting = the first's done and prev = the first's obs).  The returns are multiples of
    1/8 below 1000, so that every float64 sum is exact and its order cannot matter: the PyTorch form sums in another order."""
    rng = np.random.default_rng(case["n"] * 31 + case["D"])
    m = R.make_member(rng, returns="exact", **case)
    rep, log = _torch_side(m)
    cap, mr, n = m["cap"], m["max_rows"], m["n"]
    for launch in (5, 6):
        before = R.copy_member(m)
        _torch_record(m, rep, log, launch)
        R.record(m, launch)
        for k in ("s", "s2", "a"):
            assert np.array_equal(getattr(rep, k)[:cap].numpy(), m[k][:cap]), k
        assert np.array_equal(rep.r[:cap, 0].numpy(), m["r"][:cap]) and np.array_equal(rep.d[:cap, 0].numpy(), m["d"][:cap])
        assert int(rep.pos_dev) == m["pos"] and int(rep.size_dev) == m["size"]
        assert np.array_equal(log.rows[:mr].numpy(), m["rows"][:mr])
        assert int(log.n) == m["n_log"] and np.array_equal(log.tot.numpy(), m["tot"])
        # what the PyTorch side has no word for: the flags, prev, and everything beyond the rows
        assert np.array_equal(m["resetting"][:n], (before["done"][:n] != 0)) and np.array_equal(m["prev"][:n], before["obs"][:n])
        for k in ("s", "s2", "a", "r", "d"):
            assert (m[k][cap:] == R.SENTINEL).all(), k
        assert (m["rows"][mr:] == R.SENTINEL).all() and (m["prev"][n:] == R.SENTINEL).all() and (m["resetting"][n:] == 9).all()
        for k in ("obs", "action", "reward", "done", "counters", "last_return"):
            assert m[k].tobytes() == before[k].tobytes(), k               # inputs are read only
        # the next launch: new observations, actions, rewards and another done pattern
        m["obs"][:n] = rng.standard_normal((n, m["D"])).astype(np.float32)
        m["done"][:n] = R.pattern("alternating", n)


def test_kernel_order_sum_is_a_sum_in_the_stated_order():
    """Magnitudes 1e-12 ... 1e12: within n ulps of the exact sum (math.fsum) scaled by the sum of magnitudes; a permutation of the rows changes
    the bits (so the order is a statement, not a detail); and the order itself against explicit loops."""
    rng = np.random.default_rng(7)
    x = R.mixed_returns(rng, 2049, -12, 12).astype(np.float64)
    got = R.kernel_order_sum(x)
    assert abs(got - math.fsum(x)) <= len(x) * np.finfo(np.float64).eps * np.abs(x).sum()
    assert any(R.kernel_order_sum(rng.permutation(x)) != got for _ in range(8))
    part = [0.0] * 1024
    for i, v in enumerate(x):
        part[i % 1024] += v
    waves = []
    for w in range(16):
        lanes = part[64 * w:64 * w + 64]
        for m in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ m] for l in range(64)]
        waves.append(lanes[0])
    want = 0.0
    for v in waves:
        want += v
    assert got == want
