"""The n-step recorder of include/crowdnav.h (cn_nstep_record_*) without a GPU: cn_nstep_member and cn_nstep_pending against their
ctypes mirrors as gcc lays them out, the seven exports with their prototypes, and every refusal that comes before any device work
(FAKE pointers are compared and never dereferenced; the refusals that need a live handle are in tests/test_gpu_nstep_record.py)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from learner_handle import lib

CN_ERR_ARG, CN_ERR_CONFIG = -1, -2
NAMES = ("cn_nstep_record_create", "cn_nstep_record_destroy", "cn_nstep_record_members", "cn_nstep_record_resetting",
         "cn_nstep_record_pending", "cn_nstep_record", "cn_nstep_discount")
FAKE = 0x1000
MEMBER_FIELDS = ["rec", "gamma", "reserved_f"]
PENDING_FIELDS = ["s", "a", "ret", "count", "clock", "n", "n_step", "obs_dim", "reserved"]


def test_structs_match_their_mirrors_field_by_field(tmp_path):
    _abi, _ = lib()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    mem, pend = _abi.CnNstepMember, _abi.CnNstepPending
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("member %zu\\n", sizeof(cn_nstep_member));', 'printf("pending %zu\\n", sizeof(cn_nstep_pending));',
             'printf("max %d\\n", CN_NSTEP_MAX);', 'printf("abi %d\\n", CN_ABI_VERSION);']
    for f in mem._fields_:
        lines.append('printf("member.%s %%zu\\n", offsetof(cn_nstep_member, %s));' % (f[0], f[0]))
    for f in pend._fields_:
        lines.append('printf("pending.%s %%zu\\n", offsetof(cn_nstep_pending, %s));' % (f[0], f[0]))
    lines += ["{ int (*f)(const cn_nstep_member*, int, int, int, int, cn_nstep_record_handle*) = cn_nstep_record_create; (void)f; }",
              "{ void (*f)(cn_nstep_record_handle) = cn_nstep_record_destroy; (void)f; }",
              "{ int (*f)(cn_nstep_record_handle) = cn_nstep_record_members; (void)f; }",
              "{ uint8_t* (*f)(cn_nstep_record_handle, int) = cn_nstep_record_resetting; (void)f; }",
              "{ int (*f)(cn_nstep_record_handle, int, cn_nstep_pending*) = cn_nstep_record_pending; (void)f; }",
              "{ int (*f)(cn_nstep_record_handle, float, void*) = cn_nstep_record; (void)f; }",
              "{ float (*f)(float, int) = cn_nstep_discount; (void)f; }",
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
    assert int(got["member"]) == C.sizeof(mem) == C.sizeof(_abi.CnPopRecordMember) + 8 == 184
    assert int(got["pending"]) == C.sizeof(pend) == 5 * 8 + 4 * 4 == 56
    for f in mem._fields_:
        assert int(got["member." + f[0]]) == getattr(mem, f[0]).offset, f[0]
    for f in pend._fields_:
        assert int(got["pending." + f[0]]) == getattr(pend, f[0]).offset, f[0]
    assert [f[0] for f in mem._fields_] == MEMBER_FIELDS and [f[0] for f in pend._fields_] == PENDING_FIELDS
    assert int(got["max"]) == _abi.CN_NSTEP_MAX == 16
    assert int(got["abi"]) == _abi.EXPECTED_ABI == 7              # additive: the version stays


def test_the_seven_names_are_exported_with_prototypes():
    _abi, L = lib()
    for name in NAMES:
        assert name in _abi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.cn_nstep_record_create.argtypes[0] is C.POINTER(_abi.CnNstepMember) and len(L.cn_nstep_record_create.argtypes) == 6
    assert L.cn_nstep_record.argtypes == [C.c_void_p, C.c_float, C.c_void_p]
    assert L.cn_nstep_record_pending.argtypes[2] is C.POINTER(_abi.CnNstepPending)
    assert L.cn_nstep_record_resetting.restype is C.c_void_p and L.cn_nstep_record_destroy.restype is None
    assert L.cn_nstep_discount.restype is C.c_float and L.cn_nstep_discount.argtypes == [C.c_float, C.c_int]


def _member(_abi, base, gamma=0.99, ring=None, **kw):
    """A valid explicit-array member whose eleven written pointers are distinct between bases 0x100 apart."""
    r = dict(s=base, a=base + 8, r=base + 16, s2=base + 24, d=base + 32, capacity=64, pos_dev=base + 40, size_dev=base + 48, obs_dim=398, reserved=0)
    r.update(ring or {})
    f = dict(env=None, counters=FAKE, last_return=FAKE, prev=base + 80, obs=FAKE, action=FAKE, reward=FAKE, done=FAKE,
             ring=_abi.CnReplayRing(**r), log=_abi.CnEpisodeLog(rows=base + 56, max_rows=100, n_dev=base + 64, tot_dev=base + 72), n=16, reserved=0)
    f.update(kw)
    return _abi.CnNstepMember(rec=_abi.CnPopRecordMember(**f), gamma=gamma, reserved_f=0.0)


def _create(L, members, n_members, n_step, obs_dim, want_rc, *texts, out="fresh"):
    h = C.c_void_p()
    rc = L.cn_nstep_record_create(members, n_members, n_step, obs_dim, 0, C.byref(h) if out == "fresh" else out)
    msg = L.cn_last_error().decode()
    assert rc == want_rc, (rc, msg)
    for t in texts:
        assert t in msg, (t, msg)
    assert "cn_nstep_record_create" in msg and not h.value


def test_create_refusals_come_before_any_device_work():
    _abi, L = lib()
    arr = lambda *ms: (_abi.CnNstepMember * len(ms))(*ms)
    A, B = 0x10000, 0x20000
    good = lambda base=A, **kw: _member(_abi, base, **kw)
    # the window
    for W in (0, -1, 17, 1 << 20):
        _create(L, arr(good()), 1, W, 398, CN_ERR_ARG, "n_step", "1 ... 16")
    # the discount, per member
    for g in (float("nan"), float("inf"), -float("inf"), 0.0, -0.99, 1.0000002, 5.0):
        _create(L, arr(good(), good(B, gamma=g)), 2, 3, 398, CN_ERR_ARG, "member 1", "gamma", "(0, 1]")
    # a call that ends every episode with full windows must fit the ring: n * n_step <= capacity
    _create(L, arr(good()), 1, 5, 398, CN_ERR_ARG, "member 0", "n * n_step", "80", "ring.capacity 64")
    _create(L, arr(good(), good(B, n=33)), 2, 2, 398, CN_ERR_ARG, "member 1", "n * n_step", "66")
    _create(L, arr(good(n=17, ring=dict(capacity=16))), 1, 1, 398, CN_ERR_ARG, "member 0", "n exceeds ring.capacity")      # W = 1: cn_pop_record_create's words
    # cn_pop_record_create's checks and words, under this entry point's name
    _create(L, None, 1, 3, 398, CN_ERR_ARG, "members")
    _create(L, arr(good()), 1, 3, 398, CN_ERR_ARG, "out", out=None)
    for n in (0, -1, 65):
        _create(L, arr(*[good()] * 65), n, 3, 398, CN_ERR_ARG, "n_members", "1 ... 64")
    _create(L, arr(good()), 1, 3, 0, CN_ERR_CONFIG, "obs_dim")
    _create(L, arr(good(), good(B, n=-1)), 2, 3, 398, CN_ERR_ARG, "member 1", "n is negative")
    for field in ("prev", "obs", "action", "reward", "done"):
        _create(L, arr(good(), good(B, **{field: None})), 2, 3, 398, CN_ERR_ARG, "member 1", field + " is null")
    _create(L, arr(good(counters=None)), 1, 3, 398, CN_ERR_ARG, "member 0", "env", "counters", "last_return")
    _create(L, arr(good(ring=dict(s2=None))), 1, 3, 398, CN_ERR_ARG, "member 0", "incomplete ring")
    _create(L, arr(good(ring=dict(obs_dim=397))), 1, 3, 398, CN_ERR_CONFIG, "member 0", "ring.obs_dim")
    _create(L, arr(good(), good()), 2, 3, 398, CN_ERR_CONFIG, "member 1", "member 0", "race")
    # an accepted window with n * W == capacity exactly would go on to the device: not tried here


def test_null_handles_are_refused_everywhere():
    _abi, L = lib()
    assert L.cn_nstep_record(None, 1.0, None) == CN_ERR_ARG and b"cn_nstep_record: null handle" in L.cn_last_error()
    assert L.cn_nstep_record_resetting(None, 0) is None and b"cn_nstep_record_resetting: null handle" in L.cn_last_error()
    pd = _abi.CnNstepPending()
    assert L.cn_nstep_record_pending(None, 0, C.byref(pd)) == CN_ERR_ARG and b"cn_nstep_record_pending: null handle" in L.cn_last_error()
    assert L.cn_nstep_record_members(None) == 0
    L.cn_nstep_record_destroy(None)                                # a no-op, as free(NULL)
