"""The population-actor calls of include/crowdnav.h (cn_actor_pop_*) without a GPU: cn_actor_pop_member against its ctypes mirror as
gcc lays it out, the six exports, every refusal that can be reached without a handle (the argument checks come before any device
work, so they answer on a machine that has no GPU; the two that need a live handle -- NULL counters, a member out of range -- are in
tests/test_gpu_actor_population.py), crowdnav.train's --population-act switch, and the NumPy restatement of the pack
(tests/actor_pop_ref.py) against the header's index formula."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import actor_pop_ref as R
from conftest import ROOT
from learner_handle import lib

CN_ERR_ARG, CN_ERR_CONFIG = -1, -2
NAMES = ("cn_actor_pop_create", "cn_actor_pop_destroy", "cn_actor_pop_members", "cn_actor_pop_pack", "cn_actor_pop_forward",
         "cn_actor_pop_weights")
FAKE = 0x1000        # a non-null "device pointer": the checks compare with NULL and never dereference


def test_member_struct_matches_its_mirror_field_by_field(tmp_path):
    _abi, _ = lib()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _abi.CnActorPopMember
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(cn_actor_pop_member));', 'printf("max %d\\n", CN_ACTOR_POP_MAX);',
             'printf("abi %d\\n", CN_ABI_VERSION);']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(cn_actor_pop_member, %s));' % (f[0], f[0]))
    # the prototypes, as the header must declare them
    lines += ["{ int (*f)(const cn_actor_pop_member*, int, int, int, cn_actor_pop_handle*) = cn_actor_pop_create; (void)f; }",
              "{ void (*f)(cn_actor_pop_handle) = cn_actor_pop_destroy; (void)f; }",
              "{ int (*f)(cn_actor_pop_handle) = cn_actor_pop_members; (void)f; }",
              "{ int (*f)(cn_actor_pop_handle, void*) = cn_actor_pop_pack; (void)f; }",
              "{ int (*f)(cn_actor_pop_handle, const uint64_t*, int, void*) = cn_actor_pop_forward; (void)f; }",
              "{ int (*f)(cn_actor_pop_handle, int, cn_actor_weights*) = cn_actor_pop_weights; (void)f; }",
              "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    obj = tmp_path / "layout.o"
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"),
                    "-o", str(obj), str(src)], check=True)
    # link against nothing: the function addresses are only taken, so resolve them with stubs of the same names
    stubs = tmp_path / "stubs.c"
    stubs.write_text("\n".join("void %s(void) {}" % n for n in NAMES))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(obj), str(stubs)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls) == 96
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]
    assert [f[0] for f in cls._fields_] == ["actor", "obs", "action", "n", "reserved", "max_v", "max_w", "sigma", "reserved_f", "seed"]
    assert int(got["max"]) == _abi.CN_ACTOR_POP_MAX == 64
    assert int(got["abi"]) == _abi.EXPECTED_ABI == 7              # additive: the version stays


def test_the_six_names_are_exported_with_prototypes():
    _abi, L = lib()
    for name in NAMES:
        assert name in _abi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.cn_actor_pop_create.argtypes[0] is C.POINTER(_abi.CnActorPopMember)
    assert L.cn_actor_pop_forward.argtypes[1] is C.POINTER(C.c_uint64)
    assert L.cn_actor_pop_weights.argtypes[2] is C.POINTER(_abi.CnActorWeights)
    assert L.cn_actor_pop_destroy.restype is None


def _member(_abi, **kw):
    f = dict(actor=_abi.CnTd3Mlp(*[FAKE] * 6), obs=FAKE, action=FAKE, n=16, reserved=0, max_v=0.22, max_w=2.0, sigma=1.0,
             reserved_f=0.0, seed=1)
    null_actor = kw.pop("null_actor", None)
    f.update(kw)
    m = _abi.CnActorPopMember(**f)
    if null_actor:
        setattr(m.actor, null_actor, None)
    return m


def _create(L, members, n_members, obs_dim, want_rc, *texts, out="fresh"):
    h = C.c_void_p()
    rc = L.cn_actor_pop_create(members, n_members, obs_dim, 0, C.byref(h) if out == "fresh" else out)
    msg = L.cn_last_error().decode()
    assert rc == want_rc, (rc, msg)
    for t in texts:
        assert t in msg, (t, msg)
    assert "cn_actor_pop_create" in msg
    assert not h.value                       # *out stays NULL


def test_create_refusals_name_the_field_and_the_member():
    _abi, L = lib()
    arr = lambda *ms: (_abi.CnActorPopMember * len(ms))(*ms)
    good = _member(_abi)
    _create(L, None, 1, 398, CN_ERR_ARG, "members")
    _create(L, arr(good), 1, 398, CN_ERR_ARG, "out", out=None)
    big = arr(*[good] * 65)
    for n in (0, -1, 65, 1 << 20):
        _create(L, big, n, 398, CN_ERR_ARG, "n_members", "1 ... 64")
    for field in ("w1", "b1", "w2", "b2", "w3", "b3"):
        _create(L, arr(good, _member(_abi, null_actor=field), good), 3, 398, CN_ERR_ARG, "member 1", "actor." + field)
        _create(L, arr(_member(_abi, null_actor=field)), 1, 398, CN_ERR_ARG, "member 0", "actor." + field)
    _create(L, arr(good, good, _member(_abi, obs=None)), 3, 398, CN_ERR_ARG, "member 2", "obs")
    _create(L, arr(good, _member(_abi, action=None)), 2, 398, CN_ERR_ARG, "member 1", "action")
    _create(L, arr(_member(_abi, n=-1), good), 2, 398, CN_ERR_ARG, "member 0", "n is negative")
    _create(L, arr(good, _member(_abi, n=-(1 << 31))), 2, 398, CN_ERR_ARG, "member 1", "n is negative")
    for D in (0, -1, -398):
        _create(L, arr(good), 1, D, CN_ERR_CONFIG, "obs_dim")
    for D in (2273, 2304, 4000, (1 << 31) - 1):          # Dp 2304 is the first tile above 160 KiB, as cn_actor_forward refuses
        _create(L, arr(good), 1, D, CN_ERR_CONFIG, "obs_dim", "too wide")
    # the first failing check wins in member order
    _create(L, arr(_member(_abi, n=-1), _member(_abi, obs=None)), 2, 398, CN_ERR_ARG, "member 0")


def test_null_handles_are_refused_everywhere():
    _abi, L = lib()
    counters = (C.c_uint64 * 64)()
    w = _abi.CnActorWeights()
    assert L.cn_actor_pop_pack(None, None) == CN_ERR_ARG and b"cn_actor_pop_pack: null handle" in L.cn_last_error()
    assert L.cn_actor_pop_forward(None, counters, 1, None) == CN_ERR_ARG and b"cn_actor_pop_forward: null handle" in L.cn_last_error()
    assert L.cn_actor_pop_forward(None, None, 1, None) == CN_ERR_ARG
    assert L.cn_actor_pop_weights(None, 0, C.byref(w)) == CN_ERR_ARG and b"cn_actor_pop_weights: null handle" in L.cn_last_error()
    assert not w.w1p and not w.w2p and w.hidden == 0            # untouched
    assert L.cn_actor_pop_members(None) == 0
    L.cn_actor_pop_destroy(None)                                # a no-op, as free(NULL)


def test_population_act_switch():
    from crowdnav import train
    base = ["--algo", "td3", "--learner", "fused"]
    assert train.parse_args(base + ["--population", "2"]).population_act == "one-launch"          # the default
    for v in ("one-launch", "per-member"):
        a = train.parse_args(base + ["--population", "2", "--population-act", v])
        assert a.population_act == v and a.population == 2


@pytest.mark.parametrize("argv,text", [
    (["--population-act", "per-member"], "--population"),                                     # not without a population
    (["--algo", "td3", "--learner", "fused", "--population-act", "one-launch"], "--population"),
    (["--algo", "td3", "--learner", "fused", "--population", "2", "--population-act", "both"], "invalid choice"),
])
def test_population_act_refusals(argv, text, capsys):
    from crowdnav import train
    with pytest.raises(SystemExit) as ex:
        train.parse_args(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "--population-act" in err and text in err, err


@pytest.mark.parametrize("k_in", (1, 31, 32, 33, 398))
def test_pack_from_linear_is_the_header_formula_on_the_transposed_padded_matrix(k_in):
    """pack_from_linear (what cn_actor_pop_pack is stated to write) == the header's formula on W^T zero-padded to Dp rows, and the
    header's formula itself is checked against its definition written as nested loops.  The two wrong variants differ wherever they
    can: 'no zero rows' at every width that has padding rows (not 32), 'k and c swapped' at every width above 1 (a [256][1] matrix and
    its transpose are the same bytes)."""
    rng = np.random.default_rng(k_in)
    W = rng.standard_normal((256, k_in)).astype(np.float32)
    W[W == 0] = 1.0                                  # a zero weight could hide a missing zero row
    Dp = R.padded(k_in)
    assert Dp % 32 == 0 and 0 <= Dp - k_in < 32
    wt = R.transposed_padded(W)
    assert wt.shape == (Dp, 256) and np.array_equal(wt[:k_in], W.T) and not wt[k_in:].any()
    want = R.pack_kmajor(wt)
    loops = np.empty(Dp * 256, dtype=np.float32)     # the header's sentence, index by index
    for b in range(Dp // 32):
        for w in range(8):
            for q in range(4):
                for lane in range(64):
                    for j in range(4):
                        loops[((((b * 8 + w) * 4 + q) * 64 + lane) * 4 + j)] = wt[32 * b + 4 * (2 * q + (j >> 1)) + (lane >> 4),
                                                                                  32 * w + 2 * (lane & 15) + (j & 1)]
    assert np.array_equal(want, loops)
    got = R.pack_from_linear(W)
    assert got.dtype == np.float32 and got.shape == (Dp * 256,)
    assert np.array_equal(got, want)
    assert sorted(got[got != 0].tolist()) == sorted(W.reshape(-1).tolist())          # a permutation of W plus zeros
    assert int((got == 0).sum()) == (Dp - k_in) * 256
    no_zero, swapped = R.pack_from_linear_no_zero_rows(W), R.pack_from_linear_swapped(W)
    assert np.array_equal(no_zero, want) == (k_in == 32)
    assert np.array_equal(swapped, want) == (k_in == 1)
