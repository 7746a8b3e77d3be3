"""The learner state blob's part of include/crowdnav.h (cn_state_header, cn_state_segment, cn_td3_state_*, cn_td3_pop_state_*)
without a GPU: the two structs against their ctypes mirrors as gcc lays them out, the prototypes, the exports, the NumPy
restatement's directory (tests/state_ref.py) against the header's rules and the size formula, and the refusals that need no handle
(those that need one: tests/test_gpu_learner_state.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import state_ref
from conftest import ROOT
from learner_handle import lib

CN_ERR_ARG = -1
NAMES = ("cn_td3_state_size", "cn_td3_state_save", "cn_td3_state_load", "cn_td3_state_segment_dev",
         "cn_td3_pop_state_size", "cn_td3_pop_state_save", "cn_td3_pop_state_load", "cn_td3_pop_state_segment_dev")
STRUCTS = (("cn_state_header", "CnStateHeader", list(state_ref.HEADER_FIELDS), 48),
           ("cn_state_segment", "CnStateSegment", ["member", "kind", "index", "reserved", "offset", "bytes"], 32))
SHAPES = [(P, D, H, pbt, pop) for (D, H) in ((1, 1), (3, 5), (17, 33), (398, 256)) for (P, pbt, pop) in
          ((1, False, False), (1, False, True), (2, True, True), (3, True, True), (8, False, True), (8, True, True), (64, True, True))]


def test_structs_match_their_mirrors_field_by_field(tmp_path):
    _abi, _ = lib()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("abi %d\\n", CN_ABI_VERSION);', 'printf("magic %llu\\n", (unsigned long long)CN_STATE_MAGIC);',
             'printf("version %d\\n", CN_STATE_VERSION);', 'printf("family %d\\n", CN_STATE_FAMILY_TD3);',
             'printf("kinds %d %d %d %d %d %d %d %d %d %d %d\\n", CN_STATE_PARAM, CN_STATE_MOMENT, CN_STATE_ADAM, CN_STATE_STEPS, CN_STATE_PW, '
             'CN_STATE_COUNTER, CN_STATE_LOSS, CN_STATE_HYPER, CN_STATE_PBT, CN_STATE_PBT_LAST, CN_STATE_KINDS);',
             'printf("pbt_state %zu\\n", sizeof(cn_td3_pbt_state));']
    for cname, pyname, _, _ in STRUCTS:
        lines.append('printf("%s.sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in getattr(_abi, pyname)._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f[0], cname, f[0], cname, f[0]))
    lines += ["{ size_t (*f)(cn_td3_handle) = cn_td3_state_size; (void)f; }",
              "{ int (*f)(cn_td3_handle, void*, size_t, void*) = cn_td3_state_save; (void)f; }",
              "{ int (*f)(cn_td3_handle, const void*, size_t, void*) = cn_td3_state_load; (void)f; }",
              "{ const void* (*f)(cn_td3_handle, int, cn_state_segment*) = cn_td3_state_segment_dev; (void)f; }",
              "{ size_t (*f)(cn_td3_pop_handle) = cn_td3_pop_state_size; (void)f; }",
              "{ int (*f)(cn_td3_pop_handle, void*, size_t, void*) = cn_td3_pop_state_save; (void)f; }",
              "{ int (*f)(cn_td3_pop_handle, const void*, size_t, void*) = cn_td3_pop_state_load; (void)f; }",
              "{ const void* (*f)(cn_td3_pop_handle, int, cn_state_segment*) = cn_td3_pop_state_segment_dev; (void)f; }",
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
    got = {ln.split()[0]: ln.split()[1:] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    for cname, pyname, fields, size in STRUCTS:
        cls = getattr(_abi, pyname)
        assert int(got[cname + ".sizeof"][0]) == C.sizeof(cls) == size, cname
        assert [f[0] for f in cls._fields_] == fields, cname
        for f in cls._fields_:
            off, sz = map(int, got["%s.%s" % (cname, f[0])])
            assert off == getattr(cls, f[0]).offset and sz == getattr(cls, f[0]).size, (cname, f[0])
    assert int(got["abi"][0]) == _abi.EXPECTED_ABI == 7          # additive: the version stays
    assert int(got["magic"][0]) == _abi.CN_STATE_MAGIC == state_ref.MAGIC == int.from_bytes(b"CNSTATE\0", "little")
    assert int(got["version"][0]) == _abi.CN_STATE_VERSION == state_ref.VERSION == 1
    assert int(got["family"][0]) == _abi.CN_STATE_FAMILY_TD3 == state_ref.FAMILY_TD3
    assert got["kinds"] == [str(k) for k in range(11)] and len(_abi.CN_STATE_KIND_NAMES) == 10
    assert [state_ref.PARAM, state_ref.MOMENT, state_ref.ADAM, state_ref.STEPS, state_ref.PW, state_ref.COUNTER, state_ref.LOSS,
            state_ref.HYPER, state_ref.PBT, state_ref.PBT_LAST] == list(range(10))
    assert int(got["pbt_state"][0]) == state_ref.PBT_STATE_BYTES == C.sizeof(_abi.CnTd3PbtState)
    # the restatement's own structs are the same bytes
    assert state_ref.HEADER.size == 48 and state_ref.SEGMENT.size == 32
    hdr = _abi.CnStateHeader.from_buffer_copy(state_ref.HEADER.pack(1, 2, 3, 4, 5, 6, 7, 8, 9, 10))
    assert [getattr(hdr, f) for f in state_ref.HEADER_FIELDS] == list(range(1, 11))
    seg = _abi.CnStateSegment.from_buffer_copy(state_ref.SEGMENT.pack(-1, 2, 3, 0, 5, 6))
    assert (seg.member, seg.kind, seg.index, seg.reserved, seg.offset, seg.bytes) == (-1, 2, 3, 0, 5, 6)


@pytest.mark.parametrize("P,D,H,pbt,pop", SHAPES)
def test_the_restated_directory_keeps_the_headers_rules(P, D, H, pbt, pop):
    header, rows, total = state_ref.directory(P, D, H, 7, pbt, pop)
    assert header["n_segments"] == len(rows) == P * (77 + (1 if pop else 0)) + (2 if pbt else 0)
    at = state_ref.HEADER.size + state_ref.SEGMENT.size * len(rows)
    assert at % 16 == 0
    for m, k, i, off, nb in rows:
        assert off % 16 == 0 and off == at and nb > 0 and nb % 4 == 0, (m, k, i)      # ascending, no overlap, no gap but the padding
        at = off + state_ref.round16(nb)
    assert at == total == header["total_bytes"] == state_ref.total_bytes(P, D, H, pbt, pop)
    # per member, in PbtTensor's order: 36 parameters, 36 moments, adam, steps, pw, then the counter and the loss
    per = 77 + (1 if pop else 0)
    for p in range(P):
        mine = rows[p * per:(p + 1) * per]
        assert all(r[0] == p for r in mine)
        assert [(r[1], r[2]) for r in mine[:72]] == [(state_ref.PARAM, i) for i in range(36)] + [(state_ref.MOMENT, i) for i in range(36)]
        assert [(r[1], r[4]) for r in mine[72:77]] == [(state_ref.ADAM, 16), (state_ref.STEPS, 8), (state_ref.PW, 32), (state_ref.COUNTER, 8), (state_ref.LOSS, 4)]
        assert [r[4] for r in mine[:6]] == [4 * H * D, 4 * H, 4 * H * H, 4 * H, 8 * H, 8]                  # the actor
        assert [r[4] for r in mine[12:18]] == [4 * H * (D + 2), 4 * H, 4 * H * H, 4 * H, 4 * H, 4]         # the first critic
        assert [r[4] for r in mine[36:40]] == [4 * H * D, 4 * H * D, 4 * H, 4 * H]                          # the actor's (m, v) pairs
        if pop:
            assert mine[77][1:3] == (state_ref.HYPER, 0) and mine[77][4] == 20
    if pbt:
        assert [(r[0], r[1], r[4]) for r in rows[-2:]] == [(-1, state_ref.PBT, state_ref.PBT_STATE_BYTES), (-1, state_ref.PBT_LAST, 16 * P)]


def test_a_member_is_about_two_million_words():
    total = state_ref.total_bytes(1, 398, 256, False, False)
    assert 7.9e6 < total < 8.2e6          # about 2.0 M words, 8 MB, at 398 inputs and hidden 256


def test_pack_and_unpack_agree_and_the_padding_is_zero():
    P, D, H, B = 2, 3, 5, 2
    header, rows, total = state_ref.directory(P, D, H, B, True, True)
    rng = np.random.default_rng(0)
    tensors = [rng.integers(1, 256, nb, dtype=np.uint8) for (_, _, _, _, nb) in rows]
    blob = state_ref.pack(P, D, H, B, tensors, True, True)
    assert blob.size == total
    h2, r2 = state_ref.unpack(blob)
    assert h2 == header and r2 == rows
    covered = np.zeros(total, dtype=bool)
    covered[:state_ref.HEADER.size + state_ref.SEGMENT.size * len(rows)] = True
    for (_, _, _, off, nb), t in zip(rows, tensors):
        assert (blob[off:off + nb] == t).all()
        covered[off:off + nb] = True
    assert not blob[~covered].any() and (~covered).sum() == sum(state_ref.round16(r[4]) - r[4] for r in rows)


def test_the_names_are_exported_with_prototypes():
    _abi, L = lib()
    for name in NAMES:
        assert name in _abi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    for pre in ("cn_td3_state_", "cn_td3_pop_state_"):
        assert getattr(L, pre + "size").argtypes == [C.c_void_p] and getattr(L, pre + "size").restype is C.c_size_t
        assert getattr(L, pre + "save").argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p] and getattr(L, pre + "save").restype is C.c_int
        assert getattr(L, pre + "load").argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p] and getattr(L, pre + "load").restype is C.c_int
        assert getattr(L, pre + "segment_dev").argtypes == [C.c_void_p, C.c_int, C.POINTER(_abi.CnStateSegment)]


def test_null_handles_and_blobs_are_refused_before_any_device_work():
    _abi, L = lib()
    err = lambda: L.cn_td3_last_error().decode()
    for pre in ("cn_td3_state_", "cn_td3_pop_state_"):
        assert getattr(L, pre + "size")(None) == 0 and pre + "size: null handle" in err()
        assert getattr(L, pre + "save")(None, 0x1000, 16, None) == CN_ERR_ARG and pre + "save: null handle" in err()      # never dereferenced
        assert getattr(L, pre + "load")(None, 0x1000, 16, None) == CN_ERR_ARG and pre + "load: null handle" in err()
        assert getattr(L, pre + "save")(None, None, 0, None) == CN_ERR_ARG
        assert getattr(L, pre + "segment_dev")(None, 0, None) is None


def test_the_header_states_the_blob():
    text = open(os.path.join(ROOT, "include", "crowdnav.h")).read()
    for phrase in ("Blob = cn_state_header | cn_state_segment directory[n_segments] | payload", "multiple of 16", "are ZERO",
                   "ONE launch, enqueue-only, no host read, capturable", "BIT FOR BIT", "to every place the update reads it",
                   "Refused, nothing written"):
        assert phrase in text, phrase
