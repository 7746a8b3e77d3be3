"""Population-based training's part of include/crowdnav.h (cn_td3_pop_pbt_bind, cn_td3_pop_exploit, cn_td3_pop_pbt_state_dev) without
a GPU: the three structs against their ctypes mirrors as gcc lays them out, field by field; the prototypes parameter by parameter; the
exports; and the refusals that can be reached without a handle (those that need a live handle: tests/test_gpu_td3_pbt.py)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from learner_handle import lib

CN_ERR_ARG = -1
NAMES = ("cn_td3_pop_pbt_bind", "cn_td3_pop_exploit", "cn_td3_pop_pbt_state_dev")
STRUCTS = (("cn_td3_pbt_config", "CnTd3PbtConfig", ["n_replace", "min_episodes", "explore_mask", "reserved", "factor", "lo", "hi", "seed"], 72),
           ("cn_td3_pbt_member", "CnTd3PbtMember", ["src", "generation", "fitness", "hyper"], 32),
           ("cn_td3_pbt_state", "CnTd3PbtState", ["calls", "applied", "member"], 16 + 64 * 32))


def test_structs_match_their_mirrors_field_by_field(tmp_path):
    _abi, _ = lib()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("hypers %d\\n", CN_PBT_HYPERS);', 'printf("abi %d\\n", CN_ABI_VERSION);',
             'printf("order %d %d %d %d %d\\n", CN_PBT_LR_ACTOR, CN_PBT_LR_CRITIC, CN_PBT_GAMMA, CN_PBT_NOISE_STD, CN_PBT_NOISE_CLIP);']
    for cname, pyname, _, _ in STRUCTS:
        lines.append('printf("%s.sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in getattr(_abi, pyname)._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f[0], cname, f[0], cname, f[0]))
    lines += ["{ int (*f)(cn_td3_pop_handle, const cn_td3_pbt_config*, const cn_episode_log*) = cn_td3_pop_pbt_bind; (void)f; }",
              "{ int (*f)(cn_td3_pop_handle, const float*, void*) = cn_td3_pop_exploit; (void)f; }",
              "{ const cn_td3_pbt_state* (*f)(cn_td3_pop_handle) = cn_td3_pop_pbt_state_dev; (void)f; }",
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
    assert int(got["hypers"][0]) == _abi.CN_PBT_HYPERS == 5
    assert got["order"] == ["0", "1", "2", "3", "4"] and _abi.CN_PBT_HYPER_NAMES == ("lr_actor", "lr_critic", "gamma", "noise_std", "noise_clip")
    assert int(got["abi"][0]) == _abi.EXPECTED_ABI == 7          # additive: the version stays
    assert _abi.CnTd3PbtState.member.size == _abi.CN_TD3_POP_MAX * C.sizeof(_abi.CnTd3PbtMember)


def test_the_three_names_are_exported_with_prototypes():
    _abi, L = lib()
    for name in NAMES:
        assert name in _abi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.cn_td3_pop_pbt_bind.argtypes == [C.c_void_p, C.POINTER(_abi.CnTd3PbtConfig), C.POINTER(_abi.CnEpisodeLog)]
    assert L.cn_td3_pop_pbt_bind.restype is C.c_int
    assert L.cn_td3_pop_exploit.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p] and L.cn_td3_pop_exploit.restype is C.c_int
    assert L.cn_td3_pop_pbt_state_dev.argtypes == [C.c_void_p] and L.cn_td3_pop_pbt_state_dev.restype is C.c_void_p


def test_null_handles_are_refused_before_any_device_work():
    _abi, L = lib()
    cfg = _abi.CnTd3PbtConfig(n_replace=1, min_episodes=1, explore_mask=0, reserved=0, factor=(0.8, 1.2), lo=(0,) * 5, hi=(1,) * 5, seed=0)
    err = lambda: L.cn_td3_last_error().decode()
    assert L.cn_td3_pop_pbt_bind(None, C.byref(cfg), None) == CN_ERR_ARG and "cn_td3_pop_pbt_bind: null handle" in err()
    assert L.cn_td3_pop_pbt_bind(None, None, None) == CN_ERR_ARG and "cn_td3_pop_pbt_bind" in err()
    assert L.cn_td3_pop_exploit(None, None, None) == CN_ERR_ARG and "cn_td3_pop_exploit: null handle" in err()
    assert L.cn_td3_pop_exploit(None, 0x1000, None) == CN_ERR_ARG and "null handle" in err()      # the pointer is never dereferenced
    assert L.cn_td3_pop_pbt_state_dev(None) is None


def test_the_header_states_the_exploit_call():
    text = open(os.path.join(ROOT, "include", "crowdnav.h")).read()
    for phrase in ("cn_td3_pop_exploit(h, fitness_dev, stream): at most TWO launches, enqueue-only", "SKIPPED", "BIT FOR BIT",
                   "mix64(K ^ (k + 1)) % n", "CN_ERR_CONFIG: a member whose hyper-parameter starts outside [lo, hi]"):
        assert phrase in text, phrase
