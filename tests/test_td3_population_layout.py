"""The population calls of include/crowdnav.h (cn_td3_pop_*) against their ctypes prototypes in crowdnav/_abi.py: gcc compiles the
header with each function assigned to a pointer of the signature the issue of record gives it, and the header's parameter lists, parsed
from its text, are matched kind by kind (pointer / int, return type) with the argtypes and restype the binding sets."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SIGNATURES = {      # name: (return type, parameter types) as the header declares them
    "cn_td3_pop_create": ("int", ["const cn_td3_config*", "int", "int", "cn_td3_pop_handle*"]),
    "cn_td3_pop_destroy": ("void", ["cn_td3_pop_handle"]),
    "cn_td3_pop_update": ("int", ["cn_td3_pop_handle", "int", "void*"]),
    "cn_td3_pop_members": ("int", ["cn_td3_pop_handle"]),
    "cn_td3_pop_loss_dev": ("const float*", ["cn_td3_pop_handle"]),
    "cn_td3_pop_batch_dev": ("const float*", ["cn_td3_pop_handle", "int", "int"]),
    "cn_td3_pop_set_replay_sample": ("int", ["cn_td3_pop_handle", "int"]),
}


def _kind(ctype):
    """pointer | int, of a C type spelled in the header"""
    return "pointer" if ("*" in ctype or ctype.endswith("_handle")) else "int"


def test_header_declares_the_population_calls_with_these_signatures(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['#include "crowdnav.h"', "int main(void) {"]
    for name, (ret, params) in SIGNATURES.items():
        lines.append("  { %s (*f)(%s) = %s; (void)f; }" % (ret, ", ".join(params), name))
    lines.append("  return sizeof(cn_td3_config) == %d ? 0 : 1; }" % C.sizeof(__import__("crowdnav")._abi.CnTd3Config))
    src = tmp_path / "protos.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"), "-o",
                    str(tmp_path / "protos.o"), str(src)], check=True)


def test_ctypes_prototypes_match_the_header_parameter_by_parameter():
    from crowdnav import _abi
    hdr = open(os.path.join(ROOT, "include", "crowdnav.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _abi.lib()
    n = 0
    for name, (ret, params) in SIGNATURES.items():
        m = re.search(r"([A-Za-z_ ]+?[\s\*]+)%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "%s is not declared" % name
        got_ret = re.sub(r"\s+", " ", m.group(1)).strip().replace(" *", "*")
        got = [re.sub(r"\s+", " ", p).strip() for p in m.group(2).split(",")]
        got_types = [re.sub(r"\s*\b[a-z_0-9]+$", "", p).replace(" *", "*") for p in got]      # drop the parameter's name
        assert got_ret == ret and got_types == params, (name, got_ret, got_types)
        assert name in _abi.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for at, ct in zip(fn.argtypes, params):
            is_ptr = at is C.c_void_p or hasattr(at, "contents") or issubclass(at, C._Pointer)
            assert ("pointer" if is_ptr else "int") == _kind(ct), (name, at, ct)
            if not is_ptr:
                assert at is C.c_int, (name, at)
            n += 1
        if ret == "void":
            assert fn.restype is None, name
        elif ret == "int":
            assert fn.restype is C.c_int, name
        else:
            assert fn.restype is C.c_void_p, name
    assert n == 4 + 1 + 3 + 1 + 1 + 3 + 2
    assert L.cn_td3_pop_create.argtypes[0] is C.POINTER(_abi.CnTd3Config)      # an array of the struct the solo call takes one of
    assert L.cn_abi_version() == _abi.EXPECTED_ABI == 7                        # additive: the version stays
    assert _abi.CN_TD3_POP_MAX == 64
