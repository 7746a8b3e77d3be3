"""The tabular learners' structs as gcc lays out include/crowdnav.h against their ctypes mirrors: sizeof and every field offset."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_tabular_mirrors_match_the_header_field_by_field(tmp_path):
    from crowdnav import _abi
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    pairs = [("cn_tab_config", _abi.CnTabConfig), ("cn_tab_io", _abi.CnTabIO)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("states actions %d\\n", CN_TAB_STATES * 10 + CN_TAB_ACTIONS);', 'printf("algos x %d\\n", CN_TAB_QLEARN * 10 + CN_TAB_SARSA);']
    for cname, cls in pairs:
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        a, b, c = ln.split()
        got[(a, b)] = int(c)
    assert got[("states", "actions")] == _abi.CN_TAB_STATES * 10 + _abi.CN_TAB_ACTIONS == 9773
    assert got[("algos", "x")] == _abi.CN_TAB_QLEARN * 10 + _abi.CN_TAB_SARSA == 1
    n = 0
    for cname, cls in pairs:
        assert got[(cname, "sizeof")] == C.sizeof(cls), cname
        for f in cls._fields_:
            assert got[(cname, f[0])] == getattr(cls, f[0]).offset, (cname, f[0])
            n += 1
    assert n == 5 + 23
    assert C.sizeof(_abi.CnTabConfig) == 32 and C.sizeof(_abi.CnTabIO) == 168
