"""csrc/crowdnav_variants.h without a GPU: the header is plain C++, so a stand-alone program compiled with g++ walks its pure
selection function -- every world x the five forms, and for the three plain tracker worlds the launch facts that decide between
the fair forms and the 360-ray shape's geometries -- and prints the names, their compile units and the table's size.  Held to the
selection written out as data in tests/kernel_table_ref.py."""
import itertools
import os
import shutil
import subprocess

import pytest

import kernel_table_ref as T
from conftest import PKG

FORMS = [("step", "CN_FORM_STEP"), ("same", "CN_FORM_SAME"), ("external", "CN_FORM_EXTERNAL"), ("sequence", "CN_FORM_SEQUENCE"),
         ("policy", "CN_FORM_POLICY")]
# two launches that differ in everything a launch can differ in: a world outside the plain tracker rows must not notice
QUIET = (T.ARB_AUTO, 0, 256, 1, 0, -1, 4)          # arbitration, overlapped, n_cus, n_envs, group_envs, CN_X2, wpb
LOUD = (T.ARB_FAIR, 0, 256, 4097, 0, 1, 4)
GRID = [(arb, ov, ncu, n, grp, x2, wpb)
        for arb in (T.ARB_AUTO, T.ARB_OLDEST_FIRST, T.ARB_FAIR) for ov in (0, 1)
        for ncu, res in [(256, r) for r in (1, 2048, 2049, 4096, 4097)] + [(0, 1), (0, 4097)]
        for n, grp in ((res, 0), (1, res))                # resident = max(n_envs, group_envs): alone, or one of a group
        for x2 in (-1, 0, 1) for wpb in (0, 4)]

PROGRAM = r"""
#include <stdio.h>
#include "crowdnav_variants.h"
static const char* name_of(int id) { return id < 0 ? "NULL" : cn_kernel_info[id].name; }
int main()
{
    printf("counts %d %d %d\n", (int)CN_K_N_DYNAMIC, (int)(CN_K_COUNT - CN_K_N_DYNAMIC), (int)CN_W_COUNT);
    for (int id = 0; id < CN_K_COUNT; ++id) printf("kernel %s %d\n", cn_kernel_info[id].name, cn_kernel_info[id].tu);
@QUERIES@
    return 0;
}
"""


def query_lines(w, launches_of):
    """the program lines that ask cn_select_kernel about world `w`: launches_of(form) = the launch facts to ask each form with"""
    lines = ["    { const int w = cn_world_index(%s);" % ", ".join(str(f) for f in T.WORLDS[w][0])]
    for form, cform in FORMS:
        for L in launches_of(form):
            lines.append('      { const CnLaunchFacts f = {%d, %s, %d, %d, %d, %d, %d}; printf("select %s %s %s %%s\\n", name_of(cn_select_kernel(w, %s, f))); }'
                         % (L[0], "true" if L[1] else "false", L[2], L[3], L[4], L[5], L[6], w, form, "/".join(map(str, L)), cform))
    return lines + ["    }"]


def walk(tmp, lines):
    """Compile PROGRAM with `lines` as its queries (g++, the header alone) and run it: {(world, form, launch facts): kernel name},
    "kernels": [(name, compile unit)], "counts": the table's sizes."""
    src, exe = tmp / "walk.cpp", tmp / "walk"
    src.write_text(PROGRAM.replace("@QUERIES@", "\n".join(lines)))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), "-o", str(exe), str(src)], check=True)
    out = {"kernels": []}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        f = ln.split()
        if f[0] == "counts":
            out["counts"] = tuple(int(x) for x in f[1:])
        elif f[0] == "kernel":
            out["kernels"].append((f[1], int(f[2])))
        else:
            out[(f[1], f[2], tuple(int(x) for x in f[3].split("/")))] = None if f[4] == "NULL" else f[4]
    return out


@pytest.fixture(scope="module")
def selection(tmp_path_factory):
    """{query: kernel name}, ("kernel", name): compile unit, "counts": the table's sizes -- one compile, one run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    lines = []
    for w in T.WORLDS:
        launches = [QUIET, LOUD] + (GRID if w in T.PLAIN_TRACKER else [])
        lines += query_lines(w, lambda form: launches if form == "step" else launches[:2])
    return walk(tmp_path_factory.mktemp("kernel_table"), lines)


def test_every_world_and_form_selects_the_tables_kernel(selection):
    for w, (_, step, same, ext, seq, pol) in T.WORLDS.items():
        for L in (QUIET, LOUD):
            assert selection[(w, "same", L)] == same and selection[(w, "external", L)] == ext, (w, L)
            assert selection[(w, "sequence", L)] == seq and selection[(w, "policy", L)] == pol, (w, L)
            assert selection[(w, "step", L)] == T.want_step(w, *L), (w, L)
            if w not in T.PLAIN_TRACKER:
                assert selection[(w, "step", L)] == step, (w, L)
    assert sum(1 for row in T.WORLDS.values() if row[3] is None) == 5          # the gt worlds: no external kernel


def test_plain_tracker_step_kernel_follows_the_launch_facts(selection):
    seen = set()
    for w, L in itertools.product(T.PLAIN_TRACKER, GRID):
        assert selection[(w, "step", L)] == T.want_step(w, *L), (w, L)
        seen.add(selection[(w, "step", L)])
    assert seen == set(T.HEADLINE_ONLY) | {T.WORLDS[w][1] for w in T.PLAIN_TRACKER}      # every form of the three rows is reached
    # the thresholds, spelled out: 256 CUs, arbitration auto, one handle alone
    at = lambda n, x2=-1, wpb=4, w="s360": selection[(w, "step", (T.ARB_AUTO, 0, 256, n, 0, x2, wpb))]
    assert at(2048) == "cn_env_kernel_s360_x2" and at(2049) == "cn_env_kernel_fair_s360_w4"
    assert at(4096) == "cn_env_kernel_fair_s360_w4" and at(4097) == "cn_env_kernel_fair_s360"
    assert at(2048, x2=0) == "cn_env_kernel_fair_s360_w4" and at(2049, wpb=0) == "cn_env_kernel_fair_s360" and at(4097, x2=1) == "cn_env_kernel_s360_x2"
    assert at(1, w="generic") == "cn_env_kernel" and at(2048, w="generic") == "cn_env_kernel_fair"
    assert at(1, x2=1, w="s720") == "cn_env_kernel_s720" and at(4097, w="s720") == "cn_env_kernel_fair_s720"
    assert selection[("s360", "step", (T.ARB_AUTO, 0, 0, 4097, 0, -1, 4))] == "cn_env_kernel_s360"       # unknown CU count: nothing by size


def test_the_table_has_68_kernels_in_their_compile_units(selection):
    assert selection["counts"] == (53, 15, 15)
    names = [n for n, _ in selection["kernels"]]
    assert len(names) == len(set(names)) == 68
    assert dict(selection["kernels"]) == T.UNIT
    assert all(n.startswith("cn_policy_kernel") for n in names[53:]) and not any(n.startswith("cn_policy_kernel") for n in names[:53])
    selected = {v for k, v in selection.items() if isinstance(k, tuple) and v}
    assert selected == set(names)                                                # no kernel that no launch selects
