"""csrc/crowdnav_lds.h without a GPU: the header is plain C++, so a stand-alone program compiled with g++ walks the LDS map the step
kernels carve from and cn_create sizes launches from -- every region inside the total, the regions that are live together disjoint,
the three declared overlays inside their host region -- and prints it.  The totals and cn_near_separate are held to the values of
the commit before the map existed, when the kernel's carve and two host functions each restated the arithmetic:
tests/golden/lds_map_parent.json was written by a scratch program that included that commit's lds_scratch_bytes, lds_bytes_impl,
waves_per_cu, cn_near_separate and cn_lds_bytes unchanged and walked the grid below (only its output is kept)."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, PKG

RS = (8, 9, 13, 33, 41, 42, 64, 65, 66, 129, 130, 308, 360, 720, 1025)
PS = (0, 1, 2, 12, 20, 40, 41, 48, 100, 128)
KS = (1, 8, 16)
TS = (32, 64, 128, 1024)
COMPACT = [(720, P, K, 64) for P in PS for K in KS] + [(9, 12, 8, 128)]      # the 720-ray row; one point where the layout does not fit
REFUSED = 1 << 30
TF_COUNT, MAX_K, NMASK, MAX_TRACKS = 12, 16, 13, 64
FIELDS = ("szA", "szB", "szC", "w64", "wbase", "ped", "pedv", "nearp", "rw", "total")

PROGRAM = r"""
#include <stdio.h>
#include "crowdnav_lds.h"
static void point(int R, int P, int K, int T, int ns, int rw, int cmp)
{
    const CnLdsMap m = cn_lds_map(R - 1, P, K, (R - 1) / 4 + 2, cn_lds_trk_slots(T), ns, cmp != 0, rw != 0);
    printf("map %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", R, P, K, T, ns, rw, cmp,
           m.szA, m.szB, m.szC, m.w64, m.wbase, m.ped, m.pedv, m.nearp, m.rw, m.total);
}
int main()
{
    const int Rs[] = {@RS@}, Ps[] = {@PS@}, Ks[] = {@KS@}, Ts[] = {@TS@};
    printf("consts %d %d %d %d %d\n", (int)CN_TF_COUNT, (int)CN_MAX_K, (int)CN_NMASK, (int)CN_MAX_TRACKS, (int)CN_SHAPE_COUNT);
    for (int i = 0; i < CN_SHAPE_COUNT; ++i) { const CnShape& s = cn_shapes[i]; printf("shape %d %d %d %d %d %d\n", s.R, s.P, s.K, s.max_conf, s.trk_cap, s.near_sep); }
    for (int R : Rs) { printf("scratch %d %zu\n", R, cn_lds_sim_scratch(R));
        for (int P : Ps) for (int K : Ks) for (int T : Ts) {
            printf("near %d %d %d %d %d\n", R, P, K, T, cn_lds_near_separate(R, P, K, (R - 1) / 4 + 2, T));
            for (int ns = 0; ns < 2; ++ns) for (int rw = 0; rw < 2; ++rw) point(R, P, K, T, ns, rw, 0);
        } }
@COMPACT@
    return 0;
}
"""


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """{"map": {(R, P, K, trk_cap, near_sep, realworld, compact): {field: bytes}}, "near": {(R, P, K, trk_cap): 0 / 1}, "shape": rows,
    "scratch": {R: bytes}, "consts": ...} -- one compile, one run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("lds_map")
    src, exe = tmp / "walk.cpp", tmp / "walk"
    text = PROGRAM
    for key, vals in (("RS", RS), ("PS", PS), ("KS", KS), ("TS", TS)):
        text = text.replace("@%s@" % key, ", ".join(map(str, vals)))
    text = text.replace("@COMPACT@", "\n".join("    point(%d, %d, %d, %d, 0, %d, 1);" % (c + (rw,)) for c in COMPACT for rw in (0, 1)))
    src.write_text(text)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), "-o", str(exe), str(src)], check=True)
    out = {"map": {}, "near": {}, "shape": [], "scratch": {}}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        f = ln.split()
        v = [int(x) for x in f[1:]]
        if f[0] == "map":
            out["map"][tuple(v[:7])] = dict(zip(FIELDS, v[7:]))
        elif f[0] == "near":
            out["near"][tuple(v[:4])] = v[4]
        elif f[0] == "shape":
            out["shape"].append(tuple(v))
        elif f[0] == "scratch":
            out["scratch"][v[0]] = v[1]
        else:
            out["consts"] = tuple(v)
    return out


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "lds_map_parent.json")) as fh:
        return json.load(fh)


def regions(key, m):
    """[(name, first byte, one past the last)] of the regions that are live together at this point, by the sizes the kernel indexes"""
    R, P, K, T, ns, rw, cmp = key
    n, Wn = R - 1, (R - 1 + 63) // 64
    r = [("A", 0, m["szA"]), ("B", m["szA"], m["szA"] + m["szB"]), ("w64", m["w64"], m["w64"] + 8 * NMASK * Wn),
         ("wbase", m["wbase"], m["wbase"] + 4 * 3 * Wn), ("ped", m["ped"], m["ped"] + 8 * (2 * P + 2))]
    if not cmp:
        r.append(("pedv", m["pedv"], m["pedv"] + 8 * (2 * P + 2)))
    if ns:
        r.append(("nearp", m["nearp"], m["nearp"] + 32 * (P + 1)))
    if rw:
        r.append(("rw", m["rw"], m["rw"] + 12 * n))
    return r


def test_the_grid_is_walked_whole(walk):
    assert walk["consts"] == (TF_COUNT, MAX_K, NMASK, MAX_TRACKS, 2)
    assert len(walk["map"]) == len(RS) * len(PS) * len(KS) * len(TS) * 4 + 2 * len(COMPACT)
    assert len(walk["near"]) == len(RS) * len(PS) * len(KS) * len(TS)


def test_regions_lie_inside_the_total_and_apart(walk):
    for key, m in walk["map"].items():
        if m["total"] == REFUSED:
            continue
        assert m["total"] % 16 == 0 and m["rw"] % 16 == 0, key
        rs = regions(key, m)
        for name, lo, hi in rs:
            assert 0 <= lo <= hi <= m["total"], (key, name)
        for (na, la, ha), (nb, lb, hb) in itertools.combinations(rs, 2):
            assert ha <= lb or hb <= la, (key, na, nb)


def test_the_views_of_a_region_end_inside_it(walk):
    for key, m in walk["map"].items():
        R, P, K, T, ns, rw, cmp = key
        n, mc = R - 1, (R - 1) // 4 + 2
        assert m["szA"] >= (6 if cmp else 10) * n, key                     # end points: x, y (int32, compact int16), range (uint16)
        assert m["szB"] >= 6 * n and m["szB"] >= 8 * 64, key               # gradients + alias sources; the bbox staging buffer
        assert m["szC"] >= (12 if cmp else 32) * mc and m["szC"] % 8 == 0, key
        assert m["szC"] + 8 * 64 + 8 * (8 + 4 * K) + 4 * MAX_K <= m["szB"], key          # cpv [64], tail [8 + 4 K], kidx end inside B
        if not cmp:
            assert m["szA"] + m["szB"] >= walk["scratch"][R] == 16 * n, key              # cn_create's ped_contact / pair-matrix limits


def test_the_three_overlays_lie_inside_their_host_region(walk):
    refused = []
    for key, m in walk["map"].items():
        R, P, K, T, ns, rw, cmp = key
        assert 8 * TF_COUNT * (T if T <= MAX_TRACKS else 0) <= m["szA"], key              # the LDS tracker table in A; a wide one is in HBM
        if cmp:
            assert m["pedv"] == 0, key
            if 8 * (2 * P + 2) > m["szA"]:
                assert m["total"] == REFUSED, key
                refused.append(key)
            else:
                assert m["total"] < 160 * 1024, key
        else:
            assert m["total"] != REFUSED, key
        if not ns:
            assert m["nearp"] == m["szA"] and 32 * (P + 1) <= m["szB"], key
    assert [k[:4] for k in refused] == [(9, 12, 8, 128)] * 2


def test_totals_and_near_separate_equal_the_parent_commits(walk, parent):
    assert parent["columns"] == ["R", "P", "K", "trk_cap", "near_separate", "lds_bytes", "plain_ns0", "plain_ns1", "realworld_ns0",
                                 "realworld_ns1", "scratch_ns0", "scratch_ns1"]
    assert len(parent["points"]) == len(walk["near"])
    for R, P, K, T, sep, own, p0, p1, r0, r1, s0, s1 in parent["points"]:
        at = lambda ns, rw: walk["map"][(R, P, K, T, ns, rw, 0)]
        assert walk["near"][(R, P, K, T)] == sep, (R, P, K, T)
        assert at(sep, 0)["total"] == own, (R, P, K, T)                               # cn_lds_bytes: the handle's own near_sep
        assert [at(0, 0)["total"], at(1, 0)["total"], at(0, 1)["total"], at(1, 1)["total"]] == [p0, p1, r0, r1], (R, P, K, T)
        assert [at(ns, 0)["szA"] + at(ns, 0)["szB"] for ns in (0, 1)] == [s0, s1], (R, P, K, T)      # the simulators' scratch
    assert [tuple(c[:4]) for c in parent["compact"]] == COMPACT
    for R, P, K, T, p0, r0 in parent["compact"]:
        assert [walk["map"][(R, P, K, T, 0, rw, 1)]["total"] for rw in (0, 1)] == [p0, r0], (R, P, K, T)


def test_spot_values_of_the_four_worked_shapes(walk):
    at = lambda R, P, K, T, rw=0, cmp=0: walk["map"][(R, P, K, T, walk["near"][(R, P, K, T)], rw, cmp)]
    m = at(360, 20, 8, 32)
    assert (walk["near"][(360, 20, 8, 32)], m["szA"], m["szB"], m["total"], at(360, 20, 8, 32, rw=1)["total"]) == (1, 3592, 3808, 9440, 13776)
    assert (walk["near"][(720, 100, 8, 64)], at(720, 100, 8, 64)["total"], at(720, 100, 8, 64, cmp=1)["total"]) == (0, 18512, 13472)
    m = at(33, 48, 8, 64)                  # the overlaid near list's 49 entries of 32 bytes bind region B (1 216 bytes otherwise)
    assert (walk["near"][(33, 48, 8, 64)], m["szB"], m["total"], walk["map"][(33, 48, 8, 64, 1, 0, 0)]["szB"]) == (0, 1568, 9408, 1216)
    m = at(41, 12, 8, 32, rw=1)            # the real-world lists start after an 8-byte pad
    assert (at(41, 12, 8, 32)["total"], m["total"], m["rw"], m["nearp"] + 32 * 13) == (5312, 5808, 5312, 5304)


def test_the_compiled_shapes_are_cn_creates_values_for_them(walk):
    assert [s[0] for s in walk["shape"]] == [360, 720]
    for R, P, K, mc, tc, ns in walk["shape"]:
        assert K == 8 and mc == (R - 1) // 4 + 2 and tc == (32 if P <= 40 else 64)         # cn_create's max_conf and automatic table
        assert ns == walk["near"][(R, P, K, tc)]
