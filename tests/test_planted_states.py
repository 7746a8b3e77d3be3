"""tests/planted_states.py without a GPU.  The premise, on the oracle alone, in every world tests/test_gpu_planted_states.py uses: every
planted record passes cn_restore's record check, every named event happens in the named step under both reset conventions, no
environment raises a status bit its record does not name, all outputs are finite, every family's edge is hit by at least one record (for
the tracker family each of the four totals S-1 ... S+2 at the world's S).  The record check itself (csrc/crowdnav_snapshot_check.h, plain
C++) compiled stand-alone with g++ and the address and undefined-behaviour sanitizers -- a program with its own main, nothing is
preloaded -- reads record sets from a file and prints verdicts: every planted record passes; every environment's record at every step
of a 40-step oracle run in every world of kernel_table_ref.WORLDS and in a gt world of 16 rays passes under both reset conventions and
with auto_reset none stepped on past done (no false refusal: NCONF above max_conf, EP_STEP above max_steps are states of a run); each
single-field violation is refused with the right environment and field named; the first error wins.  And the planted arrays are the same
on both sides: join_snapshot then split_snapshot returns them byte for byte."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kernel_matrix as M
import kernel_table_ref as T
import planted_states as PS
from conftest import PKG

WORLDS = sorted({c.world for c in M.CELLS if c.form in ("step", "same")} | {"s360"})

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "crowdnav_snapshot_check.h"
int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[6];
    while (fread(hd, sizeof(int32_t), 6, f) == 6) {
        if (hd[0] != 0x43524E43 || hd[5] != (int32_t)sizeof(cn_config)) { printf("bad set header\n"); return 3; }
        const size_t slots = hd[1], N = hd[3], P = hd[4];
        cn_config c;
        if (fread(&c, sizeof(c), 1, f) != 1) return 3;
        std::vector<double> sd(N * CN_SD_COUNT), pp(N * P * 2), pv(N * P * 2), trk(N * slots * CN_TF_COUNT);
        std::vector<int32_t> si(N * CN_SI_COUNT);
        if (fread(sd.data(), 8, sd.size(), f) != sd.size() || fread(si.data(), 4, si.size(), f) != si.size() ||
            fread(pp.data(), 8, pp.size(), f) != pp.size() || fread(pv.data(), 8, pv.size(), f) != pv.size() ||
            fread(trk.data(), 8, trk.size(), f) != trk.size()) { printf("short set\n"); return 3; }
        // exactly-sized heap blocks: a read past a section's end is the address sanitizer's to report
        const CnRecordSections s = {sd.data(), si.data(), pp.data(), pv.data(), trk.data()};
        const CnRecordVerdict v = cn_check_records(c, (int)slots, hd[2], (int)N, s);
        char text[200];
        cn_record_verdict_text(v, text, sizeof(text));
        printf("%s\n", text);
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    """path of the compiled walker: walker(file) -> the verdict of every set in it"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("record_check")
    src, exe = tmp / "walk.cpp", tmp / "walk"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",          # the runtimes inside the program: it needs nothing of its environment
                    "-I", os.path.join(PKG, "csrc"), "-o", str(exe), str(src)], check=True)
    def run(path):
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        return r.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def plans(oracle_mod):
    return {w: PS.plan(w, oracle_mod) for w in WORLDS}


def _config(W, n):
    from crowdnav import Config
    return Config(**dict(W.kw, n_envs=n))


# ---- the premise ------------------------------------------------------------------------------------------------------------------------
def test_the_gpu_files_worlds_are_every_world_and_the_records_are_independent_of_the_run(plans, oracle_mod):
    assert WORLDS == sorted(T.WORLDS)
    for w, p in plans.items():
        assert len(p.records) == p.arrays["sd"].shape[0] == p.actions.shape[1] and p.actions.shape == (PS.STEPS, len(p.records), 2)
        assert p.actions.dtype == np.float32 and all((p.actions[:, e] == 0).all() for e, r in enumerate(p.records) if r.rest)
        assert len({(r.family, r.name) for r in p.records}) == len(p.records)
        assert all(r.how and set(r.expect) == {"next", "same"} for r in p.records)
        # a record edits its own environment only, and the plan is a function of the world
        PS._plans.pop(w)
        [PS._runs.pop(k) for k in list(PS._runs) if k[0] == w]
        q = PS.plan(w, oracle_mod)
        assert all(np.array_equal(p.arrays[k], q.arrays[k], equal_nan=True) for k in PS.KEYS) and np.array_equal(p.actions, q.actions)
        assert p.arrays["trk"].shape[1] == p.world.slots and p.world.slots in (32, 64, 256)


@pytest.mark.parametrize("mode", ["next", "same"])
@pytest.mark.parametrize("world", WORLDS)
def test_every_named_event_happens_in_its_step_on_the_oracle_alone(plans, oracle_mod, world, mode):
    p = plans[world]
    before, steps, _ = PS.run_oracle(p, oracle_mod, mode)
    bad = PS.check_premise(p, before, steps, mode)
    assert not bad, "\n".join(bad)
    # the overflowing environments, fixed here for the GPU file: at most the S+1 / S+2 records of the tracker family
    over = PS.overflow_records(p)
    W = p.world
    want = [] if (W.gt or not W.has_tracker or W.slots > oracle_mod.MAX_TRACKS) else ["ntracks=%d new=%d" % (nt, new) for nt in (W.slots - 1, W.slots) for new in (1, 2)
                                                                                  if nt + new > W.slots]
    assert [p.records[e].name for e in over] == want and len(over) == PS.N_OVERFLOW[world]


def test_every_familys_edge_is_hit(plans):
    for w, p in plans.items():
        for fam in PS.FAMILIES:
            have = {e for r in p.records if r.family == fam for e in r.edges}
            miss = [e for e in PS.required_edges(p.world, fam) if e not in have]
            assert not miss, (w, fam, miss)
        if p.world.has_tracker and not p.world.gt:
            totals = {r.name: r for r in p.records if r.family == "tracker"}
            S = p.world.cap
            for d in ((-1, 0) if p.world.slots > 64 else (-1, 0, 1, 2)):
                assert any("total=S%+d" % d in r.edges for r in totals.values()), (w, S, d)


# ---- the record check, compiled stand-alone -----------------------------------------------------------------------------------------------
def test_every_planted_record_passes_the_record_check(plans, walker, tmp_path):
    path = tmp_path / "planted.bin"
    with open(path, "wb") as f:
        for w in WORLDS:
            p = plans[w]
            PS.write_record_set(f, _config(p.world, len(p.records)), p.world.slots, p.world.max_conf, p.arrays)
    assert walker(path) == ["ok"] * len(WORLDS)


# a gt world of few rays and a long lidar: the pedestrians in sight (NCONF there) outnumber max_conf = (R - 1) / 4 + 2 = 5
FEW_RAYS_GT = dict(M.COMMON, risk_mode=1, n_rays=16, n_peds=20, lidar_max=3.5)


@pytest.mark.parametrize("world", sorted(T.WORLDS) + ["few_rays_gt"])
def test_no_record_of_a_40_step_oracle_run_is_refused(oracle_mod, walker, tmp_path, world):
    """under both reset conventions, and with auto_reset none: the caller never resets, the done flag is held and EP_STEP counts on"""
    from crowdnav import Config
    cfg = Config(**(FEW_RAYS_GT if world == "few_rays_gt" else M.config_kw(world)))
    slots = cfg.track_capacity or (32 if (cfg.n_peds <= 40 and not (cfg.risk_mode == 1 and cfg.n_peds > 32)) else 64)      # cn_create's rule
    max_conf = (cfg.n_rays - 1) // 4 + 2
    path = tmp_path / "run.bin"
    sets, top = 0, dict(nconf=0, ep_step=0)
    with open(path, "wb") as f:
        for mode in ("next", "same", False):
            orc = oracle_mod.Oracle(cfg.as_dict())
            orc.reset()
            PS.write_record_set(f, cfg, slots, max_conf, PS.oracle_states(orc, slots)); sets += 1
            for a in M.actions():
                M.oracle_step(orc, a, mode)
                st = PS.oracle_states(orc, slots)
                top = dict(nconf=max(top["nconf"], int(st["si"][:, PS.SI["NCONF"]].max())), ep_step=max(top["ep_step"], int(st["si"][:, PS.SI["EP_STEP"]].max())))
                PS.write_record_set(f, cfg, slots, max_conf, st); sets += 1
    assert sets == 3 * (M.STEPS + 1) and walker(path) == ["ok"] * sets
    assert top["ep_step"] == M.STEPS > cfg.max_steps                       # the run without resets did count past the time limit
    if world == "few_rays_gt":
        assert top["nconf"] > max_conf, top                                # ... and this world did see more pedestrians than max_conf


@pytest.mark.parametrize("world", ["s360", "gt", "orig", "wide", "s720"])
def test_each_single_field_violation_is_refused_by_name_and_the_first_error_wins(plans, walker, tmp_path, world):
    p = plans[world]
    W, cfg = p.world, _config(p.world, len(p.records))
    vio = PS.violations(W, p.arrays)
    path = tmp_path / "bad.bin"
    with open(path, "wb") as f:
        for _, _, edit in vio:
            a = {k: v.copy() for k, v in p.arrays.items()}
            edit(a)
            PS.write_record_set(f, cfg, W.slots, W.max_conf, a)
        # two offences in one blob: the lower environment is named; two in one environment: the rule's order (si before sd before ped before trk)
        a = {k: v.copy() for k, v in p.arrays.items()}
        a["si"][7, PS.SI["DONE"]] = 2; a["sd"][3, PS.SD["RYAW"]] = np.nan
        PS.write_record_set(f, cfg, W.slots, W.max_conf, a)
        a = {k: v.copy() for k, v in p.arrays.items()}
        a["ped_v"][4, 0, 0] = np.inf; a["sd"][4, PS.SD["RX"]] = np.nan; a["si"][4, PS.SI["EP_STEP"]] = -5; a["si"][4, PS.SI["NCONF"]] = -1
        PS.write_record_set(f, cfg, W.slots, W.max_conf, a)
    got = walker(path)
    assert len(got) == len(vio) + 2
    for (name, text, _), line in zip(vio, got):
        assert line.startswith(text), (name, line)
    assert got[-2].startswith("env 3: sd.RYAW = ") and got[-1] == "env 4: si.EP_STEP = -5"
    keys = [name.split("=")[0] for name, _, _ in vio]
    fields = {k.split(".")[1] if k.split("[")[0].split(".")[0] in ("si", "sd", "trk") else k.split("[")[0] for k in keys}
    assert {"NTRACKS", "DQ_LEN", "DQLEN", "DONE", "PENDING_RESET", "EP_STEP", "NCONF", "NENTRIES", "CROWD_HI", "T", "RX", "RY", "RYAW", "PX", "ped_p",
            "ped_v"} <= fields


# ---- equal arrays ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_join_then_split_returns_the_planted_arrays_byte_for_byte(plans, world):
    from crowdnav import _abi
    p = plans[world]
    W, N = p.world, len(p.records)
    fresh = dict(ped_init=np.arange(N * W.P * 2, dtype=np.float64).reshape(N, W.P, 2), ped_preset=np.zeros((N, W.P, 2)))
    arrs = PS.snapshot_arrays(p, fresh)
    hd = _abi.CnSnapshotHeader(magic=_abi.CN_SNAPSHOT_MAGIC, abi_version=_abi.EXPECTED_ABI, header_bytes=C.sizeof(_abi.CnSnapshotHeader),
                               sd_count=_abi.CN_SD_COUNT, si_count=_abi.CN_SI_COUNT, tf_count=_abi.CN_TF_COUNT, track_capacity=W.slots,
                               config=_config(W, N).to_c())
    hd.total_bytes = hd.header_bytes + sum(np.ascontiguousarray(arrs[k], dtype=dt).nbytes for k, dt, _ in _abi.SNAPSHOT_SECTIONS)
    hd2, back = _abi.split_snapshot(_abi.join_snapshot(hd, arrs))
    assert bytes(hd2) == bytes(hd) and set(back) == set(arrs)
    for k, dt, _ in _abi.SNAPSHOT_SECTIONS:
        assert back[k].dtype == np.dtype(dt) and back[k].tobytes() == np.ascontiguousarray(arrs[k], dtype=dt).tobytes(), k
