"""cn_step_group_* without a GPU: the group kernels' list and selection (csrc/crowdnav_variants.h, compiled with g++ like
tests/test_kernel_table.py does), the new exports in include/crowdnav.h against crowdnav._abi, the trainer's --population-step switch,
and MemberEnvs.bind_step_group's marshalling against a stand-in for the library."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import kernel_table_ref as T
from conftest import PKG, ROOT
from test_eval_layout import GOLDEN
from test_env_marshalling import N, fields, handle, own_buffers
from test_kernel_table import PROGRAM

E_ = "cn_env_kernel"
# world -> its group kernel: the STEP column with _grp
GROUP = {w: row[1] + "_grp" for w, row in T.WORLDS.items()}
X2 = E_ + "_s360_x2_grp"
NCU = 256
QUERIES = [(total, ncu, x2) for ncu in (NCU, 0) for total in (1, 8 * NCU - 1, 8 * NCU, 8 * NCU + 1, 100000) for x2 in (-1, 0, 1)]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{"group": [names in cn_group_kernel_info's order], "known": the 68 names of cn_kernel_info, (world, total, n_cus, x2): name}"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    lines = ['    printf("group_count %d %s\\n", (int)CN_G_COUNT, name_of(CN_K_none));',
             '    for (int id = 0; id < CN_G_COUNT; ++id) printf("group %s %d %d\\n", cn_group_kernel_info[id].name, (int)cn_group_kernel_info[id].compact, cn_group_kernel_info[id].geometry);']
    for w, row in T.WORLDS.items():
        lines.append("    { const int w = cn_world_index(%s);" % ", ".join(str(f) for f in row[0]))
        for total, ncu, x2 in QUERIES:
            lines.append('      printf("gselect %s %d/%d/%d %%s\\n", cn_group_kernel_info[cn_select_group_kernel(w, %dll, %d, %d)].name);'
                         % (w, total, ncu, x2, total, ncu, x2))
        lines.append("    }")
    # tests/test_kernel_table.py's program (it prints the 68 names of cn_kernel_info) with these lines as its queries
    tmp = tmp_path_factory.mktemp("step_group_table")
    out = {"group": [], "known": []}
    src, exe = tmp / "walk.cpp", tmp / "walk"
    src.write_text(PROGRAM.replace("@QUERIES@", "\n".join(lines)))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), "-o", str(exe), str(src)], check=True)
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        f = ln.split()
        if f[0] == "group_count":
            out["count"] = int(f[1])
        elif f[0] == "group":
            out["group"].append((f[1], int(f[2]), int(f[3])))
        elif f[0] == "kernel":
            out["known"].append(f[1])
        elif f[0] == "gselect":
            out[(f[1],) + tuple(int(x) for x in f[2].split("/"))] = f[3]
    return out


def test_sixteen_group_kernels_beside_the_68(table):
    names = [n for n, _, _ in table["group"]]
    assert table["count"] == 16 and len(names) == len(set(names)) == 16
    assert len(table["known"]) == len(set(table["known"])) == 68 and not set(names) & set(table["known"])
    assert set(names) == set(GROUP.values()) | {X2}
    # each is a known step kernel's name with _grp: the worlds' STEP column and the headline shape's two-wavefront form
    assert {n[:-len("_grp")] for n in names} <= set(table["known"]) and all(n.endswith("_grp") for n in names)
    # the compact LDS layout is the 720-ray shape's; two wavefronts per environment (geometry 2) the x2 form's alone
    assert {n for n, compact, _ in table["group"] if compact} == {E_ + "_s720_grp"}
    assert {n: geo for n, _, geo in table["group"] if geo} == {X2: 2}


def test_selection_over_every_world_and_both_sides_of_the_threshold(table):
    for w in T.WORLDS:
        for total, ncu, x2 in QUERIES:
            two = w == "s360" and (x2 == 1 or (x2 < 0 and total <= 8 * ncu))
            assert table[(w, total, ncu, x2)] == (X2 if two else GROUP[w]), (w, total, ncu, x2)
    at = lambda total, x2=-1, w="s360", ncu=NCU: table[(w, total, ncu, x2)]
    assert at(8 * NCU) == X2 and at(8 * NCU + 1) == E_ + "_s360_grp"
    assert at(1, x2=0) == E_ + "_s360_grp" and at(100000, x2=1) == X2
    assert at(1, ncu=0) == E_ + "_s360_grp" and at(1, x2=1, ncu=0) == X2            # unknown CU count: nothing by size
    assert at(1, x2=1, w="generic") == E_ + "_grp" and at(1, x2=1, w="s720") == E_ + "_s720_grp"


def test_header_and_binding_agree_on_the_new_exports():
    from crowdnav import _abi
    header = open(os.path.join(ROOT, "include", "crowdnav.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = re.findall(r"\b(cn_step_group_\w+)\s*\(", code)
    want = ["cn_step_group_create", "cn_step_group_step", "cn_step_group_reset", "cn_step_group_jobs", "cn_step_group_kernel_name",
            "cn_step_group_destroy"]
    assert declared == want
    assert [e for e in _abi.EXPORTS if e.startswith("cn_step_group_")] == want
    assert int(re.search(r"#define\s+CN_STEP_GROUP_MAX\s+(\d+)", code).group(1)) == _abi.CN_STEP_GROUP_MAX == 64
    assert "typedef struct cn_step_group_s* cn_step_group_handle;" in code
    assert re.search(r"#define\s+CN_ABI_VERSION\s+7\b", code) and _abi.EXPECTED_ABI == 7          # new exports only


# ---- crowdnav.train --population-step ---------------------------------------------------------------------------------------------
POP = ["--algo", "td3", "--learner", "fused", "--population", "2"]


def test_the_switch_parses_and_defaults_to_per_member():
    from crowdnav import train
    assert train.parse_args(POP).population_step == "per-member"
    assert train.parse_args(POP + ["--population-step", "per-member"]).population_step == "per-member"
    assert train.parse_args(POP + ["--population-step", "one-launch"]).population_step == "one-launch"
    assert train.parse_args([]).population_step == "per-member"


def test_the_switch_needs_a_population_and_a_known_value(capsys):
    from crowdnav import train
    for argv in (["--population-step", "one-launch"], ["--population-step", "per-member"], ["--algo", "ddpg", "--population-step", "one-launch"]):
        with pytest.raises(SystemExit):
            train.parse_args(argv)
        assert "--population-step" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(POP + ["--population-step", "grouped"])
    assert "invalid choice" in capsys.readouterr().err


def test_the_switch_is_held_beside_the_namespace_and_recorded_namespaces_stay():
    import argparse
    from crowdnav import train
    from test_eval_layout import NEW_KEYS
    for argv in (POP, POP + ["--population-step", "one-launch"]):
        a = train.parse_args(argv)
        assert "population_step" not in vars(a) and not hasattr(argparse.Namespace(**vars(a)), "population_step")
    assert vars(train.parse_args(POP)) == vars(train.parse_args(POP + ["--population-step", "one-launch"]))
    assert getattr(train.fill_defaults(argparse.Namespace(algo="td3")), "population_step", None) is None
    rec = json.load(open(os.path.join(GOLDEN, "train_namespaces_before_eval.json")))
    for argv, old in zip(rec["argvs"], rec["namespaces"]):
        new = vars(train.parse_args(argv))
        assert set(new) - set(old) == set(NEW_KEYS) | {"eval_max_steps", "eval_seed"}, argv
        for k, v in old.items():
            assert (list(new[k]) if isinstance(new[k], tuple) else new[k]) == v, (argv, k)


# ---- MemberEnvs.bind_step_group against a stand-in for the library ---------------------------------------------------------------
def fake_library(calls, rc_create=0):
    def create(n, hs, ios, out):
        calls.append(("create", n, [hs[j] for j in range(n)], [fields(ios[j]) for j in range(n)]))
        out._obj.value = 0xABC0 + len(calls)                    # (out: byref of the caller's handle)
        return rc_create
    return types.SimpleNamespace(cn_step_group_create=create,
                                 cn_step_group_step=lambda g, s: calls.append(("step", g.value, s.value)) or 0,
                                 cn_step_group_reset=lambda g, m, s: calls.append(("reset", g.value, None if m is None else list(m), s.value)) or 0,
                                 cn_step_group_kernel_name=lambda g: b"cn_env_kernel_grp",
                                 cn_step_group_destroy=lambda g: calls.append(("destroy", g.value)))


def members(J, calls):
    from crowdnav import env as E
    grp = object.__new__(E.MemberEnvs)
    grp.envs = [handle(h=0x1000 * (g + 1), stream=0x100 * (g + 1)) for g in range(J)]
    L = fake_library(calls)
    for e in grp.envs:
        e.L = L
        e.close = lambda: calls.append(("close",))
    grp.G, grp.N, grp.device = J, J * N, torch.device("cpu")
    grp._current_stream = lambda: C.c_void_p(0x77)
    return grp


@pytest.mark.parametrize("J", [1, 3])
def test_bind_step_group_marshals_one_job_per_member(J):
    calls = []
    grp = members(J, calls)
    a = torch.zeros((J * N, 2))
    call = grp.bind_step_group(a, auto_reset="next")
    assert [c[0] for c in calls] == ["create"]                  # binding creates the group and enqueues nothing
    _, n, hs, ios = calls[0]
    assert n == J and hs == [e.h.value for e in grp.envs]
    for g, e in enumerate(grp.envs):                            # job g: member g's rows of the action, its own buffers, next-step reset
        assert ios[g] == dict(own_buffers(e), action=a.data_ptr() + 4 * 2 * N * g, step_counter=None, final_obs=None, obs_f64=None,
                              auto_reset=2, reserved=0)
    call(); call()
    assert calls[1:] == [("step", calls[1][1], 0x77)] * 2 and calls[1][1] == 0xABC1     # one foreign call per step: the group, the bound stream
    assert grp.step_group_kernel(a) == "cn_env_kernel_grp"
    grp.bind_step_group(a, auto_reset="next")
    assert [c[0] for c in calls].count("create") == 1           # the same buffer and convention: the same group
    grp.bind_step_group(torch.zeros((J * N, 2)), auto_reset=False)
    assert [c[0] for c in calls].count("create") == 2 and calls[-1][3][0]["auto_reset"] == 0
    # reset(group=True): one call on the current stream; the masks' addresses per member, None = all
    m = torch.ones(N, dtype=torch.uint8)
    grp.obs = object()
    assert grp.reset(group=True, masks=[m] + [None] * (J - 1)) is grp.obs
    assert calls[-1] == ("reset", 0xABC1, [m.data_ptr()] + [None] * (J - 1), 0x77)
    grp.reset(group=True)
    assert calls[-1] == ("reset", 0xABC1, None, 0x77)
    # close(): the groups go before the handles
    del calls[:]
    grp.close()
    assert [c[0] for c in calls] == ["destroy", "destroy"] + ["close"] * J


def test_bind_step_group_raises_with_the_librarys_message(monkeypatch):
    from crowdnav import _abi
    calls = []
    grp = members(2, calls)
    L = fake_library(calls, rc_create=-2)
    for e in grp.envs:
        e.L = L
    monkeypatch.setattr(_abi, "lib", lambda: types.SimpleNamespace(cn_last_error=lambda: b"cn_step_group_create: job 1: its group kernel is x"))
    with pytest.raises(_abi.CrowdNavError, match="job 1: its group kernel"):
        grp.bind_step_group(torch.zeros((2 * N, 2)))
    assert not grp.__dict__.get("_step_groups")                 # no fallback and nothing kept
