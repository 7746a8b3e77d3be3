"""csrc/build.sh's unit list is the only list of the library's compile units: read as text, no compiler and no GPU.  Every *.hip under
csrc/ is in the list, every entry of the list is a file, and the two tools that build a library of their own (tools/profc/build.sh,
tools/ab_build.sh) carry no list of sources: nothing in them can go stale when a subsystem is added.  The same for what the units
share: a kernel is defined in one unit only (the others reach it through that unit's host launchers), and the tile sizes of the
learners' GEMM kernels are written once on the host."""
import os
import re

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")
INSTRUMENTED = "crowdnav_kernel.hip"          # tools/profc/build.sh compiles unit 1 of this file itself, with its counters


def unit_list():
    """(array name, object, source, the unit's own flags) of every entry of build.sh's UNITS and TIMING_UNITS."""
    text = open(os.path.join(CSRC, "build.sh")).read()
    units = []
    for name, body in re.findall(r"^(UNITS|TIMING_UNITS)=\((.*?)\)", text, re.S | re.M):
        for entry in re.findall(r'"([^"]*)"', body):
            f = entry.split()
            units.append((name, f[0], f[1], f[2:]))
    return text, units


def test_every_hip_source_is_a_unit_and_every_unit_is_a_file():
    text, units = unit_list()
    assert {u[0] for u in units} == {"UNITS", "TIMING_UNITS"}
    on_disk = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert sorted({u[2] for u in units}) == on_disk
    for _, obj, src, _ in units:
        assert os.path.isfile(os.path.join(CSRC, src)), src
    objs = [u[1] for u in units]
    assert len(set(objs)) == len(objs)                      # an object name is a file name in the link line
    # the list is the only place that names a source: the compile loop and the link line are derived from it
    outside = re.sub(r"^(UNITS|TIMING_UNITS)=\(.*?\)", "", text, flags=re.S | re.M)
    code = "\n".join(l for l in outside.split("\n") if not l.lstrip().startswith("#"))
    assert ".hip" not in code and '"${OBJS[@]}"' in code and "${LIST[@]}" in code


def test_a_source_compiled_more_than_once_names_its_units():
    _, units = unit_list()
    by_src = {}
    for _, _, src, flags in units:
        by_src.setdefault(src, []).append([f[len("-DCN_TU="):] for f in flags if f.startswith("-DCN_TU=")])
    for src, tus in by_src.items():
        assert tus == [[]] or (all(len(t) == 1 for t in tus) and len({t[0] for t in tus}) == len(tus)), (src, tus)
    # the kernel table's compile-unit column (tests/kernel_table_ref.py) speaks of exactly the kernel file's units
    import kernel_table_ref as T
    assert sorted(int(t[0]) for t in by_src[INSTRUMENTED]) == sorted(set(T.UNIT.values()))


def test_the_tools_carry_no_source_list():
    for rel in ("tools/profc/build.sh", "tools/ab_build.sh"):
        text = open(os.path.join(ROOT, rel)).read()
        assert set(re.findall(r"\w+\.hip\b", text)) <= {INSTRUMENTED}, rel
        assert "build.sh" in text.replace(rel, "")         # they go through csrc/build.sh instead


def sources():
    """{file name: text without comments} of every *.hip and *.h under csrc/"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(CSRC, f)).read()
            out[f] = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    return out


def kernel_definitions(text):
    """Names of the __global__ functions that `text` defines (a body follows the parameter list), not of those it only declares.  A name
    in capitals is a macro's parameter: the definition is the macro's, expanded once per row of the kernel table."""
    names = []
    for m in re.finditer(r"__global__", text):
        rest = re.sub(r"__launch_bounds__\s*\([^()]*\)", " ", text[m.end():m.end() + 4000])
        head = re.match(r"\s*void((?:\s+\w+)*?)\s+(\w+)\s*\(", rest)
        assert head, rest[:200]
        depth, i = 1, head.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(rest[i], 0)
            i += 1
        after = rest[i:].lstrip()[:1]
        assert after in "{;", (head.group(2), after)
        if after == "{":
            names.append(head.group(2))
    return names


def test_every_kernel_is_defined_in_exactly_one_unit():
    _, units = unit_list()
    src = sources()
    where = {}
    for f, text in src.items():
        for name in kernel_definitions(text):
            where.setdefault(name, []).append(f)
    assert len(where) >= 30 and "td3_fwd_kernel" in where and "cn_replay_copy_kernel" in where and "sac_act_kernel" in where
    for name, files in where.items():
        if name.isupper():                                  # the table's expansions: the kernel file alone
            assert set(files) == {INSTRUMENTED}, (name, files)
        else:
            assert len(files) == 1, (name, files)
    # a header may hold a kernel only if a single unit includes it (directly or through another header)

    def includes(f, seen):
        for h in re.findall(r'#include\s+"([^"]+)"', src[f]):
            h = os.path.basename(h)
            if h in src and h not in seen:
                seen.add(h)
                includes(h, seen)
        return seen
    users = {}
    for f in {u[2] for u in units}:
        for h in includes(f, set()):
            users.setdefault(h, set()).add(f)
    for name, files in where.items():
        for f in files:
            assert f.endswith(".hip") or len(users.get(f, ())) <= 1, (name, f, sorted(users[f]))


def test_the_gemm_tile_sizes_are_written_once_on_the_host():
    src = sources()
    for var, sizes in (("TI", "{16, 16, 32}"), ("TJ", "{16, 32, 32}")):
        # a definition of the name, scalar or table (both spellings have existed), and the table's values
        defs = [(f, m.group(0)) for f, text in src.items() for m in re.finditer(r"\b%s\b\s*(?:\[\s*\d*\s*\])?\s*=(?!=)" % var, text)]
        assert len(defs) == 1 and defs[0][0] == "crowdnav_gemm.hip", (var, defs)
        assert [f for f, text in src.items() if sizes in text] == ["crowdnav_gemm.hip"], (var, sizes)
    gemm = src["crowdnav_gemm.hip"]
    body = gemm[gemm.index("dim3 gemm_grid(int mode"):]
    body = body[:body.index("\n}\n")]
    assert "TI[3] = {16, 16, 32}" in body and "TJ[3] = {16, 32, 32}" in body
    # both users go through it: the solo launcher in the same file, the population's create in crowdnav_td3.hip
    assert gemm.count("gemm_grid(") == 2 and src["crowdnav_td3.hip"].count("gemm_grid(") == 1
    assert sorted(f for f, text in src.items() if "gemm_grid(" in text) == ["crowdnav_gemm.hip", "crowdnav_learner.h", "crowdnav_td3.hip"]
