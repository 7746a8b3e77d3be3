"""csrc/build.sh's unit list is the only list of the library's compile units: read as text, no compiler and no GPU.  Every *.hip under
csrc/ is in the list, every entry of the list is a file, and the two tools that build a library of their own (tools/profc/build.sh,
tools/ab_build.sh) carry no list of sources: nothing in them can go stale when a subsystem is added."""
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
