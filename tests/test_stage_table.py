"""csrc/crowdnav_stages.h is the only table of the step kernel's stage stamps: read as text, no compiler and no GPU.  The kernel
stamps by the rows' names, the four s_setprio changes of a FAIR kernel are a column of the table, and the profiling tools
(tools/isa_ledger.py and the three that import its parser) keep no table of their own."""
import os
import re
import sys

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_ledger as IL

KERNEL = open(os.path.join(PKG, "csrc", "crowdnav_kernel.hip")).read()
CODE = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", KERNEL, flags=re.S))       # without comments


def test_every_stamp_names_a_row_and_every_row_is_stamped():
    # (the two #define lines have the parameter k inside the parentheses: not stamps)
    env = [a for a in re.findall(r"\bCN_T\(([^()]*)\)", CODE) if a != "k"]
    pol = [a for a in re.findall(r"\bPOL_T\(([^()]*)\)", CODE) if a != "k"]
    assert sorted(env) == sorted("CN_STG_" + s.name for s in IL.stages())            # each row once: no bare number, no stray name
    assert sorted(pol) == sorted("CN_STG_" + s.name for s in IL.stages("CN_POL_STAGES"))
    for s in IL.stages("CN_HWID_SLOTS"):
        assert CODE.count("CN_STG_" + s.name) == 1
    # nothing indexes the timing row with a literal any more
    assert not re.search(r"timing\[[^\]]*\+\s*\d", CODE) and "* 32" not in "".join(re.findall(r"timing\[[^\]]*\]", CODE))


def test_slots_are_distinct_and_below_32():
    env, hw, pol = IL.stages(), IL.stages("CN_HWID_SLOTS"), IL.stages("CN_POL_STAGES")
    assert len(env) == 27 and len(hw) == 2 and len(pol) == 5
    for table in (env, hw + pol):
        slots = [s.slot for s in table]
        assert len(set(slots)) == len(slots) and all(0 <= k < 32 for k in slots)
        assert len({s.name for s in table}) == len(table) and all(s.label for s in table)
    # together they are the 32 slots of a timing row; the only slots two tables share are the two stamps inside the 150 ms advance
    # (one-step kernels) and the policy kernel's first two
    assert {s.slot for s in env + hw + pol} == set(range(32))
    assert {s.name for s in env if s.slot in {p.slot for p in hw + pol}} == {"PHYS_TRIG", "PHYS_PEDS"}
    # today's numbers, in execution order: the timing buffer, cn_debug_set_ablate's cut codes and the committed profiles keep them
    assert [s.slot for s in env] == [0, 1, 27, 28, 20, 21, 22, 23, 24] + list(range(2, 20))
    assert [s.slot for s in pol] == [27, 28, 29, 30, 31]


def test_four_rows_carry_a_fair_level_falling_in_execution_order():
    fair = [(s.slot, s.fair) for s in IL.stages() if s.fair is not None]
    assert fair == [(0, 3), (7, 2), (11, 1), (15, 0)]
    # the kernel takes the levels from the table: the macro holds no stamp number and no level of its own
    macro = re.search(r"#define CN_FAIR_AT\(k\)((?:.*\\\n)*.*)", KERNEL).group(1)
    assert "cn_stage_fair(k)" in macro and not re.search(r"\b(?:[1-9]|1[0-9])\b", macro), macro


def test_the_ledgers_stage_table_follows_the_stamps():
    table = IL.stage_table(IL.SRC)
    lines = [ln for ln, _ in table]
    assert lines == sorted(lines) and len(set(lines)) == len(lines)
    names = [n for _, n in table]
    # every name the ledger and tools/profc/report.py print (the committed profiles/r06/dynamic_ledger.txt is keyed by them)
    assert names == ["sim.peds", "sim.robot", "sim.ticks", "near_peds", "ray.cast", "layout1", "bbox", "tracker", "obs.head",
                     "obs.lidar_setup", "ray.loop", "obs.bbox_deque", "gradients", "flags", "type_machine", "association", "order_split",
                     "prefix", "confirmation", "counters", "gt_entries", "speeds", "cone_topk", "tail", "trk_writeback", "layout2",
                     "reward", "body.setup", "body.load", "body.step", "body.store", "kernel.entry"]
    rows = {s.name for s in IL.stages()}
    assert set(IL.AFTER_OBSERVE) | set(IL.AFTER_BODY) <= rows
    src = KERNEL.split("\n")
    at = dict((n, ln) for ln, n in table)
    for stamp, name in list(IL.AFTER_OBSERVE.items()) + list(IL.AFTER_BODY.items()):
        assert "CN_T(CN_STG_%s);" % stamp in src[at[name] - 1]
    # a helper that several stages call is skipped when an instruction's stage is looked up: each is a function of the file
    for h in IL.HELPERS:
        assert re.search(r"^__device__ __forceinline__ .*?\b%s\(" % h, KERNEL, re.M), h
    assert len(IL.helper_ranges(IL.SRC)) >= len(IL.HELPERS)


def test_cuts_keep_execution_order_and_name_what_a_dropped_stamp_ended():
    every = IL.cuts()
    assert [k for k, _ in every] == [s.slot for s in IL.stages()] and [w for _, w in every] == [s.label for s in IL.stages()]
    some = IL.cuts(keep=set(range(20)))
    assert [k for k, _ in some] == list(range(20))                  # slots 0..19 ascend in execution order
    label = dict(some)
    assert label[1] == "load state" and label[2] == "physics: trig of the step .. twist features" and label[9] == "aliasing"


def test_the_timing_tools_keep_no_table_of_their_own():
    for tool in ("stage_timing.py", "stage_instr.py", "wave_tail.py"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert "import isa_ledger" in text and "isa_ledger.cuts(" in text, tool
        assert not re.search(r"^(NAMES|ORDER)\s*=", text, re.M), tool
        for s in IL.stages():                                       # no label restated, no list of slot numbers
            assert '"%s"' % s.label not in text, (tool, s.label)
        assert not re.search(r"\[\s*0,\s*1,\s*20", text) and not re.search(r"\(\s*20\s*,\s*\"", text), tool
