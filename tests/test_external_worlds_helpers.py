"""What tests/test_gpu_external.py builds on, checked without a GPU: the worlds tools/fuzz_external.py draws for the external soak
(deterministic, covering what the soak claims to cover, the oracle the reference in all but a few rows), the degrading of a golden's
messages for the robots around the golden one, and which goldens count their steps the way the kernel does without a step counter."""
import os
import sys

import numpy as np

from conftest import ROOT, load_seq

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_external  # noqa: E402

# the soak of test_gpu_external.py::test_randomised_external_soak: the first SOAK_WORLDS worlds of SOAK_SEED
SOAK_SEED, SOAK_WORLDS, SOAK_ROBOTS, SOAK_CALLS = 1, 24, 16, 60
# goldens whose recorded step_counter[i] is the number of step calls since the last reset call, which is what the kernel counts by
# itself (ep_step) when cn_external_io.step_counter is NULL
COUNTS_ITS_OWN_STEPS = ("train20", "py2tie", "goal8", "timeout", "orig20", "orig_goal", "rw20", "rw_goal", "wide_tracks")
# how the episodes of the two terminal goldens end, by recorded call: the reference's get_state raises `done` for all three (ENV:1011-1023)
ENDINGS = {"goal8": {85: "goal", 172: "goal", 260: "goal", 300: "collision"}, "timeout": {40: "time-out", 81: "time-out", 122: "time-out"}}
PHASE_GOLDENS = ("train20", "py2tie", "goal8", "timeout", "orig20", "orig_goal", "rw20", "rw_goal", "wide_tracks")


def soak_worlds():
    """The worlds of the soak.  The oracle always has 64 track slots and its status word speaks of those; a world drawn with the
    automatic table (track_capacity 0: 32 slots without pedestrians) gets the 64-slot one here, so that the kernel's table is
    never the smaller of the two and the oracle's word alone says when a robot leaves the comparison.  (What a 32-slot table does
    past 32 tracks is test_gpu_parity.py::test_track_table_overflow_is_flagged_and_confined's.)"""
    rng = np.random.default_rng(SOAK_SEED)
    worlds = [fuzz_external.draw(rng, SOAK_ROBOTS, p_clock_repeat=0) for _ in range(SOAK_WORLDS)]
    for w in worlds:
        w["kw"]["track_capacity"] = w["kw"]["track_capacity"] or 64
    return worlds


def steps_since_reset(z):
    """per recorded call: the number of step calls since the last reset call, this one included"""
    n, out = 0, []
    for r in z["is_reset"]:
        n = 0 if r else n + 1
        out.append(n)
    return np.array(out)


def load_golden(name):
    """load_seq for every golden of the external replays; seq_wide_tracks.npz with the configuration test_gpu_wide_tracker.py uses"""
    if name != "wide_tracks":
        return load_seq(name)
    z = np.load(os.path.join(ROOT, "tests", "golden", "seq_wide_tracks.npz"))
    kw = {str(k): float(v) for k, v in zip(z["config_keys"], z["config_vals"])}
    for k in ("n_peds", "n_rays", "k_obstacles", "max_steps", "scan_latency_ms", "settle_ms", "ped_cycle_ms", "seed", "env_index_base"):
        kw[k] = int(kw[k])
    return z, dict(kw, track_capacity=256)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_draw_is_deterministic_and_leaves_the_world_as_drawn(oracle_mod):
    from crowdnav import Config
    a, b = soak_worlds(), soak_worlds()
    assert _same(a, b)
    rng = np.random.default_rng(SOAK_SEED)
    drawn = [fuzz_external.draw(rng, SOAK_ROBOTS, p_clock_repeat=0) for _ in range(SOAK_WORLDS)]
    assert all(_same(x["scene"], y["scene"]) and {k for k in x["kw"] if x["kw"][k] != y["kw"][k]} <= {"track_capacity"} for x, y in zip(a, drawn))
    assert {x["kw"]["track_capacity"] for x in drawn} >= {0, 64} and 0 not in {x["kw"]["track_capacity"] for x in a}
    other = fuzz_external.draw(np.random.default_rng(SOAK_SEED + 1), SOAK_ROBOTS, p_clock_repeat=0)
    assert not _same(a[0], other)
    w = a[5]
    cfg = Config(**w["kw"])
    first = list(fuzz_external.messages(w, cfg, 8))
    assert _same(w, b[5])                                              # messages() copied what it moves
    again = list(fuzz_external.messages(w, cfg, 8))
    assert all(_same(x, y) for x, y in zip(first, again))
    assert first[0][0] is True and first[0][1].shape == (SOAK_ROBOTS, cfg.n_rays) and first[0][2].shape == (SOAK_ROBOTS, 10)
    for is_reset, ranges, odom, sc in first:
        assert not (ranges < 0).any() and sc.dtype == np.int32
        assert (np.diff(np.stack([m[2][:, 5] for m in first]), axis=0) > 0).all()      # p_clock_repeat = 0: no clock repeats
    # the tool's own default does repeat clocks
    w4 = fuzz_external.draw(np.random.default_rng(SOAK_SEED), SOAK_ROBOTS)
    now = np.stack([m[2][:, 5] for m in fuzz_external.messages(w4, Config(**w4["kw"]), 60)])
    assert (np.diff(now, axis=0) == 0).any()


def test_soak_worlds_cover_kernels_rays_k_and_rounding():
    """from the drawn configurations alone: the four external kernels (layout 0 with the table in LDS, layout 0 with the wide table,
    layouts 1 and 2), the four ray counts, K = 1 and K = 16, both roundings"""
    kws = [w["kw"] for w in soak_worlds()]
    kernels = {("wide" if k["track_capacity"] >= 128 else "lds") if k["obs_layout"] == 0 else k["obs_layout"] for k in kws}
    assert kernels == {"lds", "wide", 1, 2}
    assert all(k["track_capacity"] < 128 or k["obs_layout"] == 0 for k in kws)       # (cn_create refuses a wide table elsewhere)
    assert {k["n_rays"] for k in kws} == {181, 360, 500, 720}
    assert {1, 16} <= {k["k_obstacles"] for k in kws}
    assert {k["py2_round"] for k in kws} == {0, 1}
    assert all(k["n_envs"] == SOAK_ROBOTS for k in kws)


def test_oracle_stays_the_reference_in_the_soak_worlds(oracle_mod):
    """the oracle alone through the soak's worlds: the rows its own status word takes out (64 tracks or the confirmed-object table
    outgrown; from that call to the end of the world) are at most 5 % -- 12 of 23 040, 0.05 %, all in world 20.  No world has a table
    smaller than the oracle's 64 slots."""
    left = compared = 0
    for w in soak_worlds():
        bad, kernel, l, c = fuzz_external.run_world(w, SOAK_CALLS, device=False)
        assert bad == [] and kernel is None and l + c == SOAK_ROBOTS * SOAK_CALLS
        left += l; compared += c
        assert w["kw"]["track_capacity"] >= 64
    print("left out %d of %d rows" % (left, left + compared))
    assert (left, left + compared) == (12, 23040)
    assert left <= 0.05 * (left + compared)


def test_degrading_keeps_ranges_in_the_domain():
    """ranges x U(0.7, 1.3): NaN, 0 and inf stay what they are and no range turns negative (the ABI puts those outside the domain);
    poses and step counters move, the clock, the speeds and end_timestep do not; the arguments are left alone"""
    rng = np.random.default_rng(3)
    for name in ("train20", "orig20", "rw20", "wide_tracks"):
        z, kw = load_golden(name)
        rg = np.array(z["ranges"])
        odom = np.stack([z["px"], z["py"], z["yaw"], z["v"], z["w"], z["now"], z["px"], z["py"], z["now"] * 0 + 0.15, z["now"] * 0], 1)
        sc = np.array(z["step_counter"], dtype=np.int32)
        rg0, odom0 = rg.copy(), odom.copy()
        r2, o2, s2 = fuzz_external.degrade(rng, rg, odom, sc)
        assert np.array_equal(rg, rg0, equal_nan=True) and np.array_equal(odom, odom0)
        assert not (r2 < 0).any() and r2.shape == rg.shape
        assert np.array_equal(np.isnan(r2), np.isnan(rg)) and np.array_equal(np.isinf(r2), np.isinf(rg)) and np.array_equal(r2 == 0, rg == 0)
        fin = np.isfinite(rg) & (rg > 0)
        assert (r2[fin] >= 0.7 * rg[fin]).all() and (r2[fin] <= 1.3 * rg[fin]).all() and (r2[fin] != rg[fin]).mean() > 0.99
        assert (o2[:, [0, 1, 2, 6, 7]] != odom[:, [0, 1, 2, 6, 7]]).all() and np.array_equal(o2[:, [3, 4, 5, 8, 9]], odom[:, [3, 4, 5, 8, 9]])
        assert s2.dtype == np.int32 and (s2 != sc).all()


def test_goldens_that_count_their_own_steps():
    """step_counter = NULL makes the kernel count the step calls since the last reset; the goldens it can replay that way"""
    for name in PHASE_GOLDENS:
        z, kw = load_golden(name)
        step = ~np.asarray(z["is_reset"], dtype=bool)
        own = np.array_equal(np.asarray(z["step_counter"])[step], steps_since_reset(z)[step])
        assert own == (name in COUNTS_ITS_OWN_STEPS), name


def test_endings_of_the_terminal_goldens():
    """ENDINGS from the goldens themselves: an episode that ends with the success flag reached the goal; one that ends with the failure
    flag ran out of steps if step_counter >= max_steps and hit something otherwise (a range below min_scan_range, ENV:1011-1015)"""
    for name, want in ENDINGS.items():
        z, kw = load_golden(name)
        got = {}
        for i in np.nonzero(np.asarray(z["done"], dtype=bool) & ~np.asarray(z["is_reset"], dtype=bool))[0]:
            success, failure = (bool(x) for x in z["status"][i])
            assert success != failure, (name, i)
            got[int(i)] = "goal" if success else "time-out" if z["step_counter"][i] >= kw["max_steps"] else "collision"
            assert (np.nanmin(np.where(z["ranges"][i] > 0, z["ranges"][i], np.inf)) < 0.12) == (got[int(i)] == "collision"), (name, i)
        assert got == want, (name, got)
