"""The CPU oracle (oracle/cn_oracle.c) against golden vectors produced by the REFERENCE's own Python
(oracle/make_goldens.py).  Bit-exact: observations, rewards, done flags, safety counters, the track
table and the CP scalars.  CPU only."""
import numpy as np
import pytest

from conftest import load_seq

SEQS = ["train20", "dense100", "eval60", "k4", "geos38",  # geos38: the reference under GEOS <= 3.8 empty-result semantics
        "gazebo20",   # float32 LaserScan.ranges + the diff-drive plugin's wheel-speed ramp (cn_config.scan_f32, wheel_accel)
        # recorded under oracle/make_goldens.py's goal-seeking driver, for the endings random actions never reach
        # (oracle/golden_census.py): success after a way-point chain, the step counter, an empty room; and K = 1 / 16
        "goal8", "timeout", "timeout0", "k1", "k16"]
# py2tie: the reference under Python-2.7 round() (cn_config.py2_round), its sensor data placed on exact decimal ties by
# oracle/make_goldens.py's TieSim -- replay only (the poses it was fed are not the simulator's)
REPLAY_SEQS = SEQS + ["py2tie"]
IN_KEYS = ("deque_x", "deque_y", "end_timestep", "px", "py", "yaw", "v", "w", "now", "step_counter", "is_reset")


@pytest.mark.parametrize("name", REPLAY_SEQS)
def test_sequence_replay_bit_exact(oracle_mod, name):
    z, kw = load_seq(name)
    o = oracle_mod.Oracle(n_envs=1, **kw)
    ncalls = len(z["now"])
    over_k = 0
    for i in range(ncalls):
        inp = {k: (int(z[k][i]) if k in ("step_counter", "is_reset") else float(z[k][i])) for k in IN_KEYS}
        obs, r, d, idx = o.ext_call(0, z["ranges"][i], **inp)
        if inp["is_reset"]:
            o.ext_set_done(0, False)  # TRAIN:116
        else:
            assert r == z["reward"][i], (name, i)
            assert d == bool(z["done"][i]), (name, i)
        assert np.array_equal(obs, z["obs"][i]), (name, i, np.nonzero(obs != z["obs"][i])[0][:8])
        dbg = o.debug(0)
        n = int(z["n_tracks"][i])
        assert dbg["n_tracks"] == n, (name, i)
        assert np.array_equal(dbg["track_pose"], z["track_pose"][i][:n])
        assert np.array_equal(dbg["track_dist"], z["track_dist"][i][:n])
        assert np.array_equal(dbg["track_speed"], z["track_speed"][i][:n])
        assert np.array_equal(dbg["track_vel"], z["track_vel"][i][:n])
        assert dbg["collision_prob"] == z["collision_prob"][i]
        assert dbg["ego_score"] == z["ego_score"][i]
        assert dbg["wp"] == tuple(z["wp"][i])
        assert dbg["bb"] == z["bb"][i]
        assert tuple(o.counters()[0][:3]) == tuple(z["counters"][i])
        over_k += n > o.K
    if name in ("dense100", "eval60", "k4", "geos38", "k1", "k16"):
        assert over_k > 0  # the "keep the K lowest" branch of ENV:882-883 is exercised


def test_py2_round_switch_changes_the_run_on_ties(oracle_mod):
    """The py2tie inputs sit on exact ties (ranges and coordinates on odd multiples of 1/16, a pose 0.625 m from the goal):
    replayed with Python-3 rounding (py2_round = 0) the run must differ from the reference's Python-2.7 one, starting with
    ENV:255's round(np.float64(0.625), 2) = 0.63 (Python 2.7) vs 0.62 (numpy) on the very first call."""
    z, kw = load_seq("py2tie")
    assert kw["py2_round"] == 1
    o = oracle_mod.Oracle(n_envs=1, **dict(kw, py2_round=0))
    differ = 0
    for i in range(len(z["now"])):
        inp = {k: (int(z[k][i]) if k in ("step_counter", "is_reset") else float(z[k][i])) for k in IN_KEYS}
        obs, r, d, idx = o.ext_call(0, z["ranges"][i], **inp)
        if inp["is_reset"]:
            o.ext_set_done(0, False)
        if i == 0:
            assert obs[360] == 0.62 and z["obs"][0][360] == 0.63
        differ += int(not np.array_equal(obs, z["obs"][i]))
    assert differ > 20
    L = oracle_mod.lib()
    try:                                    # the rounding primitive itself: exact ties away from zero, everything else unchanged
        L.cno_set_py2_round(1)
        for x, nd, want in ((0.0625, 3, 0.063), (-0.0625, 3, -0.063), (0.125, 2, 0.13), (0.3125, 3, 0.313), (2.675, 2, 2.67),
                            (0.0624999999, 3, 0.062), (-0.375, 2, -0.38), (1.0005, 3, 1.0)):
            assert L.cno_py_round(x, nd) == want, (x, nd)
        L.cno_set_py2_round(0)
        for x, nd, want in ((0.0625, 3, 0.062), (-0.0625, 3, -0.062), (0.125, 2, 0.12), (0.3125, 3, 0.312), (2.675, 2, 2.67)):
            assert L.cno_py_round(x, nd) == want, (x, nd)
    finally:
        L.cno_set_py2_round(0)


@pytest.mark.parametrize("name", SEQS)
def test_full_simulation_reproduces_reference_run(oracle_mod, name):
    """The oracle's own simulator + Env logic, driven only by the recorded actions, reproduces the
    run the reference made on top of the same simulator (it differs from the replay above in that
    the yaw is not passed through a quaternion)."""
    z, kw = load_seq(name)
    o = oracle_mod.Oracle(n_envs=1, **kw)
    o.set_ped_init(z["ped_init"])
    for i in range(len(z["now"])):
        if z["is_reset"][i]:
            obs = o.reset()[0]
        else:
            obs, r, d, _ = o.step(z["action"][i][None, :], step_counter=[int(z["step_counter"][i])])
            obs = obs[0]
            assert r[0] == z["reward"][i] and bool(d[0]) == bool(z["done"][i]), (name, i)
        assert np.array_equal(obs, z["obs"][i]), (name, i)


def test_function_level_goldens(oracle_mod):
    import ctypes as C
    import os
    from conftest import GOLDEN
    L = oracle_mod.lib()
    g = np.load(os.path.join(GOLDEN, "func.npz"))
    dp = C.POINTER(C.c_double)

    def p(a):
        return a.ctypes.data_as(dp)

    # A5
    for i in range(len(g["scan_in"])):
        out = np.zeros(359)
        L.cno_scan_sanitize(p(np.ascontiguousarray(g["scan_in"][i])), 360, 0.6, p(out))
        assert np.array_equal(out, g["scan_out"][i])
    # A6 + A10
    for i in range(len(g["pts_scan"])):
        out = np.zeros((359, 2))
        L.cno_scan_to_points(p(np.ascontiguousarray(g["pts_scan"][i])), 360, g["pts_pose"][i, 0], g["pts_pose"][i, 1],
                             g["pts_yaw"][i], p(out))
        assert np.array_equal(out, g["pts_out"][i])
        assert L.cno_bbox_size(p(out), 359) == g["bb_out"][i]
    # A9
    for i in range(len(g["wp_agent"])):
        out = np.zeros(2)
        L.cno_waypoint(*g["wp_agent"][i], *g["wp_goal"][i], 0.3, p(out))
        assert np.array_equal(out, g["wp_out"][i]), i
    # the survey's spot values
    out = np.zeros(2)
    L.cno_waypoint(0.75, -0.75, -1.0, 1.0, 0.3, p(out))
    assert np.allclose(out, [0.53787, -0.53787], atol=2e-4)
    L.cno_waypoint(0.9, 0.9, 1.0, 1.0, 0.3, p(out))
    assert tuple(out) == (-1.0, 1.0)  # goal inside -> x sign flipped (UTL:310-312)
    # A22
    n_none = 0
    for i in range(len(g["cp_a0"])):
        d = C.c_double(0.0)
        has = L.cno_collision_point(*g["cp_a0"][i], *g["cp_a1"][i], *g["cp_ob"][i], 0.178, C.byref(d))
        if np.isnan(g["cp_out"][i]):
            assert has == 0, i
            n_none += 1
        else:
            assert has == 1 and d.value == g["cp_out"][i], i
    assert 0 < n_none < len(g["cp_a0"])
    d = C.c_double(0.0)
    assert L.cno_collision_point(0.0, 0.5, -0.03, 0.5, -0.5, 0.5, 0.178, C.byref(d)) == 1
    assert d.value == g["cp_spot"][0] and abs(d.value - 0.39767) < 1e-4
    # A16 / A20
    for i in range(len(g["iou_p1"])):
        u = L.cno_iou(*g["iou_p1"][i], *g["iou_p2"][i], g["iou_s"][i])
        assert u == g["iou_out"][i], i
        assert (u > 0.0) == bool(g["assoc_out"][i])
    assert L.cno_iou(0.0, 0.0, 0.05, 0.0, 0.0505) == 0.338
    # A18
    for dd, e1, e0 in zip(g["est_d"], g["est_out"], g["est_out0"]):
        assert L.cno_estimate_num_obs_scans(dd, 0.6, 0.12) == int(e1)
        assert L.cno_estimate_num_obs_scans(dd, 0.6, 0.0) == int(e0)
    assert [L.cno_estimate_num_obs_scans(x, 0.6, 0.12) for x in (0.6, 0.36, 0.12)] == [3, 17, 32]


def test_function_level_goldens_collision_probability_topk_heading_box_reward(oracle_mod):
    """The rest of SURVEY 8c C3's function vectors: A23 compute_collision_prob (negative and tiny ttc included) and
    compute_general_collision_prob, A24 the top-K rule on lists with ties, A7/A8 heading (with the starting_pose offset)
    and distance, A28 the half-open goal box, A30 the full compute_reward sign table, and A22 get_collision_point
    under GEOS <= 3.8 empty-result semantics (cn_config.geos_untyped_empty)."""
    import ctypes as C
    import os
    from conftest import GOLDEN
    L = oracle_mod.lib()
    g = np.load(os.path.join(GOLDEN, "func.npz"))
    # A23
    for t, want in zip(g["cpttc_in"], g["cpttc_out"]):
        assert L.cno_collision_prob(float(t)) == want
    assert (g["cpttc_out"] < 0).sum() > 100 and L.cno_collision_prob(-1e-9) == 0.15 / -1e-9      # a negative ttc gives a negative score
    for d, want in zip(g["gcp_in"], g["gcp_out"]):
        assert L.cno_general_collision_prob(float(d), 0.6, 0.12) == want
    # A24: K lowest kept, stable among ties
    n_ties = 0
    for row, want in zip(g["topk_cp"], g["topk_idx"]):
        cp = np.ascontiguousarray(row[~np.isnan(row)])
        out = np.full(8, -1, dtype=np.int32)
        kept = L.cno_topk(cp.ctypes.data_as(C.POINTER(C.c_double)), len(cp), 8, out.ctypes.data)
        assert kept == min(8, len(cp)) and np.array_equal(out, want), (cp, out, want)
        n_ties += len(set(cp.tolist())) < len(cp)
    assert n_ties > 50
    # A7 / A8
    o = oracle_mod.Oracle(n_envs=1, n_peds=4)
    for i in range(len(g["hd_pos"])):
        h = L.cno_heading_to_goal(o.h, 0, *g["hd_wp"][i], *g["hd_pos"][i], g["hd_yaw"][i])
        assert abs(h - g["hd_out"][i]) <= 1e-15, i
        assert L.cno_distance_to_goal(*g["hd_pos"][i], *g["hd_wp"][i]) == g["dist_out"][i]
    # A28
    for b, want in zip(g["box_in"], g["box_out"]):
        assert bool(L.cno_in_box(b[0], b[1], -1.0, 1.0, 0.20)) == bool(want)
    assert g["box_out"].sum() > 0 and not g["box_out"][-4:].all()      # the four corners: half-open on two sides
    # A30: every sign combination of heading / distance change, done and not done (robot away from goal and way-point)
    robot = o.sim_state(0)[0]
    seen = set()
    for ch, ph, cd, pd, done, want in g["reward_table"]:
        r = L.cno_compute_reward(o.h, 0, ch, cd, ph, pd, 5.0, 5.0, robot[0], robot[1], int(done))
        assert r == want, (ch, ph, cd, pd, done, r, want)
        seen.add(want)
    assert seen == {-2.0, -1.0, 0.0, -202.0, -201.0, -200.0}
    # A22 under GEOS <= 3.8: the first candidate that misses ends the search with None
    n_none = n_diff = 0
    for i in range(len(g["cp_a0"])):
        d = C.c_double(0.0)
        has = L.cno_collision_point_geos(*g["cp_a0"][i], *g["cp_a1"][i], *g["cp_ob"][i], 0.178, 1, C.byref(d))
        if np.isnan(g["cp_out_geos38"][i]):
            assert has == 0, i
            n_none += 1
        else:
            assert has == 1 and d.value == g["cp_out_geos38"][i], i
        n_diff += np.isnan(g["cp_out_geos38"][i]) != np.isnan(g["cp_out"][i])
    assert n_diff > 100 and n_none < len(g["cp_a0"])          # the switch matters: many typed-empty hits become None
    assert np.array_equal(g["wp_out"], g["wp_out_geos38"])      # UTL:306-312: both branches flip the goal the same way


# ---- obs_layout 1: environment_stage_1_original.py (363 inputs), SURVEY 8f N3 -----------------------------
ORIG_SEQS = ["orig20", "orig60", "orig_goal"]


@pytest.mark.parametrize("name", ORIG_SEQS)
def test_original_layout_replay_bit_exact(oracle_mod, name):
    """get_state / compute_reward of environment_stage_1_original.py on the recorded /scan + /odom (ORIG:278-402):
    observation, reward, done, success / failure flags and the (mislabelled) previous_distance / previous_heading."""
    z, kw = load_seq(name)
    o = oracle_mod.Oracle(n_envs=1, **kw)
    assert o.D == 363
    for i in range(len(z["now"])):
        inp = {k: (int(z[k][i]) if k in ("step_counter", "is_reset") else float(z[k][i]))
               for k in ("px", "py", "yaw", "v", "w", "now", "step_counter", "is_reset")}
        obs, r, d, idx = o.ext_call(0, z["ranges"][i], deque_x=0.0, deque_y=0.0, end_timestep=0.0, **inp)
        if inp["is_reset"]:
            o.ext_set_done(0, False)  # SAC:107
        else:
            assert r == z["reward"][i] and d == bool(z["done"][i]), (name, i)
        assert np.array_equal(obs, z["obs"][i]), (name, i, np.nonzero(obs != z["obs"][i])[0][:8])
        c = o.counters()[0]
        assert (bool(c[4]), bool(c[5])) == tuple(bool(x) for x in z["status"][i]), (name, i)
    assert z["done"].sum() >= 4


@pytest.mark.parametrize("name", ORIG_SEQS)
def test_original_layout_full_simulation_reproduces_reference_run(oracle_mod, name):
    z, kw = load_seq(name)
    o = oracle_mod.Oracle(n_envs=1, **kw)
    o.set_ped_init(z["ped_init"])
    for i in range(len(z["now"])):
        if z["is_reset"][i]:
            obs = o.reset()[0]
        else:
            obs, r, d, _ = o.step(z["action"][i][None, :], step_counter=[int(z["step_counter"][i])])
            obs = obs[0]
            assert r[0] == z["reward"][i] and bool(d[0]) == bool(z["done"][i]), (name, i)
        assert np.array_equal(obs, z["obs"][i]), (name, i)


# ---- obs_layout 2: environment_stage_1_nobonus_realworld.py (370 inputs), SURVEY 8f N3 ------------------------
RW_SEQS = ["rw20", "rw60", "rw_goal"]


@pytest.mark.parametrize("name", RW_SEQS)
def test_realworld_layout_replay_bit_exact(oracle_mod, name):
    """get_state / compute_reward of environment_stage_1_nobonus_realworld.py on the recorded /scan + /odom (RW:208-849):
    observation (unrounded ranges, the one highest-CP obstacle), reward, done, safety counters, the track table, the
    collision probability, bbox size, previous distance / heading."""
    z, kw = load_seq(name)
    o = oracle_mod.Oracle(n_envs=1, **kw)
    assert o.D == 370
    for i in range(len(z["now"])):
        inp = {k: (int(z[k][i]) if k in ("step_counter", "is_reset") else float(z[k][i])) for k in IN_KEYS}
        obs, r, d, idx = o.ext_call(0, z["ranges"][i], **inp)
        if inp["is_reset"]:
            o.ext_set_done(0, False)
        else:
            assert r == z["reward"][i] and d == bool(z["done"][i]), (name, i, r, z["reward"][i])
        assert np.array_equal(obs, z["obs"][i]), (name, i, np.nonzero(obs != z["obs"][i])[0][:8])
        dbg = o.debug(0)
        n = int(z["n_tracks"][i])
        assert dbg["n_tracks"] == n, (name, i)
        assert np.array_equal(dbg["track_pose"], z["track_pose"][i][:n]) and np.array_equal(dbg["track_dist"], z["track_dist"][i][:n])
        assert np.array_equal(dbg["track_speed"], z["track_speed"][i][:n]) and np.array_equal(dbg["track_vel"], z["track_vel"][i][:n])
        assert dbg["collision_prob"] == z["collision_prob"][i] and dbg["bb"] == z["bb"][i], (name, i)
        assert tuple(o.counters()[0][:2]) == tuple(z["counters"][i]), (name, i)
        c = o.counters()[0]
        assert (bool(c[4]), bool(c[5])) == tuple(bool(x) for x in z["status"][i]), (name, i)
    assert z["end_timestep"][1] == 0.15000000000000002          # RW:880-883: 0.05 s held, 0.15 s booked


@pytest.mark.parametrize("name", RW_SEQS)
def test_realworld_layout_full_simulation_reproduces_reference_run(oracle_mod, name):
    z, kw = load_seq(name)
    o = oracle_mod.Oracle(n_envs=1, **kw)
    o.set_ped_init(z["ped_init"])
    for i in range(len(z["now"])):
        if z["is_reset"][i]:
            obs = o.reset()[0]
        else:
            obs, r, d, _ = o.step(z["action"][i][None, :], step_counter=[int(z["step_counter"][i])])
            obs = obs[0]
            assert r[0] == z["reward"][i] and bool(d[0]) == bool(z["done"][i]), (name, i)
        assert np.abs(obs - z["obs"][i]).max() <= 1e-9, (name, i, np.abs(obs - z["obs"][i]).max())


# ---- what the goldens were recorded for: a census of their branches, and proof that they bite on them ----------------------
def test_census_of_the_goldens_recorded_for_success_timeout_and_k_edges():
    """oracle/golden_census.py on the committed files: each of them still holds the branch it was recorded for (the conditions
    oracle/make_goldens.py refuses to write a file without), recomputed here from the recorded columns alone."""
    from oracle import golden_census as gc
    cen = {}
    for name in sorted(gc.REQUIRED):
        z, kw = load_seq(name)
        assert gc.unmet(name, z, kw) == [], name
        cen[name] = gc.census(z, kw)
    # layouts 0 / 1 / 2: at least three arrivals each, status [True, False]
    assert all(cen[n]["success"] >= 3 for n in ("goal8", "orig_goal", "rw_goal"))
    assert (cen["goal8"]["layout"], cen["orig_goal"]["layout"], cen["rw_goal"]["layout"]) == (0, 1, 2)
    # goal8: a success after a chain of at least three way-point bonuses, and a way-point snapped onto the goal (ENV:1121-1123)
    assert max(cen["goal8"]["bonuses_before_success"]) >= 3 and cen["goal8"]["snaps"] >= 1
    # step_counter == max_steps with nothing below min_scan_range, scored as a failure (ENV:1021-1023, 1155-1159; ORIG:311; RW:732)
    assert cen["timeout"]["timeout"] >= 2 and cen["orig_goal"]["timeout"] >= 1 and cen["rw_goal"]["timeout"] >= 1
    # the empty room: no track on any call of an episode that runs to its time limit
    assert cen["timeout0"]["timeout"] >= 1 and cen["timeout0"]["no_tracks"] == cen["timeout0"]["calls"]
    # K = 1 and K = 16: the top-K cut and a short, padded list both occur
    for name, K in (("k1", 1), ("k16", 16)):
        assert cen[name]["K"] == K and cen[name]["over_k"] > 0 and cen[name]["under_k"] > 0, (name, cen[name])
        assert cen[name]["max_tracks"] <= gc.MAXT
    import os
    from conftest import GOLDEN
    for name in gc.REQUIRED:
        assert os.path.getsize(os.path.join(GOLDEN, "seq_%s.npz" % name)) <= 1 << 20, name


def _replay(oracle_mod, z, kw):
    """(obs, reward, done, status) of every call of a layout-0 golden replayed from its recorded sensor inputs under `kw`."""
    o = oracle_mod.Oracle(n_envs=1, **kw)
    out = []
    for i in range(len(z["now"])):
        inp = {k: (int(z[k][i]) if k in ("step_counter", "is_reset") else float(z[k][i])) for k in IN_KEYS}
        obs, r, d, idx = o.ext_call(0, z["ranges"][i], **inp)
        if inp["is_reset"]:
            o.ext_set_done(0, False)
        c = o.counters()[0]
        out.append((obs, r, d, (bool(c[4]), bool(c[5]))))
    return out


def _same(got, z, i):
    obs, r, d, st = got[i]
    return (np.array_equal(obs, z["obs"][i]) and (bool(z["is_reset"][i]) or (r == z["reward"][i] and d == bool(z["done"][i])))
            and st == tuple(bool(x) for x in z["status"][i]))


def test_timeout_golden_bites_on_max_steps(oracle_mod):
    """`timeout` replayed with max_steps + 1: identical up to the first ending, where done, reward and status all differ -- the
    only thing that ended that episode is ENV:1021-1023, and ENV:1155-1159 scored it -200 and episode_failure."""
    from oracle import golden_census as gc
    z, kw = load_seq("timeout")
    end = gc.census(z, kw)["timeout_calls"][0]
    got = _replay(oracle_mod, z, dict(kw, max_steps=kw["max_steps"] + 1))
    assert all(_same(got, z, i) for i in range(end))
    obs, r, d, st = got[end]
    assert bool(z["done"][end]) and not d
    assert r == z["reward"][end] + 200.0
    assert tuple(bool(x) for x in z["status"][end]) == (False, True) and st != (False, True)


def test_goal8_golden_bites_on_the_goal_box(oracle_mod):
    """`goal8` replayed with the goal one box width (2 * goal_eps) further along x: the first recorded success is none there."""
    from oracle import golden_census as gc
    z, kw = load_seq("goal8")
    first = gc.census(z, kw)["first_success"]
    # ENV:1153: goal_reward + non_terminating_reward, the latter at least the step penalty
    assert first > 0 and tuple(bool(x) for x in z["status"][first]) == (True, False) and z["reward"][first] >= 198.0
    got = _replay(oracle_mod, z, dict(kw, goal_x=kw.get("goal_x", -1.0) - 0.4))
    obs, r, d, st = got[first]
    assert not d and st != (True, False) and r != z["reward"][first]
    assert not _same(got, z, first)


def test_k1_golden_bites_on_k(oracle_mod):
    """`k1` replayed with K = 2: everything before the obstacle slots stays what the reference returned, and the tail differs.
    ENV:882-883 keeps `sorted(..., reverse=True)[-K:]`, so with two entries the first slot now holds the second lowest CP
    instead of the lowest, and the second slot a real obstacle instead of nothing."""
    z, kw = load_seq("k1")
    assert kw["k_obstacles"] == 1
    got = _replay(oracle_mod, z, dict(kw, k_obstacles=2))
    first_differs = second_real = 0
    for i in range(len(got)):
        obs, want = got[i][0], z["obs"][i]
        assert len(want) == 370 and len(obs) == 374
        assert np.array_equal(obs[:366], want[:366]), i
        first_differs += int(not np.array_equal(obs[366:370], want[366:370]))
        second_real += int(not np.array_equal(obs[370:374], [obs[361], obs[362], 0.0, 0.0]))     # ENV:273's padding
    assert first_differs > 0 and second_real > 0, (first_differs, second_real)


def test_state_exchange_round_trip_and_first_difference(oracle_mod):
    """SURVEY 8f N4, CPU half: the oracle's state in the product's snapshot layout (cno_get_state / cno_set_state) seeds a
    second oracle that then continues identically; tools/bisect_divergence.first_state_difference names the field that differs."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bisect_divergence import first_state_difference
    kw = dict(n_envs=6, n_peds=30, seed=4, max_steps=25)
    a, b = oracle_mod.Oracle(**kw), oracle_mod.Oracle(**kw)
    a.reset()
    rng = np.random.default_rng(0)
    for t in range(40):
        a.step(np.stack([rng.uniform(0, 0.22, 6), rng.uniform(-2, 2, 6)], 1), auto_reset="next")
    for e in range(6):
        st = a.get_state(e)
        b.set_state(e, st["sd"], st["si"], st["ped_p"], st["ped_v"], st["trk"], a.get_ped_init()[e], None, st["ped_aux"])
        assert first_state_difference(st, b.get_state(e), e) is None
    assert a.get_state(0)["si"][15] > 0 and max(a.get_state(e)["si"][2] for e in range(6)) > 0     # episodes finished, live tracks
    for t in range(30):
        act = np.stack([rng.uniform(0, 0.22, 6), rng.uniform(-2, 2, 6)], 1)
        ra, rb = a.step(act, auto_reset="next"), b.step(act, auto_reset="next")
        assert all(np.array_equal(x, y) for x, y in zip(ra, rb)), t
    for e in range(6):
        assert first_state_difference(a.get_state(e), b.get_state(e), e) is None
    st = a.get_state(2)
    st["ped_p"][7, 1] += 1e-9
    assert first_state_difference(st, b.get_state(2), 2)[0] == "ped_p[7].y"
    st = a.get_state(3)
    st["sd"][6] += 1.0
    assert first_state_difference(st, b.get_state(3), 3)[0] == "sd.WPX"
    st = a.get_state(1)
    st["si"][3] += 1
    assert first_state_difference(st, b.get_state(1), 1) == ("si.EGO_VIOL", int(st["si"][3]), int(st["si"][3]) - 1)


def test_oracle_built_with_the_ub_sanitiser_replays_the_goldens():
    """`make -C oracle ubsan` (-fsanitize=undefined -fno-sanitize-recover): the same source, aborting on the first signed overflow,
    out-of-range float -> int conversion, misaligned or out-of-bounds access ...  The golden replays, the function-level vectors
    and the state round trip of this file run on it in a child interpreter (CN_ORACLE_LIB selects the library oracle.py loads)."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "ubsan"])
    env = dict(os.environ, CN_ORACLE_LIB=os.path.join(ROOT, "oracle", "_build", "libcn_oracle_ubsan.so"),
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "replay_bit_exact or function_level or state_exchange or py2_round"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "runtime error" not in r.stdout
    assert " passed" in r.stdout


def test_two_handles_with_different_py2_round_stepped_from_two_threads():
    """cn_config.py2_round is a property of the handle: the oracle keeps it thread-local and re-reads it from the handle it is
    running (ADVICE r03 / VERDICT r04: it used to be a process global).  The py2tie golden (Python-2.7 rounding, sensor data
    on exact ties) and the same inputs under Python-3 rounding replay CONCURRENTLY from two threads, many times over, and each
    thread's results equal its own single-threaded run."""
    import threading
    from oracle import oracle
    z, kw = load_seq("py2tie")
    n = min(120, len(z["now"]))

    def run(py2):
        k2 = dict(kw); k2["py2_round"] = py2
        o = oracle.Oracle(n_envs=1, **k2)
        out = []
        for i in range(n):
            inp = {k: (int(z[k][i]) if k in ("step_counter", "is_reset") else float(z[k][i])) for k in IN_KEYS}
            obs, rew, done, idx = o.ext_call(0, z["ranges"][i], **inp)
            if inp["is_reset"]:
                o.ext_set_done(0, False)
            out.append((obs.copy(), float(rew), int(done)))
        return out

    ref = {1: run(1), 0: run(0)}
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(ref[0], ref[1]))      # the switch matters on this data
    res, errs = {}, []

    def worker(py2, reps):
        try:
            for _ in range(reps):
                got = run(py2)
                for a, b in zip(got, ref[py2]):
                    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
            res[py2] = True
        except Exception as ex:      # noqa: BLE001
            errs.append((py2, repr(ex)))

    th = [threading.Thread(target=worker, args=(p_, 6)) for p_ in (0, 1)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    assert res == {0: True, 1: True}
