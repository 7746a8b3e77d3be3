"""CPU checks of tools/bisect_divergence.py::first_state_difference, the one rule every GPU-vs-oracle state comparison uses:
equality everywhere, PREV_HEAD within 1 ulp of its atan2, the CP scalars only where the oracle flags pow, and a fixed list
of slots the two sides legitimately leave different.  A state taken from an oracle run is compared with perturbed copies of itself, so loosening the rule anywhere fails here first."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_seq

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bisect_divergence as bd  # noqa: E402

SD = {n: k for k, n in enumerate(bd.SD_NAMES)}
SI = {n: k for k, n in enumerate(bd.SI_NAMES)}
TF = {n: k for k, n in enumerate(bd.TF_NAMES)}


@pytest.fixture(scope="module")
def state(oracle_mod):
    """an env of a crowded oracle run with tracks, a two-entry agent deque, a track whose deque holds one entry and one
    that holds two, and a nonzero ego score"""
    from crowdnav import Config
    cfg = Config(n_envs=16, n_peds=20, seed=11, max_steps=60)
    orc = oracle_mod.Oracle(cfg.as_dict())
    orc.reset()
    rng = np.random.default_rng(0)
    for t in range(40):
        act = np.stack([rng.uniform(0, 0.22, 16), rng.uniform(-2, 2, 16)], 1)
        orc.step(act, auto_reset="next")
        for e in range(16):
            s = orc.get_state(e)
            nt = int(s["si"][SI["NTRACKS"]])
            dql = s["trk"][:nt, TF["DQLEN"]]
            if (s["si"][SI["DQ_LEN"]] >= 1 and nt >= 2 and (dql == 1).any() and (dql == 2).any() and s["sd"][SD["EGO"]] != 0
                    and s["sd"][SD["PREV_HEAD"]] != 0 and s["trk"][:nt, TF["SPEED"]].max() > 0):
                return s
    pytest.fail("no env of the run has the slots this test perturbs")


def _copy(s):
    return {k: np.array(v, copy=True) for k, v in s.items()}


def _ulp(x, n=1):
    for _ in range(n):
        x = np.nextafter(x, np.inf)
    return x


def test_identical_state_has_no_difference(state):
    assert bd.first_state_difference(_copy(state), state, 0) is None


@pytest.mark.parametrize("field", ["EGO", "CPROB", "EP_RETURN", "PREV_DIST", "RX"])
def test_one_ulp_in_an_sd_field_is_reported(state, field):
    g = _copy(state)
    g["sd"][SD[field]] = _ulp(g["sd"][SD[field]])
    d = bd.first_state_difference(g, state, 0)
    assert d is not None and d[0] == "sd." + field


@pytest.mark.parametrize("field", ["EGO", "CPROB"])
def test_cp_scalars_may_differ_only_where_the_oracle_flags_the_c_librarys_pow(state, field):
    """an ego score / collision probability that differs is reported unless the oracle flags the step (cp_pow_sq: pow(v, 2) !=
    v * v for the agent's velocity); the flag excuses nothing else"""
    assert state["cp_pow_sq"] == 0
    g, o = _copy(state), _copy(state)
    g["sd"][SD[field]] = _ulp(g["sd"][SD[field]], 3)
    assert bd.first_state_difference(g, o, 0)[0] == "sd." + field
    o["cp_pow_sq"] = np.array(1)
    assert bd.first_state_difference(g, o, 0) is None
    for other in ("EP_RETURN", "RX", "PREV_DIST"):
        g2 = _copy(g)
        g2["sd"][SD[other]] = _ulp(g2["sd"][SD[other]])
        assert bd.first_state_difference(g2, o, 0)[0] == "sd." + other
    g2 = _copy(g)
    g2["trk"][0, TF["SPEED"]] = _ulp(g2["trk"][0, TF["SPEED"]])
    assert bd.first_state_difference(g2, o, 0)[0] == "trk[0].SPEED"


def test_one_ulp_in_a_track_speed_is_reported(state):
    g = _copy(state)
    t = int(np.argmax(g["trk"][:int(g["si"][SI["NTRACKS"]]), TF["SPEED"]]))
    g["trk"][t, TF["SPEED"]] = _ulp(g["trk"][t, TF["SPEED"]])
    assert bd.first_state_difference(g, state, 0)[0] == "trk[%d].SPEED" % t


@pytest.mark.parametrize("what", ["ped_p", "ped_v"])
def test_one_ulp_in_a_pedestrian_coordinate_is_reported(state, what):
    g = _copy(state)
    g[what][7, 1] = _ulp(g[what][7, 1])
    assert bd.first_state_difference(g, state, 0)[0] == "%s[7].y" % what


def test_an_integer_field_is_reported(state):
    g = _copy(state)
    g["si"][SI["EGO_VIOL"]] += 1
    assert bd.first_state_difference(g, state, 0)[0] == "si.EGO_VIOL"


def test_prev_head_one_ulp_passes_two_ulps_do_not(state):
    """PREV_HEAD = atan2(...) - yaw may differ by one ulp of the atan2 result (np.spacing(pi) for results in [2, pi]), not two"""
    assert bd.ATAN2_ULP == np.spacing(np.pi) == 2.0 ** -51
    h = state["sd"][SD["PREV_HEAD"]]
    for delta in (bd.ATAN2_ULP, -bd.ATAN2_ULP, float(np.spacing(h))):
        g = _copy(state)
        g["sd"][SD["PREV_HEAD"]] = h + delta
        assert g["sd"][SD["PREV_HEAD"]] != h and bd.first_state_difference(g, state, 0) is None, delta
    for delta in (2 * bd.ATAN2_ULP, -2 * bd.ATAN2_ULP):
        g = _copy(state)
        g["sd"][SD["PREV_HEAD"]] = h + delta
        assert bd.first_state_difference(g, state, 0)[0] == "sd.PREV_HEAD", delta
    g = _copy(state)
    for sign in (np.inf, -np.inf):              # two ulps of a heading in [2, pi] (the atan2's own binade)
        o = _copy(state)
        o["sd"][SD["PREV_HEAD"]] = 2.5
        g["sd"][SD["PREV_HEAD"]] = _ulp(2.5) if sign > 0 else np.nextafter(2.5, 0)
        assert bd.first_state_difference(g, o, 0) is None
        g["sd"][SD["PREV_HEAD"]] = np.nextafter(g["sd"][SD["PREV_HEAD"]], sign)
        assert bd.first_state_difference(g, o, 0)[0] == "sd.PREV_HEAD"
    g = _copy(state)
    g["sd"][SD["PREV_HEAD"]] = np.nan
    assert bd.first_state_difference(g, state, 0)[0] == "sd.PREV_HEAD"


def test_nan_matches_nan(state):
    g, o = _copy(state), _copy(state)
    for s in (g, o):
        s["sd"][SD["EGO"]] = np.nan
        s["trk"][0, TF["SPEED"]] = np.nan
        s["ped_v"][3, 0] = np.nan
    assert bd.first_state_difference(g, o, 0) is None
    o["sd"][SD["EGO"]] = 0.0
    assert bd.first_state_difference(g, o, 0)[0] == "sd.EGO"


def test_only_the_skipped_slots_changed(state):
    g = _copy(state)
    nt = int(g["si"][SI["NTRACKS"]])
    one = int(np.nonzero(g["trk"][:nt, TF["DQLEN"]] == 1)[0][0])
    g["trk"][one, TF["D1X"]] += 1.0                  # the stale second deque entry of a one-entry track
    g["trk"][one, TF["D1Y"]] -= 1.0
    g["trk"][nt:, :] = 123.0                         # rows at and beyond NTRACKS
    assert bd.first_state_difference(g, state, 0) is None
    two = int(np.nonzero(g["trk"][:nt, TF["DQLEN"]] == 2)[0][0])
    g["trk"][two, TF["D1X"]] = _ulp(g["trk"][two, TF["D1X"]])        # ... but not a live second entry
    assert bd.first_state_difference(g, state, 0)[0] == "trk[%d].D1X" % two
    # gt mode (risk_mode 1): the deque fields of the tracks are not compared, the rest is
    g = _copy(state)
    for f in ("D0X", "D0Y", "D1X", "D1Y", "DQLEN"):
        g["trk"][:nt, TF[f]] += 0.5
    assert bd.first_state_difference(g, state, 0, risk_mode=1) is None
    assert bd.first_state_difference(g, state, 0, risk_mode=0) is not None
    g["trk"][0, TF["PX"]] = _ulp(g["trk"][0, TF["PX"]])
    assert bd.first_state_difference(g, state, 0, risk_mode=1)[0] == "trk[0].PX"
    # the agent deque entries beyond DQ_LEN
    g, o = _copy(state), _copy(state)
    for s in (g, o):
        s["si"][SI["DQ_LEN"]] = 1
    g["sd"][SD["DQ1X"]] += 1.0; g["sd"][SD["DQ1Y"]] += 1.0
    assert bd.first_state_difference(g, o, 0) is None
    g["sd"][SD["DQ0X"]] = _ulp(g["sd"][SD["DQ0X"]])
    assert bd.first_state_difference(g, o, 0)[0] == "sd.DQ0X"
    for s in (g, o):
        s["si"][SI["DQ_LEN"]] = 0
    assert bd.first_state_difference(g, o, 0) is None


def test_py2tie_call_77_is_the_c_librarys_pow():
    """The one recorded call where the kernel's CP scalars differ from the reference's (tests/test_gpu_parity.py::
    test_golden_replay_through_the_kernel[py2tie]): UTL:234 computes the agent's speed as sqrt(math.pow(vx, 2) + math.pow(vy, 2)),
    and the C library's pow is not correctly rounded.  At call 77 vx = (0.371 - 0.438) / ts = -0.44666666666666566, whose exact
    square lies 0.49991 ulp above the rounded product vx * vx: pow rounds it up, the device's vx * vx (correctly rounded)
    down.  The oracle calls pow like the reference.  Restated here on the host: the speed squared both ways carries the ego
    score to the reference's value and to the kernel's."""
    z, kw = load_seq("py2tie")
    assert kw["py2_round"] == 1
    ts = float(z["end_timestep"][77])
    dq0 = (0.438, -0.457)                           # call 76's agent position and call 77's, rounded to mm (ENV:1208)
    dq1 = tuple(round(v + math.copysign(1e-12, v), 3) for v in (float(z["deque_x"][77]), float(z["deque_y"][77])))
    assert dq1 == (0.371, -0.438)
    vx, vy = (dq1[0] - dq0[0]) / ts, (dq1[1] - dq0[1]) / ts
    assert vx == -0.44666666666666566 and math.pow(vx, 2) != vx * vx and math.pow(vy, 2) == vy * vy
    speed = float(z["track_speed"][77][0])          # obstacle_vel = the first track's speed (ENV:787-793)
    dcp = 0.05379211991178494                       # distance to the collision point of the tracks at (0.503, -0.243)

    def ego(sq):
        return min(1.0, 0.15 / (dcp / (math.sqrt(sq(vx) + sq(vy)) - speed)))
    assert ego(lambda x: math.pow(x, 2)) == z["ego_score"][77] == 0.28606987975734355
    assert ego(lambda x: x * x) == 0.2860698797573434


def test_the_oracle_flags_the_c_librarys_pow_on_exactly_the_misrounded_squares(oracle_mod):
    """cn_oracle.c agent_speed's flag (cp_pow_sq, the one excuse first_state_difference has for the CP scalars): on py2tie it is
    raised by call 77 and by no earlier call; the squares behind it are the ones math.pow misrounds"""
    z, kw = load_seq("py2tie")
    o = oracle_mod.Oracle(n_envs=1, **kw)
    keys = ("deque_x", "deque_y", "end_timestep", "px", "py", "yaw", "v", "w", "now", "step_counter", "is_reset")
    flagged = []
    for i in range(78):
        inp = {k: (int(z[k][i]) if k in ("step_counter", "is_reset") else float(z[k][i])) for k in keys}
        o.ext_call(0, z["ranges"][i], **inp)
        if inp["is_reset"]:
            o.ext_set_done(0, False)
        if o.get_state(0)["cp_pow_sq"]:
            flagged.append(i)
    assert flagged == [77]
    assert o.debug(0)["ego_score"] == 0.28606987975734355
