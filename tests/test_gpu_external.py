"""cn_observe_external beyond one robot and one call per step: the documented surface a reference maintainer drives with Gazebo's or
a physical robot's /scan and /odom, held to the REFERENCE's own goldens and to the oracle, bit for bit.

A. cn_external_io.phase: the pieces of Env.step (CN_PHASE_PRE, CN_PHASE_GET_STATE, CN_PHASE_REWARD; ENV:1208-1223) launched one by one,
   or in every other grouping, leave what the one call leaves -- outputs, counters and the whole state record -- and what the
   reference returned; each piece touches only what is its own; crowdnav.env.Env's append_agent_pose / get_state / compute_reward,
   built on these calls, return the reference's lists; the four refusals.
B. 67 robots in one call (more than a wavefront has lanes, no multiple of 4): the robot fed a golden's messages returns the golden
   whatever its row, its neighbours are fed other messages and other step counters, and a robot's row equals a handle of its own.
C. tools/fuzz_external.py's randomised soak inside the gate, count-bound, with no allowance: 24 worlds x 16 robots x 60 calls."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_external  # noqa: E402
from test_external_worlds_helpers import (COUNTS_ITS_OWN_STEPS, ENDINGS, PHASE_GOLDENS, SOAK_CALLS, SOAK_ROBOTS, SOAK_WORLDS,  # noqa: E402
                                          load_golden, soak_worlds)
from test_gpu_parity import _assert_golden_cp  # noqa: E402

pytestmark = pytest.mark.gpu

PRE, GET_STATE, REWARD = 1, 2, 4
KERNEL = dict(train20="cn_env_kernel_ext", py2tie="cn_env_kernel_ext", goal8="cn_env_kernel_ext", timeout="cn_env_kernel_ext",
              orig20="cn_env_kernel_orig_ext", orig_goal="cn_env_kernel_orig_ext", rw20="cn_env_kernel_rw_ext",
              rw_goal="cn_env_kernel_rw_ext", wide_tracks="cn_env_kernel_wide_ext")
_GOLDEN = {}


def _golden(name, oracle_mod=None):
    """(arrays of the golden, its configuration, the reward to hold each call to).  The reward is the reference's, except in
    wide_tracks: the CPU oracle's for the same call, for the reason test_gpu_wide_tracker.py::_check_call gives."""
    if name not in _GOLDEN:
        z, kw = load_golden(name)
        z = {k: z[k] for k in z.files}
        reward = z["reward"]
        if name == "wide_tracks":
            o = oracle_mod.Oracle(n_envs=1, **{k: v for k, v in kw.items() if k != "track_capacity"})
            reward = np.zeros(len(z["now"]))
            for i in range(len(z["now"])):
                odom = _odom(z, i, 0)
                inp = {k: float(odom[j]) for j, k in enumerate(fuzz_external.ODOM_KEYS)}
                reward[i] = o.ext_call(0, z["ranges"][i], step_counter=int(z["step_counter"][i]), is_reset=int(z["is_reset"][i]), **inp)[1]
                if z["is_reset"][i]:
                    o.ext_set_done(0, False)
        _GOLDEN[name] = (z, kw, reward)
    return _GOLDEN[name]


def _odom(z, i, layout):
    """the odom row of recorded call i, as the golden replays of test_gpu_parity.py build it (layout 1 records no deque)"""
    if layout == 1:
        return [z["px"][i], z["py"][i], z["yaw"][i], z["v"][i], z["w"][i], z["now"][i], 0.0, 0.0, 0.0, 0.0]
    return [z["px"][i], z["py"][i], z["yaw"][i], z["v"][i], z["w"][i], z["now"][i], z["deque_x"][i], z["deque_y"][i], z["end_timestep"][i], 0.0]


def _handle(kw, n=1):
    from crowdnav import Config
    from crowdnav.env import VecEnv
    env = VecEnv(Config(n_envs=n, **kw))
    env.enable_f64_obs()
    return env


def _call(env, z, i, phase=0, counter=True):
    """recorded call i on an N = 1 handle.  A reset call is the same whatever `phase` says (phase only applies to the step flow);
    a launch without CN_PHASE_GET_STATE gets ranges of zeros, as Env.append_agent_pose / compute_reward pass them."""
    layout = env.cfg.obs_layout
    is_reset = bool(z["is_reset"][i])
    phase = 0 if is_reset else phase
    ranges = z["ranges"][i][None, :] if phase == 0 or phase & GET_STATE else np.zeros((1, env.R))
    env.observe_external(ranges, [_odom(z, i, layout)], step_counter=[int(z["step_counter"][i])] if counter else None,
                         is_reset=is_reset, phase=phase)


def _assert_golden(env, z, reward, name, i, row=0):
    """what the reference returned at call i, the comparison of test_golden_replay_through_the_kernel (layout 0),
    test_original_layout_golden_replay_and_run (1) and test_realworld_layout_golden_replay_and_run (2), plus the float32 observation"""
    import torch
    torch.cuda.synchronize()
    layout = env.cfg.obs_layout
    og = env.obs_f64[row].cpu().numpy()
    assert np.array_equal(og, z["obs"][i]), (name, i, np.nonzero(og != z["obs"][i])[0][:8])
    assert np.array_equal(env.obs[row].cpu().numpy(), z["obs"][i].astype(np.float32)), (name, i)
    if not z["is_reset"][i]:
        assert float(env.reward[row].item()) == reward[i] and bool(env.done[row].item()) == bool(z["done"][i]), (name, i)
    c = env.counters()[row].cpu().tolist()
    if layout != 0:
        assert (bool(c[4]), bool(c[5])) == tuple(bool(x) for x in z["status"][i]), (name, i)
    if layout == 1:
        return
    d = env.debug_env(row)
    n = int(z["n_tracks"][i])
    assert d["n_tracks"] == n, (name, i)
    assert np.array_equal(d["track_pose"], z["track_pose"][i][:n]) and np.array_equal(d["track_dist"], z["track_dist"][i][:n]), (name, i)
    assert np.array_equal(d["track_vel"], z["track_vel"][i][:n]), (name, i)
    assert d["bb"] == z["bb"][i], (name, i)
    if layout == 2:
        assert d["collision_prob"] == z["collision_prob"][i], (name, i)
        assert tuple(c[:2]) == tuple(int(x) for x in z["counters"][i]), (name, i)
        return
    assert np.array_equal(d["track_speed"], z["track_speed"][i][:n]), (name, i)
    _assert_golden_cp(d, z, name, i)
    assert np.array_equal(d["wp"], z["wp"][i]), (name, i)
    assert tuple(c[:3]) == tuple(int(x) for x in z["counters"][i]), (name, i)


def _hdr():
    from crowdnav import _abi
    return _abi.C.sizeof(_abi.CnSnapshotHeader)


def _assert_same(a, b, where):
    """two handles left the same outputs, counters and state records (byte for byte after the snapshot header)"""
    import torch
    torch.cuda.synchronize()
    for k in ("obs_f64", "obs", "reward", "done", "topk_idx"):
        assert torch.equal(getattr(a, k), getattr(b, k)), (k, where)
    assert torch.equal(a.counters(), b.counters()), where
    assert bytes(a.snapshot()[_hdr():]) == bytes(b.snapshot()[_hdr():]), where


SENTINEL = dict(obs_f64=-777.25, obs=-777.25, reward=-777.25, done=0xA5, topk_idx=-7)


def _fill_sentinels(env):
    saved = {k: getattr(env, k).clone() for k in SENTINEL}
    for k, v in SENTINEL.items():
        getattr(env, k).fill_(v)
    return saved


def _assert_sentinels(env, where, but=()):
    import torch
    torch.cuda.synchronize()
    for k, v in SENTINEL.items():
        if k not in but:
            assert bool((getattr(env, k) == v).all().item()), (k, where)


def _put_back(env, saved):
    for k, v in saved.items():
        getattr(env, k).copy_(v)


def _assert_pre_changed_only_its_own(before, after, z, i, layout):
    """CN_PHASE_PRE alone is the /odom callback (ENV:239-243: pose, twist, and the clock get_state reads), the deque append and
    agent_vel_timestep (ENV:1208-1209) and the step count: every other field of the state record is as it was"""
    from crowdnav import _abi
    _, a = _abi.split_snapshot(before)
    _, b = _abi.split_snapshot(after)
    SD, SI = _abi.SD, _abi.SI
    own = dict(sd=[SD[k] for k in ("RX", "RY", "RYAW", "RV", "RW", "CLOCK", "DQ0X", "DQ0Y", "DQ1X", "DQ1Y", "TS")],
               si=[SI[k] for k in ("DQ_LEN", "EP_STEP")])
    for k in a:
        x, y = (np.delete(a[k], own[k], axis=1), np.delete(b[k], own[k], axis=1)) if k in own else (a[k], b[k])
        assert x.tobytes() == y.tobytes(), (k, i)
    assert b["si"][0, SI["EP_STEP"]] == a["si"][0, SI["EP_STEP"]] + 1, i
    assert b["si"][0, SI["DQ_LEN"]] == min(2, a["si"][0, SI["DQ_LEN"]] + 1), i
    od = _odom(z, i, layout)
    assert b["sd"][0, SD["TS"]] == od[8] and tuple(b["sd"][0, :6]) == tuple(od[:6]), i


REWARD_LEAVES = ("n_tracks", "n_confirmed", "n_entries", "track_pose", "track_dist", "track_speed", "track_vel", "track_t", "track_dqlen", "bb")


def _assert_reward_left_the_tables(d1, d2, z, i, layout):
    """CN_PHASE_REWARD alone (compute_reward, ENV:1046-1162) leaves the tracker and confirmed-object tables and the deque as get_state
    left them.  The waypoint too, except on the calls where the reference's own compute_reward moves it (ENV:1109-1125: the robot
    has reached it), which the golden's wp of this call against the call before names."""
    from crowdnav import _abi
    for k in REWARD_LEAVES:
        assert np.array_equal(d1[k], d2[k], equal_nan=True), (k, i)
    SD, SI = _abi.SD, _abi.SI
    for k in ("DQ0X", "DQ0Y", "DQ1X", "DQ1Y", "TS"):
        assert d1["sd"][SD[k]] == d2["sd"][SD[k]], (k, i)
    assert d1["si"][SI["DQ_LEN"]] == d2["si"][SI["DQ_LEN"]] and d1["si"][SI["EP_STEP"]] == d2["si"][SI["EP_STEP"]], i
    if layout != 0 or np.array_equal(z["wp"][i], z["wp"][i - 1]):
        assert d1["wp"] == d2["wp"], i


# ---- A. the pieces of Env.step equal the whole ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PHASE_GOLDENS)
def test_pre_get_state_reward_one_by_one_equal_the_whole_flow(oracle_mod, name):
    """One golden per external kernel plus the terminal endings, two handles side by side: `whole` gets every recorded call with
    phase = 0, `split` gets every step call as three launches -- CN_PHASE_PRE with the odom row and ranges of zeros,
    CN_PHASE_GET_STATE with the ranges, CN_PHASE_REWARD with zeros again (it reads none).  After every call the two hold the same
    outputs, counters and state records, and what the reference returned.

    The pieces: a PRE-only launch leaves all four outputs untouched (sentinels, on the first step of every episode and every 37th
    call) and changes the deque, time-step, step-count and /odom fields of the state record only; after GET_STATE alone `done` is
    the observation's own (ENV:1011-1023, 1044) -- the reference raises it in get_state for all three endings (collision, goal,
    step_counter >= max_steps) and compute_reward only hands on the `done` it was given (ENV:1046, 1162), so it equals the
    golden's final `done` at every call, at the endings tests/test_external_worlds_helpers.py::ENDINGS names in goal8 / timeout
    included -- and leaves `reward` untouched; a REWARD-only launch leaves the tables as GET_STATE left them."""
    import torch
    z, kw, reward = _golden(name, oracle_mod)
    whole, split = _handle(kw), _handle(kw)
    assert whole.kernel_name("external") == KERNEL[name]
    layout = whole.cfg.obs_layout
    T = len(z["now"])
    n_pre_checked, ended = 0, {}
    for i in range(T):
        _call(whole, z, i)
        if z["is_reset"][i]:
            _call(split, z, i)
        else:
            probe = bool(z["is_reset"][i - 1]) or i % 37 == 5
            if probe:
                torch.cuda.synchronize()
                before, saved = split.snapshot(), _fill_sentinels(split)
            _call(split, z, i, PRE)
            if probe:
                _assert_sentinels(split, (name, i, "PRE"))
                _assert_pre_changed_only_its_own(before, split.snapshot(), z, i, layout)
                _put_back(split, saved)
                n_pre_checked += 1
                split.reward.fill_(SENTINEL["reward"])
            _call(split, z, i, GET_STATE)
            torch.cuda.synchronize()
            if probe:
                assert float(split.reward[0].item()) == SENTINEL["reward"], (name, i)
            assert bool(split.done[0].item()) == bool(z["done"][i]), (name, i, "done after get_state")
            assert np.array_equal(split.obs_f64[0].cpu().numpy(), z["obs"][i]), (name, i, "state after get_state")
            if z["done"][i]:
                ended[i] = bool(split.done[0].item())
            d1 = split.debug_env(0)
            _call(split, z, i, REWARD)
            torch.cuda.synchronize()
            _assert_reward_left_the_tables(d1, split.debug_env(0), z, i, layout)
        _assert_same(split, whole, (name, i))
        _assert_golden(split, z, reward, name, i)
        _assert_golden(whole, z, reward, name, i)
    assert n_pre_checked >= int(np.sum(z["is_reset"])) - 1
    if name in ENDINGS:
        assert ended == {i: True for i in ENDINGS[name]}, ended
    whole.close(); split.close()


GROUPINGS = {"pre+get_state, reward": (PRE | GET_STATE, REWARD), "pre, get_state+reward": (PRE, GET_STATE | REWARD), "all three bits": (7,)}


@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
@pytest.mark.parametrize("name", ["train20", "orig20"])
def test_other_groupings_of_the_phases_equal_the_whole_flow(name, grouping):
    """PRE|GET_STATE then REWARD; PRE then GET_STATE|REWARD; phase = 7 in one launch: each equals phase = 0 and the reference"""
    z, kw, reward = _golden(name)
    whole, other = _handle(kw), _handle(kw)
    for i in range(len(z["now"])):
        _call(whole, z, i)
        for ph in ((0,) if z["is_reset"][i] else GROUPINGS[grouping]):
            _call(other, z, i, ph)
        _assert_same(other, whole, (name, grouping, i))
        _assert_golden(other, z, reward, name, i)
    whole.close(); other.close()


@pytest.mark.parametrize("name", COUNTS_ITS_OWN_STEPS)
def test_without_a_step_counter_the_kernel_counts_the_steps(oracle_mod, name):
    """step_counter = NULL: the kernel uses the number of step calls since the last reset, which CN_PHASE_PRE advances.  In the
    goldens where the recorded counter is that number (test_goldens_that_count_their_own_steps: all nine), the whole flow and the three
    launches without a counter leave what the whole flow with the recorded counter leaves."""
    z, kw, reward = _golden(name, oracle_mod)
    ref, whole, split = _handle(kw), _handle(kw), _handle(kw)
    for i in range(len(z["now"])):
        _call(ref, z, i)
        _call(whole, z, i, counter=False)
        for ph in ((0,) if z["is_reset"][i] else (PRE, GET_STATE, REWARD)):
            _call(split, z, i, ph, counter=False)
        _assert_same(whole, ref, (name, i, "whole"))
        _assert_same(split, ref, (name, i, "split"))
    _assert_golden(split, z, reward, name, len(z["now"]) - 1)
    for e in (ref, whole, split):
        e.close()


def test_env_wrapper_pieces_return_the_reference_lists():
    """crowdnav.env.Env the way INTEGRATION.md tells an integrator to drive it: odom_callback -> append_agent_pose -> get_state ->
    compute_reward per recorded step of train20 returns the reference's state list, reward and done, and Env.done follows.  (The
    recorded reset calls go through the handle's external reset flow: Env.reset() is the library simulator's.)"""
    import torch
    from crowdnav.env import Env
    z, kw, reward = _golden("train20")
    env = Env(action_dim=2, max_step=kw["max_steps"], **{k: v for k, v in kw.items() if k != "max_steps"})
    for i in range(len(z["now"])):
        sc = int(z["step_counter"][i])
        if z["is_reset"][i]:
            _call(env._v, z, i)
            torch.cuda.synchronize()
            env.done = False                                                      # TRAIN:116
            assert np.array_equal(env._v.obs_f64[0].cpu().numpy(), z["obs"][i]), i
            continue
        env.odom_callback(z["px"][i], z["py"][i], z["yaw"][i], z["v"][i], z["w"][i], now=z["now"][i])
        env.append_agent_pose(z["deque_x"][i], z["deque_y"][i], z["end_timestep"][i])
        state, done = env.get_state(z["ranges"][i], sc)
        assert isinstance(state, list) and len(state) == 398 and state == z["obs"][i].tolist(), i
        assert done is bool(z["done"][i]) and env.done is done, i
        r, d = env.compute_reward(state, sc, done)
        assert isinstance(r, float) and r == reward[i] and d is bool(z["done"][i]) and env.done is d, i
        assert tuple(env._v.counters()[0, :3].cpu().tolist()) == tuple(int(c) for c in z["counters"][i]), i
    env.shutdown()


def test_phase_refusals_enqueue_nothing():
    """phase = -1, phase = 8, a phase with is_reset = 1, CN_PHASE_REWARD alone without obs_f64: CN_ERR_ARG with its message, and
    nothing is enqueued -- the outputs keep their sentinels and the state record stays as it was"""
    import torch
    from crowdnav import Config, _abi
    from crowdnav.env import VecEnv
    z, kw, reward = _golden("train20")
    env = _handle(kw)
    for i in range(3):
        _call(env, z, i)
    torch.cuda.synchronize()
    before = bytes(env.snapshot())
    _fill_sentinels(env)
    mask = "phase is a mask of CN_PHASE_\\* and only applies to the step flow"
    for phase, is_reset in ((-1, False), (8, False), (GET_STATE, True), (7, True)):
        with pytest.raises(_abi.CrowdNavError, match=mask):
            env.observe_external(z["ranges"][3][None, :], [_odom(z, 3, 0)], step_counter=[3], is_reset=is_reset, phase=phase)
    _assert_sentinels(env, "phase refusals")
    assert bytes(env.snapshot()) == before
    bare = VecEnv(Config(n_envs=1, **kw))                                         # no float64 observation
    assert bare.obs_f64 is None
    for i in range(3):
        _call(bare, z, i)
    torch.cuda.synchronize()
    before = bytes(bare.snapshot())
    for k in ("obs", "reward", "done", "topk_idx"):
        getattr(bare, k).fill_(SENTINEL[k])
    for phase in (REWARD, PRE | REWARD):
        with pytest.raises(_abi.CrowdNavError, match="CN_PHASE_REWARD alone reads the float64 state \\(obs_f64\\)"):
            bare.observe_external(z["ranges"][3][None, :], [_odom(z, 3, 0)], step_counter=[3], phase=phase)
    torch.cuda.synchronize()
    for k in ("obs", "reward", "done", "topk_idx"):
        assert bool((getattr(bare, k) == SENTINEL[k]).all().item()), k
    assert bytes(bare.snapshot()) == before
    bare.observe_external(z["ranges"][3][None, :], [_odom(z, 3, 0)], step_counter=[3], phase=7)   # (accepted without obs_f64)
    torch.cuda.synchronize()
    assert np.array_equal(bare.obs[0].cpu().numpy(), z["obs"][3].astype(np.float32)) and float(bare.reward[0].item()) == reward[3]
    env.close(); bare.close()


# ---- B. many robots per call ------------------------------------------------------------------------------------------------------
N_ROBOTS, LONE = 67, 5
LATE = [j for j in range(N_ROBOTS) if j % 7 == 0 or j == LONE]      # robots whose step counter runs far ahead of the golden's
_BATCH = {}


def _batch_messages(name, oracle_mod):
    """every call of a golden for 67 robots, all degraded by seeded noise (fuzz_external.degrade: ranges x U(0.7, 1.3), poses +
    N(0, 0.05), another step counter -- 1 to 8 ahead, and max_steps - 20 more for robots 0, 5, 7, 14, ..., whose episodes end by the
    counter at their 20th step at the latest where the golden's go on, so a robot that read a neighbour's counter would end with
    it): ranges [T,67,R], odom [T,67,10], step_counter [T,67].  The caller puts the golden into its row.
    One golden is kept at a time, with what a lone handle fed robot 5's messages left behind at every call."""
    import torch
    from crowdnav import _abi
    if name not in _BATCH:
        _BATCH.clear()
        z, kw, reward = _golden(name, oracle_mod)
        layout, T = int(kw.get("obs_layout", 0)), len(z["now"])
        od = np.array([_odom(z, i, layout) for i in range(T)], dtype=np.float64)
        rg, od, sc = fuzz_external.degrade(np.random.default_rng(67), np.repeat(z["ranges"][:, None, :], N_ROBOTS, 1),
                                           np.repeat(od[:, None, :], N_ROBOTS, 1), np.repeat(np.asarray(z["step_counter"])[:, None], N_ROBOTS, 1))
        assert not (rg < 0).any()
        sc[:, LATE] += kw["max_steps"] - 20
        lone, left = _handle(kw), []
        for i in range(T):
            lone.observe_external(rg[i, LONE][None, :], od[i, LONE][None, :], step_counter=sc[i, LONE:LONE + 1], is_reset=bool(z["is_reset"][i]))
            torch.cuda.synchronize()
            _, arrs = _abi.split_snapshot(lone.snapshot())
            left.append(([getattr(lone, k)[0].cpu().numpy().copy() for k in ("obs_f64", "obs", "reward", "done", "topk_idx")] +
                         [lone.counters()[0].cpu().numpy().copy()], {k: arrs[k][0].tobytes() for k in ("sd", "si", "trk")}))
        lone.close()
        _BATCH[name] = (rg, od, sc, left)
    return _BATCH[name]


def _run_batch(oracle_mod, name, r, phases=(0,)):
    import torch
    from crowdnav import _abi
    z, kw, reward = _golden(name, oracle_mod)
    rg, od, sc, left = _batch_messages(name, oracle_mod)
    layout, T = int(kw.get("obs_layout", 0)), len(z["now"])
    rg, od, sc = rg.copy(), od.copy(), sc.copy()
    rg[:, r] = z["ranges"]; od[:, r] = [_odom(z, i, layout) for i in range(T)]; sc[:, r] = z["step_counter"]
    assert (sc[:, np.arange(N_ROBOTS) != r] != sc[:, r:r + 1]).all()
    env = _handle(kw, n=N_ROBOTS)
    assert env.kernel_name("external") == KERNEL[name]
    zeros = np.zeros((N_ROBOTS, env.R))
    for i in range(T):
        for ph in ((0,) if z["is_reset"][i] else phases):
            env.observe_external(rg[i] if ph == 0 or ph & GET_STATE else zeros, od[i], step_counter=sc[i], is_reset=bool(z["is_reset"][i]), phase=ph)
        _assert_golden(env, z, reward, name, i, row=r)
        out, state = left[i]
        for k, want in zip(("obs_f64", "obs", "reward", "done", "topk_idx"), out):
            assert np.array_equal(getattr(env, k)[LONE].cpu().numpy(), want, equal_nan=k.startswith("obs")), (name, i, k)
        assert np.array_equal(env.counters()[LONE].cpu().numpy(), out[5]), (name, i)
        _, arrs = _abi.split_snapshot(env.snapshot())
        for k in state:
            assert arrs[k][LONE].tobytes() == state[k], (name, i, k)
    env.close()


@pytest.mark.parametrize("r", [0, 31, 66])
@pytest.mark.parametrize("name", ["train20", "orig20", "rw20", "wide_tracks"])
def test_golden_robot_among_67_whatever_its_row(oracle_mod, name, r):
    """One external launch of 67 robots per recorded call.  Robot r is fed the golden's messages, the other 66 the same messages
    degraded by seeded noise and with other step counters: row r of every output, its counters and its track table are the
    reference's, exactly as with one robot; and row 5 -- outputs, counters and the robot's state record (scalars and track
    table) -- is what a lone N = 1 handle fed robot 5's messages leaves, call by call.  A robot depends neither on its neighbours
    nor on its place in the [N,R] ranges, the [N,10] odom rows, step_counter[N] and the per-robot outputs."""
    _run_batch(oracle_mod, name, r)


def test_golden_robot_among_67_with_the_three_launches(oracle_mod):
    """the same with every step call as CN_PHASE_PRE, CN_PHASE_GET_STATE, CN_PHASE_REWARD launches of all 67 robots (train20, r = 31)"""
    _run_batch(oracle_mod, "train20", 31, phases=(PRE, GET_STATE, REWARD))


# ---- C. the external soak --------------------------------------------------------------------------------------------------------
def test_randomised_external_soak(oracle_mod):
    """tools/fuzz_external.py inside the gate: the first 24 worlds of seed 1, 16 robots and 60 calls each, the same worlds on every
    machine, through run_world against the oracle fed the same messages.  Bit for bit, with no allowance: float64 and float32
    observation, reward, done, top-K indices (layout 0), counters [:3], status & 7 -- a difference the tool's 1e-12 used to
    forgive fails here.

    A row (robot, call) is left out only by the oracle's own word: from the first call at which ITS status for that robot carries
    bit 1 or 8 (its 64 tracks or its confirmed-object table outgrown; it is no longer the reference) to the end of the world.
    Every world has at least the oracle's 64 track slots (soak_worlds), so the kernel's table is never the smaller one.
    Measured by tests/test_external_worlds_helpers.py on the CPU: 12 of 23 040 rows, 0.05 %, all in one world; the bound is 5 %.

    Clocks neither repeat nor leap here (p_clock_repeat = 0): CN_ST_DT_ZERO rows, where the reference divides by zero and sorts
    NaNs, stay the business of test_gpu_parity.py::test_external_scans_with_nan_zero_inf_and_out_of_range_values (N = 1)."""
    from crowdnav import _abi
    ran = refused = left = compared = 0
    kernels = set()
    for j, world in enumerate(soak_worlds()):
        try:
            bad, kernel, l, c = fuzz_external.run_world(world, SOAK_CALLS)
        except _abi.CrowdNavError as ex:
            assert "cn_create" in str(ex), (world["kw"], ex)           # a combination cn_create refuses, with its reason
            refused += 1
            continue
        ran += 1
        kernels.add(kernel)
        left += l; compared += c
        assert not bad, (j, kernel, bad[:4], world["kw"])
        assert l + c == SOAK_ROBOTS * SOAK_CALLS, j
    print("external soak: %d worlds ran, %d refused; %d of %d rows left out; kernels %s" % (ran, refused, left, left + compared, sorted(kernels)))
    assert ran + refused == SOAK_WORLDS and ran >= 0.8 * SOAK_WORLDS, (ran, refused)
    assert left <= 0.05 * (left + compared), (left, compared)
    assert kernels == {"cn_env_kernel_ext", "cn_env_kernel_wide_ext", "cn_env_kernel_orig_ext", "cn_env_kernel_rw_ext"}, kernels
