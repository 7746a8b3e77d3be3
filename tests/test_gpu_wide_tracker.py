"""The wide tracker table (cn_config.track_capacity 128 ... 1024, the table in HBM) on the GPU.

The reference's track list is an unbounded Python list that survives reset; the LDS table holds 32 / 64 tracks and flags an env that
outgrows it (CN_ST_TRACK_OVERFLOW).  With a wide table the env stays equal to the reference:
  * up to 64 tracks against the CPU oracle (exact there: CNO_MAX_TRACKS = 64), envs the 32-slot table flags included;
  * past 64 tracks against the reference's own Python (tests/golden/seq_wide_tracks.npz, tools/make_wide_tracker_golden.py).
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ST_OVERFLOW, ST_WIDE = 1, 16
# the goal-near-spawn world of test_gpu_parity.py::test_track_table_overflow_is_flagged_and_confined: every episode ends at its first
# step and every reset duplicates tracks, so the track lists grow
WORLD = dict(n_envs=16, n_peds=16, n_rays=361, k_obstacles=3, max_steps=49, room_half=1.1832673565816718, goal_x=0.565634967637293,
             goal_y=0.44034573709026004, spawn_x=0.6050993559998654, spawn_y=0.29646458843154355, spawn_yaw=2.8751215535007932,
             scan_latency_ms=5, settle_ms=50, ped_cycle_ms=1400, ped_vmax=0.2505021742113402, seed=634151950, env_index_base=286355,
             lidar_min=0.0, ped_radius=0.1, start_x=0.7867724988896705, start_y=-0.895986056152086)
INT_KEYS = ("n_peds", "n_rays", "k_obstacles", "max_steps", "scan_latency_ms", "settle_ms", "ped_cycle_ms", "seed", "env_index_base")


def _load_golden():
    z = np.load(os.path.join(GOLDEN, "seq_wide_tracks.npz"))
    kw = {str(k): float(v) for k, v in zip(z["config_keys"], z["config_vals"])}
    for k in INT_KEYS:
        kw[k] = int(kw[k])
    return z, kw


def _replay(env, z, i):
    odom = [z["px"][i], z["py"][i], z["yaw"][i], z["v"][i], z["w"][i], z["now"][i], z["deque_x"][i], z["deque_y"][i],
            z["end_timestep"][i], 0.0]
    env.observe_external(z["ranges"][i][None, :], [odom], step_counter=[int(z["step_counter"][i])], is_reset=bool(z["is_reset"][i]))


IN_KEYS = ("deque_x", "deque_y", "end_timestep", "px", "py", "yaw", "v", "w", "now", "step_counter", "is_reset")


def _oracle_call(o, z, i):
    """The CPU oracle fed the same call (test_oracle_golden.py's replay): its reward."""
    inp = {k: (int(z[k][i]) if k in ("step_counter", "is_reset") else float(z[k][i])) for k in IN_KEYS}
    obs, r, d, idx = o.ext_call(0, z["ranges"][i], **inp)
    if inp["is_reset"]:
        o.ext_set_done(0, False)
    return r


def _check_call(env, z, i, reward=None):
    """What the reference returned at call i, bit for bit, as in test_gpu_parity.py::test_golden_replay_through_the_kernel: the
    observation, the CP scalars, the whole track table and everything else.  The reward is held to `reward` (the CPU oracle's for the same call): in this world
    the reference's reward is 1 higher on the calls where an episode reaches its goal at its first step, in the oracle as in the
    kernel -- a difference of the reward terms that has nothing to do with the tracker and that this table does not change."""
    og = env.obs_f64[0].cpu().numpy()
    assert np.array_equal(og, z["obs"][i]), (i, np.nonzero(og != z["obs"][i])[0][:8])
    if not z["is_reset"][i]:
        assert bool(env.done[0].item()) == bool(z["done"][i]), i
        if reward is not None:
            assert float(env.reward[0].item()) == reward, i
    d = env.debug_env(0)
    n = int(z["n_tracks"][i])
    assert d["n_tracks"] == n, (i, d["n_tracks"], n)
    assert np.array_equal(d["track_pose"], z["track_pose"][i][:n]) and np.array_equal(d["track_dist"], z["track_dist"][i][:n]), i
    assert np.array_equal(d["track_speed"], z["track_speed"][i][:n]) and np.array_equal(d["track_vel"], z["track_vel"][i][:n]), i
    assert d["collision_prob"] == z["collision_prob"][i] and d["ego_score"] == z["ego_score"][i], i
    assert np.array_equal(d["wp"], z["wp"][i]) and d["bb"] == z["bb"][i], i
    assert tuple(env.counters()[0, :3].cpu().tolist()) == tuple(int(c) for c in z["counters"][i]), i
    assert not (d["status"] & ST_OVERFLOW), i
    assert bool(d["status"] & ST_WIDE) == bool(z["n_tracks"][:i + 1].max() > 64), i


@pytest.mark.parametrize("auto_reset", ["next", "same"])
def test_wide_table_equals_the_oracle_past_32_slots(oracle_mod, auto_reset):
    """track_capacity 256 in the overflow world, 160 steps: every env whose ORACLE status has no overflow bit (its list stayed within
    the oracle's 64 slots) equals the oracle bit for bit -- observation, indices, done flags, counters, track count -- including the
    envs a 32-slot handle flags at the same steps.  The wide handle never raises CN_ST_TRACK_OVERFLOW, and its CN_ST_TRACK_WIDE is
    exactly "the oracle overflowed"."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    cfg = Config(track_capacity=256, **WORLD)
    env = VecEnv(cfg)
    env.enable_f64_obs()
    narrow = VecEnv(Config(track_capacity=32, **WORLD))
    assert env.kernel_name("same" if auto_reset == "same" else "step") == ("cn_env_kernel_wide_same" if auto_reset == "same" else "cn_env_kernel_wide")
    orc = oracle_mod.Oracle(cfg.as_dict())
    env.reset(); narrow.reset(); torch.cuda.synchronize(); orc.reset()
    rng = np.random.default_rng(3)
    N = WORLD["n_envs"]
    compared_past_32 = 0
    for t in range(160):
        act = np.stack([rng.uniform(0, 0.22, N), rng.uniform(-2, 2, N)], 1).astype(np.float32)
        a = torch.from_numpy(act).cuda()
        env.step(a, auto_reset=auto_reset); narrow.step(a, auto_reset=auto_reset); torch.cuda.synchronize()
        oc, rc, dc, ic = orc.step(act.astype(np.float64), auto_reset=auto_reset)
        c = env.counters().cpu().numpy()
        ost = np.array([orc.get_state(e)["si"][9] for e in range(N)])
        clean = (ost & ST_OVERFLOW) == 0
        assert not (c[:, 6] & ST_OVERFLOW).any(), t
        assert np.array_equal((c[:, 6] & ST_WIDE) != 0, ~clean), t
        assert np.array_equal(env.obs_f64.cpu().numpy()[clean], oc[clean]), t
        assert np.array_equal(env.topk_idx.cpu().numpy()[clean], ic[clean]) and np.array_equal(env.done.cpu().numpy()[clean], dc[clean]), t
        assert np.array_equal(c[clean, :6], orc.counters()[clean]), t
        assert np.array_equal(c[clean, 7], np.array([orc.get_state(e)["si"][2] for e in range(N)])[clean]), t
        flagged32 = (narrow.counters()[:, 6].cpu().numpy() & ST_OVERFLOW) != 0
        compared_past_32 += int((clean & flagged32).sum())
    assert compared_past_32 > 0, "no env past the 32-slot table was compared"
    assert env.status_counts()["track_overflow"] == 0
    env.close(); narrow.close()


def test_wide_table_replays_the_reference_past_64_tracks(oracle_mod):
    """seq_wide_tracks.npz -- the reference's own Python in a world whose track list grows past 100 tracks -- fed through
    cn_observe_external with track_capacity 256: every call returns what the reference returned, the whole track table included.
    With track_capacity 64 the same replay raises CN_ST_TRACK_OVERFLOW and differs once the reference holds more than 64 tracks."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    z, kw = _load_golden()
    assert z["n_tracks"].max() > 64
    env = VecEnv(Config(n_envs=1, track_capacity=256, **kw))
    env.enable_f64_obs()
    assert env.kernel_name("external") == "cn_env_kernel_wide_ext"
    o = oracle_mod.Oracle(n_envs=1, **kw)
    for i in range(len(z["now"])):
        _replay(env, z, i)
        torch.cuda.synchronize()
        _check_call(env, z, i, reward=_oracle_call(o, z, i))
    env.close()
    # must differ: the 64-slot table
    first = int(np.argmax(z["n_tracks"] > 64))
    env64 = VecEnv(Config(n_envs=1, track_capacity=64, **kw))
    env64.enable_f64_obs()
    differ = 0
    for i in range(len(z["now"])):
        _replay(env64, z, i)
        torch.cuda.synchronize()
        if i < first:
            assert np.array_equal(env64.obs_f64[0].cpu().numpy(), z["obs"][i]), i
        else:
            d = env64.debug_env(0)
            differ += int(d["n_tracks"] != int(z["n_tracks"][i]) or not np.array_equal(env64.obs_f64[0].cpu().numpy(), z["obs"][i]))
    assert env64.status_counts()["track_overflow"] == 1
    assert differ > 0
    env64.close()


def test_wide_policy_rollout_and_sequence_equal_step_by_step():
    """cn_rollout_policy (the generic policy kernel with the wide table) leaves exactly what cn_actor_forward -> cn_step leaves, and
    cn_step_sequence exactly what T cn_step calls leave, in the overflow world with track_capacity 256 -- past 32 tracks."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.td3 import Agent
    cfg = Config(track_capacity=256, **dict(WORLD, n_envs=40))
    N, T = cfg.n_envs, 40
    ref, pol, seq = VecEnv(cfg), VecEnv(cfg), VecEnv(cfg)
    assert pol.kernel_name("policy") == "cn_policy_kernel_wide" and seq.kernel_name("sequence") == "cn_env_kernel_seq_wide"
    a_ref, a_pol = [Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=5, memory_size=16) for _ in range(2)]
    for ag in (a_ref, a_pol):
        ag.sync_fused_weights()
    ref.reset(); pol.reset(); seq.reset(); torch.cuda.synchronize()
    D, K = ref.D, ref.K
    act = torch.zeros((N, 2), device="cuda")
    for call in range(3):
        traj = dict(action=torch.zeros((T, N, 2), device="cuda"), obs=torch.zeros((T, N, D), device="cuda"),
                    reward=torch.zeros((T, N), device="cuda"), done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"),
                    topk_idx=torch.zeros((T, N, K), dtype=torch.int32, device="cuda"))
        pol.rollout_policy(a_pol, T, traj=traj)
        torch.cuda.synchronize()
        seq_traj = dict(obs=torch.zeros((T, N, D), device="cuda"), reward=torch.zeros((T, N), device="cuda"),
                        done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"), topk_idx=torch.zeros((T, N, K), dtype=torch.int32, device="cuda"))
        seq.step_sequence(traj["action"].contiguous(), traj=seq_traj)
        for t in range(T):
            a_ref.act_mfma(ref.obs, out=act)
            torch.cuda.synchronize()
            assert torch.equal(traj["action"][t], act), (call, t)
            ref.step(act, auto_reset="next")
            torch.cuda.synchronize()
            for tr in (traj, seq_traj):
                assert torch.equal(tr["obs"][t], ref.obs) and torch.equal(tr["reward"][t], ref.reward), (call, t)
                assert torch.equal(tr["done"][t], ref.done) and torch.equal(tr["topk_idx"][t], ref.topk_idx), (call, t)
        assert a_pol.noise_state() == a_ref.noise_state()
        for other in (pol, seq):
            assert torch.equal(other.counters(), ref.counters()), call
    assert int(ref.counters()[:, 7].max().item()) > 32, "the run never went past the 32-slot table"
    assert ref.status_counts()["track_overflow"] == 0
    for e in (ref, pol, seq):
        e.close()


def test_wide_capacity_boundaries_snapshot_and_debug_view():
    """cn_create accepts 128 / 256 / 512 / 1024 and refuses 96, 2048, -1 (naming the allowed set), and a wide table in gt mode or
    another observation layout (naming why).  A wide handle's snapshot restores onto a fresh wide handle and the two continue
    equal (the golden replay, past 64 tracks); a 64-slot handle refuses it.  debug_env returns every track past 64."""
    import torch
    from crowdnav import Config
    from crowdnav import _abi
    from crowdnav.env import VecEnv
    small = dict(n_envs=2, n_peds=4, max_steps=10, seed=1)
    for cap in (128, 256, 512, 1024):
        e = VecEnv(Config(track_capacity=cap, **small))
        assert e.track_capacity == cap and e.kernel_name() == "cn_env_kernel_wide"
        e.reset(); e.step(torch.zeros((2, 2), device="cuda"), auto_reset="next"); torch.cuda.synchronize()
        e.close()
    for cap in (96, 2048, -1):
        with pytest.raises(_abi.CrowdNavError, match="track_capacity must be one of"):
            VecEnv(Config(track_capacity=cap, **small))
    with pytest.raises(_abi.CrowdNavError, match="risk_mode lidar_tracker"):
        VecEnv(Config(track_capacity=256, risk_mode=1, **small))
    with pytest.raises(_abi.CrowdNavError, match="obs_layout 0"):
        VecEnv(Config(track_capacity=256, obs_layout=1, **small))
    z, kw = _load_golden()
    cut = int(np.argmax(z["n_tracks"] > 100))
    a = VecEnv(Config(n_envs=1, track_capacity=256, **kw))
    a.enable_f64_obs()
    for i in range(cut + 1):
        _replay(a, z, i)
    torch.cuda.synchronize()
    d = a.debug_env(0)
    assert d["n_tracks"] == int(z["n_tracks"][cut]) > 100 and len(d["track_pose"]) == d["n_tracks"]
    assert np.array_equal(d["track_pose"], z["track_pose"][cut][:d["n_tracks"]])
    blob = a.snapshot()
    b = VecEnv(Config(n_envs=1, track_capacity=256, **kw))
    b.enable_f64_obs()
    b.restore(blob)
    narrow = VecEnv(Config(n_envs=1, track_capacity=64, **kw))
    with pytest.raises(_abi.CrowdNavError):
        narrow.restore(blob)
    for i in range(cut + 1, len(z["now"])):
        for e in (a, b):
            _replay(e, z, i)
        torch.cuda.synchronize()
        _check_call(b, z, i)
        assert torch.equal(a.obs_f64, b.obs_f64) and torch.equal(a.counters(), b.counters()) and torch.equal(a.reward, b.reward), i
    for e in (a, b, narrow):
        e.close()
