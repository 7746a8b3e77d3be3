#!/usr/bin/env python
"""Generate tests/golden/seq_wide_tracks.npz: the REFERENCE's own Python (oracle/harness) in a world whose track list grows far
past 64 tracks -- the reference for the wide tracker table (cn_config.track_capacity 128 ... 1024) beyond the CPU oracle's 64 slots.

The world's goal lies within goal_eps of the spawn pose: every episode ends at its first step, and every reset seeds the tracker
again from each unmatched 'o' object while the tracks of earlier episodes survive (ENV:656-672, 722-744), so the list keeps growing.
The columns are those of oracle/make_goldens.py's seq_* goldens (what Gazebo / ROS handed get_state, what the reference returned),
with the track arrays padded to the run's peak track count.  Build-machine only (needs the reference sources that
oracle/harness/refenv.py loads); the harness and the oracle are imported and used as they are.

    python tools/make_wide_tracker_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402
from oracle.harness.refenv import Harness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "seq_wide_tracks.npz")
# the goal-near-spawn world of tests/test_gpu_parity.py::test_track_table_overflow_is_flagged_and_confined, at an env index whose
# track list grows fastest (a scan of env_index_base over 64 indices)
KW = dict(n_peds=16, n_rays=361, k_obstacles=3, max_steps=49, room_half=1.1832673565816718, goal_x=0.565634967637293,
          goal_y=0.44034573709026004, spawn_x=0.6050993559998654, spawn_y=0.29646458843154355, spawn_yaw=2.8751215535007932,
          scan_latency_ms=5, settle_ms=50, ped_cycle_ms=1400, ped_vmax=0.2505021742113402, seed=634151950, env_index_base=286355 + 57,
          lidar_min=0.0, ped_radius=0.1, start_x=0.7867724988896705, start_y=-0.895986056152086)
EPISODES = 160
CAPACITY = 256          # the track_capacity tests/test_gpu_wide_tracker.py replays this golden with
MIN_PEAK = 100          # well past the 64 slots of the LDS table / the CPU oracle


def main():
    sim = oracle.Oracle(n_envs=1, **KW)
    h = Harness(sim)
    rng = np.random.default_rng(KW["seed"] & 0xffffffff)
    keys_in = ("ranges", "px", "py", "yaw", "v", "w", "now", "step_counter", "is_reset", "deque_x", "deque_y", "end_timestep")
    cols = {k: [] for k in keys_in + ("action", "obs", "reward", "done", "counters", "n_tracks", "collision_prob", "ego_score",
                                      "wp", "bb", "status")}
    tracks = []          # per call: (pose [n, 2], dist [n], speed [n], vel [n, 2])

    def push(rec, action, obs, reward, done):
        snap = h.snapshot()
        for k in keys_in:
            cols[k].append(rec[k])
        cols["action"].append(action); cols["obs"].append(obs); cols["reward"].append(reward); cols["done"].append(done)
        cols["counters"].append(snap["counters"]); cols["n_tracks"].append(snap["n_tracks"])
        tracks.append((snap["track_pose"], snap["track_dist"], snap["track_speed"], snap["track_vel"]))
        cols["collision_prob"].append(snap["collision_prob"]); cols["ego_score"].append(snap["ego_score"])
        cols["wp"].append(snap["wp"]); cols["bb"].append(snap["bb"]); cols["status"].append(snap["status"])

    for ep in range(EPISODES):
        obs = h.reset()
        push(h.trace[-1], (0.0, 0.0), obs, 0.0, False)
        for st in range(KW["max_steps"]):
            a = (float(np.float32(rng.uniform(0.0, 0.22))), float(np.float32(rng.uniform(-2.0, 2.0))))
            obs, r, d = h.step(a, st + 1)
            push(h.trace[-1], a, obs, r, d)
            if d:
                break
    arrs = {k: np.asarray(v) for k, v in cols.items()}
    nt = arrs["n_tracks"]
    peak = int(nt.max())
    assert MIN_PEAK <= peak < CAPACITY, "peak track count %d: the golden must lie past %d and within track_capacity %d" % (peak, MIN_PEAK, CAPACITY)
    C = len(tracks)
    arrs["track_pose"] = np.zeros((C, peak, 2)); arrs["track_dist"] = np.zeros((C, peak))
    arrs["track_speed"] = np.zeros((C, peak)); arrs["track_vel"] = np.zeros((C, peak, 2))
    for i, (pose, dist, speed, vel) in enumerate(tracks):
        n = len(dist)
        arrs["track_pose"][i, :n] = pose; arrs["track_dist"][i, :n] = dist
        arrs["track_speed"][i, :n] = speed; arrs["track_vel"][i, :n] = vel
    arrs["ped_init"] = sim.get_ped_init()
    arrs["config_keys"] = np.array(sorted(KW.keys()))
    arrs["config_vals"] = np.array([float(KW[k]) for k in sorted(KW.keys())])
    np.savez_compressed(OUT, **arrs)
    print("seq_wide_tracks: calls=%d  tracks mean %.1f max %d  (>64 on %d calls)  done=%d  %.0f KB" % (
        C, nt.mean(), peak, int((nt > 64).sum()), int(arrs["done"].sum()), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
