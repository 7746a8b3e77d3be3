"""What the recorded sequence goldens (tests/golden/seq_<name>.npz) contain, branch by branch, and what each of them has to contain.

Pure numpy on the recorded columns: oracle/make_goldens.py refuses to write a file that misses its conditions, and
tests/test_oracle_golden.py recomputes them from the committed files, so a regenerated golden cannot quietly lose the branch
it was recorded for.

An ending is a call with done set.  By the status the reference left and the call's own inputs it is one of
  success    status [True, False]: the robot is in the goal box (ENV:1017-1019, 1148-1153; ORIG:307; RW:728)
  time-out   status [False, True], step_counter == max_steps and no range of the observation below min_scan_range: only the
             step counter can have ended it (ENV:1021-1023, ORIG:311, RW:732), and compute_reward scored it as a collision
  collision  every other failure
A way-point bonus (layout 0 only, ENV:1109-1125) shows in the reward: the non-terminating part is -2 + {0, 1} + {0, 1} + 200, so
with the +-200 of an ending taken off it is at least 198, which nothing else reaches.  The snap is a bonus call that leaves the
way-point exactly on the original goal (ENV:1121-1123)."""
import numpy as np

MAXT = 24


def _cfg(kw, key, default):
    return kw[key] if key in kw else default


def census(z, kw):
    """Counts over one sequence file.  `kw` is the file's configuration (config_keys / config_vals as a dict)."""
    R = int(_cfg(kw, "n_rays", 360))
    K = int(_cfg(kw, "k_obstacles", 8))
    layout = int(_cfg(kw, "obs_layout", 0))
    max_steps = int(kw["max_steps"])
    min_range = float(_cfg(kw, "min_scan_range", 0.12))
    goal = (float(_cfg(kw, "goal_x", -1.0)), float(_cfg(kw, "goal_y", 1.0)))
    done = np.asarray(z["done"]).astype(bool)
    status = np.asarray(z["status"]).astype(bool)
    reward = np.asarray(z["reward"], dtype=np.float64)
    out = dict(calls=len(done), K=K, layout=layout, episodes=int(np.asarray(z["is_reset"]).sum()), success=0, collision=0, timeout=0,
               bonuses=0, snaps=0, bonuses_before_success=[], success_at_min_range=0, first_success=-1, timeout_calls=[])
    in_episode = 0
    for i in range(len(done)):
        if z["is_reset"][i]:
            in_episode = 0
            continue
        ok, fail = bool(status[i][0]), bool(status[i][1])
        ending = 200.0 * (done[i] and ok) - 200.0 * (done[i] and fail)
        if layout == 0 and reward[i] - ending >= 198.0:
            out["bonuses"] += 1
            in_episode += 1
            out["snaps"] += int(tuple(z["wp"][i]) == goal)
        if not done[i]:
            continue
        clear = bool(np.asarray(z["obs"][i][:R - 1]).min() >= min_range)
        if ok and not fail:
            out["success"] += 1
            out["bonuses_before_success"].append(in_episode)
            out["success_at_min_range"] += int(not clear)
            if out["first_success"] < 0:
                out["first_success"] = i
        elif int(z["step_counter"][i]) == max_steps and clear:
            out["timeout"] += 1
            out["timeout_calls"].append(i)
        else:
            out["collision"] += 1
    if "n_tracks" in z:
        nt = np.asarray(z["n_tracks"])
        # a short list: 0 < n_tracks < K, padded to K.  With K = 1 the only list below K is the empty one
        short = (nt < K) & ((nt > 0) | (K == 1))
        out.update(max_tracks=int(nt.max()), over_k=int((nt > K).sum()), under_k=int(short.sum()), no_tracks=int((nt == 0).sum()))
    return out


# name -> what the file was recorded for (conditions, not measurements: the counts themselves are in DESIGN.md section 4)
REQUIRED = {
    "goal8": dict(success=3, chain=3, snaps=1),
    "timeout": dict(timeout=2, tracks_at_timeout=True),
    "timeout0": dict(timeout=1, empty=True),
    "k1": dict(both_sides_of_k=True),
    "k16": dict(both_sides_of_k=True),
    "orig_goal": dict(success=3, timeout=1),
    "rw_goal": dict(success=3, timeout=1),
}


def unmet(name, z, kw):
    """The conditions of REQUIRED[name] that the file misses, as a list of strings (empty: the file may be written)."""
    c = census(z, kw)
    req = REQUIRED.get(name, {})
    bad = []
    if c.get("max_tracks", 0) > MAXT:
        bad.append("n_tracks %d > MAXT" % c["max_tracks"])
    if c["success"] < req.get("success", 0):
        bad.append("%d success endings, %d wanted" % (c["success"], req["success"]))
    if c["timeout"] < req.get("timeout", 0):
        bad.append("%d time-out endings, %d wanted" % (c["timeout"], req["timeout"]))
    if "chain" in req and max(c["bonuses_before_success"] + [0]) < req["chain"]:
        bad.append("no success after %d way-point bonuses: %r" % (req["chain"], c["bonuses_before_success"]))
    if c["snaps"] < req.get("snaps", 0):
        bad.append("no way-point snapped onto the goal")
    if req.get("both_sides_of_k") and not (c["over_k"] > 0 and c["under_k"] > 0):
        bad.append("n_tracks > K on %d calls, a short list on %d" % (c["over_k"], c["under_k"]))
    if req.get("tracks_at_timeout") and not any(int(z["n_tracks"][i]) > 0 for i in c["timeout_calls"]):
        bad.append("no time-out ending with a live track")
    if req.get("empty") and not (int(kw["n_peds"]) == 0 and c["no_tracks"] == c["calls"]):
        bad.append("not an empty room: n_peds %r, %d of %d calls without tracks" % (kw["n_peds"], c["no_tracks"], c["calls"]))
    return bad
