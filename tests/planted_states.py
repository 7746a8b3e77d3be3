"""Planted state records: states a short random rollout almost never reaches, written into one environment each and stepped from
there.  No tests here: tests/test_planted_states.py checks the premise on the CPU oracle alone (every record passes cn_restore's
record check, csrc/crowdnav_snapshot_check.h; every named event happens in the named step; no status bit a record does not name;
finite outputs; every family's edge is hit), tests/test_gpu_planted_states.py plants the same arrays into a handle of every step,
same-call and the s360 sequence cell of tests/kernel_matrix.py and holds four steps to the oracle, bit for bit.

The base is the oracle's own state after reset() and three fixed steps (tracks and deques are live, ep_step = 3).  A record edits ONE
environment's arrays -- records are independent per environment, so one handle of N = len(records) environments carries every family
at once -- and names what it expects: an event and the step (0 ... 3) it falls in.  Events:
    none       no episode ends in the four steps
    goal       the step ends the episode inside the goal box (ENV:1015, success)
    collision  ... with a range below min_scan_range (ENV:1011; 0.105 in the original layout, ORIG:282), failure
    timeout    ... with step_counter >= max_steps (ENV:1019) and nothing else, failure
    held       the planted done flag is returned again (ENV:1011 `if not self.done` skips the three tests), failure unless in the goal box
    reset      reset convention "next": the call is spent on Env.reset() (reward 0, done 0, ep_step 0); the follow-up of a done
    overflow   the track list outgrows the tracker slots S in this step: CN_ST_TRACK_OVERFLOW on the device.  The oracle holds 64 tracks
               (CNO_MAX_TRACKS): at S = 64 it raises the same bit, at S = 32 its list is simply longer than S afterwards -- "the oracle
               overflowed" is either.  These are the only environments not held to equality afterwards.
An expectation may differ between the reset conventions ("next" / "same").  A record's `how` says in one line how the reference reaches
the state.  Records whose outputs would be NaN or inf (a time step of 0: CN_ST_DT_ZERO) belong to the external-path tests and are left out.

Both sides are planted from the same arrays: the oracle through set_state, the kernel through join_snapshot + restore (ped_init and
ped_preset from the handle's own fresh snapshot: they are functions of the configuration).  Records that need the robot at rest keep
action 0 for all four steps; the others get seeded actions."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

import kernel_matrix as M
from bisect_divergence import SD_NAMES, SI_NAMES, TF_NAMES  # tools/ (kernel_matrix puts it on the path)

SD = {n: i for i, n in enumerate(SD_NAMES)}
SI = {n: i for i, n in enumerate(SI_NAMES)}
TF = {n: i for i, n in enumerate(TF_NAMES)}
ST_TRACK_OVERFLOW, ST_TTC_ZERO, ST_DT_ZERO, ST_CONF_OVERFLOW, ST_TRACK_WIDE = 1, 2, 4, 8, 16     # include/crowdnav.h CN_ST_*
STEPS, BASE_STEPS = 4, 3
BASE_SEED, ACTION_SEED = 17, 23
FAMILIES = ("episode_end", "thresholds", "angles", "pedestrians", "tracker", "clocks")
EVENTS = ("none", "goal", "collision", "timeout", "held", "reset", "overflow")
MID = (0.35, -0.25)             # a place from which no wall is in lidar range, in every world's room
IOU_HALF = 0.0505               # ENV:688 is_associated's box
PI = math.pi

# family, name, how (reachability, one line), edit(E), expect {mode: (event, step)}, rest (action 0), edges (tags), status (bits the record
# names besides its event), after0 (None or f(before, after, W) -> None | text: what the first step must have left, on the oracle)
# actions (None, or the (v, w) of each of the four steps instead of the seeded ones)
Record = namedtuple("Record", "family name how edit expect rest edges status after0 actions", defaults=(False, (), 0, None, None))


def both(event, step=0):
    return {"next": (event, step), "same": (event, step)}


# ---- a world: the configuration and what follows from it -------------------------------------------------------------------------
class World:
    def __init__(self, name, oracle_mod):
        from crowdnav import Config
        self.name, self.oracle_mod, self.L = name, oracle_mod, oracle_mod.lib()
        self.kw = M.config_kw(name)
        c = self.cfg = Config(**self.kw).as_dict()
        self.P, self.R, self.K, self.max_steps = c["n_peds"], c["n_rays"], c["k_obstacles"], c["max_steps"]
        self.gt, self.layout = c["risk_mode"] == 1, c["obs_layout"]
        self.contact, self.sf, self.wheels = bool(c["ped_contact"]), c["ped_mode"] == 2, c["wheel_accel"] > 0
        # cn_create: tracker slots and the confirmed-object table
        self.slots = c["track_capacity"] or (32 if (self.P <= 40 and not (self.gt and self.P > 32)) else 64)
        self.max_conf = (self.R - 1) // 4 + 2
        self.cap = min(self.slots, oracle_mod.MAX_TRACKS)          # what both sides can hold: the wide world's totals stay <= 64
        self.h, self.r = c["room_half"], c["ped_radius"]
        self.lim = self.h - c["robot_clearance"]                    # robot_advance's clamp
        self.step_ms = c["dt_ms"] + c["scan_latency_ms"]
        self.T, self.stagger = c["ped_cycle_ms"], c["ped_stagger_ms"]
        self.goal = (c["goal_x"], c["goal_y"])
        self.goal_eps = c["goal_eps"] if self.layout == 0 else 0.20          # ORIG:500, RW:720 use the literal
        self.min_range = 0.105 if self.layout == 1 else c["min_scan_range"]  # ORIG:282
        self.has_tracker = self.layout != 1                                   # the original layout has no tracker
        self.L.cno_set_py2_round(c["py2_round"])

    def config(self, n_envs, env_index_base=0):
        return dict(self.cfg, n_envs=n_envs, env_index_base=env_index_base)

    def round3(self, x):
        return float(self.L.cno_py_round(float(x), 3))

    def in_box(self, x, y):
        """ENV:1285-1319 restated: the half-open goal box"""
        gx, gy, eps = self.goal[0], self.goal[1], self.goal_eps
        return x <= gx + eps and x > gx - eps and y <= gy + eps and y > gy - eps

    def min_scan(self, x, y, yaw, peds):
        """the smallest range Env.get_state sees from this pose (the oracle's raycast, a pure function; NaN-free here)"""
        rg = np.zeros(self.R)
        cc = self.oracle_mod.make_config(**self.config(1))
        pp = np.ascontiguousarray(peds, dtype=np.float64).reshape(-1, 2)
        dp = C.POINTER(C.c_double)
        self.L.cno_raycast(C.byref(cc), float(x), float(y), float(yaw), pp.ctypes.data_as(dp), int(pp.shape[0]), rg.ctypes.data_as(dp))
        scan = np.where(np.isinf(rg) | (rg > self.cfg["max_scan_range"]) | (rg == 0), 0.6 if self.layout == 1 else self.cfg["max_scan_range"], rg)
        return float(scan[1:].min())                                     # get_scan_ranges reverses and drops the last: ray 0 is not seen

    def ray_dir(self, k):
        """unit vector of ray k in the robot frame (cno_raycast's table)"""
        s, c = C.c_double(), C.c_double()
        self.L.cno_det_sincos(float(k) * (self.cfg["lidar_span"] / (self.R - 1)), C.byref(s), C.byref(c))
        return c.value, s.value

    def instants_in(self, i, t0, t1):
        """does pedestrian i get a new velocity in [t0, t1)?  CROWD:128-144: at i * stagger + m * cycle"""
        offs = i * self.stagger
        m = 0 if t0 <= offs else (t0 - offs + self.T - 1) // self.T
        return offs + m * self.T < t1


# ---- one environment's arrays while a record edits them -----------------------------------------------------------------------------
class Env:
    def __init__(self, W, e, arrays):
        self.W, self.e = W, e
        for k in ("sd", "si", "ped_p", "ped_v", "trk", "ped_aux"):
            setattr(self, k, arrays[k][e])

    @property
    def crowd_ms(self):
        return (int(np.uint32(self.si[SI["CROWD_HI"]])) << 32) | int(np.uint32(self.si[SI["CROWD_LO"]]))

    def set_crowd(self, ms):
        self.si[SI["CROWD_LO"]] = np.array(ms & 0xFFFFFFFF, dtype=np.uint32).astype(np.int32)
        self.si[SI["CROWD_HI"]] = ms >> 32

    def stand(self, x, y, yaw):
        """the robot stood here for the last step: pose, zero twist, the agent's deque holds the rounded position (ENV:1208); in the
        risk layout the way-point, previous distance and heading are those of this pose (ENV:246-265)"""
        W, sd = self.W, self.sd
        sd[SD["RX"]], sd[SD["RY"]], sd[SD["RYAW"]], sd[SD["RV"]], sd[SD["RW"]] = x, y, yaw, 0.0, 0.0
        sd[SD["DQ0X"]], sd[SD["DQ0Y"]] = W.round3(x), W.round3(y)
        self.si[SI["DQ_LEN"]] = 1
        if W.layout == 0:
            wp = (C.c_double * 2)()
            W.L.cno_waypoint(x, y, W.goal[0], W.goal[1], W.cfg["waypoint_radius"], wp)
            sd[SD["WPX"]], sd[SD["WPY"]] = wp[0], wp[1]
            sd[SD["PREV_DIST"]] = float(W.L.cno_np_around(W.L.cno_distance_to_goal(x, y, wp[0], wp[1]), 2))
            ga = math.atan2(wp[1] - (y + W.cfg["start_y"]), wp[0] - (x + W.cfg["start_x"])) - yaw
            ga = ga - 2 * PI if ga > PI else (ga + 2 * PI if ga < -PI else ga)
            sd[SD["PREV_HEAD"]] = float(W.L.cno_py_round(ga, 2))

    def park(self, keep=0, quiet_steps=STEPS):
        """every pedestrian but `keep` of them to a place out of the robot's sight (>= 0.95 m away, >= 0.2 m from a wall, 0.16 m apart),
        at rest as after a reset.  Returns the kept indices (the caller places them): `keep` itself if it is a list, else that many
        pedestrians whose next velocity assignment is not within `quiet_steps` steps (ped_mode 0), so what the caller gives them holds."""
        W = self.W
        t0 = self.crowd_ms
        if isinstance(keep, int):
            quiet = [i for i in range(W.P) if not W.instants_in(i, t0, t0 + quiet_steps * W.step_ms)]
            if len(quiet) < keep:
                quiet = [i for i in range(W.P) if not W.instants_in(i, t0, t0 + W.step_ms)]
            kept = quiet[:keep]
            assert len(kept) == keep, (W.name, keep)
        else:
            kept = list(keep)           # these pedestrians, whatever their schedule
        rx, ry = self.sd[SD["RX"]], self.sd[SD["RY"]]
        g = np.arange(-W.h + 0.2, W.h - 0.2 + 1e-9, 0.16)
        pts = [(x, y) for x in g for y in g if math.hypot(x - rx, y - ry) >= 0.95]
        pts.sort(key=lambda p: (-round(math.hypot(p[0] - rx, p[1] - ry), 6), p))
        others = [i for i in range(W.P) if i not in kept]
        assert len(pts) >= len(others), (W.name, len(pts))
        for i, p in zip(others, pts):
            self.ped_p[i] = p
            self.ped_v[i] = 0.0
        return kept

    def put(self, i, x, y, vx=0.0, vy=0.0):
        self.ped_p[i] = (x, y)
        self.ped_v[i] = (vx, vy)

    @property
    def lidar(self):
        sd = self.sd
        ox = self.W.cfg["lidar_offset_x"]
        return sd[SD["RX"]] + ox * math.cos(sd[SD["RYAW"]]), sd[SD["RY"]] + ox * math.sin(sd[SD["RYAW"]])

    def probe(self, action=(0.0, 0.0), **si_edits):
        """this environment's state one oracle step on (a scratch oracle of one environment with this one's global index): what the
        reference makes of the scene"""
        W = self.W
        orc = W.oracle_mod.Oracle(W.config(1, self.e))
        si = self.si.copy()
        for k, v in si_edits.items():
            si[SI[k]] = v
        orc.set_state(0, self.sd, si, self.ped_p, self.ped_v, self.trk, None, None, self.ped_aux)
        out = orc.step(np.array([action], dtype=np.float64), auto_reset=False)
        return orc.get_state(0, trk_cap=self.trk.shape[0]), out

    def track(self, slot, pose, dist, dqlen=1, d0=None, d1=None, t=None, speed=-1.0, vel=(0.0, 0.0)):
        r = self.trk[slot]
        r[:] = 0.0
        r[TF["PX"]], r[TF["PY"]], r[TF["DIST"]] = pose[0], pose[1], dist
        d0 = pose if d0 is None else d0
        r[TF["D0X"]], r[TF["D0Y"]] = d0
        if dqlen > 1:
            r[TF["D1X"]], r[TF["D1Y"]] = pose if d1 is None else d1
        r[TF["T"]] = self.sd[SD["CLOCK"]] if t is None else t          # the stamp of the last observation (ENV:990-996)
        r[TF["SPEED"]], r[TF["VX"]], r[TF["VY"]], r[TF["DQLEN"]] = speed, vel[0], vel[1], float(dqlen)


# ---- families -------------------------------------------------------------------------------------------------------------------------
def episode_end(W):
    """ep_step at max_steps - 2 and max_steps - 1, each alone, inside the goal box and inside min_scan_range of a wall; goal and collision
    in one call; pending_reset x done under both reset conventions.  Edges: timeout, timeout+goal, timeout+collision, goal+collision,
    pending x done."""
    ms = W.max_steps
    gx, gy = W.goal

    def ep(k):
        def f(E):
            E.si[SI["EP_STEP"]] = ms - k
        return f

    def in_goal(k):
        def f(E):
            E.si[SI["EP_STEP"]] = ms - k
            E.stand(gx + 0.05, gy - 0.05, 0.7)
            E.park()
        return f

    def at_wall(k):
        def f(E):
            E.si[SI["EP_STEP"]] = ms - k
            E.stand(W.lim, 0.3, PI / 2)          # driven into the +x wall: the clamp's limit, 0.09 m from it
            E.park()
        return f

    def goal_and_collision(E):
        E.stand(gx + 0.05, gy - 0.05, 0.0)
        i, = E.park(keep=1)
        E.put(i, gx + 0.05, gy - 0.05 - 0.15)    # a pedestrian 0.15 m beside the robot: its surface 0.10 m from the lidar

    def flags(p, d):
        def f(E):
            E.si[SI["PENDING_RESET"]], E.si[SI["DONE"]] = p, d
        return f

    out = [
        Record("episode_end", "ep_step=max-2", "an episode two calls before its time limit", ep(2), both("timeout", 1), edges=("timeout",)),
        Record("episode_end", "ep_step=max-1", "an episode one call before its time limit", ep(1), both("timeout", 0), edges=("timeout",)),
        Record("episode_end", "ep_step=max-2 in goal", "the robot drove into the goal box", in_goal(2), both("goal", 0), rest=True, edges=("goal",)),
        Record("episode_end", "ep_step=max-1 in goal", "... on the last call before the time limit", in_goal(1), both("goal", 0), rest=True,
               edges=("timeout+goal",)),
        Record("episode_end", "ep_step=max-2 at wall", "the robot drove into a wall (robot_advance's clamp)", at_wall(2), both("collision", 0),
               rest=True, edges=("collision",)),
        Record("episode_end", "ep_step=max-1 at wall", "... on the last call before the time limit", at_wall(1), both("collision", 0), rest=True,
               edges=("timeout+collision",)),
    ]
    if not W.contact:          # (contact keeps a pedestrian's surface robot_clearance = 0.09 m from the robot's centre: 0.15 m is inside)
        out.append(Record("episode_end", "goal and collision", "a pedestrian walks up to the robot standing in the goal box", goal_and_collision,
                          both("goal", 0), rest=True, edges=("goal+collision",)))
    out += [
        Record("episode_end", "pending=0 done=0", "any running episode", flags(0, 0), both("none"), edges=("p0d0",)),
        Record("episode_end", "pending=1 done=0", "a run stepped with reset convention next; a caller may switch to same-call resets, which "
               "ignore the flag", flags(1, 0), {"next": ("reset", 0), "same": ("none", 0)}, edges=("p1d0",)),
        Record("episode_end", "pending=0 done=1", "a finished episode the caller (auto_reset none) has not reset yet", flags(0, 1), both("held", 0),
               edges=("p0d1",)),
        Record("episode_end", "pending=1 done=1", "the state right after an episode's last call under reset convention next", flags(1, 1),
               {"next": ("reset", 0), "same": ("held", 0)}, edges=("p1d1",)),
    ]
    return out


EDGES = {"episode_end": ["timeout", "goal", "collision", "timeout+goal", "timeout+collision", "p0d0", "p1d0", "p0d1", "p1d1"]}


def _neighbours(x):
    return (("", x), ("-", math.nextafter(x, -math.inf)), ("+", math.nextafter(x, math.inf)))


def thresholds(W):
    """The robot at rest (rv = rw = 0, action 0) at goal distance goal_eps and its two float64 neighbours on eight bearings (the half-open
    box of ENV:1285: the east and north edges are inside, the west and south edges outside); at the pose where the smallest range crosses
    min_scan_range, and its two neighbours; in a corner; at waypoint_radius from its way-point.  What each expects is worked out from the
    stated comparison (in_box restated in World.in_box; the range from the oracle's raycast, a pure function of the pose), never from a
    run."""
    gx, gy, eps = W.goal[0], W.goal[1], W.goal_eps
    out = []
    for name, (ux, uy) in {"E": (1, 0), "NE": (1, 1), "N": (0, 1), "NW": (-1, 1), "W": (-1, 0), "SW": (-1, -1), "S": (0, -1), "SE": (1, -1)}.items():
        for tag, k in (("", 0), ("-", -1), ("+", 1)):          # - / +: one float64 towards / away from the goal
            def coord(g, u):
                c = g + u * eps
                return c if (k == 0 or u == 0) else math.nextafter(c, c + u * k)
            x, y = coord(gx, ux), coord(gy, uy)

            def f(E, x=x, y=y):
                E.stand(x, y, 0.7)
                E.park()
            inside = W.in_box(x, y)
            out.append(Record("thresholds", "goal_eps %s%s" % (name, tag), "the robot stops on the goal box's edge", f,
                              both("goal" if inside else "none"), rest=True, edges=("goal_eps inside" if inside else "goal_eps outside",)))
    # the wall: facing away from the +x wall (the lidar sits behind the centre: 0.032 m closer to it); bisect x to the first pose whose
    # smallest range is not below min_scan_range
    yaw, y0 = 3.0, 0.3
    lo, hi = W.lim - 0.2, W.lim                                       # far: no collision ... at the clamp: collision
    assert W.min_scan(lo, y0, yaw, []) >= W.min_range > W.min_scan(hi, y0, yaw, []), W.name
    while math.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if W.min_scan(mid, y0, yaw, []) >= W.min_range else (lo, mid)
    for tag, x in (("last free", lo), ("first hit", hi), ("second hit", math.nextafter(hi, math.inf)), ("second free", math.nextafter(lo, -math.inf))):
        def f(E, x=x):
            E.stand(x, y0, yaw)
            E.park()
        hit = W.min_scan(x, y0, yaw, []) < W.min_range
        out.append(Record("thresholds", "min_scan_range %s" % tag, "the robot stops where a wall's range crosses min_scan_range", f,
                          both("collision" if hit else "none"), rest=True, edges=("min_scan hit" if hit else "min_scan free",)))

    def corner(E):
        E.stand(W.lim, -W.lim, 3 * PI / 4)          # its back to the corner: the lidar sits 0.032 m behind the centre, closer to both walls
        E.park()
    out.append(Record("thresholds", "corner", "the robot drove into a corner: both clamps", corner, both("collision"), rest=True, edges=("corner",)))

    def waypoint(x, y):
        def f(E):
            E.stand(x, y, 2.0)
            E.park()
        return f
    if W.layout == 0:          # (the other layouts have no way-points)
        out.append(Record("thresholds", "waypoint_radius west", "the goal lies due west: the way-point is a vertex of UTL:296's ring, at waypoint_radius",
                          waypoint(0.2, gy), both("none"), rest=True, edges=("waypoint_radius",)))
        out.append(Record("thresholds", "waypoint_radius diagonal", "the way-point on the ring's edge towards the goal", waypoint(0.3, -0.3), both("none"),
                          rest=True, edges=("waypoint_radius",)))
    return out


EDGES["thresholds"] = ["goal_eps inside", "goal_eps outside", "min_scan hit", "min_scan free", "corner"]


def angles(W):
    """Yaw in {0, -0.0, +-pi/2, pi, the neighbours of +-pi inside (-pi, pi], 3.14}; the way-point exactly ahead, behind (both signs of pi),
    left and right; prev_head at +-pi.  Left out as unreachable: yaw = -pi and anything beyond +-pi -- robot_advance wraps `th <= -pi` to
    th + 2 pi and `th > pi` to th - 2 pi after every interval, and the spawn yaw is 3.14."""
    out = []

    def yaw(v):
        def f(E):
            E.sd[SD["RYAW"]] = v
        return f
    for name, v in (("0", 0.0), ("-0.0", -0.0), ("pi/2", PI / 2), ("-pi/2", -PI / 2), ("pi", PI), ("pi-", math.nextafter(PI, 0.0)),
                    ("-pi+", math.nextafter(-PI, 0.0)), ("3.14", 3.14)):
        out.append(Record("angles", "yaw %s" % name, "turning on the spot passes every yaw in (-pi, pi] (-0.0: a turn of -0.0 from it)", yaw(v),
                          both("none"), edges=("yaw",)))

    def heading(h):
        def f(E):
            x, y = MID
            E.stand(x, y, 0.0)                                         # (sets the way-point of this position)
            if W.layout == 0:
                tx, ty = E.sd[SD["WPX"]], E.sd[SD["WPY"]]
            else:
                tx, ty = W.goal
            off = (W.cfg["start_x"], W.cfg["start_y"]) if W.layout != 1 else (0.0, 0.0)      # ENV:223-224, RW:186 add starting_point; ORIG:244 not
            ga = math.atan2(ty - (y + off[1]), tx - (x + off[0]))
            v = ga - h
            v = v - 2 * PI if v > PI else (v + 2 * PI if v <= -PI else v)
            E.stand(x, y, v)
            E.park()
        return f
    for name, h in (("ahead", 0.0), ("behind +pi", PI), ("behind -pi", -PI), ("left", PI / 2), ("right", -PI / 2)):
        out.append(Record("angles", "goal %s" % name, "the robot turned until the way-point's bearing was this", heading(h), both("none"), rest=True,
                          edges=("heading",)))

    def prev_head(v):
        def f(E):
            E.sd[SD["PREV_HEAD"]] = v
        return f
    out.append(Record("angles", "prev_head pi", "a reset stores the unrounded heading (ENV:1244): pi with the goal exactly behind", prev_head(PI),
                      both("none"), edges=("prev_head",)))
    out.append(Record("angles", "prev_head -pi", "... -pi from the other side (ENV:232 wraps only below -pi)", prev_head(-PI), both("none"),
                      edges=("prev_head",)))
    return out


EDGES["angles"] = ["yaw", "heading", "prev_head"]


def _rings(W, n, ox, oy):
    """n places around (ox, oy) within lidar range: rings from 0.58 m inwards to 0.34 m, as far apart as n allows"""
    radii = [0.58, 0.50, 0.42, 0.34]
    total = sum(2 * PI * r for r in radii)
    gap = min(0.16, total / (n + len(radii)))
    pts = []
    for r in radii:
        m = int(2 * PI * r / gap)
        pts += [(ox + r * math.cos(2 * PI * j / m + r), oy + r * math.sin(2 * PI * j / m + r)) for j in range(m)]
    assert len(pts) >= n, (W.name, n, len(pts))
    return pts[:n]


def pedestrians(W):
    """A pedestrian on the robot; at ped_radius from the lidar origin and that distance's two neighbours; centred on a ray; tangent to a ray;
    two and three coincident; at the wall clamp; every velocity 0; a pedestrian coming at the robot with the robot's own speed (the
    relative_vel == 0 branch, ENV:826: gt worlds, where the obstacle's speed is the pedestrian's true one); every pedestrian of the world
    inside lidar_max.  Left out: overlapping discs in the contact and social-force worlds (contact keeps discs apart and the robot's
    clearance free; the social force between coincident pedestrians has no direction: NaN)."""
    out = []
    soft = not (W.contact or W.sf)            # pedestrians pass through each other and the robot
    x0, y0 = MID

    def scene(place, keep=1, yaw=0.0):
        def f(E):
            E.stand(x0, y0, yaw)
            kept = E.park(keep=keep)
            place(E, kept)
        return f
    if soft:
        out.append(Record("pedestrians", "on the robot", "a pedestrian walks through the robot's centre (no contact in this world)",
                          scene(lambda E, k: E.put(k[0], x0, y0)), both("collision"), rest=True, edges=("on robot",)))
        for tag, d in _neighbours(W.r):
            def place(E, k, d=d):
                ox, oy = E.lidar
                E.put(k[0], ox + d, oy)
            out.append(Record("pedestrians", "lidar on the surface%s" % tag, "a pedestrian's surface passes through the lidar origin", scene(place),
                              both("collision"), rest=True, edges=("surface",)))
        for n in (2, 3):
            def place(E, k):
                for i in k:
                    E.put(i, x0 + 0.4, y0 + 0.1)
            out.append(Record("pedestrians", "%d coincident" % n, "pedestrians pass through each other: the same place at the same time", scene(place, n),
                              both("none"), rest=True, edges=("coincident",)))
    kray = 40

    def on_ray(E, k):
        ox, oy = E.lidar
        c, s = W.ray_dir(kray)
        E.put(k[0], ox + 0.4 * c, oy + 0.4 * s)

    def tangent(E, k):
        ox, oy = E.lidar
        c, s = W.ray_dir(kray)
        E.put(k[0], ox + 0.4 * c - W.r * s, oy + 0.4 * s + W.r * c)
    out.append(Record("pedestrians", "centred on a ray", "a pedestrian crosses a ray's line with its centre", scene(on_ray), both("none"), rest=True,
                      edges=("on ray",)))
    out.append(Record("pedestrians", "tangent to a ray", "a pedestrian's edge touches a ray's line", scene(tangent), both("none"), rest=True,
                      edges=("tangent",)))

    def clamp(E):
        lo, hi = -W.h + W.r, W.h - W.r
        kept = E.park(keep=min(4, W.P))
        for i, (x, y, vx, vy) in zip(kept, ((hi, hi, 0.15, 0.1), (lo, 0.4, -0.12, 0.05), (-0.6, lo, 0.02, -0.19), (lo, hi, -0.1, 0.1))):
            E.put(i, x, y, vx, vy)
    out.append(Record("pedestrians", "wall clamp", "pedestrians walking into walls and corners stay clamped there", clamp, both("none"), edges=("clamp",)))

    def still(E):
        E.ped_v[:] = 0.0
    out.append(Record("pedestrians", "velocity 0", "every pedestrian's velocity is 0 after a reset until its next assignment", still, both("none"),
                      edges=("v=0",)))

    def everyone(E):
        E.stand(x0, y0, 0.0)
        ox, oy = E.lidar
        for i, p in enumerate(_rings(W, W.P, ox, oy)):
            E.put(i, p[0], p[1])
    if soft or W.P <= 60:
        out.append(Record("pedestrians", "all in range", "the whole crowd gathers around the robot", everyone, both("none"), rest=True, edges=("all in range",)))
    if W.gt and not W.wheels and not W.sf and not W.contact:
        out.append(_relative_vel_zero(W))
    return out


EDGES["pedestrians"] = ["on ray", "tangent", "clamp", "v=0"]


def _relative_vel_zero(W):
    """gt world: the robot drives along +x at the commanded speed; a pedestrian ahead comes at it with exactly the speed the agent's deque
    will show (|dx rounded| / end_timestep, UTL:227-236), so agent_vel - obstacle_vel == 0 while the cone's segment (twice that
    displacement long) crosses the pedestrian's 0.178 m ring: ENV:826's branch."""
    x0, y0 = MID
    v_cmd = float(np.float32(0.1))
    dt = W.cfg["dt_ms"] / 1000.0

    def f(E):
        E.stand(x0, y0, 0.0)
        i, = E.park(keep=1, quiet_steps=1)
        clock = float(E.sd[SD["CLOCK"]])
        ts = (clock + dt) - clock                                         # ENV:1202 end_timestep as the simulator's clock gives it
        x1 = W.round3(x0 + (v_cmd * dt))                                  # robot_advance: fma(ds, cos 0, x), then ENV:1208's round
        dx = x1 - float(E.sd[SD["DQ0X"]])
        speed = abs(dx / ts)
        assert 0 < speed <= W.cfg["ped_vmax"]
        # the pedestrian's surface point 0.178 m + one displacement ahead of where the robot started, at scan time
        lat = W.cfg["scan_latency_ms"] / 1000.0
        px_scan = float(E.sd[SD["DQ0X"]]) + 0.178 + dx + W.r
        E.put(i, px_scan + speed * (dt + lat), y0, -speed, 0.0)

    def after0(before, after, W_):
        tr = after["trk"][0]
        if int(after["si"][SI["NTRACKS"]]) != 1:
            return "expected exactly one pedestrian in sight, got %d" % int(after["si"][SI["NTRACKS"]])
        dx = after["sd"][SD["DQ0X"]] - before["sd"][SD["DQ0X"]]
        dy = after["sd"][SD["DQ0Y"]] - before["sd"][SD["DQ0Y"]]
        ts = after["sd"][SD["TS"]]
        agent = math.sqrt(math.pow(dx / ts, 2) + math.pow(dy / ts, 2))
        if agent != tr[TF["SPEED"]]:
            return "agent speed %r != obstacle speed %r" % (agent, tr[TF["SPEED"]])
        return None
    return Record("pedestrians", "relative_vel == 0", "a pedestrian walks towards the robot at the robot's own speed", f, both("none"), edges=("relative_vel=0",),
                  after0=after0, actions=[(v_cmd, 0.0)] + [(0.0, 0.0)] * (STEPS - 1))


def _touching(px, half=IOU_HALF):
    """the first x east of px at which is_associated's boxes no longer overlap: ix = (px + half) - (x - half) <= 0 (UTL:422-460)"""
    x = px + 2 * half
    while (px + half) - (x - half) > 0.0:
        x = math.nextafter(x, math.inf)
    while (px + half) - (math.nextafter(x, -math.inf) - half) <= 0.0:
        x = math.nextafter(x, -math.inf)
    return x


def tracker(W):
    """For the world's tracker slots S: ntracks in {0, 1, K-1, K, K+1, S-2, S-1, S} with the step confirming 0, 1 and 2 new objects, so the
    totals S-1, S, S+1, S+2 all occur; CN_ST_TRACK_OVERFLOW is expected exactly where the total exceeds S.  The planted tracks all sit on a
    current detection (the reference duplicates tracks at every reset, ENV:723-743 after ENV:683's clear, so equal poses are reachable),
    with deque lengths 1 and 2, found by asking the oracle what it makes of the scene (Env.probe); every one of them matches (ENV:702), the
    other detections become tracks.  Also: one track whose box only touches the detection's (IoU exactly 0: dropped by ENV:715, the
    detection becomes a new track); a matched track with speed 0 (same pose twice).  gt worlds rebuild the list from the pedestrians in
    sight at every step: there the family is the number in sight (0, 1, 2) over the same planted lists, ids 0 and P-1 among them, deque
    length 0.  The wide world plants totals up to 64, what the oracle holds.  The original layout has no tracker: no records."""
    if not W.has_tracker:
        return []
    S, K = W.cap, W.K
    out = []
    x0, y0 = MID
    bearings = (0.3, 2.4, -1.9)

    def scene(E, n_vis):
        """n_vis pedestrians in sight, 0.4 m (or the first distance at which the reference confirms each as an object) from the robot"""
        E.stand(x0, y0, 0.0)
        kept = E.park(keep=n_vis)
        for d in (0.40, 0.35, 0.45, 0.30, 0.50):
            for j, i in enumerate(kept):
                E.put(i, x0 + d * math.cos(bearings[j]), y0 + d * math.sin(bearings[j]))
            st, _ = E.probe(NTRACKS=0)
            if int(st["si"][SI["NTRACKS"]]) == n_vis:
                return kept, st
        raise AssertionError("%s: no scene in which the reference confirms %d objects" % (W.name, n_vis))

    def lidar_record(nt, new, dq2_every=2):
        def f(E):
            n_vis = new + (1 if nt else 0)
            kept, st = scene(E, n_vis)
            E.si[SI["NTRACKS"]] = nt
            E.trk[:] = 0.0
            if nt:
                a = E.ped_p[kept[0]]
                j = int(np.argmin([math.hypot(t[TF["PX"]] - a[0], t[TF["PY"]] - a[1]) for t in st["trk"][:n_vis]]))
                pose, dist = (st["trk"][j, TF["PX"]], st["trk"][j, TF["PY"]]), st["trk"][j, TF["DIST"]]
                for s in range(nt):
                    if s % dq2_every == 1:        # two entries, 4 mm apart and 4 mm from the detection (popleft, ENV:678, then the match appends)
                        near = (pose[0] + 0.004, pose[1])
                        E.track(s, near, dist, dqlen=2, d0=(pose[0] + 0.008, pose[1]), d1=near, speed=0.025, vel=(0.026, 0.0))
                    else:                         # one entry at the detection itself: the match finds it where it was, speed 0
                        E.track(s, pose, dist)
        return f

    def after_total(total):
        def g(before, after, W_):
            want = min(total, W_.oracle_mod.MAX_TRACKS)
            got = int(after["si"][SI["NTRACKS"]])
            if got != want:
                return "track list holds %d after the step, the record says %d" % (got, want)
            if not W_.gt and total <= W_.slots and got and not (after["trk"][:got, TF["DQLEN"]] >= 1).all():
                return "a live track without a deque entry"
            return None
        return g

    if not W.gt:
        counts = sorted({0, 1, K - 1, K, K + 1, S - 2, S - 1, S})
        for nt in counts:
            for new in (0, 1, 2):
                total = nt + new
                if total > W.oracle_mod.MAX_TRACKS and W.slots > W.oracle_mod.MAX_TRACKS:
                    continue                          # the wide world: totals stay within what the oracle holds
                over = total > W.slots
                edges = ["total=S%+d" % (total - S)] if S - 1 <= total <= S + 2 else []
                edges += ["dqlen=1"] if nt else []
                edges += ["dqlen=2", "duplicates", "on detection", "speed=0"] if nt > 1 else []
                out.append(Record("tracker", "ntracks=%d new=%d" % (nt, new), "tracks duplicated at resets sit on one pedestrian; %d more walk into sight" % new,
                                  lidar_record(nt, new), both("overflow" if over else "none"), rest=True, edges=tuple(edges), after0=after_total(total)))

        def touching(E):
            kept, st = scene(E, 1)
            t = st["trk"][0]
            E.si[SI["NTRACKS"]] = 1
            E.trk[:] = 0.0
            E.track(0, (_touching(t[TF["PX"]]), t[TF["PY"]]), t[TF["DIST"]])
        out.append(Record("tracker", "box touches", "a track of a pedestrian that has moved one box width since", touching, both("none"), rest=True,
                          edges=("iou=0",), after0=after_total(1)))
    else:
        P = W.P
        for nt in sorted({0, 1, K, min(P, S)}):
            for vis, ids in ((0, None), (1, (0,)), (2, (0, P - 1)), (2, None)):
                def f(E, nt=nt, vis=vis, ids=ids):
                    E.stand(x0, y0, 0.0)
                    kept = E.park(keep=list(ids) if ids else vis)
                    for j, i in enumerate(kept):
                        E.put(i, x0 + 0.4 * math.cos(bearings[j]), y0 + 0.4 * math.sin(bearings[j]))
                    E.si[SI["NTRACKS"]] = nt
                    E.trk[:] = 0.0
                    for s in range(nt):                                   # last step's list: pedestrian s was in sight (deque length 0, T = its id)
                        E.track(s, (x0 + 0.3, y0), 0.25, dqlen=0, t=float(s % P), speed=0.1, vel=(0.05, -0.05))
                edges = ("in sight=%d" % vis,) + (("ids 0 and P-1",) if ids and len(ids) == 2 else ()) + (("dqlen=0",) if nt else ())
                out.append(Record("tracker", "ntracks=%d in sight=%d%s" % (nt, vis, " ids" if ids else ""), "the list of the pedestrians that were in sight; %d are now" % vis,
                                  f, both("none"), rest=True, edges=edges, after0=after_total(vis)))
    return out


def tracker_edges(W):
    if not W.has_tracker:
        return []
    if W.gt:
        return ["in sight=0", "in sight=1", "in sight=2", "ids 0 and P-1", "dqlen=0"]
    wide = W.slots > W.oracle_mod.MAX_TRACKS
    return ["total=S-1", "total=S+0"] + ([] if wide else ["total=S+1", "total=S+2"]) + ["dqlen=1", "dqlen=2", "duplicates", "on detection", "speed=0", "iou=0"]


def clocks(W):
    """crowd_ms so that this step's advance carries out of CROWD_LO (2^32 - 16 as in a seven-hour run, and 2^32 - step: LO lands on 0);
    crowd_ms == 0, T - 10, T - dt_ms modulo ped_cycle_ms T and on the last pedestrian's assignment instant, each once small and once above
    2^32; every cold counter non-zero and distinct, the violation counters, obstacle steps, success, failure and episodes at 2^24 where
    a float32 stops counting by one, an informational status bit already set; ep_return and last_return large enough that the float32 cast
    rounds -- each carried through a step that ends nothing and through one that ends the episode.  Left out as unreachable: crowd_ms ==
    T - 1 modulo T -- the clock advances by dt_ms, scan_latency_ms and settle_ms, all multiples of 10 ms.  (The original layout has no
    confirmed-object or entry table, ORIG:278-322: there an observation stores NCONF = NENTRIES = 0 on both sides, whatever was planted.)  (The counters' values are
    carried, not computed: a run reaches 2^24 violations only with a max_steps of that size; success / failure beyond 1 only as sums a
    caller restored.)"""
    out = []
    T, step = W.T, W.step_ms

    def crowd(ms):
        def f(E):
            E.set_crowd(ms)
        return f
    out.append(Record("clocks", "carry 2^32-16", "27 M calls into a run the clock's low word carries", crowd(2 ** 32 - 16), both("none"), edges=("carry",),
                      after0=lambda b, a, W_: None if (int(a["si"][SI["CROWD_HI"]]), int(a["si"][SI["CROWD_LO"]])) == (1, step - 16) else "no carry: %r" % a["si"][12:14]))
    out.append(Record("clocks", "carry to 0", "... and lands on 2^32 exactly", crowd(2 ** 32 - step), both("none"), edges=("carry",),
                      after0=lambda b, a, W_: None if (int(a["si"][SI["CROWD_HI"]]), int(a["si"][SI["CROWD_LO"]])) == (1, 0) else "no carry: %r" % a["si"][12:14]))
    last = ((W.P - 1) * W.stagger) % T
    for name, ph in (("0", 0), ("T-10", T - 10), ("T-dt", (T - W.cfg["dt_ms"]) % T), ("last instant", last)):
        for tag, cycles in (("small", 3), ("above 2^32", 2 ** 32 // T + 5)):
            out.append(Record("clocks", "crowd phase %s %s" % (name, tag), "the crowd's clock is a multiple of 10 ms: every such phase is passed", crowd(cycles * T + ph),
                              both("none"), edges=("phase %s" % name, tag)))

    def counters(end):
        def f(E):
            si = E.si
            si[SI["EGO_VIOL"]], si[SI["SOCIAL_VIOL"]], si[SI["OBST_STEPS"]] = 2 ** 24, 2 ** 24 - 1, 2 ** 24 + 1
            si[SI["SUCCESS"]], si[SI["FAILURE"]], si[SI["EPISODES"]] = 2 ** 24 + 3, 2 ** 24 - 3, 2 ** 24 + 5
            si[SI["STATUS"]] |= ST_TRACK_WIDE
            si[SI["NCONF"]], si[SI["NENTRIES"]] = 5, 3
            E.park()                                   # (nobody near: the step that ends nothing must not meet a pedestrian)
            if end:
                si[SI["EP_STEP"]] = W.max_steps - 1
        return f
    out.append(Record("clocks", "cold counters", "counters of a long run, all non-zero", counters(False), both("none"), edges=("cold",)))
    out.append(Record("clocks", "cold counters, episode ends", "... at the call that ends the episode", counters(True), both("timeout"), edges=("cold", "cold end")))

    def returns(end):
        def f(E):
            E.sd[SD["EP_RETURN"]], E.sd[SD["LAST_RETURN"]] = 16777217.0, -33554435.0          # 2^24 + 1, -(2^25 + 3): not float32 values
            if end:
                E.si[SI["EP_STEP"]] = W.max_steps - 1
        return f
    out.append(Record("clocks", "large returns", "returns of a long episode: the float32 cast rounds", returns(False), both("none"), edges=("returns",)))
    out.append(Record("clocks", "large returns, episode ends", "... at the call that ends the episode", returns(True), both("timeout"), edges=("returns",)))
    return out


EDGES["clocks"] = ["carry", "phase 0", "phase T-10", "phase T-dt", "phase last instant", "small", "above 2^32", "cold", "cold end", "returns"]


def records(W):
    out = episode_end(W) + thresholds(W) + angles(W) + pedestrians(W) + tracker(W) + clocks(W)
    assert all(r.family in FAMILIES and all(ev in EVENTS for ev, _ in r.expect.values()) for r in out)
    return out


def required_edges(W, family):
    return tracker_edges(W) if family == "tracker" else EDGES[family]


# ---- a plan: every record of a world in one set of arrays ---------------------------------------------------------------------------------
Plan = namedtuple("Plan", "world records arrays base actions")
KEYS = ("sd", "si", "ped_p", "ped_v", "trk", "ped_aux")
_plans = {}


def base_actions(n):
    return M.actions(BASE_STEPS, n, BASE_SEED)


def plan(world, oracle_mod):
    """The planted arrays of a world (cached: the records are a function of the world's configuration): N = len(records) environments,
    arrays sd / si / ped_p / ped_v / trk [N, slots, 12] / ped_aux, and the [STEPS, N, 2] float32 actions (0 for the records at rest)."""
    if world in _plans:
        return _plans[world]
    W = World(world, oracle_mod)
    recs = records(W)
    N = len(recs)
    orc = oracle_mod.Oracle(W.config(N))
    orc.reset()
    for a in base_actions(N):
        _, _, done, _ = orc.step(a.astype(np.float64), auto_reset=False)
        assert not done.any(), (world, "an episode ended inside the base")
    states = [orc.get_state(e, trk_cap=W.slots) for e in range(N)]
    base = {k: np.stack([s[k] for s in states]) for k in KEYS}
    arrays = {k: v.copy() for k, v in base.items()}
    for e, r in enumerate(recs):
        r.edit(Env(W, e, arrays))
    acts = M.actions(STEPS, N, ACTION_SEED).copy()
    acts[:, [r.rest for r in recs]] = 0.0
    for e, r in enumerate(recs):
        if r.actions is not None:
            acts[:, e] = np.asarray(r.actions, dtype=np.float32)
    _plans[world] = Plan(W, recs, arrays, base, acts)
    return _plans[world]


def plant_oracle(p, oracle_mod):
    """a fresh oracle of the plan's world holding the planted arrays (its own ped_init / ped_preset: functions of the configuration)"""
    N = len(p.records)
    orc = oracle_mod.Oracle(p.world.config(N))
    orc.reset()
    a = p.arrays
    for e in range(N):
        orc.set_state(e, a["sd"][e], a["si"][e], a["ped_p"][e], a["ped_v"][e], a["trk"][e], None, None, a["ped_aux"][e])
    return orc


def snapshot_arrays(p, fresh):
    """the sections of a blob to restore: the planted arrays, ped_init and ped_preset from `fresh`, the split of the handle's own snapshot"""
    return dict({k: p.arrays[k] for k in KEYS}, ped_init=fresh["ped_init"], ped_preset=fresh["ped_preset"])


def oracle_states(orc, slots):
    """every environment's state record, stacked: KEYS, and cp_pow_sq [N] (the flag of bisect_divergence.first_state_difference's rule)"""
    states = [orc.get_state(e, trk_cap=slots) for e in range(orc.N)]
    return {k: np.stack([s[k] for s in states]) for k in KEYS + ("cp_pow_sq",)}


_runs = {}


def run_oracle(p, oracle_mod, mode):
    """plant and step the oracle alone (once per world and reset convention; nothing changes the result afterwards): the states before,
    [(outputs, states after the step)] for the STEPS steps, and the oracle's counters [N, 6] and last returns [N] at the end"""
    key = (p.world.name, mode)
    if key not in _runs:
        orc = plant_oracle(p, oracle_mod)
        before = oracle_states(orc, p.world.slots)
        steps = []
        for a in p.actions:
            out = M.oracle_step(orc, a, mode)
            steps.append((out, oracle_states(orc, p.world.slots)))
        _runs[key] = (before, steps, (orc.counters(), orc.returns()))
    return _runs[key]


def first_state_record_difference(snapshot, states, risk_mode, skip=()):
    """kernel_matrix.first_state_record_difference against stored oracle states (oracle_states) instead of a live oracle, leaving out the
    environments in `skip`: the same rule, bisect_divergence.first_state_difference, environment by environment"""
    from bisect_divergence import first_state_difference
    from crowdnav import _abi
    _, arrs = _abi.split_snapshot(snapshot)
    for e in range(arrs["sd"].shape[0]):
        if e in skip:
            continue
        g = {k: arrs[k][e] for k in KEYS}
        o = {k: states[k][e] for k in KEYS}
        if all(np.array_equal(g[k], o[k], equal_nan=(k != "si")) for k in KEYS):
            continue
        d = first_state_difference(g, dict(o, cp_pow_sq=int(states["cp_pow_sq"][e])), e, risk_mode=risk_mode)
        if d is not None:
            return "state of env %d, %s: got %r, oracle %r" % ((e,) + tuple(d))
    return None


def oracle_overflowed(si, W):
    """[N] bool: the oracle's statement of "the track list outgrew S" (see the module docstring)"""
    return ((si[:, SI["STATUS"]] & ST_TRACK_OVERFLOW) != 0) | (si[:, SI["NTRACKS"]] > W.slots)


# how many records of a world name the overflow: the S+1 / S+2 totals of the lidar tracker worlds (ntracks S-1 with 2 new, S with 1 and 2);
# none where the list is rebuilt every step (gt), absent (orig) or wide
N_OVERFLOW = {"rw": 3, "orig": 0, "wide": 0, "wa": 3, "gt_wa": 0, "sfd": 3, "gt_sfd": 0, "sf": 3, "gt_sf": 0, "ct": 3, "gt_ct": 0, "gt": 0, "generic": 3,
              "s360": 3, "s720": 3}


def overflow_records(p):
    return [e for e, r in enumerate(p.records) if any(ev == "overflow" for ev, _ in r.expect.values())]


def check_premise(p, before, steps, mode):
    """every named event in its step, no status bit a record does not name, finite outputs, the first step's after0: a list of texts"""
    W, bad = p.world, []
    n = W.R - 1
    for e, r in enumerate(p.records):
        event, at = r.expect[mode]
        who = "%s / %s (env %d, %s)" % (r.family, r.name, e, mode)
        prev = {k: before[k][e] for k in KEYS}
        ended, over = [], []
        for t, (out, st) in enumerate(steps):
            si, sd = st["si"][e], st["sd"][e]
            for k in ("obs", "reward", "final"):
                if not np.isfinite(out[k][e]).all():
                    bad.append("%s: step %d %s not finite" % (who, t, k))
            if out["done"][e]:
                if prev["si"][SI["DONE"]]:
                    kind = "held"
                elif si[SI["SUCCESS"]] == 1 and si[SI["FAILURE"]] == 0:      # compute_reward's verdict (ENV:1131): inside the goal box
                    kind = "goal"
                elif sd[SD["LAST_EP_STEPS"]] < W.max_steps or float(out["final"][e][:n].min()) < W.min_range:
                    kind = "collision"
                else:
                    kind = "timeout"
                ended.append((kind, t))
            elif mode == "next" and prev["si"][SI["PENDING_RESET"]] and si[SI["EP_STEP"]] == 0 and out["reward"][e] == 0.0:
                ended.append(("reset", t))
            if oracle_overflowed(st["si"][e:e + 1], W)[0] and not oracle_overflowed(prev["si"][None], W)[0]:
                over.append(t)
            if t == 0 and r.after0 is not None:
                d = r.after0(prev, {k: st[k][e] for k in KEYS}, W)
                if d:
                    bad.append("%s: %s" % (who, d))
            prev = {k: st[k][e] for k in KEYS}
        if event == "overflow":
            if over[:1] != [at] or ended:
                bad.append("%s: expected the track list to outgrow the slots in step %d and nothing else, got %s, %s" % (who, at, over, ended))
        elif over:
            bad.append("%s: the track list outgrew the slots in step %s, which the record does not name" % (who, over))
        if event == "none" and ended:
            bad.append("%s: expected no event, got %s" % (who, ended))
        if event not in ("none", "overflow") and ended[:1] != [(event, at)]:
            bad.append("%s: expected %s in step %d, got %s" % (who, event, at, ended))
        raised = int(steps[-1][1]["si"][e][SI["STATUS"]]) & ~int(before["si"][e][SI["STATUS"]])
        named = r.status | (ST_TRACK_OVERFLOW if event == "overflow" else 0)
        if raised & ~named:
            bad.append("%s: raised status bits %d, named %d" % (who, raised, named))
    return bad



# ---- cn_restore's record check (csrc/crowdnav_snapshot_check.h): record sets for the stand-alone walker, and one violation per field -----
RECORD_SET_MAGIC = 0x43524E43          # "CNRC"


def write_record_set(f, cfg, slots, max_conf, arrays):
    """One set for the walker of tests/test_planted_states.py: int32 {magic, slots, max_conf, N, P, sizeof(cn_config)}, the cn_config, then
    sd, si, ped_p, ped_v, trk as cn_snapshot lays them out.  cfg: a crowdnav.Config whose n_envs is the set's N."""
    c = cfg.to_c()
    N, P = arrays["sd"].shape[0], cfg.n_peds
    assert c.n_envs == N and arrays["trk"].shape == (N, slots, 12) and arrays["ped_p"].shape == (N, P, 2)
    f.write(np.array([RECORD_SET_MAGIC, slots, max_conf, N, P, C.sizeof(c)], dtype=np.int32).tobytes())
    f.write(bytes(c))
    for k, dt in (("sd", np.float64), ("si", np.int32), ("ped_p", np.float64), ("ped_v", np.float64), ("trk", np.float64)):
        f.write(np.ascontiguousarray(arrays[k], dtype=dt).tobytes())


def violations(W, arrays):
    """[(name, the verdict's text up to the value, edit(arrays))]: every field of the record check out of range once, each in an
    environment of its own choosing; `arrays` (valid records, as a plan's) is only read.  A violation of a tracker row first makes the
    row live (NTRACKS >= 1 with a valid row) where the world's records have no tracks."""
    N = arrays["sd"].shape[0]
    out = []

    def si(field, value, e):
        def f(a):
            a["si"][e, SI[field]] = value
        out.append(("si.%s=%d" % (field, value), "env %d: si.%s = " % (e, field), f))

    def sd(field, value, e):
        def f(a):
            a["sd"][e, SD[field]] = value
        out.append(("sd.%s=%r" % (field, value), "env %d: sd.%s = " % (e, field), f))

    def ped(section, i, c, value, e):
        def f(a):
            a[section][e, i, c] = value
        out.append(("%s[%d].%s=%r" % (section, i, "xy"[c], value), "env %d: %s[%d].%s = " % (e, section, i, "xy"[c]), f))

    def trk(field, value, e, slot=0):
        def f(a):
            if a["si"][e, SI["NTRACKS"]] <= slot:
                a["si"][e, SI["NTRACKS"]] = slot + 1
                a["trk"][e, :slot + 1] = 0.0
            a["trk"][e, slot, TF[field]] = value
        out.append(("trk[%d].%s=%r" % (slot, field, value), "env %d: trk[%d].%s = " % (e, slot, field), f))
    envs = iter(np.random.default_rng(5).permutation(N).tolist() * 2)
    for field, bad in (("NTRACKS", (W.slots + 1, -1)), ("DQ_LEN", (3, -1)), ("DONE", (2, -1)), ("PENDING_RESET", (2, -1)), ("EP_STEP", (-1, -2 ** 31)),
                       ("NCONF", (max(W.max_conf, W.slots) + 1, -1)), ("NENTRIES", (W.slots + 1, -1)), ("CROWD_HI", (-1, -2 ** 31))):
        for v in bad:
            si(field, v, next(envs))
    for field, bad in (("RX", (math.nan, math.inf, math.nextafter(W.h, math.inf))), ("RY", (math.nan, -math.inf, -math.nextafter(W.h, math.inf))), ("RYAW", (math.nan, math.inf))):
        for v in bad:
            sd(field, v, next(envs))
    ped("ped_p", 0, 0, math.nan, next(envs)); ped("ped_p", W.P - 1, 1, math.nextafter(W.h, math.inf), next(envs)); ped("ped_p", W.P // 2, 0, -math.inf, next(envs))
    ped("ped_v", 0, 1, math.nan, next(envs)); ped("ped_v", W.P - 1, 0, math.inf, next(envs))
    trk("DQLEN", 3.0, next(envs)); trk("DQLEN", -1.0, next(envs)); trk("DQLEN", 1.5, next(envs)); trk("DQLEN", math.nan, next(envs))
    trk("PX", math.nan, next(envs)); trk("SPEED", math.inf, next(envs), slot=1); trk("VY", -math.inf, next(envs))
    if W.gt:
        trk("T", float(W.P), next(envs)); trk("T", -1.0, next(envs)); trk("T", 0.5, next(envs)); trk("T", math.nan, next(envs))
    else:
        trk("T", math.nan, next(envs)); trk("D0X", math.inf, next(envs))
    return out
