/*
 * crowdnav.h -- C-ABI of libcrowdnav.so, the MI355X-native batched crowd-navigation environment.
 *
 * The reference has no FFI layer: its hot path is the Python object `Env`
 * (turtlebot3_rl_sim/src/environment_stage_1_nobonus.py:42) driven by
 * start_td3_training.py:106-166 and backed by Gazebo + a separate crowd node
 * (crowd_behaviors/simulate_crowd.py).  This header is the boundary a drop-in replacement
 * exports; each entry point cites the reference interface it replaces.
 * The Python binding a maintainer would add is shown in INTEGRATION.md and shipped in
 * drl-based-mapless-crowd-navigation-with-perceived-risk_amd/crowdnav/_abi.py.
 *
 * Conventions
 *   - plain pointers and sizes only; every array is caller-owned
 *   - "dev" pointers are device (HBM) pointers on the handle's GPU, "host" pointers are host memory
 *   - cn_reset / cn_step only enqueue work on `stream` (a hipStream_t; NULL = default stream)
 *     and return immediately; no hidden synchronisation
 *   - return value 0 = OK, negative = error; cn_last_error() gives a thread-local message;
 *     nothing throws across the boundary
 *   - there is NO CPU fallback: cn_create fails (CN_ERR_NO_DEVICE) when no HIP device exists
 */
#ifndef CROWDNAV_H
#define CROWDNAV_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CN_ABI_VERSION 7
#define CN_MAX_TRACKS 64      /* largest per-env capacity of the LDS tracker table (ENV:656-743): one lane per track */
#define CN_MAX_TRACKS_WIDE 1024   /* largest per-env capacity of the wide (HBM) tracker table: track_capacity 128 ... 1024 */
#define CN_MAX_K 16

enum {
    CN_OK = 0,
    CN_ERR_ARG = -1,
    CN_ERR_CONFIG = -2,
    CN_ERR_NO_DEVICE = -3,
    CN_ERR_HIP = -4,
    CN_ERR_SIZE = -5
};

/* per-env status bits (cn_get_counters column 6), all sticky:
 *   CN_ST_TRACK_OVERFLOW  the track list outgrew track_capacity; the tracks that did not fit were dropped (risk features from a
 *                         truncated list from then on)
 *   CN_ST_TTC_ZERO        a time-to-collision of exactly 0 was met
 *   CN_ST_DT_ZERO         the agent's time step was exactly 0 (UTL:227-236 divide by it)
 *   CN_ST_CONF_OVERFLOW   the confirmed-object table overflowed
 *   CN_ST_TRACK_WIDE      informational: the track list has once held more than CN_MAX_TRACKS (64) tracks -- only a wide table
 *                         (track_capacity >= 128) keeps them; past this point a 64-slot tracker would have overflowed */
enum { CN_ST_TRACK_OVERFLOW = 1, CN_ST_TTC_ZERO = 2, CN_ST_DT_ZERO = 4, CN_ST_CONF_OVERFLOW = 8, CN_ST_TRACK_WIDE = 16 };

/* Every field of Env.__init__'s rosparam reads (ENV:71-91), the robot/lidar constants of the
 * URDF/XACRO and world files, and the crowd node's constants.  SURVEY.md appendix B cites each. */
enum { CN_LAYOUT_RISK = 0, CN_LAYOUT_ORIGINAL = 1, CN_LAYOUT_REALWORLD = 2 };
/* where the perceived-risk features (rows A21-A24) take their obstacles from */
enum { CN_RISK_LIDAR_TRACKER = 0, CN_RISK_GT = 1 };

typedef struct cn_config {
    int32_t n_envs;          /* N environments in this handle (this GPU's shard) */
    int32_t n_peds;          /* P pedestrians (obstacle cylinders) per env */
    int32_t n_rays;          /* R lidar samples (XACRO:157 -> 360); the observation uses R-1 */
    int32_t k_obstacles;     /* K tracked obstacles in the observation (ENV:55 -> 8) */
    int32_t max_steps;       /* Env(max_step=...) (ENV:43,91) */
    int32_t ped_mode;        /* 0: U(-vmax,vmax) velocity per cycle (CROWD:98-126); 1: constant preset table;
                              * 2: social-force pedestrians (BASELINE north_star; Helbing-Molnar: goal attraction + pedestrian,
                              *    wall and robot repulsion, 10 ms ticks; sf_* below; no reference source -- CROWD:98-126 is a
                              *    random-velocity walker -- so it is pinned by analytic known-answer cases only) */
    int32_t dt_ms;           /* time.sleep(0.15) in Env.step (ENV:1201) -> 150 */
    int32_t scan_latency_ms; /* wait_for_message('scan') (ENV:1218,1238) -> 10 */
    int32_t settle_ms;       /* trainer's time.sleep(0.1) after reset (TRAIN:114) -> 100 */
    int32_t ped_cycle_ms;    /* crowd node cycle: 0.1 s x number of obstacles (CROWD:128-144) */
    int32_t ped_stagger_ms;  /* 0.1 s between consecutive obstacles' updates (CROWD:144) -> 100 */
    int32_t track_capacity;  /* tracker slots per env: 0 = auto (32 for <= 40 pedestrians -- <= 32 with risk_mode gt --, else 64), or 32 / 64
                              * (the table lives in LDS), or 128 / 256 / 512 / 1024: a WIDE table, used in place in HBM, for long runs
                              * whose track list (the reference's is unbounded and survives reset) outgrows 64 -- opt-in, slower, and
                              * only for obs_layout 0 with risk_mode lidar_tracker and the plain simulator (ped_mode 0 / 1, no
                              * ped_contact, no wheel_accel); cn_create refuses it elsewhere and names why */
    int32_t obs_layout;      /* CN_LAYOUT_RISK (0): environment_stage_1_nobonus.py, obs = R-1 + 7 + 4K (TD3 / DDPG trainers);
                              * CN_LAYOUT_ORIGINAL (1): environment_stage_1_original.py:278-402, obs = R-1 + 4 =
                              * rounded ranges + heading + distance + rounded (x, y) (SAC / DQN / Q-learning trainers);
                              * CN_LAYOUT_REALWORLD (2): environment_stage_1_nobonus_realworld.py:208-749, obs = R-1 + 11 = unrounded
                              * ranges + heading + distance + rounded (x, y) + the constant yaw 3.14 + rounded twist features +
                              * pose and velocity of the one obstacle with the highest collision probability (the physical-robot
                              * script: set dt_ms = 50, RW:880-883; normally driven through cn_observe_external) */
    int32_t geos_untyped_empty; /* shapely/GEOS version switch for UTL:279,306 `str(i) != 'LINESTRING EMPTY'`:
                              * 0: GEOS >= 3.9 typed empties (a miss prints 'LINESTRING EMPTY' and is skipped);
                              * 1: GEOS <= 3.8 (the reference's Python-2.7 / shapely <= 1.7 platform): a miss prints
                              *    'GEOMETRYCOLLECTION EMPTY', the comparison is true, `.geoms` of the empty result is
                              *    empty and the [0] raises -> get_collision_point returns None on the FIRST candidate
                              *    that misses, and get_local_goal_waypoints takes its except branch */
    int32_t ped_contact;     /* 0: pedestrians pass through each other and the robot (round-1 simulator);
                              * 1: frictionless rigid contact, disc-disc and disc-robot (WORLD:86-145 mu = 0 cylinders) */
    int32_t risk_mode;       /* CN_RISK_LIDAR_TRACKER (0): the reference's lidar segmentation + tracker (ENV:329-760);
                              * CN_RISK_GT (1): A21-A24 fed with the simulator's own pedestrians (nearest surface point,
                              *    true velocity) within lidar range and line of sight; indices = pedestrian ids */
    int32_t py2_round;       /* 0: Python-3 round() (ties-to-even on the exact binary value; round(np.float64, n) is numpy's
                              *    multiply / rint / divide) -- what the goldens were recorded under;
                              * 1: Python-2.7 round(), the reference's platform (README.md:108-110): exact ties go AWAY from zero,
                              *    and round(np.float64, n) is the builtin's correctly rounded decimal too (ENV:255, ORIG:280, RW:209).
                              *    Every round() site: ENV:1208, 329-346, 1025-1042, UTL:122-123, 460 ... (np.around at ENV:1042 stays numpy) */
    int32_t sf_tick_ms;      /* ped_mode 2: physics tick of the social-force integrator, ms; 0 -> 10 (the contact model's tick).  The model is
                              * an explicit scheme, so the tick is part of its definition: 10 ms resolves a 0.2 m/s crowd to 2 mm per tick,
                              * 50 ms (the usual choice for social-force crowds, tau = 0.5 s) costs a fifth */
    int32_t scan_f32;        /* 0: the simulated lidar hands Env.get_state float64 ranges (rounds 1-3);
                              * 1: every range is rounded to float32 first -- what sensor_msgs/LaserScan.ranges (float32[]) carries from
                              *    gazebo_ros_laser (XACRO:172-175) to ENV:1218's wait_for_message.  Simulator side only: the reference code
                              *    behind it is unchanged, but its exact-equality tests (`round(scan, 3) == 0.6`, ENV:324-346) then see
                              *    float32-representable inputs.  Externally supplied scans (cn_observe_external) are taken as they are */
    int32_t waypoint_reward; /* ENV:1116 `waypoint_reward = 200` -> 200.  The published training log (results/td3/revamped/
                              * new_tracking_cp_gcp_nobonus_corrected_3/td3_training.csv, 3021 episodes) never contains it -- its largest
                              * episode return is 173 < 200 -- while the committed reward pays it whenever the robot comes within
                              * goal_eps of a way-point 0.3 m ahead, i.e. on most steps of a diagonal run:
                              * 0 reproduces the reward the log was recorded under ("nobonus") */
    int64_t env_index_base;  /* global index of env 0: RNG streams are keyed by global index */
    uint64_t seed;
    double room_half;        /* WORLD:926-1108 -> 1.40 */
    double ped_radius;       /* WORLD:109 -> 0.0505 */
    double ped_vmax;         /* CROWD:101-102 -> 0.2 */
    double robot_clearance;  /* robot centre kept this far from the walls -> 0.09 */
    double lidar_min;        /* XACRO:164 -> 0.08 */
    double lidar_max;        /* XACRO:165 -> 0.60 */
    double lidar_span;       /* XACRO:159-160 -> 6.28 rad */
    double lidar_offset_x;   /* URDF:134-138 -> -0.032 */
    double max_scan_range;   /* turtlebot3_world.yaml:7 -> 0.6 */
    double min_scan_range;   /* turtlebot3_world.yaml:8 -> 0.12 (0.0 for evaluation); must be < max_scan_range (ENV:581 divides by the difference) */
    double goal_x, goal_y;   /* desired_pose (turtlebot3_world.yaml:10-13) */
    double start_x, start_y; /* starting_pose: the heading offset of ENV:223-224 only */
    double spawn_x, spawn_y, spawn_yaw; /* launch-file spawn pose (1.0, -1.0, 3.14) */
    double waypoint_radius;  /* ENV:250 -> 0.3 */
    double goal_eps;         /* ENV:1285,1303 -> 0.20 */
    /* ped_mode 2 (social force).  Per pedestrian i: desired speed v0_i = ped_vmax (0.5 + 0.5 u_i), a goal point drawn uniformly
     * in the room (re-drawn when within sf_goal_eps of it), and per 10 ms tick
     *   a = (v0 e_goal - v) / sf_tau + sum_j q(sf_A exp((2 r - d_ij) / sf_B) n_ij)       (other pedestrians; q rounds each component to
     *                                                                                    the nearest multiple of 2^-36 m/s^2, which makes
     *                                                                                    the sum exact and independent of its order -- the
     *                                                                                    kernels evaluate every unordered pair once and
     *                                                                                    scatter +-; needs n_peds sf_A e^(2r/sf_B) < 2^15)
     *     + sum_walls sf_wall_A exp((r - d_w) / sf_wall_B) n_w                            (-x, +x, -y, +y)
     *     + sf_A exp((r + robot_clearance - d_ir) / sf_B) n_ir                            (the robot)
     *   v <- v + a h, |v| capped at 1.3 v0;  x <- clamp(x + v h) into the room   (semi-implicit Euler, h = sf_tick_ms) */
    double sf_tau;           /* relaxation time -> 0.5 s (Helbing & Molnar 1995) */
    double sf_A;             /* pedestrian / robot repulsion strength, m/s^2 -> 0.8 (2.1 at full walking speed, scaled to 0.2 m/s crowds) */
    double sf_B;             /* ... and range, m -> 0.10 */
    double sf_wall_A;        /* wall repulsion strength, m/s^2 -> 1.0 */
    double sf_wall_B;        /* ... and range, m -> 0.05 */
    double sf_goal_eps;      /* a goal counts as reached within this distance -> 0.10 */
    /* Wheel dynamics of the diff-drive plugin (XACRO:57-72: libgazebo_ros_diff_drive.so, updateRate 100, wheelSeparation 0.160,
     * wheelAcceleration 1, wheelTorque 10).  wheel_accel = 0: kinematic robot, the commanded twist is the twist (rounds 1-3).
     * wheel_accel > 0 (XACRO:70 -> 1.0 m/s^2): the plugin's wheel-speed ramp, restated from gazebo_ros_pkgs'
     * gazebo_ros_diff_drive.cpp (UpdateChild / getWheelVelocities / UpdateOdometryEncoder; third-party, not vendored by the
     * reference, so this is its published algorithm and not a pinned parity): on plugin ticks of 10 ms
     *   target wheel speeds  tl = v_cmd - w_cmd * sep / 2,  tr = v_cmd + w_cmd * sep / 2
     *   if |tl - cl| < 0.01 or |tr - cr| < 0.01:  cl = tl, cr = tr          (either wheel within tolerance releases both)
     *   else  cl += clamp(tl - cl, -a h, +a h),  cr += clamp(tr - cr, -a h, +a h)
     *   the tick's twist v = (cl + cr) / 2, w = (cr - cl) / sep moves the robot by the mid-point rule; /odom reports that twist.
     * A commanded 0 <-> 0.22 m/s then takes 0.22 s (1.5 control periods), a full turn command w = 2 rad/s 0.16 s.
     * Requires obs_layout 0 and the plain simulator (ped_contact 0, ped_mode 0 / 1). */
    double wheel_accel;      /* m/s^2 at the wheel rim; 0 = off */
    double wheel_separation; /* XACRO:68 -> 0.160 */
} cn_config;

typedef struct cn_env_s* cn_handle;

/* Replaces Env.step(action, step_counter, mode="continuous") -> (state, reward, done)
 * (ENV:1164-1225) for N envs at once. */
typedef struct cn_step_io {
    const float* action;         /* dev [N,2]  (v, w), already clipped by the caller (TD3:214-215) */
    const int32_t* step_counter; /* dev [N] 1-based (TRAIN:125) or NULL = per-env internal counter */
    float* obs;                  /* dev [N, D], D = cn_obs_dim(): 366+4K (obs_layout 0) or R-1+4 (obs_layout 1);
                                  * with auto_reset: first obs of the new episode where done */
    float* final_obs;            /* dev [N, 366+4K] or NULL: the observation Env.step returned (terminal if done) */
    double* obs_f64;             /* dev [N, 366+4K] or NULL: `obs` in float64 (the reference's dtype) */
    float* reward;               /* dev [N] */
    uint8_t* done;               /* dev [N] */
    int32_t* topk_idx;           /* dev [N,K] or NULL: tracker slot of each feature row, -1 = padding */
    int32_t auto_reset;          /* 0: none.  1: finished envs run Env.reset() (+TRAIN:114-116) inside the same call.
                                  * 2: "next-step" reset -- a finished env spends the NEXT call on Env.reset() (its
                                  *    action is ignored, reward 0, done 0, obs = first observation of the new episode) */
    int32_t reserved;
} cn_step_io;

/* Env.get_state + Env.compute_reward on EXTERNALLY supplied sensor data (ENV:245-1162): what the reference's
 * `Env` does when Gazebo -- or the physical robot of environment_stage_1_nobonus_realworld.py -- delivers the
 * /scan and /odom messages.  The library's own simulator is bypassed; tracker / waypoint / deque state is the
 * handle's.  This is also how the golden runs recorded from the reference are replayed through the kernel. */
typedef struct cn_external_io {
    const double* ranges;        /* dev [N,R] LaserScan.ranges as delivered: finite values >= 0, +inf = no return, NaN (ENV:1218,1238); a negative
                                  * range is not a LaserScan value and is outside the domain (clip before the call) */
    const double* odom;          /* dev [N,10]: position x, y, yaw, linear_twist.x, angular_twist.z (ENV:239-243),
                                  *   time.time() inside get_state, position x, y at the end of time.sleep (ENV:1208),
                                  *   end_timestep (ENV:1202), reserved */
    const int32_t* step_counter; /* dev [N] (ignored for the reset flow) */
    float* obs;                  /* dev [N, 366+4K] */
    double* obs_f64;             /* dev [N, 366+4K] or NULL */
    float* reward;               /* dev [N] */
    uint8_t* done;               /* dev [N] */
    int32_t* topk_idx;           /* dev [N,K] or NULL */
    int32_t is_reset;            /* 1: Env.reset() flow (ENV:1243-1262 + TRAIN:116), 0: Env.step() flow (ENV:1208-1223) */
    int32_t phase;               /* 0: the whole flow selected by is_reset.  Otherwise a mask of the pieces of Env.step, so that
                                  * get_state and compute_reward can be called separately as ENV:1222-1223 does:
                                  *   CN_PHASE_PRE          ENV:1208-1209 agent_pose_deque.append + agent_vel_timestep (odom[6..8])
                                  *   CN_PHASE_GET_STATE    Env.get_state(scan, step_counter, action) -> obs, done (ENV:245-1044)
                                  *   CN_PHASE_REWARD       Env.compute_reward(state, step_counter, done) -> reward, done
                                  *                         (ENV:1046-1162): reads state[R-1], state[R] from obs_f64 (or obs)
                                  *                         and `done` as INPUTS, position from odom[0..1]
                                  * A launch writes only what its pieces return: CN_PHASE_PRE alone writes no output.  Held by
                                  * tests/test_gpu_external.py: every grouping of the pieces leaves what phase 0 leaves and what
                                  * the reference returned, and each piece touches only its own part of the state. */
} cn_external_io;
enum { CN_PHASE_ALL = 0, CN_PHASE_PRE = 1, CN_PHASE_GET_STATE = 2, CN_PHASE_REWARD = 4 };

int cn_abi_version(void);
const char* cn_last_error(void);

/* Env.__init__ (ENV:43-168).  device = HIP device ordinal. */
int cn_create(const cn_config* cfg, int device, cn_handle* out);
void cn_destroy(cn_handle h);
int cn_obs_dim(cn_handle h);                       /* 366 + 4K (ENV:1038-1039) */
int cn_config_of(cn_handle h, cn_config* out);

/* World description (WORLD initial poses / scripted-crowd velocity tables), host arrays [N,P,2]. */
int cn_set_ped_init(cn_handle h, const double* xy_host);
int cn_get_ped_init(cn_handle h, double* xy_host);
int cn_set_ped_preset_vel(cn_handle h, const double* vxy_host);

/* Env.reset() (ENV:1227-1263) followed by the trainer's sleep(0.1) and `env.done = False`
 * (TRAIN:114-116).  mask: dev [N] or NULL (= all). obs_f64 may be NULL. */
int cn_reset(cn_handle h, const uint8_t* mask, float* obs, double* obs_f64, void* stream);
int cn_step(cn_handle h, const cn_step_io* io, void* stream);
/* Issue arbitration between the environments that share a SIMD (one environment = one wavefront).
 * The hardware serves a SIMD's OLDEST wavefront first; when the environments on a SIMD start together (a launch that fills
 * the device by itself) the launch then lasts as long as the wavefront that was starved.  CN_ARB_FAIR runs cn_step's kernel
 * with falling s_setprio levels -- whoever is behind gets the issue slots, all finish together: +8 % for one launch of 4096
 * environments per step -- and costs ~5 % when launches of several handles OVERLAP on the device (stream groups), where
 * oldest-first is the better pipeline.  CN_ARB_AUTO (the default): fair when this handle's launch alone puts at least two
 * wavefronts on every SIMD of the device (n_envs >= 8 x compute units) and it is stepped by cn_step or by a cn_step_multi
 * that names no other handle; oldest-first inside a cn_step_multi over several handles.  Changes when instructions issue, never a result.  Only the default configuration's kernel
 * (obs_layout 0, lidar_tracker, no contact / social force, reset on the next step or none) has a fair variant: elsewhere
 * the setting is accepted and ignored.  cn_get_arbitration returns what cn_step would use: CN_ARB_OLDEST_FIRST or CN_ARB_FAIR. */
#define CN_ARB_AUTO 0
#define CN_ARB_OLDEST_FIRST 1
#define CN_ARB_FAIR 2
int cn_set_arbitration(cn_handle h, int mode);
int cn_get_arbitration(cn_handle h);
/* Stream groups (ABI 6): how many environments the caller keeps in flight on this device TOGETHER with this handle's -- the sum over
 * the handles whose launches overlap (crowdnav.env.VecEnvGroups sets it for every group).  0 (the default) = this handle alone.
 * The 360-ray step kernels run four environments per workgroup while that total is resident at once (<= 16 wavefronts per CU) and
 * one per workgroup beyond; results are identical either way. */
int cn_set_group_envs(cn_handle h, int64_t total_envs);
/* Name of the device kernel a call on this handle launches right now (diagnostics: bench.py and the profile summaries key the
 * PMC counters of a run by it).  what: 0 = cn_step with auto_reset 0 / 2 and cn_reset, 1 = cn_step with auto_reset 1 (same-call
 * reset), 2 = cn_step_sequence, 3 = cn_observe_external, 4 = cn_step inside a cn_step_multi over several handles.  Handles whose
 * shape is the headline one (360 rays, 20 pedestrians, K = 8, default tracker slots) get kernels compiled for exactly that
 * shape (`..._s360`: the LDS map, word counts and loop bounds are constants there); results are identical.  NULL on error. */
const char* cn_kernel_name(cn_handle h, int what);
/* Diagnostics (bench.py's sustained leg): enqueues a one-thread kernel on `stream` that lives for `span_us` microseconds of the
 * constant 100 MHz counter (s_memrealtime) and stores in out_dev[0] the shader-clock cycles (s_memtime) and in out_dev[1] the 100 MHz
 * ticks that passed meanwhile: out[0] / (out[1] / 100) is the clock in MHz the chip ran at during that interval under whatever load
 * the other streams put on it.  (One wave, one die: the two counters are per XCD and readings of different kernels do not subtract.)
 * No reference counterpart. */
int cn_device_clock(int64_t* out_dev, int span_us, int device, void* stream);
/* n calls of cn_step in one crossing of the boundary: handle i steps with ios[i] on streams[i] (env batches run as
 * independent stream groups, DESIGN.md section 6: the launches are the same, the host thread pays the foreign-call
 * overhead once per step instead of once per group).  Stops at the first error and returns it. */
int cn_step_multi(int n, const cn_handle* handles, const cn_step_io* ios, void* const* streams);
/* n handles' environments in ONE launch, whatever n is: job j = handles[j] stepping with ios[j] rides in the grid's z dimension and
 * reads its argument block from row j of a device table that cn_step_group_create builds and uploads once (so the buffers of ios[j]
 * are bound for the group's life).  After cn_step_group_step every job's outputs and its whole state record are, bit for bit, what
 * cn_step(handles[j], &ios[j], stream) leaves; after cn_step_group_reset what cn_reset(handles[j], masks[j], ios[j].obs,
 * ios[j].obs_f64, stream) leaves (masks NULL, or masks[j] NULL: every environment of the job; masks[j]: dev [N_j]).  The handles
 * stay usable on their own between the group's calls; the caller orders a group's calls among themselves and against the handles'
 * own (one stream, or streams that wait for each other): cn_step_group_reset writes the masks' addresses into its table with a small
 * copy ahead of its launch.  cn_step_group_create refuses, before any device work and naming the job: n outside 1 ...
 * CN_STEP_GROUP_MAX, a null handle or null action / obs / reward / done, auto_reset 1 (the same-call reset has no group kernel),
 * handles on different devices, of different worlds or group kernels (one launch runs one kernel: cn_step_group_kernel_name; the
 * headline shape takes its two-wavefront kernel while all jobs' environments together are at most 8 x compute units), the same
 * handle twice, a handle with the profiling build's stage timing or ablation mask set.  No fair, four-per-workgroup, same-call-reset,
 * external, sequence or policy form.  Destroy a group BEFORE its handles. */
typedef struct cn_step_group_s* cn_step_group_handle;
#define CN_STEP_GROUP_MAX 64
int cn_step_group_create(int n, const cn_handle* handles, const cn_step_io* ios, cn_step_group_handle* out);
int cn_step_group_step(cn_step_group_handle g, void* stream);                     /* ONE launch */
int cn_step_group_reset(cn_step_group_handle g, const uint8_t* const* masks, void* stream);   /* ONE launch; masks NULL or per job NULL = all */
int cn_step_group_jobs(cn_step_group_handle g);
const char* cn_step_group_kernel_name(cn_step_group_handle g);
void cn_step_group_destroy(cn_step_group_handle g);
int cn_observe_external(cn_handle h, const cn_external_io* io, void* stream);

/* The actor's output stage as one launch (no handle needed): action = clip(heads(logits) + N(0, sigma)).
 * Replaces td3.py:103-104 (sigmoid*max_v, tanh*max_w), td3.py:67-78,209-211 (Gaussian exploration) and
 * td3.py:214-215 (clip).  logits, action: dev [n,2] float32; noise is keyed by (seed, counter, row). */
int cn_policy_tail(const float* logits, float* action, int n, float max_v, float max_w, float sigma,
                   uint64_t seed, uint64_t counter, int device, void* stream);   /* device: HIP ordinal, -1 = current */

/* The whole TD3 actor as one launch: Actor.forward (td3.py:96-106: Linear(obs_dim,256)-ReLU-Linear(256,256)-ReLU-
 * Linear(256,2), sigmoid*max_v / tanh*max_w heads) + Agent.act's exploration noise and clip (td3.py:209-215), in
 * float32 on the f32 matrix cores.  Weights are caller-owned device arrays:
 *   w1p = cn_actor_pack_weights(linear1.weight^T [obs_dim_padded][256], zero rows from obs_dim up to a multiple of 32),
 *   w2p = cn_actor_pack_weights(linear2.weight^T [256][256]), w3 [2][256] = linear3.weight, biases as in PyTorch.
 * obs: dev [n, obs_dim] float32; action: dev [n,2].
 * cn_actor_pack_weights reorders a K-major [k_rows][256] float32 matrix (k_rows a multiple of 32) into the order the kernel's
 * wavefronts consume it -- packed[((((b*8 + w)*4 + q)*64 + lane)*4 + j] = wt[32 b + 4 (2 q + (j >> 1)) + (lane >> 4)][32 w +
 * 2 (lane & 15) + (j & 1)] -- so every lane streams 16-byte loads out of L2 and a wavefront's block is 4 KB contiguous
 * (k_rows * 256 floats, same size as the input; in and out must not alias).  Call it once per weight update. */
typedef struct cn_actor_weights {
    const float* w1p; const float* b1; const float* w2p; const float* b2; const float* w3; const float* b3;
    int32_t obs_dim, obs_dim_padded, hidden, reserved;
} cn_actor_weights;
int cn_actor_pack_weights(const float* wt_dev, int k_rows, float* packed_dev, int device, void* stream);
int cn_actor_forward(const cn_actor_weights* w, const float* obs, float* action, int n, float max_v, float max_w,
                     float sigma, uint64_t seed, uint64_t counter, int device, void* stream);

/* A population's actors: n_members independent actors (the members of cn_td3_pop_create, or any actors of one observation width)
 * run by ONE cn_actor_forward-like launch and re-packed by ONE launch, instead of one launch per member and four per re-pack (two
 * transposing copies + two cn_actor_pack_weights).  The launches are small and latency-bound; side by side in one grid, tiles of
 * different members share the card's CUs.
 * The handle owns, per member, the packed w1p [Dp x 256] and w2p [256 x 256] buffers (Dp = obs_dim rounded up to a multiple of 32)
 * and one job per member in a device table.  A member's pointers never change after create; the table is uploaded once.  Members
 * agree in obs_dim (and the hidden width, 256), which fix the LDS tile; n, max_v, max_w, sigma and seed are per member.  actor: the
 * member's nn.Linear storages as in cn_td3_config.actor.  obs / action may be NULL for a member with n == 0.  device: HIP ordinal,
 * -1 = current.
 * cn_actor_pop_pack (one launch): after it member p's w1p / w2p equal BYTE FOR BYTE what cn_actor_pack_weights gives for
 * linear1.weight^T zero-padded to Dp rows / linear2.weight^T.  It reads the [out][in] storages directly and writes every element of
 * the packed buffers, the zero rows included.  Call it after create and after every weight update, before the next forward.
 * cn_actor_pop_forward (one launch): action_p equals BIT FOR BIT what cn_actor_forward(weights_p, obs_p, action_p, n_p, max_v_p,
 * max_w_p, add_noise ? sigma_p : 0, seed_p, counters[p], ...) writes, whatever n_members and p are; rows at and beyond n_p are not
 * touched.  counters: HOST array [n_members], passed by value with the launch: no host-to-device copy, nothing read back, capturable
 * on one stream (a captured call keeps the counters it was captured with).  If every n_p is 0, no launch is made.
 * cn_actor_pop_weights: the cn_actor_weights of a member -- the handle's packed buffers, the member's own biases and w3 -- valid while
 * the handle lives; the member can then also be driven by cn_actor_forward / cn_rollout_policy.
 * Refused before any device work, text in cn_last_error naming the field and the member: a NULL handle / members / out / counters,
 * n_members outside 1 ... CN_ACTOR_POP_MAX, a NULL pointer inside a member, n < 0, member out of range -- CN_ERR_ARG; obs_dim < 1 or
 * an obs_dim whose tile exceeds 160 KiB of LDS (from 2273, as cn_actor_forward) -- CN_ERR_CONFIG. */
#define CN_ACTOR_POP_MAX 64
typedef struct cn_td3_mlp { float *w1, *b1, *w2, *b2, *w3, *b3; } cn_td3_mlp;   /* Linear(in, H) - ReLU - Linear(H, H) - ReLU - Linear(H, out) */
typedef struct cn_actor_pop_member {
    cn_td3_mlp actor;        /* the member's nn.Linear storages, as cn_td3_config.actor: weight [out][in] row-major, bias [out] */
    const float* obs;        /* dev [n, obs_dim] */
    float* action;           /* dev [n, 2] */
    int32_t n, reserved;     /* n >= 0; members may differ */
    float max_v, max_w, sigma, reserved_f;
    uint64_t seed;           /* exploration-noise key, as cn_actor_forward's */
} cn_actor_pop_member;
typedef struct cn_actor_pop_s* cn_actor_pop_handle;
int cn_actor_pop_create(const cn_actor_pop_member* members, int n_members, int obs_dim, int device, cn_actor_pop_handle* out);
void cn_actor_pop_destroy(cn_actor_pop_handle h);
int cn_actor_pop_members(cn_actor_pop_handle h);
int cn_actor_pop_pack(cn_actor_pop_handle h, void* stream);                       /* ONE launch */
int cn_actor_pop_forward(cn_actor_pop_handle h, const uint64_t* counters, int add_noise, void* stream);   /* ONE launch */
int cn_actor_pop_weights(cn_actor_pop_handle h, int member, cn_actor_weights* out);

/* The TD3 update -- Agent.learn (td3.py:225-285) with the hyper-parameters of start_td3_training.py:62-72 -- as a short chain
 * of launches on the caller's stream (crowdnav_td3.hip; the kernels: crowdnav_gemm.hip): the forward and backward GEMMs of the six 3-layer networks on the f32
 * matrix cores, weight gradients folded into the Adam step (a gradient never exists in memory), the TD target / MSE gradient /
 * heads evaluated inside those GEMMs, replay sampling and target-policy noise drawn on the device.  7 launches for the critic
 * step, 5 more when the actor and the targets move (every policy_delay-th update); through PyTorch the same update is ~150
 * kernels.
 * The parameters stay the caller's: device pointers to the nn.Linear storages (weight [out][in] row-major float32, bias
 * [out]) of actor / critics and their targets, stepped in place.  Adam's moments and step counters are the handle's (zero at
 * cn_td3_create, like a fresh torch.optim.Adam).  Arithmetic: float32 throughout like the reference; same formulas as
 * torch.optim.Adam (no weight decay, no amsgrad) and F.mse_loss; results agree with the PyTorch update up to summation order.
 * (cn_td3_mlp, one network's storages, is declared above with cn_actor_pop_member.) */
typedef struct cn_td3_config {
    int32_t obs_dim;         /* actor input width (TRAIN:88 -> 398); the critics take obs_dim + 2 (TD3:114) */
    int32_t hidden;          /* TRAIN:65 -> 256 */
    int32_t batch;           /* TRAIN:62 -> 128 */
    int32_t policy_delay;    /* TRAIN:72 -> 2 (the caller passes do_actor itself; kept for the record) */
    float gamma, tau;        /* td3.yaml -> 0.99, 0.005 */
    float lr_actor, lr_critic, beta1, beta2, eps;   /* 3e-4, 3e-4, torch.optim.Adam's 0.9, 0.999, 1e-8 */
    float noise_std, noise_clip;                    /* TRAIN:70-71 -> 0.2, 0.5 (target-policy smoothing, TD3:240-243) */
    float max_v, max_w;                             /* TRAIN:67-68 -> 0.22, 2.0 (the actor's heads, TD3:103-104) */
    float reserved;
    cn_td3_mlp actor, actor_t, q1, q1_t, q2, q2_t;
    /* the replay ring on the device (rows obs_dim / 2 / 1 / obs_dim / 1 floats wide; done as 0 / 1) and its live size (an int64
     * on the device, read at update time: indices are drawn uniformly below it).  May all be NULL when every update passes
     * an explicit batch. */
    const float *replay_s, *replay_a, *replay_r, *replay_s2, *replay_d;
    const int64_t* replay_size_dev;
    uint64_t seed;           /* keys the replay indices and the target-policy noise with the handle's update counter */
} cn_td3_config;
typedef struct cn_td3_batch {   /* an explicit batch instead of a replay sample (parity tests): [B, obs_dim], [B, 2], [B], [B, obs_dim], [B] */
    const float *s, *a, *r, *s2, *d;
    const float* target_noise;   /* [B, 2] unit-variance noise BEFORE the scale and clip (TD3:240-242), or NULL = drawn on the device */
} cn_td3_batch;
typedef struct cn_td3_s* cn_td3_handle;
int cn_td3_create(const cn_td3_config* cfg, int device, cn_td3_handle* out);
void cn_td3_destroy(cn_td3_handle h);
/* One update.  do_actor != 0: also the actor step and the three soft updates (TD3:264-285).  batch NULL = sample the replay.
 * Enqueues only (capturable into a hipGraph). */
int cn_td3_update(cn_td3_handle h, int do_actor, const cn_td3_batch* batch, void* stream);
const float* cn_td3_loss_dev(cn_td3_handle h);      /* device pointer: the first critic's MSE loss of the last update */
/* Device pointer, read only: the batch the last update gathered (its first launch, td3_prep_kernel, writes these buffers and the
 * later launches only read them), valid until the next update is enqueued.  what = 0: [s | a] [batch][obs_dim + 2]; 1: s2 in the
 * same layout, where only the columns < obs_dim are defined; 2: r [batch]; 3: d [batch]; 4: the target-policy noise after the
 * scale and the clip [batch][2].  Other values of what, or a NULL handle: NULL.
 * On the replay path row m of update number c (counting from 0 at cn_td3_create; every update counts, whether it passes an
 * explicit batch or not, whether it steps the actor or not) is ring row mix64(mix64(seed ^ mix64(c)) ^ m) % max(*replay_size_dev, 1)
 * (mix64: splitmix64's finaliser), and its noise is Box-Muller on the same hash with c ^ 0x5bd1e995 in place of c.  That draw is
 * WITH replacement (CN_SAMPLE_WITH_REPLACEMENT, the mode of a fresh handle).
 * With cn_td3_set_replay_sample(h, CN_SAMPLE_DISTINCT) the rows of an update are DISTINCT, as the reference's random.sample gives
 * them (td3.py:31-32, ddpg.py:33-34, sac.py:34-35, memory.py:23): row m is a keyed bijection of [0, n) evaluated at m, still a pure
 * function of (seed, c, m, live size) -- no communication between rows, no host read, the same single prep launch.  All integers
 * are unsigned 64-bit; sums are exact (never wrapped at 2^64: (L + h) % a is evaluated as (L + h % a) % a):
 *   n = max(*replay_size_dev, 1)                       (read when the update runs)
 *   a = the least integer with a*a >= n;  b = ceil(n / a)          (a*b >= n, and (a*b - n) / (a*b) <= 1/4)
 *   K = mix64(seed ^ mix64(c ^ 0x9E3779B97F4A7C15))
 *   x = m mod n
 *   repeat (at most 64 times):
 *       L = x / b;  R = x % b
 *       for i = 0..3:   i even: L = (L + mix64(mix64(K ^ (i+1)) ^ R)) % a
 *                       i odd : R = (R + mix64(mix64(K ^ (i+1)) ^ L)) % b
 *       x = L*b + R
 *   until x < n
 *   row = x        (if the 64th pass still left x >= n: x mod n -- never expected: probability <= 4^-64)
 * Each round is invertible on Z_a x Z_b, so the four are a bijection there, and walking its cycle until x < n makes it a bijection
 * of [0, n).  Rows m = 0 .. batch-1 with batch <= n are therefore distinct, and at batch == n a permutation of the whole ring.
 * batch > n is outside the reference's domain (random.sample raises; the Python callers gate on ready(batch)); it is not refused,
 * because the size lives on the device: x = m mod n makes every ring row appear floor(batch / n) or ceil(batch / n) times.
 * The target-policy noise does not depend on the mode. */
const float* cn_td3_batch_dev(cn_td3_handle h, int what);
/* How the replay path draws its rows.  The setters store the mode in the handle on the host: the next update enqueued uses it, an
 * update already captured into a hipGraph keeps the mode it was captured with.  A fresh handle is CN_SAMPLE_WITH_REPLACEMENT.  Any
 * other value: CN_ERR_ARG (text in cn_td3_last_error) and the handle keeps its mode.  An explicit batch is not sampled at all. */
enum { CN_SAMPLE_WITH_REPLACEMENT = 0, CN_SAMPLE_DISTINCT = 1 };
int cn_td3_set_replay_sample(cn_td3_handle h, int mode);
/* The B ring rows that an update of a handle with this seed, at update counter `counter`, in this mode would gather: int64 [B] on
 * the device, *size_dev read on the device when the launch runs (the updates call the same device function).  B >= 1.  One launch,
 * enqueue-only.  crowdnav.td3.DeviceReplay.sample(batch, replace=False) draws through it. */
int cn_replay_sample_indices(uint64_t seed, uint64_t counter, int B, const int64_t* size_dev, int mode, int64_t* rows_dev,
                             int device, void* stream);
const char* cn_td3_last_error(void);

/* A population: n_members independent TD3 learners updated by the 7 (+ 5) launches of ONE cn_td3_update -- seed studies and
 * hyper-parameter sweeps on one card, where a single update is a chain of small dependent launches that leave most of it idle.
 * Member p's work rides in the grid's z dimension of the same kernels (their *_pop_kernel instantiations, which read their jobs from
 * tables in device memory that cn_td3_pop_create builds and uploads once; cn_td3_pop_update only enqueues, does no host read and no
 * copy, and is capturable on one stream like cn_td3_update).
 * Statement: after any sequence of cn_td3_pop_update calls, member p equals a solo handle made by cn_td3_create from cfgs[p] (on its
 * own copies of the parameters and the ring) and given cn_td3_update(h, do_actor, NULL, stream) with the same sequence of do_actor
 * values, in the same sampling mode: the six networks, Adam's state, the loss and the gathered batch (cn_td3_pop_batch_dev), BIT FOR
 * BIT.  It depends neither on n_members nor on p: a member's tile is computed by the same instructions in the same order as a solo
 * handle's, from the member's own update counter, seed and *replay_size_dev (all read on the device).
 * Per member (cfgs[p]): seed, lr_actor, lr_critic, gamma, noise_std, noise_clip, the six networks, the replay ring and its size.
 * Shared -- the grid and the launch-level scalars are one, so cfgs[p] must equal cfgs[0] in: obs_dim, hidden, batch, policy_delay,
 * beta1, beta2, eps, tau, max_v, max_w; otherwise CN_ERR_CONFIG naming the field and the member.
 * Also refused: n_members outside 1 ... 64, a NULL parameter pointer, a member without a replay ring (there is no explicit-batch form)
 * -- CN_ERR_ARG; two members naming the same parameter tensor (pointer equality over all members' cn_td3_mlp fields: they would race
 * inside a launch) -- CN_ERR_CONFIG.  Texts in cn_td3_last_error.
 * cn_td3_pop_loss_dev: [n_members], member p's first-critic MSE of the last update.  cn_td3_pop_batch_dev(h, p, what): as
 * cn_td3_batch_dev for member p; a member or what out of range: NULL.  cn_td3_pop_set_replay_sample: as cn_td3_set_replay_sample, one
 * mode for all members (an unknown mode: CN_ERR_ARG and the handle keeps its mode). */
typedef struct cn_td3_pop_s* cn_td3_pop_handle;
int cn_td3_pop_create(const cn_td3_config* cfgs, int n_members, int device, cn_td3_pop_handle* out);
void cn_td3_pop_destroy(cn_td3_pop_handle h);
int cn_td3_pop_update(cn_td3_pop_handle h, int do_actor, void* stream);      /* replay path only */
int cn_td3_pop_members(cn_td3_pop_handle h);
const float* cn_td3_pop_loss_dev(cn_td3_pop_handle h);                        /* [n_members] */
const float* cn_td3_pop_batch_dev(cn_td3_pop_handle h, int member, int what); /* as cn_td3_batch_dev */
int cn_td3_pop_set_replay_sample(cn_td3_pop_handle h, int mode);
/* The replay source of a population: whose rings a member's batch is drawn from.  CN_REPLAY_OWN (what a fresh handle has): member p
 * samples its own ring, the statement above.  CN_REPLAY_SHARED: every member samples the UNION of all members' rings, laid end to
 * end in member order -- the rings stay where they are, nothing is copied, and only the update's first launch (the sample and
 * gather, td3_prep_shared_kernel in place of td3_prep_kernel) reads differently; the 6 + 5 GEMM launches are the same.
 * cn_td3_pop_set_replay_source(h, source) stores the source in the handle on the host, like the sampling mode: the next update
 * enqueued uses it, an update already captured into a hipGraph keeps the source it was captured with.  Any other value: CN_ERR_ARG
 * (text in cn_td3_last_error) and the handle keeps its source.
 * Batch row m of member p at its update number c (member p's own counter) in CN_REPLAY_SHARED -- all integers unsigned 64-bit,
 * everything read on the device when the launch runs:
 *   n_q   = max(*replay_size_dev of member q, 0)          q = 0 .. P-1
 *   pre_q = n_0 + ... + n_{q-1}                            (pre_0 = 0)
 *   N     = max(pre_P, 1)
 *   x     = the row that cn_td3_batch_dev's statement gives for (seed_p, c, m) with N in place of the ring's live size: the hash for
 *           CN_SAMPLE_WITH_REPLACEMENT, the keyed bijection for CN_SAMPLE_DISTINCT, unchanged
 *   q*    = the least q with x < pre_{q+1};  if there is none (every ring empty): q* = p
 *   row   = x - pre_{q*}                                   (0 when every ring is empty)
 * Row m of member p's batch is row `row` of member q*'s ring (s, a, r, s2, d).  The target-policy noise is what it is with
 * CN_REPLAY_OWN: keyed by (seed_p, c, m), scaled and clipped with member p's noise_std / noise_clip.  The draw is uniform over the
 * union's live rows.  In CN_SAMPLE_DISTINCT with batch <= N the pairs (q*, row) of one update are distinct, and at batch == N a
 * permutation of the union.  With P == 1 the shared source gathers the rows the own source gathers.
 * Statement: after any sequence of shared updates, member p equals a solo handle made by cn_td3_create from cfgs[p] and given, at
 * each update, cn_td3_update(h, do_actor, &batch, stream) with the explicit batch of the rows named above and target_noise = NULL:
 * the six networks, Adam's state, the loss and cn_td3_pop_batch_dev(h, p, 0..4), BIT FOR BIT.  It does not depend on P, or on p
 * beyond what the rule says.  The launch reads the same device tables as the own source's, so what cn_td3_pop_exploit and
 * cn_td3_pop_state_load rewrite in them holds for both.  No atomics, no host read, no copy; capturable on one stream.
 * cn_td3_pop_batch_src_dev(h, member): device int64 [batch][2], {q*, row} of the member's rows in the last shared update; NULL for
 * a bad handle or member, or before the first shared update is enqueued.
 * cn_replay_sample_shared: the [B][2] pairs {q*, row} that a shared update of member `self` with this seed, at update counter
 * `counter`, in this mode would gather, from the P live sizes that size_dev_table (a DEVICE array of P device pointers) names -- the
 * same device function, without any rings, as cn_replay_sample_indices is for one ring.  One launch, enqueue-only.  B < 1, P outside
 * 1 ... 64, self outside 0 ... P-1, an unknown mode or a NULL pointer: CN_ERR_ARG, text in cn_td3_last_error. */
enum { CN_REPLAY_OWN = 0, CN_REPLAY_SHARED = 1 };
int cn_td3_pop_set_replay_source(cn_td3_pop_handle h, int source);
const int64_t* cn_td3_pop_batch_src_dev(cn_td3_pop_handle h, int member);
int cn_replay_sample_shared(uint64_t seed, uint64_t counter, int B, const int64_t* const* size_dev_table, int P, int self, int mode,
                            int64_t* rows_dev, int device, void* stream);

/* The DDPG update -- Agent.learn of the reference's ddpg.py:198-243, the baseline learner of start_ddpg_training.py -- on the
 * same GEMM kernels as cn_td3_update (crowdnav_gemm.hip; the update: crowdnav_ddpg.hip), 8 launches per update.  One critic and one target critic, no policy
 * delay, no target-policy noise: y = r + (1 - d) gamma Q_t(s2, pi_t(s2)) (ddpg.py:219-222), critic loss mean((Q(s, a) - y)^2)
 * (:228-230), actor loss -mean Q(s, pi(s)) (:216-217) back-propagated through the critic's PRE-update weights (the actor step,
 * :233-235, precedes the critic step, :237-239; the gradient the actor loss leaves on the critic is discarded by the critic's
 * zero_grad), then both Adam steps and the soft updates of both targets (:241-242, soft_update :244-254).  Parameters, Adam
 * state and arithmetic as cn_td3_*: the caller's nn.Linear storages stepped in place, moments zero at create, float32. */
typedef struct cn_ddpg_config {
    int32_t obs_dim;         /* actor input width; the critic takes obs_dim + 2 (ddpg.py:97) */
    int32_t hidden;          /* TRAIN_DDPG:58 -> 256 */
    int32_t batch;           /* TRAIN_DDPG:55 -> 64 */
    int32_t reserved0;
    float gamma, tau;        /* ddpg.yaml -> 0.99, 0.001 */
    float lr_actor, lr_critic, beta1, beta2, eps;   /* ddpg.yaml 1e-4, 1e-3; torch.optim.Adam's 0.9, 0.999, 1e-8 (ddpg.py:138, 143) */
    float max_v, max_w;                             /* TRAIN_DDPG:60-61 -> 0.22, 2.0 (the actor's heads, ddpg.py:87-88) */
    float reserved1;
    cn_td3_mlp actor, actor_t, critic, critic_t;
    const float *replay_s, *replay_a, *replay_r, *replay_s2, *replay_d;   /* as cn_td3_config (ReplayBuffer, ddpg.py:21-39) */
    const int64_t* replay_size_dev;
    uint64_t seed;           /* keys the replay indices with the handle's update counter */
} cn_ddpg_config;
typedef struct cn_ddpg_s* cn_ddpg_handle;
/* Shape limits as cn_td3_create's (obs_dim >= 1, 1 <= hidden, batch <= 4096); errors through cn_td3_last_error.
 * Replaces the construction of ddpg.py:131-151 minus the networks themselves (the caller's, hard-copied to the targets). */
int cn_ddpg_create(const cn_ddpg_config* cfg, int device, cn_ddpg_handle* out);
void cn_ddpg_destroy(cn_ddpg_handle h);
/* One update: ddpg.py:198-243 (learn), with soft_update (:244-254).  batch NULL = sample the replay (ReplayBuffer.sample,
 * ddpg.py:33-36, uniform on the device); an explicit batch must have target_noise == NULL.  Enqueues only (capturable into a
 * hipGraph on one stream), reads nothing from the host. */
int cn_ddpg_update(cn_ddpg_handle h, const cn_td3_batch* batch, void* stream);
const float* cn_ddpg_loss_dev(cn_ddpg_handle h);    /* device pointer: the critic's MSE loss of the last update (ddpg.py:230) */
const float* cn_ddpg_batch_dev(cn_ddpg_handle h, int what);   /* as cn_td3_batch_dev, same indices; what = 4 (no noise): NULL */
int cn_ddpg_set_replay_sample(cn_ddpg_handle h, int mode);    /* as cn_td3_set_replay_sample */
/* Agent.act(state, step, add_noise=True) (ddpg.py:170-196) with its OUNoise (:44-64) and the trainer's noise.reset() at an episode's
 * end (start_ddpg_training.py:161) for n rows as ONE launch on the caller's stream (no handle; capturable; copies nothing between
 * host and device, reads nothing back).  The matrix part is cn_actor_forward's tile on the same packed weights (cn_actor_weights: 16
 * rows per workgroup, v_mfma_f32_16x16x4_f32), so pi below is the float32 head value cn_actor_forward computes, bit for bit.
 * Per row e and component o (0: v, 1: w), every float64 operation rounded on its own (no FMA):
 *   x0 = reset && reset[e] ? mu : state[e][o]
 *   x1 = x0 + (theta * (mu - x0) + sigma * U)              ddpg.py:59-61
 *   state[e][o] = x1;  noise_out[e][o] = x1 (if given)
 *   action[e][o] = clip((float)((double)pi + x1))          numpy's float32 `action += noise` with a float64 noise, then :191-192:
 *                                                          v to [0, max_v], w to [-max_w, max_w]
 * U = u[e][o], or with u == NULL drawn on the device, a multiple of 2^-53 in [0, 1) like random.random():
 *   U = (mix64(mix64(seed ^ mix64(counter ^ 0x4F55)) ^ (2 e + o)) >> 11) * 2^-53,
 *   mix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 * (64-bit wrap-around; e = the row within this call).  A row's draw depends on (seed, counter, e, o) alone: not on n, not on the tile.
 * The caller owns sigma's decay (ddpg.py:63), as OUNoise.sample does: sigma is this call's value.
 * add_noise == 0: the deterministic policy, action = clip(pi); state, reset, u and noise_out are not touched (and may be NULL).
 * Rows at and beyond n are not touched.  device: HIP ordinal, -1 = current.
 * Refused before any device work, text in cn_last_error naming the field: a NULL actor / io / pointer inside actor / obs / action, a
 * NULL state with add_noise != 0, n < 0 -- CN_ERR_ARG; actor->hidden other than 256, obs_dim < 1, an obs_dim_padded that is not
 * obs_dim rounded up to a multiple of 32, an obs_dim whose tile exceeds 160 KiB of LDS (from 2273, as cn_actor_forward) --
 * CN_ERR_CONFIG.  n == 0 launches nothing and returns 0. */
typedef struct cn_ddpg_act_io {
    const float* obs;            /* dev [n][obs_dim] float32 */
    double* state;               /* dev [n][2] float64: the OU state, read and written in place; the caller's */
    const uint8_t* reset;        /* dev [n] or NULL; non-zero = the row's state is mu before this call's update */
    const double* u;             /* dev [n][2] float64 uniforms, or NULL = drawn on the device */
    float* action;               /* dev [n][2] float32, output */
    double* noise_out;           /* dev [n][2] float64 or NULL: the new state beside the action */
    double mu, theta, sigma;     /* ddpg.py:45-52 -> 0.0, 0.15, 0.2 */
    uint64_t seed, counter;      /* key of the device draw */
    float max_v, max_w;          /* the heads' ranges: 0.22, 2.0 */
    int32_t n, add_noise;        /* n >= 0 rows; add_noise 0 = the deterministic policy */
} cn_ddpg_act_io;
int cn_ddpg_act(const cn_actor_weights* actor, const cn_ddpg_act_io* io, int device, void* stream);

/* DQN -- the reference's discrete learner (deepq.py, start_dqn_training.py) -- on the same GEMM kernels (crowdnav_gemm.hip; crowdnav_dqn.hip).
 * Network (deepq.py:102-127, TRAIN_DQN:55-57): Linear(obs_dim, H) - ReLU - Linear(H, H) - ReLU - Linear(H, 3), H = 300.
 * One update = learnOnMiniBatch (deepq.py:219-266) with Memory.getMiniBatch (memory.py:22-28):
 *   - B rows sampled on the device: with replacement by default (td3_prep_kernel's hash), or distinct as memory.py:23's
 *     random.sample after cn_dqn_set_replay_sample(h, CN_SAMPLE_DISTINCT) (the bijection stated at cn_td3_batch_dev; s, s2, r, d,
 *     the action and the final flags of row m all come from the same ring row).  The reference's min(size, len) does not arise:
 *     the replay path is live only above learn_start rows, and the callers keep learn_start >= batch;
 *   - Y = Q(s), Y[a] = r if final else r + gamma max Q'(s2) (deepq.py:240-256), Q' = the online net until the first target copy,
 *     the target net after it; every final sample appends the row (s2, [r, r, r]) right after its own (:257-262): B + F rows;
 *   - model.fit(batch_size = B, epochs = 1) shuffles them and takes two steps when F > 0: the first B shuffled rows, then the
 *     other F on the stepped weights, both against the Y computed before either; loss per chunk = Keras mse (mean over the 3
 *     outputs and the chunk's rows); RMSprop a = rho a + (1 - rho) g^2, p -= lr g / (sqrt(a) + eps), accumulators zero at create.
 *     No second step at all when F = 0;
 *   - the hard copy online -> target after every target_every-th update (TRAIN_DQN:123-124, counted in updates here: the
 *     reference counts its non-terminal env-steps, stepCounter).
 * The replay path is a no-op (counter included) while the ring holds no more than learn_start rows (TRAIN_DQN:114, deepq.py:221).
 * Enqueue-only, no host read, capturable into a hipGraph; 16 launches, those of chunk 2 returning at once on the device when F = 0.  Errors through cn_td3_last_error. */
typedef struct cn_dqn_config {
    int32_t obs_dim;         /* network inputs: TRAIN_DQN:55 -> 361 (the first 361 columns of the obs_layout-1 row) */
    int32_t obs_ld;          /* row stride of s / s2 in the replay ring and in an explicit batch (>= obs_dim; the env's 363) */
    int32_t hidden;          /* TRAIN_DQN:57 -> 300 */
    int32_t batch;           /* TRAIN_DQN:52 -> 64 (also Keras's fit batch size) */
    float gamma, lr, rho, eps;   /* dqn.yaml 0.99, 2.5e-4; RMSprop(rho = 0.9, epsilon = 1e-6) (deepq.py:124) */
    int32_t target_every;    /* TRAIN_DQN:51 -> 10000 */
    int32_t learn_start;     /* TRAIN_DQN:53 -> 64 */
    cn_td3_mlp q, q_t;       /* the online and target networks (nn.Linear storages; linear3 has 3 outputs) */
    const float *replay_s, *replay_a, *replay_r, *replay_s2, *replay_d;   /* as cn_td3_config; rows of s / s2 obs_ld wide, the action
                                                                           * index in column 0 of replay_a [.][2] */
    const int64_t* replay_size_dev;
    uint64_t seed;           /* keys the replay indices and the shuffle with the handle's update counter */
} cn_dqn_config;
typedef struct cn_dqn_batch {   /* an explicit batch (tests): s, s2 [B][obs_ld], a [B] action indices, r [B], d [B] */
    const float* s; const int32_t* a; const float* r; const float* s2; const float* d;
    const int32_t* perm;         /* the shuffle: X_batch row at each of the B + F positions, or NULL = drawn on the device */
} cn_dqn_batch;
typedef struct cn_dqn_s* cn_dqn_handle;
int cn_dqn_create(const cn_dqn_config* cfg, int device, cn_dqn_handle* out);
void cn_dqn_destroy(cn_dqn_handle h);
int cn_dqn_update(cn_dqn_handle h, const cn_dqn_batch* batch, void* stream);
const float* cn_dqn_loss_dev(cn_dqn_handle h);      /* device pointer: [2] the losses of chunk 1 and chunk 2 (0 when F = 0) */
/* Device pointers, read only, into what the last update computed: 0 = the stacked rows [2B][obs_ld] (s, then s2), 1 = r [B],
 * 2 = d [B], 3 = a [B] (int32), 4 = the chunk of each stacked row [2B] (int32: 0 none, 1, 2), 5 = flags [8] (int32: live, second
 * step, F, Q' is the target net, target copied), 6 = Y [2B][3], 7 = the pre-step Q [2B][3] (chunk 1's forward; chunk 2's is kept apart), 8 = the update counter (uint64). */
const void* cn_dqn_batch_dev(cn_dqn_handle h, int what);
int cn_dqn_set_replay_sample(cn_dqn_handle h, int mode);      /* as cn_td3_set_replay_sample */
/* Action selection (TRAIN_DQN:103-104, deepq.py:151-184) for n rows as ONE launch: Q on the f32 matrix cores, argmax with ties to
 * the lowest index, and with probability epsilon a uniform index instead, drawn from (seed, counter, row).  epsilon: episodes_dev
 * NULL = `epsilon` itself; else the schedule TRAIN_DQN:89-90 (if eps > epsilon_min: eps *= epsilon_discount, once per episode
 * begun, before its first step) applied *episodes_dev + 1 times to `epsilon` (at most 2^22 times), in float64 on the doubles given.  Writes the index [n] and the twist of
 * environment_stage_1_original.py:412-425 [n][2]: (0.22, 0), (0.22, 2.0), (0.22, -2.0); q_out [n][3] optional. */
typedef struct cn_dqn_act_io {
    const float* obs; int64_t obs_ld;
    int32_t n, obs_dim, hidden, reserved;     /* hidden <= 480 */
    cn_td3_mlp q;
    double epsilon, epsilon_discount, epsilon_min;   /* epsilon_min > 0 */
    const int64_t* episodes_dev;
    uint64_t seed, counter;
    int32_t* action; float* twist; float* q_out;
} cn_dqn_act_io;
int cn_dqn_act(const cn_dqn_act_io* io, int device, void* stream);

/* SAC -- the reference's fourth neural learner (sac.py; start_sac_training.py cannot run: its arguments are shifted by one, so
 * every value is taken AT ITS NAME) -- on the same GEMM kernels (crowdnav_gemm.hip; crowdnav_sac.hip), float32.
 * Networks: actor Linear(D, H) - ReLU - Linear(H, H) - ReLU - {mean_linear (H, 2), log_std_linear (H, 2)} (SAC:43-76);
 * Q Linear(D + 2, H) - ReLU - Linear(H, H) - ReLU - Linear(H, 1) (:109-125); V and its copy V_t Linear(D, Hv) - ReLU -
 * Linear(Hv, Hv) - ReLU - Linear(Hv, 1) with Hv = hidden_v (as the reference constructs them, :175-176, Hv = 2).
 * One update = Agent.learn (SAC:231-290), every forward pass on the pre-update weights:
 *   log_std clamped to [log_std_min, log_std_max]; z = eps exp(log_std) + mean with eps a unit normal -- a VALUE (Normal.sample,
 *   not rsample: no gradient through z); t = tanh z; log_prob = sum_k [Normal.log_prob(z) - log(1 - t^2 + logp_eps)];
 *   a_new = (sigmoid(t0) max_v, tanh(t1) max_w) (the action is squashed twice, :84-91);
 *   q_loss = MSE(Q(s, a), r + (1 - d) gamma V_t(s2));  value_loss = MSE(V(s), Q(s, a_new) - log_prob);
 *   policy_loss = mean(log_prob (log_prob - (Q(s, a_new) - V(s)))_detached) + mean_lambda mean(mean^2)
 *                 + std_lambda mean(log_std^2) [clamped value] + z_lambda mean(sum z^2) [no gradient];
 *   three Adam steps (Q, V, actor; torch.optim.Adam's formulas, moments zero at create), then the soft update:
 *     soft_update = 0 (the reference as committed): sac.py:290 calls soft_update(V_t, V) against the signature
 *       soft_update(local, target), so it is V that moves, V <- (1 - tau) V + tau V_t, and V_t keeps its initial value;
 *     soft_update = 1 (what the call intends): V_t <- (1 - tau) V_t + tau V from the stepped V, folded into V's Adam step.
 * 10 launches (11 with soft_update = 0): prep | F (actor, Q, V, V_t first layers) | F (second layers, Q / V / V_t outputs) |
 * heads | F, F (Q on (s, a_new)) | losses and row gradients | G (three jobs) | H (Q, V) | H (actor) [| pull].  Q(s, a_new) needs the
 * action and the action needs the actor's trunk, every loss needs Q(s, a_new), and backward is G then H: those are the data
 * dependencies; the heads and the losses are kernels of their own rather than new branches in the GEMM kernels, which the TD3
 * and DDPG updates share.  Enqueue-only, no host read, capturable into a hipGraph on one stream. */
typedef struct cn_sac_actor { float *w1, *b1, *w2, *b2, *mean_w, *mean_b, *log_std_w, *log_std_b; } cn_sac_actor;
typedef struct cn_sac_config {
    int32_t obs_dim;         /* actor and V input width (the env's: 363 with obs_layout 1, 398 with 0); Q takes obs_dim + 2 */
    int32_t hidden;          /* start_sac_training.py:58-67 -> 256 (actor, Q) */
    int32_t hidden_v;        /* V / V_t hidden width: 2 as written (SAC:175-176), `hidden` as intended */
    int32_t batch;           /* -> 64 */
    float gamma, tau;        /* sac.yaml -> 0.99, 5e-3 */
    float lr_actor, lr_v, lr_q, beta1, beta2, eps;   /* 3e-4 x 3; torch.optim.Adam's 0.9, 0.999, 1e-8 */
    float max_v, max_w, log_std_min, log_std_max;    /* 0.22, 2.0, -20, 2 */
    float mean_lambda, std_lambda, z_lambda, logp_eps;   /* 1e-3, 1e-3, 0, 1e-6 (SAC:78) */
    int32_t soft_update;     /* 0 = as written, 1 = intended (above) */
    int32_t reserved;
    cn_sac_actor actor;
    cn_td3_mlp q, v, v_t;
    const float *replay_s, *replay_a, *replay_r, *replay_s2, *replay_d;   /* as cn_td3_config */
    const int64_t* replay_size_dev;
    uint64_t seed;           /* keys the replay indices and eps with the handle's update counter */
} cn_sac_config;
typedef struct cn_sac_s* cn_sac_handle;
/* Limits as cn_td3_create's: obs_dim >= 1, 1 <= hidden, hidden_v, batch <= 4096.  Errors through cn_td3_last_error. */
int cn_sac_create(const cn_sac_config* cfg, int device, cn_sac_handle* out);
void cn_sac_destroy(cn_sac_handle h);
/* batch NULL = sample the replay.  batch->target_noise = the unit eps [B][2] of the sample learn() USES (the second Normal.sample
 * of the call: forward() draws one first and drops it), or NULL = drawn on the device: Box-Muller on
 * mix64(mix64(seed ^ mix64(c ^ 0x5bd1e995)) ^ m), c = the update counter, m = the row -- cn_td3_update's draw, unscaled. */
int cn_sac_update(cn_sac_handle h, const cn_td3_batch* batch, void* stream);
const float* cn_sac_loss_dev(cn_sac_handle h);      /* device pointer: [3] q_loss, value_loss, policy_loss of the last update */
/* what = 0 .. 3 as cn_td3_batch_dev; 4: eps [batch][2]; 5: a record per row [batch][12] = mean[2], clamped log_std[2], raw
 * log_std[2], z[2], log_prob, Q(s, a_new), a_new[2]; 6: d policy_loss / d (mean[2], log_std[2]) [batch][4]; 7: d q_loss / d Q [batch];
 * 8: d value_loss / d V [batch]. */
const float* cn_sac_batch_dev(cn_sac_handle h, int what);
int cn_sac_set_replay_sample(cn_sac_handle h, int mode);      /* as cn_td3_set_replay_sample */
/* Agent.act (SAC:206-229) for n rows as ONE launch: trunk on the f32 matrix cores, both heads, the clamp, z = eps std + mean
 * (deterministic != 0: z = mean), the double squash, the clip to v in [0, max_v], w in [-max_w, max_w].  eps [n][2] or NULL = drawn
 * from (seed, counter, row) as above with c = counter, m = row.  Writes twist [n][2]; mean, log_std (clamped), z [n][2] optional. */
typedef struct cn_sac_act_io {
    const float* obs; int64_t obs_ld;
    int32_t n, obs_dim, hidden, deterministic;     /* hidden <= 480 */
    cn_sac_actor actor;
    float max_v, max_w, log_std_min, log_std_max;
    const float* eps;
    uint64_t seed, counter;
    float *twist, *mean, *log_std, *z;
} cn_sac_act_io;
int cn_sac_act(const cn_sac_act_io* io, int device, void* stream);

/* Q-learning and SARSA -- the reference's tabular learners (qlearn.py, sarsa.py; start_qlearn_training.py,
 * start_sarsa_training.py) -- with ONE table shared by the n rows of a launch (crowdnav_tab.hip).
 * State: the last two columns of the obs_layout-1 row (observation[-2], [-1]: round(x, 3), round(y, 3) of the robot,
 * environment_stage_1_original.py:315-320) digitised as np.digitize does -- d = the number of distance edges <= column `col`
 * (30 edges round(0.1 k, 2), d in 0..30), h = the number of radian edges <= column `col + 1` (32 edges
 * round(-3.14 + 0.19625 k, 2), h in 0..32) -- and keyed by the STRING str(d) + str(h): 977 distinct keys, 46 of them shared by two
 * pairs ((1, 10) and (11, 0) are both '110').  The handle numbers the keys 0..976 in order of first appearance for d ascending,
 * then h ascending (state_of[31][33]).  The rows are float32 and are compared against the edges narrowed to float32: the two
 * columns are multiples of 0.001 below 16 narrowed to float32, narrowing is monotone and keeps such multiples distinct, so the
 * count equals np.digitize on the double.  That is the whole domain: an observation that is NaN, or of magnitude 16 and above, is
 * outside it, and what it is digitised to is not specified (the state index stays within 0..976 all the same: a count of edges).
 * Table: q[977][3] float64 and present[977][3] bytes (the dict {(key, action): float}; an absent entry reads 0.0, an entry that
 * holds 0.0 is present), count_same / count_diff (int64).  All on the device; cn_tab_set / cn_tab_get move the whole table.
 * One launch, cn_tab_learn_act, for n rows:
 *   1. learn (io.learn != 0), the bootstrap reads: every row reads the table AS IT STOOD WHEN THE LAUNCH BEGAN.
 *        Q-learning: value = reward + gamma max_a Q(s2, a);   SARSA: a2 = chooseAction(s2) from u_learn, value = reward + gamma Q(s2, a2)
 *      with s = state(obs_prev row), s2 = state(obs row), reward widened to double;
 *   2. the writes, for the rows with keep[i] != 0 (keep NULL = all) and 0 <= action_prev[i] <= 2, PER CELL (s, action_prev) IN
 *      ASCENDING ROW ORDER, by learnQ's rule: a cell absent at that moment becomes (double)reward, present, count_same += 1;
 *      otherwise q = q + alpha (value - q), count_diff += 1.  Rows of different cells do not interact;
 *   3. act (io.act != 0): chooseAction(state(obs row)) from u_act on the table AFTER all writes -> action, twist.
 * For n = 1 this is the reference's loop statement for statement.  Arithmetic: float64, every product, sum and difference
 * rounded on its own (no FMA).  max / min keep the first of equal values, as Python's.
 * chooseAction, draws u[0..4] of the row (a slot always means the same draw, consumed or not):
 *   SARSA (sarsa.py:39-55): u[0] < epsilon -> action int(u[1] * 3); else the argmax, several maxima -> best[int(u[4] * count)];
 *   Q-learning (qlearn.py:47-72): u[0] < epsilon -> mag = max(|min q|, |max q|), q[i] = (q[i] + u[1 + i] * mag) - .5 * mag, the
 *   maximum again; then the argmax with the same tie break.  (random.choice(seq) = seq[int(random() * len(seq))], Python 2.)
 * u_learn / u_act [n][5] float64, or NULL = drawn on the device: u[j] = (x >> 11) * 2^-53 with
 *   x = mix64(mix64(mix64(seed ^ mix64(counter ^ C)) ^ row) ^ j), mix64 = splitmix64's finaliser,
 *   C = 0x6a09e667f3bcc909 for u_learn, 0xbb67ae8584caa73b for u_act.
 * epsilon / epsilon_discount / epsilon_min / episodes_dev: as cn_dqn_act_io (the schedule of start_sarsa_training.py:51-52).
 * Outputs: action [n] and twist [n][2] (act; the twists of cn_dqn_act), optional state [n], state_prev [n] (0..976), q_row [n][3]
 * (the row chooseAction ended with, Q-learning's noise included; SARSA's random branch: the plain row).  state_prev is written for
 * every row of a learning launch, also one that keep or an action_prev outside 0..2 leaves unwritten.  `done` is not read by the
 * arithmetic (the reference learns from a terminal transition like any other).
 * One workgroup; enqueue-only, no host read, capturable into a hipGraph on one stream.  Errors through cn_tab_last_error. */
#define CN_TAB_STATES 977
#define CN_TAB_ACTIONS 3
enum { CN_TAB_QLEARN = 0, CN_TAB_SARSA = 1 };
typedef struct cn_tab_config {
    int32_t algo;            /* CN_TAB_QLEARN | CN_TAB_SARSA */
    int32_t reserved;
    double alpha, gamma;     /* qlearn.yaml / sarsa.yaml -> 0.2, 0.9 */
    uint64_t seed;           /* keys the device draws with io.counter */
} cn_tab_config;
typedef struct cn_tab_s* cn_tab_handle;
int cn_tab_create(const cn_tab_config* cfg, int device, cn_tab_handle* out);      /* an empty table, counters 0 */
void cn_tab_destroy(cn_tab_handle h);
/* Host arrays q [977][3] float64, present [977][3] bytes, counts [2] int64 = {count_same, count_diff} (NULL: set zeroes them, get
 * skips them).  Both wait for the device's queued work; a q value whose present byte is 0 is stored as 0.0. */
int cn_tab_set(cn_tab_handle h, const double* q_host, const uint8_t* present_host, const int64_t* counts_host);
int cn_tab_get(cn_tab_handle h, double* q_host, uint8_t* present_host, int64_t* counts_host);
/* Host copies [31][33] int32, [30] and [32] float64 of the handle's key table and edges (any may be NULL). */
int cn_tab_tables(cn_tab_handle h, int32_t* state_of_host, double* distance_bins_host, double* radian_bins_host);
typedef struct cn_tab_io {
    const float* obs_prev;   /* [n] rows, row stride obs_ld; read when learn != 0 */
    const float* obs;        /* [n] rows: s2 of the learn phase, the state of the act phase */
    int64_t obs_ld;
    int32_t n, col;          /* columns col, col + 1 are read (the env's 363-wide row: col = 361) */
    int32_t learn, act;
    const int32_t* action_prev; const float* reward;   /* [n]; read when learn != 0 */
    const uint8_t* done;     /* [n] or NULL; not read */
    const uint8_t* keep;     /* [n] or NULL = all rows */
    double epsilon, epsilon_discount, epsilon_min;     /* epsilon_min > 0 */
    const int64_t* episodes_dev;
    const double *u_learn, *u_act;                     /* [n][5] or NULL */
    uint64_t counter;
    int32_t* action; float* twist;                     /* [n], [n][2]; written when act != 0 */
    int32_t *state, *state_prev; double* q_row;        /* optional: [n], [n] (learn != 0), [n][3] (act != 0) */
} cn_tab_io;
int cn_tab_learn_act(cn_tab_handle h, const cn_tab_io* io, void* stream);
const char* cn_tab_last_error(void);

/* The collection loop's bookkeeping between Env.step and Agent.learn (start_td3_training.py:129-149) for a batch of environments,
 * without a host read: ReplayBuffer.add (td3.py:24-31) into a ring on the device, and the per-episode record TRAIN:139-149 prints
 * and utils.record_data writes.  (crowdnav.td3.DeviceReplay and crowdnav.train.DeviceEpisodeLog do the same through ~35 PyTorch
 * kernels per launch; next to a 0.065 ms update that is a seventh of a training launch.)  Both enqueue only.
 *
 * cn_replay_write: rows i < n with keep[i] != 0 (keep NULL = all) go to consecutive ring slots (*pos_dev + rank) mod capacity in
 * row order; then *pos_dev advances by their number and *size_dev grows up to capacity.  Rows not kept (an environment's reset
 * launch under the next-step reset convention) are not written.  Arrays: s, s2 [capacity][obs_dim], a [capacity][2], r, d
 * [capacity]; done / keep are bytes; n <= capacity.  slot_scratch: n int32 of device scratch. */
typedef struct cn_replay_ring {
    float *s, *a, *r, *s2, *d;
    int64_t capacity;
    int64_t* pos_dev;        /* next write position */
    int64_t* size_dev;       /* fill level (what cn_td3_config.replay_size_dev points at) */
    int32_t obs_dim, reserved;
} cn_replay_ring;
int cn_replay_write(const cn_replay_ring* ring, const float* s, const float* a, const float* r, const float* s2,
                    const uint8_t* done, const uint8_t* keep, int n, int32_t* slot_scratch, int device, void* stream);
/* cn_episode_log_add: one 8-float row per environment with done[i] != 0, appended at *n_dev in row order (rows past max_rows are
 * dropped, *n_dev keeps counting): {success, failure, return, steps, ego violations, social violations, obstacle-present steps,
 * launch} from the counter columns 4, 5, 13, 10, 11, 12 (cn_get_counters) and last_return (cn_get_returns); and the running
 * totals tot_dev[5] += {episodes, successes, sum of returns, sum of steps, number of rows with transitions[i] != 0}. */
typedef struct cn_episode_log {
    float* rows;             /* [max_rows][8] */
    int64_t max_rows;
    int64_t* n_dev;
    double* tot_dev;         /* [5] */
} cn_episode_log;
int cn_episode_log_add(const cn_episode_log* log, const uint8_t* done, const int32_t* counters, int counter_cols,
                       const float* last_return, const uint8_t* transitions, float launch, int n, int device, void* stream);

/* A population's recorder: the bookkeeping above for n_members members -- every member's cn_replay_write, its cn_get_counters /
 * cn_get_returns, its cn_episode_log_add, and the `prev <- obs`, `keep = !resetting`, `resetting <- done` around them -- as TWO
 * launches whatever n_members is, instead of about five small dependent launches per member.  Member p rides in the grid's z
 * dimension; its job is a row of a device table that cn_pop_record_create builds and uploads once (a member's pointers never change).
 * Per member: its replay ring and episode log; prev [n][obs_dim] (the observation the actions were computed from), obs [n][obs_dim],
 * action [n][2], reward [n], done [n] bytes; and where the counters and the last return come from: env != NULL -- read straight from
 * that environment's state records (CN_SI_SUCCESS, CN_SI_FAILURE, CN_SD_LAST_EGO_VIOL, CN_SD_LAST_SOCIAL_VIOL, CN_SD_LAST_OBST_STEPS,
 * CN_SD_LAST_EP_STEPS, CN_SD_LAST_RETURN, with cn_get_counters' / cn_get_returns' conversions; n must equal its n_envs) -- or
 * env == NULL and explicit counters [n][CN_COUNTER_COLS] and last_return [n], as cn_episode_log_add takes them.  n may differ between
 * members; n == 0 is allowed with NULL row pointers.  obs_dim is one for all members and must equal every ring's obs_dim.
 * The handle owns, per member, n int32 of slot scratch and the byte array resetting [n], zero at create (cn_pop_record_resetting: its
 * device pointer, so that a caller may set it, e.g. when resuming; member out of range or a NULL handle: NULL).
 * Statement: after cn_pop_record(h, launch, stream), for every member p, whatever n_members and p are:
 *   - ring_p (the five arrays below capacity, *pos_dev, *size_dev) is BYTE FOR BYTE what cn_replay_write(&ring_p, prev_p, action_p,
 *     reward_p, obs_p, done_p, keep, n_p, ...) leaves, with keep[i] = !resetting_p[i] as it stood before the call;
 *   - log_p (rows below max_rows, *n_dev, tot_dev[5]) is BIT FOR BIT what cn_episode_log_add(&log_p, done_p, counters, 14,
 *     last_return, keep, launch, n_p, ...) leaves, counters / last_return being what cn_get_counters / cn_get_returns of env_p return at
 *     that point, or the explicit arrays (the float64 totals are summed in cn_episode_log_add's order: the kernels share its code);
 *   - afterwards resetting_p[i] = (done_p[i] != 0) and prev_p equals obs_p over all n_p rows, kept or not: the next call's previous
 *     observation costs no launch of its own;
 *   - rows at and beyond n_p of any buffer, and ring rows that receive nothing, are not touched.  If every n_p is 0, no launch is made.
 * Launch A, grid (1, 1, P) x 1024: the keep scan and the slots, the ring's position and fill level, the episode log, resetting <- done.
 * Launch B, grid (max n_p, 1, P) x 256: a row's copy into its slot, then prev <- obs for the row.  (Not one launch: every copying
 * workgroup would have to read *pos_dev before one of them advances it.)  Enqueue-only: no host read, no copy, `launch` by value;
 * capturable on one stream.
 * Refused before any device work, text in cn_last_error naming the field and the member.  CN_ERR_ARG: a NULL handle / members / out;
 * n_members outside 1 ... CN_POP_RECORD_MAX; n < 0; a NULL row pointer in a member with n > 0; neither env nor both explicit arrays; n
 * different from the env's n_envs; an incomplete ring or log; n > ring.capacity; log.max_rows < 0; a member index out of range.
 * CN_ERR_CONFIG: obs_dim < 1; ring.obs_dim != obs_dim; two members naming the same ring array, pos_dev, size_dev, log rows / n_dev /
 * tot_dev, or prev (they would race inside a launch). */
#define CN_POP_RECORD_MAX 64
typedef struct cn_pop_record_member {
    cn_handle env;               /* or NULL: then counters and last_return below */
    const int32_t* counters;     /* dev [n][CN_COUNTER_COLS]; read when env == NULL */
    const float* last_return;    /* dev [n]; read when env == NULL */
    float* prev;                 /* dev [n][obs_dim]: read (the transition's s), then overwritten with obs */
    const float* obs;            /* dev [n][obs_dim] (the transition's s2) */
    const float* action;         /* dev [n][2] */
    const float* reward;         /* dev [n] */
    const uint8_t* done;         /* dev [n] */
    cn_replay_ring ring;
    cn_episode_log log;
    int32_t n, reserved;         /* n >= 0; members may differ */
} cn_pop_record_member;
typedef struct cn_pop_record_s* cn_pop_record_handle;
int cn_pop_record_create(const cn_pop_record_member* members, int n_members, int obs_dim, int device, cn_pop_record_handle* out);
void cn_pop_record_destroy(cn_pop_record_handle h);
int cn_pop_record_members(cn_pop_record_handle h);
uint8_t* cn_pop_record_resetting(cn_pop_record_handle h, int member);        /* dev [n_member] bytes, owned by the handle */
int cn_pop_record(cn_pop_record_handle h, float launch, void* stream);        /* at most TWO launches */

/* The n-step recorder: cn_pop_record's job -- replay write, episode log, prev <- obs, resetting <- done, for n_members <=
 * CN_POP_RECORD_MAX members in TWO launches -- but the ring rows it writes are n-step transitions: (s_t, a_t, R, s_{t+m}, d) with
 * R = sum_{k<m} gamma^k r_{t+k}, m = n_step for a row with d = 0 and m <= n_step for the rows an episode's end flushes (d = 1).
 * Window and discount: n_step = W, 1 ... CN_NSTEP_MAX, is one value for the handle; gamma is per member.  cn_nstep_discount(gamma, k)
 * starts with acc = 1.0 in float64, multiplies k times by (double)gamma and casts to float (no pow); it is host code and needs no
 * device.  w[k] = cn_nstep_discount(gamma_p, k), and the bootstrap discount a learner must use with this recorder's rows is
 * cn_nstep_discount(gamma_p, W).
 * Pending store: per member and environment e the handle owns W slots, all zero at create -- s [n][W][obs_dim], a [n][W][2], ret [n][W],
 * count [n] (the entries pending) and clock [n] (the pushes since the last flush).  An entry pushed at local time tau lies in slot
 * tau mod W.  cn_nstep_record_pending gives the device pointers, so that a caller may save and restore them (with
 * cn_nstep_record_resetting's flags they are the handle's whole state).
 * Statement: cn_nstep_record(h, launch, stream) does, for every member p and every row e < n_p, with keep = !resetting_p[e] as it
 * stood before the call:
 *   1. not kept (the environment's reset launch): nothing is pushed and nothing emitted, whatever done_p[e] is; count and clock stay.
 *   2. kept, in this order: every pending entry of age k >= 1 (pushed k calls of kept rows ago: 1 <= k <= count) takes
 *      ret = ret + w[k] * reward_p[e], the float32 product and the float32 sum rounded separately (no FMA); then the new entry
 *      (prev_p[e], action_p[e], ret = reward_p[e]) is pushed -- its return is ASSIGNED, so a -0.0f survives --; count and clock advance.
 *   3. emission into ring_p, at consecutive slots from *pos_dev modulo capacity, rows ordered by e ascending and oldest first within
 *      an environment: if done_p[e], all count entries, each as (s, a, ret, s2 = obs_p[e], d = 1), then count = clock = 0; else if
 *      count == W, the oldest entry as (s, a, ret, s2 = obs_p[e], d = 0), then count = W - 1.  *pos_dev advances by the rows emitted
 *      and *size_dev grows by them up to capacity, as in cn_replay_write.  An entry emitted by the call that pushes it (an episode's
 *      last, or every entry when W = 1) goes from prev straight into the ring: the store's slot for it is not written.
 *   4. the episode log, resetting_p <- done_p and prev_p <- obs_p are exactly cn_pop_record's; tot_dev[4] counts the kept rows.
 *   5. rows at and beyond n_p, ring rows that receive nothing and pending slots that hold no entry are not touched (the slot of an
 *      emitted entry keeps what it held, with the returns as step 2 left them).  If every n_p is 0, no launch is made.
 * Consequences: with W = 1 the ring, log, prev and resetting are byte for byte what cn_pop_record leaves.  A row with d = 0 always
 * spans exactly W steps, which is why one bootstrap discount per member suffices; a row with d = 1 is never bootstrapped from.  A call
 * emits at most n_p * W rows per member, hence the refusal below.
 * Launch A (plan), grid (1, 1, P) x 1024: per row the returns' update (at most W - 1 multiply-adds), the number of emitted rows and
 * their scan into first slots, a descriptor {first slot, rows emitted, the pre-call count and clock} for launch B, count and clock,
 * the ring's position and fill level, the episode log, resetting <- done.  Launch B (copy), grid (max n_p, W, P) x 256: workgroup
 * (e, 0) takes the new entry from prev into the ring or into its slot of the store (the one free slot: count <= W - 1 before the push)
 * and then runs prev <- obs for the row; workgroup (e, j >= 1) copies the (j - 1)-th oldest pending entry into its ring slot if it is
 * emitted.  Launch A writes nothing that B reads in its pre-call form.  Enqueue-only, capturable on one stream.
 * Refused before any device work, text in cn_last_error naming the field and the member: everything cn_pop_record_create refuses,
 * with its codes and words; CN_ERR_ARG: n_step outside 1 ... CN_NSTEP_MAX; a member's gamma not finite or outside (0, 1];
 * n * n_step > ring.capacity (a call could overrun itself); a NULL pending `out`. */
#define CN_NSTEP_MAX 16
typedef struct cn_nstep_member { cn_pop_record_member rec; float gamma, reserved_f; } cn_nstep_member;
typedef struct cn_nstep_pending {
    float *s, *a, *ret;          /* dev [n][n_step][obs_dim], [n][n_step][2], [n][n_step] */
    int32_t *count, *clock;      /* dev [n] */
    int32_t n, n_step, obs_dim, reserved;
} cn_nstep_pending;
typedef struct cn_nstep_record_s* cn_nstep_record_handle;
int cn_nstep_record_create(const cn_nstep_member* members, int n_members, int n_step, int obs_dim, int device, cn_nstep_record_handle* out);
void cn_nstep_record_destroy(cn_nstep_record_handle h);
int cn_nstep_record_members(cn_nstep_record_handle h);
uint8_t* cn_nstep_record_resetting(cn_nstep_record_handle h, int member);    /* dev [n_member] bytes, owned by the handle */
int cn_nstep_record_pending(cn_nstep_record_handle h, int member, cn_nstep_pending* out);   /* device pointers, owned by the handle */
int cn_nstep_record(cn_nstep_record_handle h, float launch, void* stream);    /* at most TWO launches */
float cn_nstep_discount(float gamma, int k);                                  /* host only, no device */

/* Evaluation on the device: J jobs at once, a job being one greedy actor in one world with its own environment handle.  One step of an
 * evaluation is three enqueues whatever J is -- cn_actor_pop_forward, cn_step_multi, cn_eval_record -- and nothing is read back until
 * the end: every environment contributes exactly its FIRST `quota` episodes (short episodes would otherwise be over-represented), the
 * handle counts them per environment, and cn_eval_finish turns the sums into per-job summaries and a per-group fitness that
 * cn_td3_pop_exploit takes as it stands.  Job j rides in the grid's z dimension; its row of a device table is built and uploaded once by
 * cn_eval_create.  Per job: done [n] bytes, its episode log, where the counters and the last return come from (env, or env == NULL and
 * explicit counters [n][CN_COUNTER_COLS] and last_return [n], as cn_pop_record_member), the quota, and the group whose fitness it feeds.
 * The handle owns, per job, finished [n] int32 (episodes counted per environment) and the byte scratch counted [n], and one
 * cn_eval_state (cn_eval_state_dev: device, read-only for the caller, alive as long as the handle).  At create the state is what
 * cn_eval_reset leaves and summary / fitness are zero.
 * Statement, for every job j, whatever n_jobs and j are:
 * cn_eval_reset(h, stream), ONE launch: finished_j = 0, sums[j] = 0, remaining[j] = n_j, *log_j.n_dev = 0, log_j.tot_dev[0..4] = 0;
 *     summary and fitness are not touched.
 * cn_eval_record(h, launch, stream), ONE launch, grid (1, 1, J) x 1024:
 *   - counted[i] = done_j[i] != 0 && finished_j[i] < quota_j, evaluated for all i < n_j before anything is written;
 *   - log_j (rows below max_rows, *n_dev, tot_dev[5]) is BIT FOR BIT what cn_episode_log_add(&log_j, counted, counters, 14, last_return,
 *     counted, launch, n_j, ...) leaves, counters / last_return being what cn_get_counters / cn_get_returns of env_j return at that
 *     point, or the explicit arrays (the kernel instantiates cn_episode_log_add's code on the counted bytes);
 *   - sums[j][k] += the float64 sum over the counted rows, in cn_episode_log_add's order (thread t of 1024 adds its rows i = t mod 1024
 *     in ascending order, the 64 lanes of a wavefront combine by the xor butterfly 32, 16, ..., 1, the 16 wave totals are added in
 *     order), of -- with success, failure, ret, steps, ego, social, obst the log row's columns 0 ... 6 --
 *       k = 0: 1 (episodes)        1: success              2: failure          3: 1 where success == 0 and failure == 0 (time-outs)
 *           4: ret                 5: steps                6: 1.0 - (double)ego / (double)obst where obst > 0, else nothing
 *           7: 1.0 - (double)social / (double)obst where obst > 0   8: 1 where obst > 0     9: steps where success != 0
 *       k = 10, 11: nothing (they stay 0).  A row that is not counted adds 0.0.
 *   - then finished_j[i] += counted[i] and remaining[j] = #{i < n_j : finished_j[i] < quota_j};
 *   - a job whose remaining[j] was 0 before the call, or with n_j == 0, changes nothing at all; rows at and beyond n_j of any buffer are
 *     not touched.  If every n_j is 0, no launch is made.
 * cn_eval_finish(h, metric, fitness_dev, stream), ONE launch of a single workgroup: with s = sums[j], summary[j] = {s0, s1 / s0,
 *     s2 / s0, s3 / s0, s4 / s0, s5 / s0, s6 / s8, s7 / s8} = {episodes, success rate, failure rate, time-out rate, mean return, mean
 *     steps, mean ego score, mean social score}: the quotients in float64, then cast to float; 0 / 0 gives NaN.  fitness[g], g <
 *     n_groups, = (float) of the float64 mean, over the jobs with group == g in job order, of summary[j][1] (CN_EVAL_SUCCESS_RATE) or
 *     summary[j][4] (CN_EVAL_MEAN_RETURN); a group without jobs gives NaN (cn_td3_pop_exploit ranks NaN last).  The same n_groups values
 *     go to fitness_dev when it is not NULL.  fitness at and beyond n_groups is not touched.
 * All three are enqueue-only: no host read, no copy, `launch` by value; capturable on one stream.  No atomics: every job's outputs
 * belong to its own workgroup.
 * Refused before any device work, text in cn_last_error naming the field and the job.  CN_ERR_ARG: a NULL handle / jobs / out; n_jobs or
 * n_groups outside 1 ... CN_EVAL_MAX; group outside 0 ... n_groups - 1; n < 0; quota < 1; a NULL done with n > 0; neither env nor both
 * explicit arrays with n > 0; n different from the env's n_envs; an incomplete log; log.max_rows < 0; an unknown metric.
 * CN_ERR_CONFIG: two jobs naming the same log rows, n_dev or tot_dev (they would race inside a launch). */
#define CN_EVAL_MAX 64
#define CN_EVAL_COLS 12
enum { CN_EVAL_SUCCESS_RATE = 0, CN_EVAL_MEAN_RETURN = 1 };
typedef struct cn_eval_job {
    cn_handle env;               /* or NULL: then counters [n][CN_COUNTER_COLS] and last_return [n], as cn_pop_record_member */
    const int32_t* counters; const float* last_return;
    const uint8_t* done;         /* dev [n] */
    cn_episode_log log;          /* the job's counted episodes */
    int32_t n, quota;            /* n >= 0, quota >= 1 */
    int32_t group, reserved;     /* 0 ... n_groups-1: whose fitness this job feeds */
} cn_eval_job;
typedef struct cn_eval_state {   /* device, read-only for the caller */
    int32_t remaining[CN_EVAL_MAX];            /* envs of job j still below quota */
    double  sums[CN_EVAL_MAX][CN_EVAL_COLS];
    float   summary[CN_EVAL_MAX][8];           /* by cn_eval_finish */
    float   fitness[CN_EVAL_MAX];              /* by group, by cn_eval_finish */
} cn_eval_state;
typedef struct cn_eval_s* cn_eval_handle;
int  cn_eval_create(const cn_eval_job* jobs, int n_jobs, int n_groups, int device, cn_eval_handle* out);
void cn_eval_destroy(cn_eval_handle h);
int  cn_eval_jobs(cn_eval_handle h);
int  cn_eval_reset(cn_eval_handle h, void* stream);                       /* ONE launch */
int  cn_eval_record(cn_eval_handle h, float launch, void* stream);        /* ONE launch, grid (1,1,J) x 1024 */
int  cn_eval_finish(cn_eval_handle h, int metric, float* fitness_dev /* [n_groups] or NULL */, void* stream);  /* ONE launch */
const cn_eval_state* cn_eval_state_dev(cn_eval_handle h);

/* Population-based training on a cn_td3_pop handle: every so often the n_replace worst members take over the networks and the
 * optimizer state of members among the n_replace best (exploit) and perturb the hyper-parameters they inherit (explore).  The
 * hyper-parameters lie by value in the device tables that cn_td3_pop_create built; cn_td3_pop_exploit rewrites them there, so
 * the cn_td3_pop_update calls after it train with the new values and cost what they cost before.
 * cn_td3_pop_pbt_bind(h, cfg, logs): allocates the device state (zero: calls, applied, generation, fitness, last; src = the member's
 * own index; hyper[] = the members' cn_td3_config values) and keeps cfg.  logs: n_members episode logs whose tot_dev feed the
 * fitness, or NULL (every cn_td3_pop_exploit then passes fitness_dev).  Binding again starts over.  Not enqueue-only.
 * cn_td3_pop_exploit(h, fitness_dev, stream): at most TWO launches, enqueue-only, no host read and no copy, capturable on one stream
 * like cn_td3_pop_update.  Statement, with P = n_members, n = n_replace, c = state.calls before the call:
 *   fitness   fitness_dev != NULL: fitness_p = fitness_dev[p] and the call is applied.  NULL: with e_p = tot_p[0] - last_p[0] (new
 *             episodes) and r_p = tot_p[2] - last_p[1] (their returns' sum), last_p[2] float64 owned by the handle: if any e_p <
 *             min_episodes the call is SKIPPED -- calls = c + 1 and nothing else on the device changes; else fitness_p = (float)(r_p /
 *             e_p), the quotient in float64, and after the call last_p = {tot_p[0], tot_p[2]} for every member.
 *   rank      p stands before q when fitness_p > fitness_q (float comparison: -0.0 equals 0.0), or when q's is NaN and p's is not, or when
 *             neither holds either way and p < q.  top[k] = the k-th member of that order, bottom[k] = the (P - 1 - k)-th, k = 0 .. n-1:
 *             disjoint, since n <= P / 2.
 *   source    K = mix64(seed ^ mix64(c));  bottom[k] copies from top[mix64(K ^ (k + 1)) % n]   (mix64: cn_td3_batch_dev's, above)
 *   exploit   dst receives, BIT FOR BIT, src's 36 parameter tensors (the six networks, targets included), Adam's moments of the three
 *             optimised networks, the bias corrections, step counters and running beta products of the tick (adam[4], steps[2],
 *             pw[4]).  It keeps its own update counter, seed, replay ring, workspaces and loss slot.
 *   explore   for k < CN_PBT_HYPERS: v = state.member[src].hyper[k]; if bit k of explore_mask is set, v = v * factor[mix64(K ^
 *             mix64(0x100 + 8 dst + k)) >> 63] (float32); v = min(max(v, lo[k]), hi[k]); state.member[dst].hyper[k] = v, and v is
 *             written wherever the update tables hold hyper-parameter k of member dst.
 *   state     member[dst] = {src, generation + 1, fitness_dst, hyper as above}; a member that is not replaced: {its own index,
 *             generation unchanged, fitness_p, hyper unchanged}, and nothing of it is written besides.  calls = c + 1, applied + 1.
 * The second launch copies; no member is both read and written.  After an applied call a member that was replaced equals its source
 * in everything an update reads except the counter, the seed, the ring and the hyper-parameters that were perturbed.
 * Refused before any device work, text in cn_td3_last_error -- CN_ERR_ARG: a NULL handle or cfg; n_replace outside 1 ... n_members / 2
 * (a population of one cannot bind); min_episodes < 1; a factor that is not finite and > 0; lo > hi or a bound that is not finite;
 * explore_mask bits at or above CN_PBT_HYPERS; a log with a NULL rows, n_dev or tot_dev or a negative max_rows; cn_td3_pop_exploit before a
 * bind, or with fitness_dev NULL when no logs were bound.  CN_ERR_CONFIG: a member whose hyper-parameter starts outside [lo, hi].
 * cn_td3_pop_pbt_state_dev: the device state, read-only for the caller, valid until the next bind or the handle's end; NULL before
 * a bind or for a NULL handle. */
enum { CN_PBT_LR_ACTOR = 0, CN_PBT_LR_CRITIC, CN_PBT_GAMMA, CN_PBT_NOISE_STD, CN_PBT_NOISE_CLIP, CN_PBT_HYPERS };   /* 5 */
typedef struct cn_td3_pbt_config {
    int32_t  n_replace;      /* the n worst members copy from the n best; 1 ... n_members / 2 */
    int32_t  min_episodes;   /* log-fed fitness: every member needs this many NEW episodes, else the call changes nothing; >= 1 */
    uint32_t explore_mask;   /* bit k: hyper-parameter k of a replaced member is perturbed; the others are taken from its source unchanged */
    int32_t  reserved;
    float    factor[2];      /* e.g. 0.8, 1.2; both finite and > 0 */
    float    lo[CN_PBT_HYPERS], hi[CN_PBT_HYPERS];   /* clamp after the perturbation; lo <= hi, finite */
    uint64_t seed;           /* keys source choice and factor choice with the call counter */
} cn_td3_pbt_config;
typedef struct cn_td3_pbt_member {  /* device, read-only for the caller */
    int32_t src;             /* last applied call: the member copied from, or its own index if it survived */
    int32_t generation;      /* how many times this member has been replaced */
    float   fitness;         /* as ranked in the last applied call */
    float   hyper[CN_PBT_HYPERS];   /* what the update tables hold for this member NOW */
} cn_td3_pbt_member;
typedef struct cn_td3_pbt_state {   /* device */
    uint64_t calls, applied;        /* every cn_td3_pop_exploit counts in calls; applied counts only those that were not skipped */
    cn_td3_pbt_member member[64];
} cn_td3_pbt_state;
int cn_td3_pop_pbt_bind(cn_td3_pop_handle h, const cn_td3_pbt_config* cfg, const cn_episode_log* logs /* [n_members] or NULL */);
int cn_td3_pop_exploit(cn_td3_pop_handle h, const float* fitness_dev /* [n_members], or NULL = from the bound logs */, void* stream);
const cn_td3_pbt_state* cn_td3_pop_pbt_state_dev(cn_td3_pop_handle h);

/* A learner's whole state as one blob in device memory, out and in by ONE launch each (csrc/crowdnav_state.hip), whatever the number
 * of members.  Statement: a handle that loads a blob continues, BIT FOR BIT, as the handle that saved it would have -- every
 * cn_td3_update / cn_td3_pop_update / cn_td3_pop_exploit after the load writes the bytes it would have written after the save.  (The
 * replay ring, the seed and the configuration are the caller's: the same ring contents and the same configuration are assumed.)
 * Blob = cn_state_header | cn_state_segment directory[n_segments] | payload.  Every segment's offset is a multiple of 16; a segment
 * holds `bytes` bytes and the bytes up to the next multiple of 16 are ZERO, so equal states give equal blobs.  The payload's first
 * segment starts at sizeof(cn_state_header) + n_segments * sizeof(cn_state_segment) (a multiple of 16); the segments follow each other
 * in directory order without other gaps; total_bytes = the last segment's offset + its bytes rounded up to 16.
 * Segments, in this order.  Per member p = 0 .. n_members-1 (a solo handle is member 0):
 *   CN_STATE_PARAM    index 0..35: network (actor, actor_t, q1, q1_t, q2, q2_t) x tensor (w1, b1, w2, b2, w3, b3), float32 -- the
 *                     nn.Linear storages that the configuration names, so the blob is self-contained
 *   CN_STATE_MOMENT   index 0..35: optimised network (actor, q1, q2) x tensor x (m, v), float32, the sizes of the parameters
 *   CN_STATE_ADAM     float32[4]    CN_STATE_STEPS  float32[2]    CN_STATE_PW  float64[4]   (the tick's: bias corrections, step
 *                     counters, running beta products)
 *   CN_STATE_COUNTER  uint64: the update counter that keys the replay sampling (cn_td3_pop_exploit never copies it)
 *   CN_STATE_LOSS     float32: the first critic's MSE of the last update
 *   CN_STATE_HYPER    populations only: float32[CN_PBT_HYPERS] in CN_PBT_* order, as the device tables of cn_td3_pop_update hold them
 *                     NOW (a solo handle trains with its configuration's values and has no such segment)
 * then, member = -1, only when cn_td3_pop_pbt_bind was called (header.pbt_bound = 1):
 *   CN_STATE_PBT      cn_td3_pbt_state, whole          CN_STATE_PBT_LAST  float64[n_members][2], the log-fed fitness' `last`
 * The workspace (the gathered batch, activations, partial sums) is not part of the state: every update rewrites what it reads of it.
 * cn_td3_state_size / cn_td3_pop_state_size: total_bytes for this handle (0 for a NULL handle or on an error, text in
 *   cn_td3_last_error).  The first call builds the launch's job table in device memory (it allocates and synchronises); it is kept
 *   until the handle ends or cn_td3_pop_pbt_bind is called.  Call it before capturing a save into a graph.
 * _save(h, blob_dev, bytes, stream): ONE launch, enqueue-only, no host read, capturable.  Writes header, directory, payload and the
 *   zero padding -- every byte of [blob_dev, blob_dev + bytes) and none outside: a consistent picture at its point in the stream.
 * _load(h, blob_dev, bytes, stream): waits for `stream`, reads header and directory to the host (one small synchronous copy), then ONE
 *   launch.  A population's load writes each hyper-parameter to every place the update reads it (both chains' tick tables, both
 *   sampling modes' prep tables, every job that carries gamma); with PBT bound, the PBT state and `last` as well.
 * Both: the launch is one workgroup per piece of at most 4096 words of a segment; plain vector loads and stores, 16 bytes wide where
 *   the live tensor and its place in the blob reach a 16-byte boundary together, 4 bytes otherwise: any 4-byte alignment of the live
 *   tensors and of blob_dev works.
 * Refused, nothing written, text in cn_td3_last_error -- CN_ERR_ARG: a NULL handle or blob_dev; blob_dev not 4-byte aligned; bytes
 *   other than the handle's size; (load) a wrong magic or version.  CN_ERR_CONFIG: (load) a header whose family, n_members, obs_dim,
 *   hidden, batch, pbt_bound, n_segments or total_bytes, or a directory entry, differs from the handle's (the text names the field).
 * cn_td3_state_segment_dev / cn_td3_pop_state_segment_dev(h, i, seg_out): directory entry i of this handle (seg_out may be NULL) and
 *   the live device address its bytes are copied from, read-only for the caller (tests and tools); NULL for i out of range (seg_out
 *   is then left alone) and for CN_STATE_HYPER, whose values live scattered in the tables (seg_out is filled in). */
#define CN_STATE_MAGIC 0x0045544154534E43ull      /* "CNSTATE" little-endian */
#define CN_STATE_VERSION 1
enum { CN_STATE_FAMILY_TD3 = 1 };                 /* (DDPG, SAC, DQN: later lists of the same table) */
enum { CN_STATE_PARAM = 0, CN_STATE_MOMENT, CN_STATE_ADAM, CN_STATE_STEPS, CN_STATE_PW, CN_STATE_COUNTER, CN_STATE_LOSS,
       CN_STATE_HYPER, CN_STATE_PBT, CN_STATE_PBT_LAST, CN_STATE_KINDS };
typedef struct cn_state_header {
    uint64_t magic;            /* CN_STATE_MAGIC */
    int32_t  version;          /* CN_STATE_VERSION */
    int32_t  family;           /* CN_STATE_FAMILY_* */
    int32_t  n_members;        /* 1 for a solo handle */
    int32_t  obs_dim, hidden, batch;
    int32_t  pbt_bound;        /* 1: the CN_STATE_PBT and CN_STATE_PBT_LAST segments are present */
    int32_t  n_segments;
    uint64_t total_bytes;      /* header + directory + payload, padding included */
} cn_state_header;
typedef struct cn_state_segment {
    int32_t  member;           /* 0 .. n_members-1, or -1 for the population's own segments */
    int32_t  kind;             /* CN_STATE_* */
    int32_t  index;            /* within the kind */
    int32_t  reserved;         /* 0 */
    uint64_t offset;           /* from the blob's start; a multiple of 16 */
    uint64_t bytes;            /* without the padding */
} cn_state_segment;
size_t cn_td3_state_size(cn_td3_handle h);
int cn_td3_state_save(cn_td3_handle h, void* blob_dev, size_t bytes, void* stream);
int cn_td3_state_load(cn_td3_handle h, const void* blob_dev, size_t bytes, void* stream);
const void* cn_td3_state_segment_dev(cn_td3_handle h, int i, cn_state_segment* seg_out);
size_t cn_td3_pop_state_size(cn_td3_pop_handle h);
int cn_td3_pop_state_save(cn_td3_pop_handle h, void* blob_dev, size_t bytes, void* stream);
int cn_td3_pop_state_load(cn_td3_pop_handle h, const void* blob_dev, size_t bytes, void* stream);
const void* cn_td3_pop_state_segment_dev(cn_td3_pop_handle h, int i, cn_state_segment* seg_out);

/* n_steps calls of cn_step (auto_reset = 2, the next-step reset convention) with OPEN-LOOP actions -- scripted or recorded
 * actions, action repeat, the uniform-random warm-up phase of an off-policy learner -- as ONE launch: a wavefront keeps its
 * environment for the whole launch and walks its steps at its own pace (no launch boundary and no device-wide join between
 * steps).  Results are bit-identical to n_steps cn_step calls.  Slot t of a buffer starts `stride` ELEMENTS after slot t - 1;
 * stride 0 = one slot (actions: the same [N, 2] held for every step; outputs: every step overwrites the slot).
 *   action  dev n_steps slots [N, 2] float32;  obs dev n_steps slots [N, D] float32 (slot t = the observation step t returns)
 *   reward / done / topk_idx (or NULL): n_steps slots [N] / [N] / [N, K]
 * Every configuration cn_create accepts has this form (round 5: social force, wheel ramp, both risk modes, the 720-ray shape; round 6:
 * the contact ticks and obs_layout 1 / 2): cn_kernel_name(h, 2) says which kernel runs it. */
typedef struct cn_sequence_io {
    const float* action;
    float* obs;
    float* reward;
    uint8_t* done;
    int32_t* topk_idx;
    int64_t action_stride, obs_stride, reward_stride, done_stride, topk_stride;
    int32_t n_steps, reserved;
} cn_sequence_io;
int cn_step_sequence(cn_handle h, const cn_sequence_io* io, void* stream);

/* n_steps control periods with the POLICY IN THE LOOP, as ONE launch: per period a_t = actor(o_t) + exploration noise, clipped
 * (cn_actor_forward's arithmetic, noise keyed by (seed, counter + t, env row)), then Env.step(a_t) (cn_step, auto_reset = 2) --
 * the collection loop of start_td3_training.py:104-168 (agent.act -> env.step) for every environment of the handle without a
 * launch or a device-wide join between periods: a workgroup = 16 environments joins only with itself, the actor runs on its CU's
 * matrix cores between two steps.  Results are bit-identical to n_steps x (cn_actor_forward, cn_step) with counters counter,
 * counter + 1, ...  The weights are those of `actor` for the whole launch (a learner that updates every period sees a policy
 * lag of at most n_steps periods; n_steps = 1 is the per-period loop as one launch instead of two).
 *   obs0     dev [N, D]: the observation the first action is computed from (cn_reset's / the previous call's last slot; may
 *            alias slot 0 of obs when obs_stride = 0)
 *   action   dev n_steps slots [N, 2] float32, OUTPUT: slot t = the action period t took
 *   obs / reward / done / topk_idx (or NULL): as cn_sequence_io (slot t = what period t's step returned)
 * Requirements: 8 environments of the handle's shape fitting one CU's LDS (16 per workgroup where they fit; obs_layout 2 always runs
 * 8: its observation needs more registers than a 16-wave workgroup leaves a wave), and an actor of cn_actor_pack_weights' layout for
 * this handle's observation width cn_obs_dim(h) -- 366 + 4 K, or 363 / 370 for obs_layout 1 / 2 at 360 rays -- with hidden = 256.
 * Every configuration cn_create accepts has this form as well (cn_kernel_name(h, 5)). */
typedef struct cn_policy_io {
    const float* obs0;
    float* action;
    float* obs;
    float* reward;
    uint8_t* done;
    int32_t* topk_idx;
    int64_t action_stride, obs_stride, reward_stride, done_stride, topk_stride;
    int32_t n_steps, reserved;
    float max_v, max_w, sigma, reserved_f;
    uint64_t seed, counter;
} cn_policy_io;
int cn_rollout_policy(cn_handle h, const cn_actor_weights* actor, const cn_policy_io* io, void* stream);

/* get_episode_status / get_*_safety_violation_status inputs (ENV:1265-1283).
 * out: dev [N,14] = ego_viol, social_viol, obstacle_present_steps, ep_steps, success, failure, status, n_tracks,
 *                  episodes finished since cn_create, reset pending (auto_reset == 2),
 *                  and the LAST FINISHED episode's ego_viol, social_viol, obstacle_present_steps, ep_steps as they stood
 *                  when Env.step returned done (what TRAIN:142-147 reads before the next reset zeroes them) */
#define CN_COUNTER_COLS 14
int cn_get_counters(cn_handle h, int32_t* out, void* stream);
/* return of the last finished episode and running return, dev [N] each (either may be NULL) */
int cn_get_returns(cn_handle h, float* last_return, float* running_return, void* stream);

/* Parity/debug view of one env (synchronises).  host buffers, any may be NULL:
 *   scalars[24] (layout: CN_SD_* below), robot_ped (5 + 4P doubles: x,y,yaw,v,w, ped xy, ped vxy),
 *   tracks [track_capacity][12] one record per slot (CN_TF_*; the first n_tracks slots are live), ints[16] */
int cn_debug_env(cn_handle h, int env, double* scalars, double* robot_ped, double* tracks, int32_t* ints);

/* Sizing diagnostics (no handle, no GPU): LDS bytes one env of obs_layout 0 needs for n_rays / n_peds / k with max_conf
 * confirmed-object slots ((n_rays - 1) / 4 + 2 inside cn_create) and track_capacity slots; cn_create refuses > 160 KiB.
 * cn_near_separate: 1 when the near-pedestrian list gets its own LDS region at no cost in wavefronts per CU. */
size_t cn_lds_bytes(int n_rays, int n_peds, int k, int max_conf, int track_capacity);
int cn_near_separate(int n_rays, int n_peds, int k, int max_conf, int track_capacity);

/* Whole-state snapshot for deterministic replay and for stepping the CPU oracle from a GPU state.
 * Blob = cn_snapshot_header | sd [N][CN_SD_COUNT] f64 | si [N][CN_SI_COUNT] i32 | ped_p [N][P][2] f64 | ped_v [N][P][2] f64
 *        | trk [N][track_capacity][CN_TF_COUNT] f64 | ped_init [N][P][2] f64 | ped_preset [N][P][2] f64 | ped_aux [N][P][3] f64
 * (ped_aux: goal x, y and goal counter of ped_mode 2; zeros otherwise).  The header carries the ABI version and the FULL cn_config of the handle
 * that wrote it (env_index_base, seed, layout and mode switches included): cn_restore refuses a blob whose header does not
 * match the restoring handle field for field (CN_ERR_CONFIG, the message names the first field that differs) -- a state only
 * means something under the configuration that produced it.  Then it checks the payload's records (csrc/crowdnav_snapshot_check.h
 * states the rule): every stored field that a kernel uses as a count, an index, a loop bound or a flag -- CN_SI_NTRACKS, CN_SI_DQ_LEN,
 * CN_TF_DQLEN, the done / pending flags, CN_SI_EP_STEP, CN_SI_NCONF / CN_SI_NENTRIES, the crowd clock's sign, with risk_mode gt the
 * pedestrian id in CN_TF_T -- must be in the range the simulator produces, and poses, pedestrians and live track fields finite and
 * inside the room (odometry from cn_observe_external or poses from cn_set_ped_init outside room_half: clamp them before the call);
 * otherwise CN_ERR_CONFIG, the message names environment and field, and nothing is written to the handle.
 * crowdnav.env.VecEnv.save_snapshot / load_snapshot wrap the blob
 * in an .npz with the header spelled out; oracle/ (test infrastructure) loads that file into the CPU oracle. */
#define CN_SNAPSHOT_MAGIC 0x50414E534E43ull       /* "CNSNAP" little-endian */
typedef struct cn_snapshot_header {
    uint64_t magic;
    int32_t abi_version;       /* CN_ABI_VERSION of the writer */
    int32_t header_bytes;      /* sizeof(cn_snapshot_header) */
    int32_t sd_count, si_count, tf_count, track_capacity;   /* CN_SD_COUNT, CN_SI_COUNT, CN_TF_COUNT, resolved tracker slots */
    uint64_t total_bytes;      /* header + payload */
    cn_config config;
} cn_snapshot_header;
size_t cn_snapshot_size(cn_handle h);
int cn_snapshot(cn_handle h, void* host_buf, size_t size);
int cn_restore(cn_handle h, const void* host_buf, size_t size);

/* float64 scalar record per env */
enum {
    CN_SD_RX = 0, CN_SD_RY, CN_SD_RYAW, CN_SD_RV, CN_SD_RW, CN_SD_CLOCK, CN_SD_WPX, CN_SD_WPY,
    CN_SD_PREV_DIST, CN_SD_PREV_HEAD, CN_SD_DQ0X, CN_SD_DQ0Y, CN_SD_DQ1X, CN_SD_DQ1Y, CN_SD_TS,
    CN_SD_BB, CN_SD_EGO, CN_SD_CPROB, CN_SD_EP_RETURN, CN_SD_LAST_RETURN,
    CN_SD_LAST_EGO_VIOL, CN_SD_LAST_SOCIAL_VIOL, CN_SD_LAST_OBST_STEPS, CN_SD_LAST_EP_STEPS, CN_SD_COUNT = 24
};
/* int32 scalar record per env */
enum {
    CN_SI_DONE = 0, CN_SI_DQ_LEN, CN_SI_NTRACKS, CN_SI_EGO_VIOL, CN_SI_SOCIAL_VIOL, CN_SI_OBST_STEPS,
    CN_SI_SUCCESS, CN_SI_FAILURE, CN_SI_EP_STEP, CN_SI_STATUS, CN_SI_NCONF, CN_SI_NENTRIES,
    CN_SI_CROWD_LO, CN_SI_CROWD_HI, CN_SI_PENDING_RESET, CN_SI_EPISODES, CN_SI_COUNT = 16
};
/* track record fields (ENV:663-670: pose, range, deque(<=2), time stamp, speed, velocity) */
enum {
    CN_TF_PX = 0, CN_TF_PY, CN_TF_DIST, CN_TF_D0X, CN_TF_D0Y, CN_TF_D1X, CN_TF_D1Y, CN_TF_T, CN_TF_SPEED,
    CN_TF_VX, CN_TF_VY, CN_TF_DQLEN, CN_TF_COUNT = 12
};

#ifdef __cplusplus
}
#endif
#endif
