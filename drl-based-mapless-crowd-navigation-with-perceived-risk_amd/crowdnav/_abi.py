"""ctypes binding of libcrowdnav.so (include/crowdnav.h).  This is the binding INTEGRATION.md shows
a maintainer of the reference adding; there is no CPU fallback -- importing works anywhere, but
creating an environment raises unless the HIP library loads and a GPU is present."""
import ctypes as C
import os
import subprocess

from .config import CnConfig

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libcrowdnav.so")
BUILD_SH = os.path.join(_PKG, "csrc", "build.sh")

CN_MAX_TRACKS = 64
CN_MAX_TRACKS_WIDE = 1024   # the wide tracker table (track_capacity 128 ... 1024, include/crowdnav.h)
TRACK_CAPACITIES = (0, 32, 64, 128, 256, 512, 1024)      # what cn_create accepts for cn_config.track_capacity
STATUS_BITS = {"track_overflow": 1, "ttc_zero": 2, "dt_zero": 4, "conf_overflow": 8, "track_wide": 16}   # include/crowdnav.h CN_ST_*
EXPECTED_ABI = 7       # the version the ctypes structs below were written against (include/crowdnav.h CN_ABI_VERSION)
CN_PHASE_ALL, CN_PHASE_PRE, CN_PHASE_GET_STATE, CN_PHASE_REWARD = 0, 1, 2, 4
CN_SD_COUNT = 24
CN_SI_COUNT = 16
CN_TF_COUNT = 12
CN_ARB_AUTO, CN_ARB_OLDEST_FIRST, CN_ARB_FAIR = 0, 1, 2      # include/crowdnav.h: cn_set_arbitration
CN_COUNTER_COLS = 14
SD = dict(RX=0, RY=1, RYAW=2, RV=3, RW=4, CLOCK=5, WPX=6, WPY=7, PREV_DIST=8, PREV_HEAD=9, DQ0X=10, DQ0Y=11,
          DQ1X=12, DQ1Y=13, TS=14, BB=15, EGO=16, CPROB=17, EP_RETURN=18, LAST_RETURN=19)
SI = dict(DONE=0, DQ_LEN=1, NTRACKS=2, EGO_VIOL=3, SOCIAL_VIOL=4, OBST_STEPS=5, SUCCESS=6, FAILURE=7, EP_STEP=8,
          STATUS=9, NCONF=10, NENTRIES=11, PENDING_RESET=14, EPISODES=15)
TF = dict(PX=0, PY=1, DIST=2, D0X=3, D0Y=4, D1X=5, D1Y=6, T=7, SPEED=8, VX=9, VY=10, DQLEN=11)

EXPORTS = ["cn_abi_version", "cn_last_error", "cn_create", "cn_destroy", "cn_obs_dim", "cn_config_of",
           "cn_set_ped_init", "cn_get_ped_init", "cn_set_ped_preset_vel", "cn_reset", "cn_step", "cn_step_multi", "cn_set_arbitration", "cn_get_arbitration", "cn_set_group_envs", "cn_kernel_name", "cn_device_clock",
           "cn_observe_external",
           "cn_policy_tail", "cn_actor_pack_weights", "cn_actor_forward", "cn_step_sequence", "cn_rollout_policy", "cn_get_counters",
           "cn_get_returns", "cn_debug_env", "cn_lds_bytes", "cn_near_separate", "cn_snapshot_size", "cn_snapshot", "cn_restore",
           "cn_td3_create", "cn_td3_destroy", "cn_td3_update", "cn_td3_loss_dev", "cn_td3_batch_dev", "cn_td3_last_error",
           "cn_ddpg_create", "cn_ddpg_destroy", "cn_ddpg_update", "cn_ddpg_loss_dev", "cn_ddpg_batch_dev", "cn_ddpg_act",
           "cn_dqn_create", "cn_dqn_destroy", "cn_dqn_update", "cn_dqn_loss_dev", "cn_dqn_batch_dev", "cn_dqn_act",
           "cn_sac_create", "cn_sac_destroy", "cn_sac_update", "cn_sac_loss_dev", "cn_sac_batch_dev", "cn_sac_act",
           "cn_tab_create", "cn_tab_destroy", "cn_tab_set", "cn_tab_get", "cn_tab_tables", "cn_tab_learn_act", "cn_tab_last_error",
           "cn_td3_set_replay_sample", "cn_ddpg_set_replay_sample", "cn_dqn_set_replay_sample", "cn_sac_set_replay_sample",
           "cn_replay_sample_indices", "cn_replay_write", "cn_episode_log_add",
           "cn_td3_pop_create", "cn_td3_pop_destroy", "cn_td3_pop_update", "cn_td3_pop_members", "cn_td3_pop_loss_dev",
           "cn_td3_pop_batch_dev", "cn_td3_pop_set_replay_sample",
           "cn_td3_pop_set_replay_source", "cn_td3_pop_batch_src_dev", "cn_replay_sample_shared",
           "cn_td3_pop_pbt_bind", "cn_td3_pop_exploit", "cn_td3_pop_pbt_state_dev",
           "cn_td3_state_size", "cn_td3_state_save", "cn_td3_state_load", "cn_td3_state_segment_dev",
           "cn_td3_pop_state_size", "cn_td3_pop_state_save", "cn_td3_pop_state_load", "cn_td3_pop_state_segment_dev",
           "cn_actor_pop_create", "cn_actor_pop_destroy", "cn_actor_pop_members", "cn_actor_pop_pack", "cn_actor_pop_forward",
           "cn_actor_pop_weights",
           "cn_pop_record_create", "cn_pop_record_destroy", "cn_pop_record_members", "cn_pop_record_resetting", "cn_pop_record",
           "cn_nstep_record_create", "cn_nstep_record_destroy", "cn_nstep_record_members", "cn_nstep_record_resetting",
           "cn_nstep_record_pending", "cn_nstep_record", "cn_nstep_discount",
           "cn_eval_create", "cn_eval_destroy", "cn_eval_jobs", "cn_eval_reset", "cn_eval_record", "cn_eval_finish", "cn_eval_state_dev",
           "cn_step_group_create", "cn_step_group_step", "cn_step_group_reset", "cn_step_group_jobs", "cn_step_group_kernel_name",
           "cn_step_group_destroy"]
CN_STEP_GROUP_MAX = 64      # include/crowdnav.h: cn_step_group_create's n is 1 ... 64
CN_EVAL_MAX = 64            # include/crowdnav.h: cn_eval_create's n_jobs and n_groups are 1 ... 64
CN_EVAL_COLS = 12           # include/crowdnav.h: the columns of cn_eval_state.sums[j]
CN_EVAL_SUCCESS_RATE, CN_EVAL_MEAN_RETURN = 0, 1      # include/crowdnav.h: cn_eval_finish's metric
EVAL_METRIC = {"success": CN_EVAL_SUCCESS_RATE, "return": CN_EVAL_MEAN_RETURN}
CN_TD3_POP_MAX = 64         # include/crowdnav.h: cn_td3_pop_create's n_members is 1 ... 64
CN_ACTOR_POP_MAX = 64       # include/crowdnav.h: cn_actor_pop_create's n_members is 1 ... 64
CN_POP_RECORD_MAX = 64      # include/crowdnav.h: cn_pop_record_create's n_members is 1 ... 64
CN_NSTEP_MAX = 16           # include/crowdnav.h: cn_nstep_record_create's n_step is 1 ... 16
CN_PBT_HYPER_NAMES = ("lr_actor", "lr_critic", "gamma", "noise_std", "noise_clip")      # include/crowdnav.h: CN_PBT_LR_ACTOR ... in order
CN_PBT_HYPERS = len(CN_PBT_HYPER_NAMES)
CN_STATE_MAGIC, CN_STATE_VERSION, CN_STATE_FAMILY_TD3 = 0x0045544154534E43, 1, 1      # include/crowdnav.h: cn_state_header
CN_STATE_KIND_NAMES = ("param", "moment", "adam", "steps", "pw", "counter", "loss", "hyper", "pbt", "pbt_last")      # CN_STATE_PARAM ... in order
CN_SAMPLE_WITH_REPLACEMENT, CN_SAMPLE_DISTINCT = 0, 1      # include/crowdnav.h: cn_*_set_replay_sample
REPLAY_SAMPLE = {"with": CN_SAMPLE_WITH_REPLACEMENT, "without": CN_SAMPLE_DISTINCT}
CN_REPLAY_OWN, CN_REPLAY_SHARED = 0, 1      # include/crowdnav.h: cn_td3_pop_set_replay_source
REPLAY_SOURCE = {"own": CN_REPLAY_OWN, "shared": CN_REPLAY_SHARED}


def replay_sample_mode(name):
    """"with" | "without" -> CN_SAMPLE_*; anything else is a ValueError."""
    try:
        return REPLAY_SAMPLE[name]
    except (KeyError, TypeError):
        raise ValueError("replay_sample must be 'with' or 'without', not %r" % (name,))


def replay_source(name):
    """"own" | "shared" -> CN_REPLAY_*; anything else is a ValueError."""
    try:
        return REPLAY_SOURCE[name]
    except (KeyError, TypeError):
        raise ValueError("replay_source must be 'own' or 'shared', not %r" % (name,))


class CnStepIO(C.Structure):
    _fields_ = [("action", C.c_void_p), ("step_counter", C.c_void_p), ("obs", C.c_void_p), ("final_obs", C.c_void_p),
                ("obs_f64", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("topk_idx", C.c_void_p),
                ("auto_reset", C.c_int32), ("reserved", C.c_int32)]


class CnExternalIO(C.Structure):
    _fields_ = [("ranges", C.c_void_p), ("odom", C.c_void_p), ("step_counter", C.c_void_p), ("obs", C.c_void_p),
                ("obs_f64", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("topk_idx", C.c_void_p),
                ("is_reset", C.c_int32), ("phase", C.c_int32)]


CN_SNAPSHOT_MAGIC = 0x50414E534E43        # "CNSNAP"


class CnSnapshotHeader(C.Structure):
    """Mirror of `cn_snapshot_header` (include/crowdnav.h): what a snapshot blob starts with."""
    _fields_ = [("magic", C.c_uint64), ("abi_version", C.c_int32), ("header_bytes", C.c_int32),
                ("sd_count", C.c_int32), ("si_count", C.c_int32), ("tf_count", C.c_int32), ("track_capacity", C.c_int32),
                ("total_bytes", C.c_uint64), ("config", CnConfig)]


# What follows the header in a cn_snapshot blob, in order (include/crowdnav.h): name, dtype, shape from the header's N, P, tracker
# slots and record counts.  split_snapshot, join_snapshot and VecEnv.load_snapshot walk this list.
SNAPSHOT_SECTIONS = (
    ("sd", "float64", lambda N, P, cap, hd: (N, hd.sd_count)),
    ("si", "int32", lambda N, P, cap, hd: (N, hd.si_count)),
    ("ped_p", "float64", lambda N, P, cap, hd: (N, P, 2)),
    ("ped_v", "float64", lambda N, P, cap, hd: (N, P, 2)),
    ("trk", "float64", lambda N, P, cap, hd: (N, cap, hd.tf_count)),
    ("ped_init", "float64", lambda N, P, cap, hd: (N, P, 2)),
    ("ped_preset", "float64", lambda N, P, cap, hd: (N, P, 2)),
    ("ped_aux", "float64", lambda N, P, cap, hd: (N, P, 3)),
)


def split_snapshot(buf):
    """A cn_snapshot blob (uint8 array) -> (header, dict of arrays): sd [N,24] f64, si [N,16] i32, ped_p / ped_v [N,P,2],
    trk [N,cap,12], ped_init / ped_preset [N,P,2], ped_aux [N,P,3].  Views into `buf`."""
    import numpy as np
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    if buf.size < C.sizeof(CnSnapshotHeader):
        raise CrowdNavError("truncated snapshot: %d bytes are less than a header" % buf.size)
    hd = CnSnapshotHeader.from_buffer_copy(buf[:C.sizeof(CnSnapshotHeader)].tobytes())
    if hd.magic != CN_SNAPSHOT_MAGIC or hd.header_bytes != C.sizeof(CnSnapshotHeader):
        raise CrowdNavError("not a libcrowdnav snapshot (magic / header size)")
    shapes = [shape(hd.config.n_envs, hd.config.n_peds, hd.track_capacity, hd) for _, _, shape in SNAPSHOT_SECTIONS]
    ends = np.cumsum([hd.header_bytes] + [int(np.prod(s)) * np.dtype(dt).itemsize for s, (_, dt, _) in zip(shapes, SNAPSHOT_SECTIONS)])
    if ends[-1] != hd.total_bytes or ends[-1] > buf.size:      # before any view is taken: a short blob is this error, not numpy's
        raise CrowdNavError("truncated snapshot: %d bytes, header says %d" % (buf.size, hd.total_bytes))
    return hd, {name: buf[ends[i]:ends[i + 1]].view(dt).reshape(shapes[i]) for i, (name, dt, _) in enumerate(SNAPSHOT_SECTIONS)}


def join_snapshot(hd, arrays):
    """Inverse of split_snapshot: header + arrays -> blob for cn_restore."""
    import numpy as np
    return np.concatenate([np.frombuffer(bytes(hd), dtype=np.uint8)] +
                          [np.ascontiguousarray(arrays[k], dtype=dt).reshape(-1).view(np.uint8) for k, dt, _ in SNAPSHOT_SECTIONS])


def config_to_dict(c):
    return {name: getattr(c, name) for name, _ in CnConfig._fields_}


class CnActorWeights(C.Structure):
    _fields_ = [("w1p", C.c_void_p), ("b1", C.c_void_p), ("w2p", C.c_void_p), ("b2", C.c_void_p), ("w3", C.c_void_p),
                ("b3", C.c_void_p), ("obs_dim", C.c_int32), ("obs_dim_padded", C.c_int32), ("hidden", C.c_int32),
                ("reserved", C.c_int32)]


class CnTd3Mlp(C.Structure):
    """Mirror of `cn_td3_mlp`: device pointers to one network's nn.Linear storages."""
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "w2", "b2", "w3", "b3")]


class CnActorPopMember(C.Structure):
    """Mirror of `cn_actor_pop_member` (include/crowdnav.h): one member of cn_actor_pop_create."""
    _fields_ = [("actor", CnTd3Mlp), ("obs", C.c_void_p), ("action", C.c_void_p), ("n", C.c_int32), ("reserved", C.c_int32),
                ("max_v", C.c_float), ("max_w", C.c_float), ("sigma", C.c_float), ("reserved_f", C.c_float), ("seed", C.c_uint64)]


class CnTd3Config(C.Structure):
    """Mirror of `cn_td3_config` (include/crowdnav.h)."""
    _fields_ = [("obs_dim", C.c_int32), ("hidden", C.c_int32), ("batch", C.c_int32), ("policy_delay", C.c_int32),
                ("gamma", C.c_float), ("tau", C.c_float), ("lr_actor", C.c_float), ("lr_critic", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("noise_std", C.c_float), ("noise_clip", C.c_float), ("max_v", C.c_float),
                ("max_w", C.c_float), ("reserved", C.c_float),
                ("actor", CnTd3Mlp), ("actor_t", CnTd3Mlp), ("q1", CnTd3Mlp), ("q1_t", CnTd3Mlp), ("q2", CnTd3Mlp), ("q2_t", CnTd3Mlp),
                ("replay_s", C.c_void_p), ("replay_a", C.c_void_p), ("replay_r", C.c_void_p), ("replay_s2", C.c_void_p), ("replay_d", C.c_void_p),
                ("replay_size_dev", C.c_void_p), ("seed", C.c_uint64)]


class CnDdpgConfig(C.Structure):
    """Mirror of `cn_ddpg_config` (include/crowdnav.h)."""
    _fields_ = [("obs_dim", C.c_int32), ("hidden", C.c_int32), ("batch", C.c_int32), ("reserved0", C.c_int32),
                ("gamma", C.c_float), ("tau", C.c_float), ("lr_actor", C.c_float), ("lr_critic", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("max_v", C.c_float), ("max_w", C.c_float), ("reserved1", C.c_float),
                ("actor", CnTd3Mlp), ("actor_t", CnTd3Mlp), ("critic", CnTd3Mlp), ("critic_t", CnTd3Mlp),
                ("replay_s", C.c_void_p), ("replay_a", C.c_void_p), ("replay_r", C.c_void_p), ("replay_s2", C.c_void_p), ("replay_d", C.c_void_p),
                ("replay_size_dev", C.c_void_p), ("seed", C.c_uint64)]


class CnDdpgActIO(C.Structure):
    """Mirror of `cn_ddpg_act_io` (include/crowdnav.h)."""
    _fields_ = [("obs", C.c_void_p), ("state", C.c_void_p), ("reset", C.c_void_p), ("u", C.c_void_p), ("action", C.c_void_p),
                ("noise_out", C.c_void_p), ("mu", C.c_double), ("theta", C.c_double), ("sigma", C.c_double),
                ("seed", C.c_uint64), ("counter", C.c_uint64), ("max_v", C.c_float), ("max_w", C.c_float),
                ("n", C.c_int32), ("add_noise", C.c_int32)]


class CnDqnConfig(C.Structure):
    """Mirror of `cn_dqn_config` (include/crowdnav.h)."""
    _fields_ = [("obs_dim", C.c_int32), ("obs_ld", C.c_int32), ("hidden", C.c_int32), ("batch", C.c_int32),
                ("gamma", C.c_float), ("lr", C.c_float), ("rho", C.c_float), ("eps", C.c_float),
                ("target_every", C.c_int32), ("learn_start", C.c_int32), ("q", CnTd3Mlp), ("q_t", CnTd3Mlp),
                ("replay_s", C.c_void_p), ("replay_a", C.c_void_p), ("replay_r", C.c_void_p), ("replay_s2", C.c_void_p), ("replay_d", C.c_void_p),
                ("replay_size_dev", C.c_void_p), ("seed", C.c_uint64)]


class CnDqnBatch(C.Structure):
    """Mirror of `cn_dqn_batch`: s, a (int32 indices), r, s2, d, perm (int32, or None)."""
    _fields_ = [(n, C.c_void_p) for n in ("s", "a", "r", "s2", "d", "perm")]


class CnDqnActIO(C.Structure):
    """Mirror of `cn_dqn_act_io` (include/crowdnav.h)."""
    _fields_ = [("obs", C.c_void_p), ("obs_ld", C.c_int64), ("n", C.c_int32), ("obs_dim", C.c_int32), ("hidden", C.c_int32),
                ("reserved", C.c_int32), ("q", CnTd3Mlp), ("epsilon", C.c_double), ("epsilon_discount", C.c_double),
                ("epsilon_min", C.c_double), ("episodes_dev", C.c_void_p), ("seed", C.c_uint64),
                ("counter", C.c_uint64), ("action", C.c_void_p), ("twist", C.c_void_p), ("q_out", C.c_void_p)]


class CnSacActor(C.Structure):
    """Mirror of `cn_sac_actor`: the trunk's two layers, then the two heads."""
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "w2", "b2", "mean_w", "mean_b", "log_std_w", "log_std_b")]


class CnSacConfig(C.Structure):
    """Mirror of `cn_sac_config` (include/crowdnav.h)."""
    _fields_ = [("obs_dim", C.c_int32), ("hidden", C.c_int32), ("hidden_v", C.c_int32), ("batch", C.c_int32),
                ("gamma", C.c_float), ("tau", C.c_float), ("lr_actor", C.c_float), ("lr_v", C.c_float), ("lr_q", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("max_v", C.c_float), ("max_w", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("mean_lambda", C.c_float), ("std_lambda", C.c_float), ("z_lambda", C.c_float), ("logp_eps", C.c_float),
                ("soft_update", C.c_int32), ("reserved", C.c_int32),
                ("actor", CnSacActor), ("q", CnTd3Mlp), ("v", CnTd3Mlp), ("v_t", CnTd3Mlp),
                ("replay_s", C.c_void_p), ("replay_a", C.c_void_p), ("replay_r", C.c_void_p), ("replay_s2", C.c_void_p), ("replay_d", C.c_void_p),
                ("replay_size_dev", C.c_void_p), ("seed", C.c_uint64)]


class CnSacActIO(C.Structure):
    """Mirror of `cn_sac_act_io` (include/crowdnav.h)."""
    _fields_ = [("obs", C.c_void_p), ("obs_ld", C.c_int64), ("n", C.c_int32), ("obs_dim", C.c_int32), ("hidden", C.c_int32),
                ("deterministic", C.c_int32), ("actor", CnSacActor),
                ("max_v", C.c_float), ("max_w", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("eps", C.c_void_p), ("seed", C.c_uint64), ("counter", C.c_uint64),
                ("twist", C.c_void_p), ("mean", C.c_void_p), ("log_std", C.c_void_p), ("z", C.c_void_p)]


CN_TAB_STATES, CN_TAB_ACTIONS = 977, 3
CN_TAB_QLEARN, CN_TAB_SARSA = 0, 1


class CnTabConfig(C.Structure):
    """Mirror of `cn_tab_config` (include/crowdnav.h)."""
    _fields_ = [("algo", C.c_int32), ("reserved", C.c_int32), ("alpha", C.c_double), ("gamma", C.c_double), ("seed", C.c_uint64)]


class CnTabIO(C.Structure):
    """Mirror of `cn_tab_io` (include/crowdnav.h)."""
    _fields_ = [("obs_prev", C.c_void_p), ("obs", C.c_void_p), ("obs_ld", C.c_int64), ("n", C.c_int32), ("col", C.c_int32),
                ("learn", C.c_int32), ("act", C.c_int32), ("action_prev", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("keep", C.c_void_p), ("epsilon", C.c_double), ("epsilon_discount", C.c_double), ("epsilon_min", C.c_double),
                ("episodes_dev", C.c_void_p), ("u_learn", C.c_void_p), ("u_act", C.c_void_p), ("counter", C.c_uint64),
                ("action", C.c_void_p), ("twist", C.c_void_p), ("state", C.c_void_p), ("state_prev", C.c_void_p), ("q_row", C.c_void_p)]


class CnTd3Batch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("s", "a", "r", "s2", "d", "target_noise")]


class CnReplayRing(C.Structure):
    """Mirror of `cn_replay_ring` (include/crowdnav.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("s", "a", "r", "s2", "d")] + [("capacity", C.c_int64), ("pos_dev", C.c_void_p),
                                                                         ("size_dev", C.c_void_p), ("obs_dim", C.c_int32), ("reserved", C.c_int32)]


class CnEpisodeLog(C.Structure):
    """Mirror of `cn_episode_log` (include/crowdnav.h)."""
    _fields_ = [("rows", C.c_void_p), ("max_rows", C.c_int64), ("n_dev", C.c_void_p), ("tot_dev", C.c_void_p)]


class CnTd3PbtConfig(C.Structure):
    """Mirror of `cn_td3_pbt_config` (include/crowdnav.h)."""
    _fields_ = [("n_replace", C.c_int32), ("min_episodes", C.c_int32), ("explore_mask", C.c_uint32), ("reserved", C.c_int32),
                ("factor", C.c_float * 2), ("lo", C.c_float * CN_PBT_HYPERS), ("hi", C.c_float * CN_PBT_HYPERS), ("seed", C.c_uint64)]


class CnTd3PbtMember(C.Structure):
    """Mirror of `cn_td3_pbt_member` (include/crowdnav.h)."""
    _fields_ = [("src", C.c_int32), ("generation", C.c_int32), ("fitness", C.c_float), ("hyper", C.c_float * CN_PBT_HYPERS)]


class CnStateHeader(C.Structure):
    """Mirror of `cn_state_header` (include/crowdnav.h)."""
    _fields_ = [("magic", C.c_uint64), ("version", C.c_int32), ("family", C.c_int32), ("n_members", C.c_int32), ("obs_dim", C.c_int32),
                ("hidden", C.c_int32), ("batch", C.c_int32), ("pbt_bound", C.c_int32), ("n_segments", C.c_int32), ("total_bytes", C.c_uint64)]


class CnStateSegment(C.Structure):
    """Mirror of `cn_state_segment` (include/crowdnav.h)."""
    _fields_ = [("member", C.c_int32), ("kind", C.c_int32), ("index", C.c_int32), ("reserved", C.c_int32), ("offset", C.c_uint64),
                ("bytes", C.c_uint64)]


class CnTd3PbtState(C.Structure):
    """Mirror of `cn_td3_pbt_state` (include/crowdnav.h)."""
    _fields_ = [("calls", C.c_uint64), ("applied", C.c_uint64), ("member", CnTd3PbtMember * CN_TD3_POP_MAX)]


class CnPopRecordMember(C.Structure):
    """Mirror of `cn_pop_record_member` (include/crowdnav.h): one member of cn_pop_record_create."""
    _fields_ = [("env", C.c_void_p), ("counters", C.c_void_p), ("last_return", C.c_void_p), ("prev", C.c_void_p), ("obs", C.c_void_p),
                ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("ring", CnReplayRing), ("log", CnEpisodeLog),
                ("n", C.c_int32), ("reserved", C.c_int32)]


class CnNstepMember(C.Structure):
    """Mirror of `cn_nstep_member` (include/crowdnav.h): one member of cn_nstep_record_create."""
    _fields_ = [("rec", CnPopRecordMember), ("gamma", C.c_float), ("reserved_f", C.c_float)]


class CnNstepPending(C.Structure):
    """Mirror of `cn_nstep_pending` (include/crowdnav.h): a member's pending store, device pointers owned by the handle."""
    _fields_ = [("s", C.c_void_p), ("a", C.c_void_p), ("ret", C.c_void_p), ("count", C.c_void_p), ("clock", C.c_void_p),
                ("n", C.c_int32), ("n_step", C.c_int32), ("obs_dim", C.c_int32), ("reserved", C.c_int32)]


class CnEvalJob(C.Structure):
    """Mirror of `cn_eval_job` (include/crowdnav.h): one job of cn_eval_create."""
    _fields_ = [("env", C.c_void_p), ("counters", C.c_void_p), ("last_return", C.c_void_p), ("done", C.c_void_p), ("log", CnEpisodeLog),
                ("n", C.c_int32), ("quota", C.c_int32), ("group", C.c_int32), ("reserved", C.c_int32)]


class CnEvalState(C.Structure):
    """Mirror of `cn_eval_state` (include/crowdnav.h)."""
    _fields_ = [("remaining", C.c_int32 * CN_EVAL_MAX), ("sums", (C.c_double * CN_EVAL_COLS) * CN_EVAL_MAX),
                ("summary", (C.c_float * 8) * CN_EVAL_MAX), ("fitness", C.c_float * CN_EVAL_MAX)]


class CnSequenceIO(C.Structure):
    """Mirror of `cn_sequence_io` (include/crowdnav.h)."""
    _fields_ = [("action", C.c_void_p), ("obs", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("topk_idx", C.c_void_p),
                ("action_stride", C.c_int64), ("obs_stride", C.c_int64), ("reward_stride", C.c_int64), ("done_stride", C.c_int64),
                ("topk_stride", C.c_int64), ("n_steps", C.c_int32), ("reserved", C.c_int32)]


class CnPolicyIO(C.Structure):
    """Mirror of `cn_policy_io` (include/crowdnav.h)."""
    _fields_ = [("obs0", C.c_void_p), ("action", C.c_void_p), ("obs", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("topk_idx", C.c_void_p),
                ("action_stride", C.c_int64), ("obs_stride", C.c_int64), ("reward_stride", C.c_int64), ("done_stride", C.c_int64),
                ("topk_stride", C.c_int64), ("n_steps", C.c_int32), ("reserved", C.c_int32),
                ("max_v", C.c_float), ("max_w", C.c_float), ("sigma", C.c_float), ("reserved_f", C.c_float),
                ("seed", C.c_uint64), ("counter", C.c_uint64)]


class CrowdNavError(RuntimeError):
    pass


def build(force=False):
    """Compile libcrowdnav.so for gfx950 (hipcc cross-compiles without a GPU).  Safe to call from several ranks
    at once: the staleness check and the build run under a file lock and build.sh renames the finished library into
    place, so no process ever maps a half-written file."""
    import fcntl
    srcs = [os.path.join(_PKG, "csrc", f) for f in os.listdir(os.path.join(_PKG, "csrc"))]
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "crowdnav.h"))

    def stale():
        return force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(s) for s in srcs)

    if stale():
        os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
        with open(os.path.join(os.path.dirname(LIB_PATH), ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            try:
                if stale():          # another rank may have built it while we waited
                    subprocess.check_call(["bash", BUILD_SH])
            finally:
                fcntl.flock(lk, fcntl.LOCK_UN)
    return LIB_PATH


def build_timing(force=False):
    """Compile the PROFILING build lib/libcrowdnav_timing.so (stage time stamps, ablation mask, PMC calibration kernels:
    tools/stage_timing.py, tools/ablate.py, tools/calib_pmc.py).  Never loaded by the product."""
    tpath = LIB_PATH.replace("libcrowdnav.so", "libcrowdnav_timing.so")
    srcs = [os.path.join(_PKG, "csrc", f) for f in os.listdir(os.path.join(_PKG, "csrc"))]
    if force or not os.path.exists(tpath) or os.path.getmtime(tpath) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["bash", BUILD_SH, "timing"])
    return tpath


_lib = None


def lib():
    global _lib
    if _lib is None:
        try:
            build()          # no-op when lib/libcrowdnav.so is newer than every source
        except Exception as ex:  # hipcc missing: use what is there, or fail loudly below
            if not os.path.exists(LIB_PATH):
                raise CrowdNavError("libcrowdnav.so is not built (%s) and cannot be built here (%s); there is no CPU "
                                    "fallback" % (LIB_PATH, ex))
            import warnings
            warnings.warn("libcrowdnav.so could not be rebuilt (%s); loading the existing %s -- its ABI version is "
                          "checked below" % (ex, LIB_PATH))
        # PyTorch-ROCm ships its own HIP / ROCr runtime libraries; the caller's tensors live in THAT runtime.  Importing
        # torch first makes libcrowdnav.so's libamdhip64 dependency resolve to the copy that is already loaded.  Loaded
        # the other way round the process ends up with two runtimes and cn_create sees no device (CN_ERR_NO_DEVICE).
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.cn_abi_version.restype = C.c_int
        if L.cn_abi_version() != EXPECTED_ABI:   # a stale library with other struct layouts would corrupt kernel arguments
            raise CrowdNavError("%s reports ABI %d but this binding is written against ABI %d: rebuild it "
                                "(csrc/build.sh)" % (LIB_PATH, L.cn_abi_version(), EXPECTED_ABI))
        L.cn_last_error.restype = C.c_char_p
        L.cn_kernel_name.argtypes = [C.c_void_p, C.c_int]; L.cn_kernel_name.restype = C.c_char_p
        L.cn_set_group_envs.argtypes = [C.c_void_p, C.c_int64]
        L.cn_device_clock.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.cn_create.argtypes = [C.POINTER(CnConfig), C.c_int, C.POINTER(vp)]
        L.cn_destroy.argtypes = [vp]; L.cn_destroy.restype = None
        L.cn_obs_dim.argtypes = [vp]
        L.cn_config_of.argtypes = [vp, C.POINTER(CnConfig)]
        L.cn_set_ped_init.argtypes = [vp, vp]
        L.cn_get_ped_init.argtypes = [vp, vp]
        L.cn_set_ped_preset_vel.argtypes = [vp, vp]
        L.cn_reset.argtypes = [vp, vp, vp, vp, vp]
        L.cn_step.argtypes = [vp, C.POINTER(CnStepIO), vp]
        L.cn_step_multi.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(CnStepIO), C.POINTER(vp)]
        L.cn_step_group_create.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(CnStepIO), C.POINTER(vp)]
        L.cn_step_group_step.argtypes = [vp, vp]
        L.cn_step_group_reset.argtypes = [vp, C.POINTER(vp), vp]
        L.cn_step_group_jobs.argtypes = [vp]
        L.cn_step_group_kernel_name.argtypes = [vp]; L.cn_step_group_kernel_name.restype = C.c_char_p
        L.cn_step_group_destroy.argtypes = [vp]; L.cn_step_group_destroy.restype = None
        L.cn_set_arbitration.argtypes = [vp, C.c_int]
        L.cn_get_arbitration.argtypes = [vp]
        L.cn_observe_external.argtypes = [vp, C.POINTER(CnExternalIO), vp]
        L.cn_policy_tail.argtypes = [vp, vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_uint64, C.c_int, vp]
        L.cn_actor_pack_weights.argtypes = [vp, C.c_int, vp, C.c_int, vp]
        L.cn_actor_forward.argtypes = [C.POINTER(CnActorWeights), vp, vp, C.c_int, C.c_float, C.c_float, C.c_float,
                                       C.c_uint64, C.c_uint64, C.c_int, vp]
        L.cn_step_sequence.argtypes = [vp, C.POINTER(CnSequenceIO), vp]
        L.cn_rollout_policy.argtypes = [vp, C.POINTER(CnActorWeights), C.POINTER(CnPolicyIO), vp]
        L.cn_get_counters.argtypes = [vp, vp, vp]
        L.cn_get_returns.argtypes = [vp, vp, vp, vp]
        L.cn_debug_env.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.cn_snapshot_size.argtypes = [vp]; L.cn_snapshot_size.restype = C.c_size_t
        L.cn_snapshot.argtypes = [vp, vp, C.c_size_t]
        L.cn_restore.argtypes = [vp, vp, C.c_size_t]
        L.cn_td3_create.argtypes = [C.POINTER(CnTd3Config), C.c_int, C.POINTER(vp)]
        L.cn_td3_destroy.argtypes = [vp]; L.cn_td3_destroy.restype = None
        L.cn_td3_update.argtypes = [vp, C.c_int, C.POINTER(CnTd3Batch), vp]
        L.cn_td3_loss_dev.argtypes = [vp]; L.cn_td3_loss_dev.restype = vp
        L.cn_td3_batch_dev.argtypes = [vp, C.c_int]; L.cn_td3_batch_dev.restype = vp
        L.cn_td3_last_error.restype = C.c_char_p
        L.cn_td3_pop_create.argtypes = [C.POINTER(CnTd3Config), C.c_int, C.c_int, C.POINTER(vp)]      # an array of n_members configs
        L.cn_td3_pop_destroy.argtypes = [vp]; L.cn_td3_pop_destroy.restype = None
        L.cn_td3_pop_update.argtypes = [vp, C.c_int, vp]
        L.cn_td3_pop_members.argtypes = [vp]
        L.cn_td3_pop_loss_dev.argtypes = [vp]; L.cn_td3_pop_loss_dev.restype = vp
        L.cn_td3_pop_batch_dev.argtypes = [vp, C.c_int, C.c_int]; L.cn_td3_pop_batch_dev.restype = vp
        L.cn_td3_pop_set_replay_sample.argtypes = [vp, C.c_int]
        L.cn_td3_pop_set_replay_source.argtypes = [vp, C.c_int]
        L.cn_td3_pop_batch_src_dev.argtypes = [vp, C.c_int]; L.cn_td3_pop_batch_src_dev.restype = vp
        L.cn_replay_sample_shared.argtypes = [C.c_uint64, C.c_uint64, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]
        L.cn_td3_pop_pbt_bind.argtypes = [vp, C.POINTER(CnTd3PbtConfig), C.POINTER(CnEpisodeLog)]      # logs: an array of n_members, or None
        L.cn_td3_pop_exploit.argtypes = [vp, vp, vp]
        L.cn_td3_pop_pbt_state_dev.argtypes = [vp]; L.cn_td3_pop_pbt_state_dev.restype = vp
        for pre in ("cn_td3_state_", "cn_td3_pop_state_"):
            getattr(L, pre + "size").argtypes = [vp]; getattr(L, pre + "size").restype = C.c_size_t
            getattr(L, pre + "save").argtypes = [vp, vp, C.c_size_t, vp]
            getattr(L, pre + "load").argtypes = [vp, vp, C.c_size_t, vp]
            getattr(L, pre + "segment_dev").argtypes = [vp, C.c_int, C.POINTER(CnStateSegment)]; getattr(L, pre + "segment_dev").restype = vp
        L.cn_actor_pop_create.argtypes = [C.POINTER(CnActorPopMember), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]      # an array of members
        L.cn_actor_pop_destroy.argtypes = [vp]; L.cn_actor_pop_destroy.restype = None
        L.cn_actor_pop_members.argtypes = [vp]
        L.cn_actor_pop_pack.argtypes = [vp, vp]
        L.cn_actor_pop_forward.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int, vp]      # counters: a host array [n_members]
        L.cn_actor_pop_weights.argtypes = [vp, C.c_int, C.POINTER(CnActorWeights)]
        L.cn_pop_record_create.argtypes = [C.POINTER(CnPopRecordMember), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]      # an array of members
        L.cn_pop_record_destroy.argtypes = [vp]; L.cn_pop_record_destroy.restype = None
        L.cn_pop_record_members.argtypes = [vp]
        L.cn_pop_record_resetting.argtypes = [vp, C.c_int]; L.cn_pop_record_resetting.restype = vp
        L.cn_pop_record.argtypes = [vp, C.c_float, vp]
        L.cn_nstep_record_create.argtypes = [C.POINTER(CnNstepMember), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.cn_nstep_record_destroy.argtypes = [vp]; L.cn_nstep_record_destroy.restype = None
        L.cn_nstep_record_members.argtypes = [vp]
        L.cn_nstep_record_resetting.argtypes = [vp, C.c_int]; L.cn_nstep_record_resetting.restype = vp
        L.cn_nstep_record_pending.argtypes = [vp, C.c_int, C.POINTER(CnNstepPending)]
        L.cn_nstep_record.argtypes = [vp, C.c_float, vp]
        L.cn_nstep_discount.argtypes = [C.c_float, C.c_int]; L.cn_nstep_discount.restype = C.c_float
        L.cn_eval_create.argtypes = [C.POINTER(CnEvalJob), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]      # an array of jobs
        L.cn_eval_destroy.argtypes = [vp]; L.cn_eval_destroy.restype = None
        L.cn_eval_jobs.argtypes = [vp]
        L.cn_eval_reset.argtypes = [vp, vp]
        L.cn_eval_record.argtypes = [vp, C.c_float, vp]
        L.cn_eval_finish.argtypes = [vp, C.c_int, vp, vp]
        L.cn_eval_state_dev.argtypes = [vp]; L.cn_eval_state_dev.restype = vp
        L.cn_ddpg_create.argtypes = [C.POINTER(CnDdpgConfig), C.c_int, C.POINTER(vp)]
        L.cn_ddpg_destroy.argtypes = [vp]; L.cn_ddpg_destroy.restype = None
        L.cn_ddpg_update.argtypes = [vp, C.POINTER(CnTd3Batch), vp]
        L.cn_ddpg_loss_dev.argtypes = [vp]; L.cn_ddpg_loss_dev.restype = vp
        L.cn_ddpg_batch_dev.argtypes = [vp, C.c_int]; L.cn_ddpg_batch_dev.restype = vp
        L.cn_ddpg_act.argtypes = [C.POINTER(CnActorWeights), C.POINTER(CnDdpgActIO), C.c_int, vp]
        L.cn_dqn_create.argtypes = [C.POINTER(CnDqnConfig), C.c_int, C.POINTER(vp)]
        L.cn_dqn_destroy.argtypes = [vp]; L.cn_dqn_destroy.restype = None
        L.cn_dqn_update.argtypes = [vp, C.POINTER(CnDqnBatch), vp]
        L.cn_dqn_loss_dev.argtypes = [vp]; L.cn_dqn_loss_dev.restype = vp
        L.cn_dqn_batch_dev.argtypes = [vp, C.c_int]; L.cn_dqn_batch_dev.restype = vp
        L.cn_dqn_act.argtypes = [C.POINTER(CnDqnActIO), C.c_int, vp]
        L.cn_sac_create.argtypes = [C.POINTER(CnSacConfig), C.c_int, C.POINTER(vp)]
        L.cn_sac_destroy.argtypes = [vp]; L.cn_sac_destroy.restype = None
        L.cn_sac_update.argtypes = [vp, C.POINTER(CnTd3Batch), vp]
        L.cn_sac_loss_dev.argtypes = [vp]; L.cn_sac_loss_dev.restype = vp
        L.cn_sac_batch_dev.argtypes = [vp, C.c_int]; L.cn_sac_batch_dev.restype = vp
        L.cn_sac_act.argtypes = [C.POINTER(CnSacActIO), C.c_int, vp]
        L.cn_tab_create.argtypes = [C.POINTER(CnTabConfig), C.c_int, C.POINTER(vp)]
        L.cn_tab_destroy.argtypes = [vp]; L.cn_tab_destroy.restype = None
        L.cn_tab_set.argtypes = [vp, vp, vp, vp]
        L.cn_tab_get.argtypes = [vp, vp, vp, vp]
        L.cn_tab_tables.argtypes = [vp, vp, vp, vp]
        L.cn_tab_learn_act.argtypes = [vp, C.POINTER(CnTabIO), vp]
        L.cn_tab_last_error.restype = C.c_char_p
        for fam in ("td3", "ddpg", "dqn", "sac"):
            getattr(L, "cn_%s_set_replay_sample" % fam).argtypes = [vp, C.c_int]
        L.cn_replay_sample_indices.argtypes = [C.c_uint64, C.c_uint64, C.c_int, vp, C.c_int, vp, C.c_int, vp]
        L.cn_replay_write.argtypes = [C.POINTER(CnReplayRing), vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp]
        L.cn_episode_log_add.argtypes = [C.POINTER(CnEpisodeLog), vp, vp, C.c_int, vp, vp, C.c_float, C.c_int, C.c_int, vp]
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise CrowdNavError("libcrowdnav error %d: %s" % (rc, lib().cn_last_error().decode()))
