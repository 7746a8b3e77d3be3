// crowdnav_snapshot_check.h -- the record check of cn_restore: is every stored field that a kernel uses as a count, an index, a
// loop bound or a flag inside the range a run produces?  cn_restore checks the header and the configuration first and then calls
// cn_check_records() on the payload BEFORE it synchronises or copies anything: a damaged env*.npy behind `train --resume`, or an
// edited snapshot, is an error message (CN_ERR_CONFIG naming environment and field) and never an out-of-bounds access.
// Plain C++: no HIP, no device (tests/test_planted_states.py compiles it alone with g++ and the sanitizers and walks it on the CPU).
//
// The rule, per environment e, in this order (the first offence is the one reported):
//   si   DONE, PENDING_RESET in {0, 1};  DQ_LEN in {0, 1, 2} (slot index of the agent's two-entry deque);
//        NTRACKS in [0, slots] (loop bound and slot index of the tracker table);  EP_STEP >= 0 (a counter: with auto_reset none, or
//        with a caller's step_counter, it runs past max_steps while a done flag is held);
//        NCONF in [0, max(max_conf, slots)] (the confirmed objects of the lidar tracker, at most max_conf; with risk_mode gt the
//        pedestrians in sight, at most the tracker slots), NENTRIES in [0, slots];
//        CROWD_HI >= 0 (the crowd clock CROWD_HI : CROWD_LO is a non-negative 64-bit count of milliseconds; every CROWD_LO is valid)
//   sd   RX, RY, RYAW finite, |RX|, |RY| <= room_half (the simulator keeps the robot inside the walls; from outside them every wall
//        distance of the ray cast is negative)
//   ped  every position finite and within room_half, every velocity finite
//   trk  of the slots below NTRACKS: DQLEN exactly 0, 1 or 2; with risk_mode gt, T an integer in [0, n_peds) (it is the pedestrian
//        id the top-K indices are read from); every field finite
// Everything else in a record is data: counters, returns, clocks, the status word and way-point fields take any value.
// The simulator produces nothing outside these ranges.  Two calls can: cn_observe_external stores the caller's odometry as it is, and
// cn_set_ped_init the caller's poses; a snapshot taken with either outside room_half is refused on restore (clamp before the call).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/crowdnav.h"

struct CnRecordVerdict {
    int ok;                  // 1: every record passes
    int env;                 // else: the first offending environment,
    const char* section;     //   "si" | "sd" | "ped_p" | "ped_v" | "trk",
    const char* field;       //   the field's name (CN_SI_* / CN_SD_* / CN_TF_* without the prefix; "x" / "y" for a pedestrian),
    int index;               //   the pedestrian or tracker slot (-1 for si / sd),
    double value;            //   and what was stored there
};

// the payload's sections, as cn_snapshot lays them out: sd [N][CN_SD_COUNT], si [N][CN_SI_COUNT], ped_p / ped_v [N][P][2], trk [N][slots][CN_TF_COUNT]
struct CnRecordSections { const double* sd; const int32_t* si; const double* ped_p; const double* ped_v; const double* trk; };

inline CnRecordVerdict cn_record_bad(int env, const char* section, const char* field, int index, double value)
{
    CnRecordVerdict v = {0, env, section, field, index, value};
    return v;
}

inline CnRecordVerdict cn_check_records(const cn_config& c, int slots, int max_conf, int n_envs, const CnRecordSections& s)
{
    static const char* const TF[CN_TF_COUNT] = {"PX", "PY", "DIST", "D0X", "D0Y", "D1X", "D1Y", "T", "SPEED", "VX", "VY", "DQLEN"};
    const int P = c.n_peds;
    const bool gt = c.risk_mode == CN_RISK_GT;
    for (int e = 0; e < n_envs; ++e) {
        const int32_t* si = s.si + (size_t)e * CN_SI_COUNT;
        const double* sd = s.sd + (size_t)e * CN_SD_COUNT;
#define CN_SI_RANGE(F, LO, HI) if (si[CN_SI_##F] < (LO) || si[CN_SI_##F] > (HI)) return cn_record_bad(e, "si", #F, -1, (double)si[CN_SI_##F]);
        CN_SI_RANGE(DONE, 0, 1) CN_SI_RANGE(DQ_LEN, 0, 2) CN_SI_RANGE(NTRACKS, 0, slots) CN_SI_RANGE(EP_STEP, 0, INT32_MAX)
        CN_SI_RANGE(NCONF, 0, (max_conf > slots ? max_conf : slots)) CN_SI_RANGE(NENTRIES, 0, slots) CN_SI_RANGE(CROWD_HI, 0, INT32_MAX) CN_SI_RANGE(PENDING_RESET, 0, 1)
#undef CN_SI_RANGE
        if (!isfinite(sd[CN_SD_RX]) || fabs(sd[CN_SD_RX]) > c.room_half) return cn_record_bad(e, "sd", "RX", -1, sd[CN_SD_RX]);
        if (!isfinite(sd[CN_SD_RY]) || fabs(sd[CN_SD_RY]) > c.room_half) return cn_record_bad(e, "sd", "RY", -1, sd[CN_SD_RY]);
        if (!isfinite(sd[CN_SD_RYAW])) return cn_record_bad(e, "sd", "RYAW", -1, sd[CN_SD_RYAW]);
        for (int i = 0; i < 2 * P; ++i) {
            const double x = s.ped_p[(size_t)e * 2 * P + i];
            if (!isfinite(x) || fabs(x) > c.room_half) return cn_record_bad(e, "ped_p", (i & 1) ? "y" : "x", i >> 1, x);
        }
        for (int i = 0; i < 2 * P; ++i) {
            const double x = s.ped_v[(size_t)e * 2 * P + i];
            if (!isfinite(x)) return cn_record_bad(e, "ped_v", (i & 1) ? "y" : "x", i >> 1, x);
        }
        for (int t = 0; t < si[CN_SI_NTRACKS]; ++t) {
            const double* r = s.trk + ((size_t)e * slots + t) * CN_TF_COUNT;
            const double q = r[CN_TF_DQLEN];
            if (!(q == 0.0 || q == 1.0 || q == 2.0)) return cn_record_bad(e, "trk", "DQLEN", t, q);
            if (gt && !(r[CN_TF_T] >= 0.0 && r[CN_TF_T] < (double)P && r[CN_TF_T] == floor(r[CN_TF_T]))) return cn_record_bad(e, "trk", "T", t, r[CN_TF_T]);
            for (int f = 0; f < CN_TF_COUNT; ++f)
                if (!isfinite(r[f])) return cn_record_bad(e, "trk", TF[f], t, r[f]);
        }
    }
    CnRecordVerdict ok = {1, -1, "", "", -1, 0.0};
    return ok;
}

// "env 3: si.NTRACKS = 65" / "env 0: trk[4].DQLEN = 3" -- the text cn_restore's error and the stand-alone walker print
inline int cn_record_verdict_text(const CnRecordVerdict& v, char* out, size_t size)
{
    if (v.ok) return snprintf(out, size, "ok");
    if (v.index < 0) return snprintf(out, size, "env %d: %s.%s = %.17g", v.env, v.section, v.field, v.value);
    return snprintf(out, size, "env %d: %s[%d].%s = %.17g", v.env, v.section, v.index, v.field, v.value);
}
