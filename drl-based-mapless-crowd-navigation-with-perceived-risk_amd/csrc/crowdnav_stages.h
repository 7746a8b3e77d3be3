// crowdnav_stages.h -- the one table of the step kernel's stage stamps: the 32 slots of a row of the timing buffer [env][32]
// (cn_debug_set_timing; profiling build only) and the four stamps at which a FAIR kernel lowers its s_setprio level (product
// behaviour).  crowdnav_kernel.hip stamps with CN_T(CN_STG_<NAME>) / POL_T(CN_STG_POL_<NAME>) and takes the levels from here;
// tools/isa_ledger.py parses this file (stages()) for its own ledger and for stage_timing.py, stage_instr.py and wave_tail.py, which
// keep no table of their own (tests/test_stage_table.py).  Plain C++: no HIP, no device.
//
// A row:  X(NAME, slot, "label", fair_level), the rows IN EXECUTION ORDER (env_kernel_body / observe)
//   slot         index into the env's timing row, and k of cn_debug_set_ablate's cut code (k + 1) << 8.  The numbers are history
//                (20-24, 27, 28 were added between 1 and 2 later) and stay: the committed profiles are keyed by them.
//   label        what ENDS at the stamp
//   fair_level   the s_setprio level a FAIR kernel takes at the stamp (an SFENCE kernel: a scheduling fence), CN_FAIR_NONE elsewhere
// PHYS_TRIG / PHYS_PEDS (27, 28) are stamped by the one-step kernels inside the 150 ms advance (tools/stage_timing_physics.py) and
// share their slots with the policy kernel's first two stamps, which writes them once per workgroup and period instead.
#pragma once

#define CN_FAIR_NONE (-1)
#define CN_STAGES(X) \
    X(ENTRY,     0,  "kernel entry, parameter loads, LDS map", 3) \
    X(LOAD,      1,  "load state",                             CN_FAIR_NONE) \
    X(PHYS_TRIG, 27, "physics: trig of the step",              CN_FAIR_NONE) \
    X(PHYS_PEDS, 28, "physics: pedestrians",                   CN_FAIR_NONE) \
    X(PHYS,      20, "physics: robot (dt)",                    CN_FAIR_NONE) \
    X(SCAN_LAT,  21, "deque, robot (scan latency)",            CN_FAIR_NONE) \
    X(OBS_ENTRY, 22, "observe entry",                          CN_FAIR_NONE) \
    X(DIST_HEAD, 23, "way-point (step 1), distance, heading",  CN_FAIR_NONE) \
    X(WAYPOINT,  24, "way-point refresh",                      CN_FAIR_NONE) \
    X(TWIST,     2,  "twist features",                         CN_FAIR_NONE) \
    X(NEAR,      3,  "lidar set-up, near-pedestrian list",     CN_FAIR_NONE) \
    X(RAYS,      4,  "ray loop (cast, end points, obs)",       CN_FAIR_NONE) \
    X(BBOX,      5,  "scan min, bbox / deque at step 0",       CN_FAIR_NONE) \
    X(GRAD,      6,  "gradients",                              CN_FAIR_NONE) \
    X(FLAGS,     7,  "flag words",                             2) \
    X(TYPES,     8,  "type machine",                           CN_FAIR_NONE) \
    X(ALIAS,     9,  "aliasing",                               CN_FAIR_NONE) \
    X(ASSOC,     10, "association (IoU)",                      CN_FAIR_NONE) \
    X(ORDER,     11, "order / split words",                    1) \
    X(BASES,     12, "word bases",                             CN_FAIR_NONE) \
    X(CONFIRM,   13, "confirmation, counters",                 CN_FAIR_NONE) \
    X(TRACKER,   14, "tracker",                                CN_FAIR_NONE) \
    X(SPEEDS,    15, "speeds, defaults",                       0) \
    X(CONE,      16, "collision cone, top-K",                  CN_FAIR_NONE) \
    X(TAIL,      17, "counters, done, tail",                   CN_FAIR_NONE) \
    X(OUTPUTS,   18, "tracker write-back, reward, outputs",    CN_FAIR_NONE) \
    X(STORE,     19, "state write-back",                       CN_FAIR_NONE)

// not time stamps: where the wavefront runs (env_kernel_body, next to ENTRY; tools/wave_fairness.py, policy_phase_timing.py)
#define CN_HWID_SLOTS(X) \
    X(HW_ID,  25, "HW_ID register: wave slot, SIMD, CU, SE") \
    X(XCC_ID, 26, "XCC_ID register")

// the policy kernel's stamps (policy_sequence_body: wave 0 of a workgroup, in the row of its first environment; the last period stays)
#define CN_POL_STAGES(X) \
    X(POL_PERIOD, 27, "period start") \
    X(POL_LOCK,   28, "lock wait, barrier") \
    X(POL_ACTOR,  29, "actor tile, barrier") \
    X(POL_STEP,   30, "Env.step of wave 0") \
    X(POL_WAIT,   31, "wait for the slowest wave")

// CN_STG_<NAME> = the slot, for the rows of all three tables (the policy kernel's: CN_STG_POL_<NAME>)
#define CN_STG_ENUM_(NAME, SLOT, ...) CN_STG_##NAME = SLOT,
enum { CN_STAGES(CN_STG_ENUM_) CN_HWID_SLOTS(CN_STG_ENUM_) CN_POL_STAGES(CN_STG_ENUM_) CN_STAGE_SLOTS = 32 };

// the s_setprio level of the stamp in `slot`, CN_FAIR_NONE where the level stays
#define CN_STG_FAIR_(NAME, SLOT, LABEL, FAIR) if (slot == SLOT) return FAIR;
constexpr int cn_stage_fair(int slot) { CN_STAGES(CN_STG_FAIR_) return CN_FAIR_NONE; }
