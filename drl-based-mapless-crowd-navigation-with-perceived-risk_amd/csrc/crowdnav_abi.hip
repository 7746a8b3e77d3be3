// crowdnav_abi.hip -- host side of libcrowdnav.so: the C-ABI declared in include/crowdnav.h.
// Owns the per-env SoA state in HBM, builds the constant tables, and enqueues the fused step
// kernel on the caller's stream.  No CPU fallback exists: without a HIP device cn_create fails.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>

#include "crowdnav_device.h"
#include "crowdnav_host.h"
#include "crowdnav_actor.h"
#include "crowdnav_lds.h"
#include "crowdnav_variants.h"
#include "crowdnav_snapshot_check.h"

// every kernel that takes CnKParams, from the table (crowdnav_variants.h): declarations, then the functions in cn_kernel_info's order --
// [0, CN_K_N_DYNAMIC) are launched with cn_create's dynamic LDS size, [CN_K_N_DYNAMIC, CN_K_COUNT) are the policy kernels (both ranges
// get hipFuncAttributeMaxDynamicSharedMemorySize above 64 KiB)
typedef void (*cn_kernel_fn)(CnKParams);
#define CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) extern "C" __global__ void NAME(CnKParams p);
CN_DYNAMIC_LDS_KERNELS CN_POLICY_KERNELS
#undef CN_KERNEL
#define CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) NAME,
static const cn_kernel_fn kKernelFn[] = { CN_DYNAMIC_LDS_KERNELS CN_POLICY_KERNELS };
#undef CN_KERNEL
static_assert(sizeof(kKernelFn) / sizeof(kKernelFn[0]) == CN_K_COUNT && CN_K_N_DYNAMIC == 53 && CN_K_COUNT - CN_K_N_DYNAMIC == 15,
              "the table's 53 dynamic-LDS kernels and 15 policy kernels");
// the group kernels (CN_GROUP_KERNELS: cn_step_group_*), in cn_group_kernel_info's order
typedef void (*cn_group_fn)(const CnKParams*);
#define CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) extern "C" __global__ void NAME(const CnKParams* jobs);
CN_GROUP_KERNELS
#undef CN_KERNEL
#define CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) NAME,
static const cn_group_fn kGroupFn[] = { CN_GROUP_KERNELS };
#undef CN_KERNEL
static_assert(sizeof(kGroupFn) / sizeof(kGroupFn[0]) == CN_G_COUNT, "the table's group kernels");
extern "C" __global__ void cn_bbox_kernel(CnKParams p, double* out);
extern "C" __global__ void cn_gather_kernel(CnKParams p, float* last_ret, float* run_ret, int32_t* counters);

static thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

static void destroy_handle(cn_env_s* h)
{
    if (!h) return;
    DeviceScope scope(h->device);
    (void)hipFree(h->d_lidar); (void)hipFree(h->d_poly); (void)hipFree(h->d_state);
    (void)hipFree(h->d_ped_init); (void)hipFree(h->d_ped_preset);
    (void)hipFree(h->d_trk); (void)hipFree(h->d_ped_aux);
    delete h;
}
struct HandleDeleter { void operator()(cn_env_s* h) const { destroy_handle(h); } };

// Host restatement of the kernel's association table for bb = bb_spawn (crowdnav_kernel.hip, "ENV:448-485"): the same IEEE
// operations in the same order (+ - * / floor ceil; this file is compiled with -ffp-contract=off like the kernel), so the
// table a wavefront copies equals the one it would compute.  Pinned by the rollout parity tests: the oracle evaluates the IoU
// itself; simulated runs take the copied table, cn_observe_external replays (box size from the external scan) the computed one.
static void build_assoc_table(CnKParams& k, int16_t* tab)
{
    k.assoc_fast = 0; k.assoc_k1 = 0;
    const double Tm = 2000.0 * k.bb_spawn;
    const int K1 = (int)floor(Tm - 1e-7), K2 = (int)ceil(Tm + 1e-7);
    if (!((K2 == K1 + 1) && K1 >= 0 && K1 <= 254)) return;
    const double c_hi = 0.0005 * (1.0 + 1e-6), c_lo = 0.0005 * (1.0 - 1e-6);
    const double T2 = Tm * Tm;
    const double Phi = T2 * (2.0 * c_hi) / (1.0 + c_hi), Plo = T2 * (2.0 * c_lo) / (1.0 + c_lo);
    for (int d = 0; d <= K1 + 1; ++d) {
        int m = -1;
        if (d <= K1) {
            const double fx = Tm - (double)d;
            const double mm = fmin(ceil(Tm - Phi / fx) - 1.0, (double)K1);
            m = mm < 0.0 ? -1 : (int)mm;
            if (m >= 0 && !(fx * (Tm - (double)m) > Phi)) return;
            if (m + 1 <= K1 && !(fx * (Tm - (double)(m + 1)) < Plo)) return;
        }
        tab[d] = (int16_t)m;
    }
    k.assoc_k1 = K1; k.assoc_fast = 1;
}

// An environment's LDS working set is crowdnav_lds.h's map, for cn_create's sizes (env_kernel_body carves the same regions)
int cn_near_separate(int R, int P, int K, int max_conf, int trk_cap) { return cn_lds_near_separate(R, P, K, max_conf, trk_cap); }
size_t cn_lds_bytes(int R, int P, int K, int max_conf, int trk_cap)
{
    return cn_lds_map(R - 1, P, K, max_conf, cn_lds_trk_slots(trk_cap), cn_near_separate(R, P, K, max_conf, trk_cap), false, false).total;
}

extern "C" int cn_abi_version(void) { return CN_ABI_VERSION; }
extern "C" const char* cn_last_error(void) { return g_err.c_str(); }

static void default_ped_init(const cn_config& c, int env, double* xy)
{
    // seeded uniform in the room, rejected within 0.4 m of the robot spawn
    int64_t gid = c.env_index_base + env;
    double lo = -c.room_half + 0.1, span = 2.0 * c.room_half - 0.2;
    for (int i = 0; i < c.n_peds; ++i) {
        uint32_t att = 0;
        for (;;) {
            double x = fma(span, cn_rng_u01(c.seed, gid, 2u, (uint32_t)i, 2 * att), lo);
            double y = fma(span, cn_rng_u01(c.seed, gid, 2u, (uint32_t)i, 2 * att + 1), lo);
            double dx = x - c.spawn_x, dy = y - c.spawn_y;
            ++att;
            if (fma(dx, dx, dy * dy) >= 0.16 || att > 1000) { xy[2 * i] = x; xy[2 * i + 1] = y; break; }
        }
    }
}

static double angle_increment_deg(int R)
{
    // UTL:113 `max_angle / (resolution - 1)` with Python-2 integer operands (360/359 == 1).
    // For R-1 > 360 Python 2 would give 0; defined as true division (outside the reference's range).
    if (R - 1 <= 360) return (double)(360 / (R - 1));
    return 360.0 / (double)(R - 1);
}

// One field of every env's record <- a dense host array [N, width bytes]
static int field_to_device(cn_env_s* h, size_t off, const void* host, size_t width)
{
    if (!width) return CN_OK;
    CN_HIPCHK(fail, hipMemcpy2D(h->d_state + off, h->stride, host, width, width, (size_t)h->cfg.n_envs, hipMemcpyHostToDevice));
    return CN_OK;
}
#define FIELD(call) do { int rc_ = (call); if (rc_ != CN_OK) return rc_; } while (0)

static int upload_initial_state(cn_env_s* h)
{
    const cn_config& c = h->cfg;
    const int N = c.n_envs, P = c.n_peds;
    std::vector<double> sd((size_t)N * CN_SD_COUNT, 0.0);
    std::vector<int32_t> si((size_t)N * CN_SI_COUNT, 0);
    for (int e = 0; e < N; ++e) {  // Env.__init__ (ENV:43-168)
        double* s = &sd[(size_t)e * CN_SD_COUNT];
        s[CN_SD_RX] = c.spawn_x; s[CN_SD_RY] = c.spawn_y; s[CN_SD_RYAW] = c.spawn_yaw;
        s[CN_SD_WPX] = c.goal_x; s[CN_SD_WPY] = c.goal_y;
        if (c.obs_layout == CN_LAYOUT_REALWORLD) {   // RW:80 `collision_prob = None` (below every number in Python 2), RW:103 bbox constant
            s[CN_SD_CPROB] = -INFINITY; s[CN_SD_BB] = 0.0210;
        }
    }
    CN_HIPCHK(fail, hipMemset(h->d_state, 0, (size_t)N * h->stride));
    FIELD(field_to_device(h, CN_ST_OFF_SD, sd.data(), CN_SD_COUNT * 8));
    FIELD(field_to_device(h, CN_ST_OFF_SI, si.data(), CN_SI_COUNT * 4));
    if (P > 0) {
        CN_HIPCHK(fail, hipMemcpy(h->d_ped_init, h->ped_init.data(), (size_t)N * P * 16, hipMemcpyHostToDevice));
        FIELD(field_to_device(h, CN_ST_OFF_PED_P, h->ped_init.data(), (size_t)P * 16));
        CN_HIPCHK(fail, hipMemset(h->d_ped_preset, 0, (size_t)N * P * 16));
    }
    CN_HIPCHK(fail, hipMemset(h->d_trk, 0, (size_t)N * CN_TF_COUNT * h->trk_cap * 8));
    {   // ped_mode 2: every pedestrian's first goal (goal 0 of its counter-based sequence); zeros otherwise
        std::vector<double> aux((size_t)N * (P > 0 ? P : 1) * 3, 0.0);
        if (c.ped_mode == 2) {
            const double lo = -c.room_half + 0.1, span = 2.0 * c.room_half - 0.2;
            for (int e = 0; e < N; ++e)
                for (int i = 0; i < P; ++i) {
                    double* a = &aux[((size_t)e * P + i) * 3];
                    a[0] = fma(span, cn_rng_u01(c.seed, c.env_index_base + e, 3u, (uint32_t)i, 0u), lo);
                    a[1] = fma(span, cn_rng_u01(c.seed, c.env_index_base + e, 3u, (uint32_t)i, 1u), lo);
                }
        }
        CN_HIPCHK(fail, hipMemcpy(h->d_ped_aux, aux.data(), aux.size() * 8, hipMemcpyHostToDevice));
    }
    return CN_OK;
}

struct KernelChoice { cn_kernel_fn fn; const char* name; bool compact = false; int wpb = 1; bool x2 = false; };      // compact: launched with h->lds_shape; wpb: environments (waves) per workgroup
static size_t lds_of(const cn_env_s* h, const KernelChoice& kc) { return kc.compact ? h->lds_shape : h->lds; }
// Which kernel a call of `form` (CN_FORM_*) on this handle runs: cn_select_kernel's row of the table.  overlapped: a cn_step that is one
// of several in a cn_step_multi.  fn == nullptr: the world has no such form.
static CnLaunchFacts launch_facts(const cn_env_s* h, bool overlapped) { return CnLaunchFacts{h->arbitration, overlapped, h->n_cus, h->cfg.n_envs, h->group_envs, h->x2, h->wpb4}; }
static KernelChoice kernel_of(const cn_env_s* h, int form, bool overlapped = false)
{
    const int id = cn_select_kernel(h->world, form, launch_facts(h, overlapped));
    if (id < 0) return KernelChoice{nullptr, nullptr};
    const CnKernelInfo& ki = cn_kernel_info[id];
    return KernelChoice{kKernelFn[id], ki.name, ki.compact, ki.geometry == CN_GEO_W4 ? h->wpb4 : 1, ki.geometry == CN_GEO_X2};
}

extern "C" int cn_create(const cn_config* cfg, int device, cn_handle* out)
{
    if (!cfg || !out) return fail(CN_ERR_ARG, "cn_create: null argument");
    const cn_config& c = *cfg;
    if (c.n_envs < 1 || c.n_peds < 0 || c.n_peds > 4096 || c.n_rays < 8 || c.n_rays > 1025 || c.k_obstacles < 1 ||
        c.k_obstacles > CN_MAX_K || c.ped_cycle_ms < 1 || c.dt_ms < 1 || c.scan_latency_ms < 1 || c.settle_ms < 0 ||
        c.max_steps < 1 ||
        !(c.obs_layout == CN_LAYOUT_RISK || c.obs_layout == CN_LAYOUT_ORIGINAL || c.obs_layout == CN_LAYOUT_REALWORLD) ||
        !(c.geos_untyped_empty == 0 || c.geos_untyped_empty == 1) || !(c.ped_contact == 0 || c.ped_contact == 1) ||
        !(c.risk_mode == CN_RISK_LIDAR_TRACKER || c.risk_mode == CN_RISK_GT) || !(c.py2_round == 0 || c.py2_round == 1) ||
        c.ped_mode < 0 || c.ped_mode > 2 || !(c.scan_f32 == 0 || c.scan_f32 == 1))
        return fail(CN_ERR_CONFIG, "cn_create: config out of range");
    const int tc = c.track_capacity;
    if (!(tc == 0 || tc == 32 || tc == 64 || tc == 128 || tc == 256 || tc == 512 || tc == 1024))
        return fail(CN_ERR_CONFIG, "cn_create: track_capacity must be one of 0 (auto), 32, 64 (LDS table) or 128, 256, 512, 1024 "
                                   "(wide table in HBM); got " + std::to_string(tc));
    if (tc > CN_MAX_TRACKS) {
        if (c.risk_mode == CN_RISK_GT)
            return fail(CN_ERR_CONFIG, "cn_create: a wide track_capacity (> 64) is for risk_mode lidar_tracker: in gt mode the entries are "
                                       "the pedestrians in range, rebuilt every observation, and track_capacity 64 already holds them");
        if (c.obs_layout != CN_LAYOUT_RISK || c.ped_contact || c.ped_mode == 2 || c.wheel_accel > 0.0)
            return fail(CN_ERR_CONFIG, "cn_create: a wide track_capacity (> 64) is built for obs_layout 0 with the plain simulator "
                                       "(ped_mode 0 / 1, ped_contact 0, wheel_accel 0) only");
    }
    if (!(c.wheel_accel >= 0.0) || (c.wheel_accel > 0.0 && (c.ped_contact || c.ped_mode == 2 || c.obs_layout != CN_LAYOUT_RISK || !(c.wheel_separation > 0.0))))
        return fail(CN_ERR_CONFIG, "cn_create: wheel_accel must be >= 0 and needs obs_layout 0, the plain simulator (ped_contact 0, ped_mode 0 / 1) "
                                   "and a positive wheel_separation");
    if (c.ped_mode == 2 && (c.ped_contact || c.obs_layout != CN_LAYOUT_RISK || !(c.sf_tau > 0.0) || !(c.sf_B > 0.0) ||
                            !(c.sf_wall_B > 0.0) || !(c.sf_goal_eps >= 0.0) || c.sf_tick_ms < 0 || 64 * (size_t)c.n_peds > cn_lds_sim_scratch(c.n_rays)))
        return fail(CN_ERR_CONFIG, "cn_create: ped_mode 2 (social force) needs obs_layout 0, ped_contact 0, positive sf_tau / sf_B / "
                                   "sf_wall_B and n_peds <= (n_rays - 1) / 4");
    // the pedestrians' repulsion is summed on a 2^-36 grid (include/crowdnav.h): exact while the sum stays below 2^16
    if (c.ped_mode == 2 && !((double)c.n_peds * fabs(c.sf_A) * exp(2.0 * c.ped_radius / c.sf_B) < 32768.0))
        return fail(CN_ERR_CONFIG, "cn_create: ped_mode 2: n_peds * sf_A * exp(2 ped_radius / sf_B) must stay below 2^15 (exact force sums)");
    if (!(c.max_scan_range > c.min_scan_range))    // ENV:581, UTL:322 divide by their difference (ZeroDivisionError in the reference)
        return fail(CN_ERR_CONFIG, "cn_create: max_scan_range must exceed min_scan_range");
    if (c.obs_layout == CN_LAYOUT_REALWORLD && (c.n_rays - 1 > 65535 / 2))
        return fail(CN_ERR_CONFIG, "cn_create: config out of range");
    if (c.risk_mode == CN_RISK_GT && c.obs_layout != CN_LAYOUT_RISK)
        return fail(CN_ERR_CONFIG, "cn_create: risk_mode gt needs the risk observation layout (obs_layout 0)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(CN_ERR_NO_DEVICE, "cn_create: no HIP device (libcrowdnav has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(CN_ERR_ARG, "cn_create: bad device ordinal");
    DeviceScope scope(device);
    // every failure path below (HIPCHK returns) releases what was allocated so far
    std::unique_ptr<cn_env_s, HandleDeleter> guard(new cn_env_s());
    cn_env_s* h = guard.get();
    h->cfg = c;
    h->device = device;
    { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) h->n_cus = ncu; }
    const int N = c.n_envs, P = c.n_peds, R = c.n_rays, K = c.k_obstacles;
    h->D = c.obs_layout == CN_LAYOUT_ORIGINAL ? (R - 1) + 4 : (c.obs_layout == CN_LAYOUT_REALWORLD ? (R - 1) + 11 : (R - 1) + 7 + 4 * K);
    h->max_conf = (R - 1) / 4 + 2;
    // (risk_mode gt lists the simulator's own pedestrians in range: up to P entries, so 33-40 pedestrians take the larger table there --
    // tools/fuzz_parity.py found a 36-pedestrian gt world with more than 32 of them in range)
    h->trk_cap = c.track_capacity ? c.track_capacity : ((P <= 40 && !(c.risk_mode == CN_RISK_GT && P > 32)) ? 32 : 64);
    h->wide = h->trk_cap > CN_MAX_TRACKS;
    const int near_sep = cn_near_separate(R, P, K, h->max_conf, h->trk_cap);
    const bool rw_lists = c.obs_layout == CN_LAYOUT_REALWORLD;
    const CnLdsMap M = cn_lds_map(R - 1, P, K, h->max_conf, cn_lds_trk_slots(h->trk_cap), near_sep, false, rw_lists);
    h->lds = M.total;
    if (c.ped_contact && c.obs_layout != CN_LAYOUT_RISK)
        return fail(CN_ERR_CONFIG, "cn_create: ped_contact is built for the risk observation layout (obs_layout 0) only");
    if (c.ped_contact && 32 * (size_t)P > cn_lds_sim_scratch(R))   // contact corrections: 4 doubles per pedestrian in LDS regions A + B
        return fail(CN_ERR_CONFIG, "cn_create: ped_contact needs n_peds <= (n_rays - 1) / 2");
    if (h->lds > 160 * 1024) { return fail(CN_ERR_CONFIG, "cn_create: per-env working set exceeds 160 KiB of LDS"); }
    // tables
    const int Wb = (R + 63) / 64;
    std::vector<double> lidar(4 * (size_t)R + 2 * (size_t)Wb), poly(128);
    double step = c.lidar_span / (double)(R - 1);
    for (int k = 0; k < R; ++k) cn_det_sincos((double)k * step, &lidar[R + k], &lidar[k]);
    for (int j = 0; j < R - 1; ++j) {  // UTL:121-123 math.radians(i * angle_increment)
        double a = ((double)j * angle_increment_deg(R)) * (M_PI / 180.0);
        lidar[2 * R + j] = sin(a); lidar[3 * R + j] = cos(a);
    }
    for (int q = 0; q < Wb; ++q) {   // axis of 64-ray block q: ray 64 q + 32 (robot frame)
        int kq = 64 * q + 32 < R ? 64 * q + 32 : R - 1;
        lidar[4 * (size_t)R + 2 * q] = lidar[kq]; lidar[4 * (size_t)R + 2 * q + 1] = lidar[R + kq];
    }
    for (int k = 0; k < 64; ++k) { double a = -(double)k * M_PI / 32.0; poly[k] = cos(a); poly[64 + k] = sin(a); }
    CN_HIPCHK(fail, hipMalloc(&h->d_lidar, lidar.size() * 8));
    CN_HIPCHK(fail, hipMalloc(&h->d_poly, poly.size() * 8 + 512));      // + the association table (256 shorts, below)
    CN_HIPCHK(fail, hipMemcpy(h->d_lidar, lidar.data(), lidar.size() * 8, hipMemcpyHostToDevice));
    CN_HIPCHK(fail, hipMemcpy(h->d_poly, poly.data(), poly.size() * 8, hipMemcpyHostToDevice));
    size_t pb = (size_t)N * (P > 0 ? P : 1) * 16;
    h->stride = CN_ST_STRIDE(P);
    CN_HIPCHK(fail, hipMalloc(&h->d_state, (size_t)N * h->stride));
    CN_HIPCHK(fail, hipMalloc(&h->d_ped_init, pb));
    CN_HIPCHK(fail, hipMalloc(&h->d_ped_preset, pb));
    // (a wide handle: + [N][trk_cap] doubles behind the tables, the entries' collision probabilities -- scratch inside one call)
    CN_HIPCHK(fail, hipMalloc(&h->d_trk, (size_t)N * (CN_TF_COUNT + (h->wide ? 1 : 0)) * h->trk_cap * 8));
    CN_HIPCHK(fail, hipMalloc(&h->d_ped_aux, (size_t)N * (P > 0 ? P : 1) * 24));
    h->ped_init.resize((size_t)N * P * 2);
    for (int e = 0; e < N; ++e) default_ped_init(c, e, &h->ped_init[(size_t)e * P * 2]);
    int rc = upload_initial_state(h);
    if (rc != CN_OK) return rc;

    CnKParams& k = h->kp;
    memset(&k, 0, sizeof(k));
    k.N = N; k.P = P; k.R = R; k.K = K;
    k.max_steps = c.max_steps; k.ped_mode = c.ped_mode; k.dt_ms = c.dt_ms; k.scan_latency_ms = c.scan_latency_ms;
    k.settle_ms = c.settle_ms; k.ped_cycle_ms = c.ped_cycle_ms; k.ped_stagger_ms = c.ped_stagger_ms;
    k.geos_untyped_empty = c.geos_untyped_empty; k.ped_contact = c.ped_contact; k.risk_mode = c.risk_mode; k.py2_round = c.py2_round;
    k.lidar_min_positive = c.lidar_min > 0.0 ? 1 : 0;
    k.scan_f32 = c.scan_f32; k.waypoint_reward = c.waypoint_reward; k.wheel_accel = c.wheel_accel; k.wheel_sep = c.wheel_separation;
    k.sf_tau = c.sf_tau; k.sf_A = c.sf_A; k.sf_B = c.sf_B; k.sf_wall_A = c.sf_wall_A; k.sf_wall_B = c.sf_wall_B;
    k.sf_goal_eps2 = c.sf_goal_eps * c.sf_goal_eps; k.sf_tick_ms = c.sf_tick_ms > 0 ? c.sf_tick_ms : 10;
    // pair matrix G [P][P] + next state + goal records in the simulator's LDS scratch (regions A + B)?
    {   // dense social force: the near-pair list behind next / aux [8 P] and acc [2 P] doubles of the scratch
        const size_t scr = M.szA + M.szB, used = 80 * (size_t)P;
        size_t cap = scr > used ? (scr - used) / 2 : 0;
        k.sf_pair_cap = (c.ped_mode == 2 && P <= 128) ? (int32_t)(cap > 60000 ? 60000 : cap) : 0;
    }
    k.sf_pair_matrix = (c.ped_mode == 2 && P >= 2 && P < 256 && 8 * (size_t)P * P + 64 * (size_t)P + (size_t)P * (P - 1) + 16 <= cn_lds_sim_scratch(R)) ? 1 : 0;
    k.near_sep = near_sep;
    // the kernels compiled for a shape assume exactly the six values of its row (crowdnav_lds.h; env_kernel_body, SHAPE != 0)
    auto is_shape = [&](const CnShape& s) {
        return R == s.R && P == s.P && K == s.K && h->max_conf == s.max_conf && h->trk_cap == s.trk_cap && near_sep == s.near_sep &&
               !getenv("CN_NO_SHAPE_KERNELS");
    };
    h->shape360 = is_shape(cn_shapes[CN_SHAPE_360]);
    h->shape720 = is_shape(cn_shapes[CN_SHAPE_720])
                  && c.room_half + c.lidar_max + 1.0 < 32.0;       // the _s720 kernels keep end points as int16 thousandths
    // Four environments per workgroup for the 360-ray step kernels when the whole launch is resident at once (n_envs <= 16 wavefronts
    // x CUs): a quarter of the workgroups for the dispatcher to create, + 2-3 % in every decomposition at 4096 envs; with several
    // rounds of wavefronts (16384 envs) the coarser release of LDS / wave slots costs 3.6 % instead, and the 720-ray shape (12
    // wavefronts per CU, 1.33 rounds at 4096) loses 7-25 % (profiles/r05/ab_wpb.txt).  Decided per launch in cn_select_kernel() from
    // max(n_envs, cn_set_group_envs).  CN_WPB=1 / 2 / 4 / 8 / 16 overrides for A/B runs.
    h->world = cn_world_index(c.obs_layout, h->wide, c.risk_mode == CN_RISK_GT, c.wheel_accel > 0.0,
                              c.ped_mode == 2 && !k.sf_pair_matrix && P <= 128 /* dense social force: per-lane near masks */,
                              c.ped_mode == 2, c.ped_contact != 0, h->shape360, h->shape720);
    h->wpb4 = 4;
    if (getenv("CN_X2")) h->x2 = atoi(getenv("CN_X2")) ? 1 : 0;
    if (getenv("CN_WPB")) { h->wpb4 = atoi(getenv("CN_WPB")); if (h->wpb4 != 2 && h->wpb4 != 4 && h->wpb4 != 8 && h->wpb4 != 16) h->wpb4 = 0; }
    if (h->shape720) h->lds_shape = cn_lds_map(R - 1, P, K, h->max_conf, cn_lds_trk_slots(h->trk_cap), near_sep, true, rw_lists).total;
    k.max_conf = h->max_conf; k.trk_cap = h->trk_cap; k.env_index_base = c.env_index_base; k.seed = c.seed;
    k.room_half = c.room_half; k.ped_radius = c.ped_radius; k.ped_vmax = c.ped_vmax; k.robot_clearance = c.robot_clearance;
    k.lidar_min = c.lidar_min; k.lidar_max = c.lidar_max; k.lidar_offset_x = c.lidar_offset_x;
    k.ped_inv_cycle = 1.0 / (double)c.ped_cycle_ms;
    k.max_scan_range = c.max_scan_range; k.min_scan_range = c.min_scan_range; k.goal_x = c.goal_x; k.goal_y = c.goal_y;
    k.start_x = c.start_x; k.start_y = c.start_y; k.spawn_x = c.spawn_x; k.spawn_y = c.spawn_y; k.spawn_yaw = c.spawn_yaw;
    k.waypoint_radius = c.waypoint_radius; k.goal_eps = c.goal_eps; k.angle_inc_deg = angle_increment_deg(R); k.lidar_step = step;
    { static const double trig[CN_TRIG_COUNT] = CN_TRIG_TABLE; static_assert(sizeof(trig) == sizeof(k.trig), "CnKParams::trig"); memcpy(k.trig, trig, sizeof(trig)); }
    k.blk_dir = h->d_lidar + 4 * (size_t)R;
    {   // near_peds' block test  oc . u_q >= cos(beta) sqrt(d^2 - r^2) - sin(beta) r  is  theta <= beta + asin(r / d)  only while
        // beta + asin(r / d) <= pi (cos decreasing).  With few rays a block's half-width beta = 32.5 steps passes pi / 2 (R < 130) or
        // even pi (R < 66) and the test would clear bits of pedestrians a ray can hit (found by tools/fuzz_parity.py: 13 / 42 / 46
        // rays).  There the block bits are switched off: (cb, sb) = (-1, 1) makes the threshold -(sqrt(d^2 - r^2) + r) <= -d,
        // which every direction passes, so every listed pedestrian is tested in every block.
        const double beta = 32.5 * fabs(step);
        const bool cone_ok = beta < 1.5707;
        k.blk_cb = cone_ok ? cos(beta) : -1.0; k.blk_sb = cone_ok ? sin(beta) : 1.0;
    }
    k.lidar_c = h->d_lidar; k.lidar_s = h->d_lidar + R; k.ang_s = h->d_lidar + 2 * R; k.ang_c = h->d_lidar + 3 * R; k.poly_c = h->d_poly; k.poly_s = h->d_poly + 64;
    k.state = h->d_state; k.state_stride = (int64_t)h->stride; k.ped_init = h->d_ped_init;
    k.ped_preset = h->d_ped_preset; k.trk = h->d_trk; k.ped_aux = h->d_ped_aux;
    {   // the reset path's bounding-box size at the spawn pose (a constant of the configuration), from the device's own arithmetic
        double* d_out = nullptr;
        CN_HIPCHK(fail, hipMalloc(&d_out, sizeof(double)));
        hipLaunchKernelGGL(cn_bbox_kernel, dim3(1), dim3(64), 0, (hipStream_t)0, k, d_out);
        hipError_t e1 = hipGetLastError(), e2 = hipMemcpy(&k.bb_spawn, d_out, sizeof(double), hipMemcpyDeviceToHost);
        (void)hipFree(d_out);
        CN_HIPCHK(fail, e1); CN_HIPCHK(fail, e2);
        k.bb_spawn_valid = 1;
        int16_t tab[256] = {0};
        build_assoc_table(k, tab);
        k.assoc_tab = (const int16_t*)(h->d_poly + 128);
        CN_HIPCHK(fail, hipMemcpy((void*)k.assoc_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
    }
    if (h->shape360 && h->wpb4) {     // the _w4 kernels are only ever launched for the headline shape (cn_select_kernel)
        const size_t w4 = (size_t)h->wpb4 * ((h->lds + 15) & ~(size_t)15);      // what launch() asks for
        if (w4 > 160 * 1024) h->wpb4 = 0;                                        // (a CN_WPB override that does not fit a CU's LDS: one per workgroup)
        else if (w4 > 64 * 1024) {
            for (int id : {CN_K_cn_env_kernel_s360_w4, CN_K_cn_env_kernel_fair_s360_w4})
                CN_HIPCHK(fail, hipFuncSetAttribute((const void*)kKernelFn[id], hipFuncAttributeMaxDynamicSharedMemorySize, (int)w4));
        }
    }
    if (h->lds > 64 * 1024)
    {
        for (int id = 0; id < CN_K_N_DYNAMIC; ++id) CN_HIPCHK(fail, hipFuncSetAttribute((const void*)kKernelFn[id], hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds));
        for (int id = 0; id < CN_G_COUNT; ++id) CN_HIPCHK(fail, hipFuncSetAttribute((const void*)kGroupFn[id], hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds));
    }
    {   // cn_rollout_policy: 16 (or 8) environments per workgroup, their working sets 16-byte aligned one after the other (the
        // actor's 16-row tile is laid out compactly over them between two steps), + the workgroup's actions
        // (this world's policy kernel: the 720-ray shape's has the compact layout)
        h->pol_wave_lds = (lds_of(h, kernel_of(h, CN_FORM_POLICY)) + 15) & ~(size_t)15;
        const size_t tile = actor_tile_bytes((h->D + 31) & ~31);
        const char* pe_env = getenv("CN_POL_ENVS");             // experiments: CN_POL_ENVS=8 forces the 8-environment workgroups
        // (cn_policy_kernel_rw is compiled for 8 waves: the RW observation needs more than the 128 vector registers a 16-wave workgroup leaves a wave)
        for (int pe = ((pe_env && atoi(pe_env) == 8) || h->cfg.obs_layout == CN_LAYOUT_REALWORLD) ? 8 : 16; pe >= 8 && !h->pol_lds; pe -= 8) {
            size_t off = (size_t)pe * h->pol_wave_lds;
            if (off < tile) off = (tile + 15) & ~(size_t)15;
            const size_t tot = off + (size_t)pe * 2 * sizeof(float);
            if (tot <= 160 * 1024) { h->pol_lds = tot; h->pol_envs = pe; h->pol_act_off = off; }
        }
        if (h->pol_lds > 64 * 1024)
            for (int id = CN_K_N_DYNAMIC; id < CN_K_COUNT; ++id) CN_HIPCHK(fail, hipFuncSetAttribute((const void*)kKernelFn[id], hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->pol_lds));
    }
    *out = guard.release();
    return CN_OK;
}

extern "C" void cn_destroy(cn_handle h) { destroy_handle(h); }

#ifdef CN_TIMING
// PROFILING BUILD ONLY (libcrowdnav_timing.so; not in crowdnav.h, not in the product library): stage time stamps
// (tools/stage_timing.py) and the stage-skipping mask for time attribution (tools/ablate.py)
extern "C" int cn_debug_set_timing(cn_handle h, long long* dev_buf) { if (!h) return CN_ERR_ARG; h->kp.timing = dev_buf; return CN_OK; }
extern "C" int cn_debug_set_ablate(cn_handle h, int mask) { if (!h) return CN_ERR_ARG; h->kp.ablate = mask; return CN_OK; }
#endif

extern "C" int cn_obs_dim(cn_handle h) { return h ? h->D : fail(CN_ERR_ARG, "null handle"); }

extern "C" int cn_config_of(cn_handle h, cn_config* out)
{
    if (!h || !out) return fail(CN_ERR_ARG, "cn_config_of: null argument");
    *out = h->cfg;
    return CN_OK;
}

extern "C" int cn_set_ped_init(cn_handle h, const double* xy)
{
    if (!h || !xy) return fail(CN_ERR_ARG, "cn_set_ped_init: null argument");
    DeviceScope scope(h->device);
    size_t cnt = (size_t)h->cfg.n_envs * h->cfg.n_peds * 2;
    h->ped_init.assign(xy, xy + cnt);
    CN_HIPCHK(fail, hipDeviceSynchronize());
    CN_HIPCHK(fail, hipMemcpy(h->d_ped_init, xy, cnt * 8, hipMemcpyHostToDevice));
    FIELD(field_to_device(h, CN_ST_OFF_PED_P, xy, (size_t)h->cfg.n_peds * 16));
    return CN_OK;
}

extern "C" int cn_get_ped_init(cn_handle h, double* xy)
{
    if (!h || !xy) return fail(CN_ERR_ARG, "cn_get_ped_init: null argument");
    memcpy(xy, h->ped_init.data(), h->ped_init.size() * 8);
    return CN_OK;
}

extern "C" int cn_set_ped_preset_vel(cn_handle h, const double* vxy)
{
    if (!h || !vxy) return fail(CN_ERR_ARG, "cn_set_ped_preset_vel: null argument");
    DeviceScope scope(h->device);
    CN_HIPCHK(fail, hipDeviceSynchronize());
    CN_HIPCHK(fail, hipMemcpy(h->d_ped_preset, vxy, (size_t)h->cfg.n_envs * h->cfg.n_peds * 16, hipMemcpyHostToDevice));
    return CN_OK;
}

extern "C" const char* cn_kernel_name(cn_handle h, int what)
{
    if (!h || what < 0 || what > 5) { fail(CN_ERR_ARG, "cn_kernel_name: bad argument"); return nullptr; }
    return kernel_of(h, what == 4 ? CN_FORM_STEP : what, what == 4).name;      // (every world has cn_step_sequence and cn_rollout_policy; gt has no external kernel: NULL)
}

// Both counters are per-XCD (two one-thread kernels can land on different dies: their readings do not subtract), so the interval
// is taken INSIDE one wave: it reads both, idles on s_sleep until `span_ticks` of the 100 MHz counter have passed, reads both again.
__global__ void cn_clock_kernel(long long* out, long long span_ticks)
{
    const long long t0 = (long long)__builtin_amdgcn_s_memtime(), r0 = (long long)__builtin_amdgcn_s_memrealtime();
    long long r1 = r0;
    while (r1 - r0 < span_ticks) { __builtin_amdgcn_s_sleep(32); r1 = (long long)__builtin_amdgcn_s_memrealtime(); }
    out[0] = (long long)__builtin_amdgcn_s_memtime() - t0;
    out[1] = r1 - r0;
}
extern "C" int cn_device_clock(int64_t* out_dev, int span_us, int device, void* stream)
{
    if (!out_dev || span_us < 1 || span_us > 1000000) return fail(CN_ERR_ARG, "cn_device_clock: null argument or span outside 1 us .. 1 s");
    DeviceScope scope(device);
    hipLaunchKernelGGL(cn_clock_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)out_dev, (long long)span_us * 100);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

static int launch(cn_handle h, const CnKParams& kp, hipStream_t st, bool overlapped = false)
{
    DeviceScope scope(h->device);
    const bool ext = kp.mode == CN_MODE_EXT_STEP || kp.mode == CN_MODE_EXT_RESET;
    const KernelChoice kc = kernel_of(h, ext ? CN_FORM_EXTERNAL : (kp.mode == CN_MODE_STEP && kp.auto_reset == 1) ? CN_FORM_SAME : CN_FORM_STEP, overlapped);
    if (!kc.fn)
        return fail(CN_ERR_CONFIG, "cn_observe_external: risk_mode gt reads the library simulator's pedestrians; "
                                   "external /scan + /odom only exist in lidar_tracker mode");
    if (kc.x2) {
        CnKParams k2 = kp;
        k2.wave_lds = (int32_t)((lds_of(h, kc) + 15) & ~(size_t)15);
        hipLaunchKernelGGL(kc.fn, dim3(kp.N), dim3(128), (size_t)k2.wave_lds + 256, st, k2);
    } else if (kc.wpb > 1) {
        CnKParams k4 = kp;
        k4.wave_lds = (int32_t)((lds_of(h, kc) + 15) & ~(size_t)15);
        hipLaunchKernelGGL(kc.fn, dim3((kp.N + kc.wpb - 1) / kc.wpb), dim3(64 * kc.wpb), (size_t)k4.wave_lds * kc.wpb, st, k4);
    } else
    hipLaunchKernelGGL(kc.fn, dim3(kp.N), dim3(64), lds_of(h, kc), st, kp);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_reset(cn_handle h, const uint8_t* mask, float* obs, double* obs_f64, void* stream)
{
    if (!h || !obs) return fail(CN_ERR_ARG, "cn_reset: null argument");
    CnKParams kp = h->kp;
    kp.mode = CN_MODE_RESET; kp.mask = mask; kp.obs = obs; kp.obs_f64 = obs_f64;
    return launch(h, kp, (hipStream_t)stream);
}

static int step_one(cn_handle h, const cn_step_io* io, void* stream, bool overlapped)
{
    if (!h || !io || !io->action || !io->obs || !io->reward || !io->done) return fail(CN_ERR_ARG, "cn_step: null argument");
    CnKParams kp = h->kp;
    kp.mode = CN_MODE_STEP; kp.auto_reset = io->auto_reset;
    kp.action = io->action; kp.step_counter = io->step_counter; kp.obs = io->obs; kp.final_obs = io->final_obs;
    kp.obs_f64 = io->obs_f64; kp.reward = io->reward; kp.done = io->done; kp.topk_idx = io->topk_idx;
    return launch(h, kp, (hipStream_t)stream, overlapped);
}

extern "C" int cn_step(cn_handle h, const cn_step_io* io, void* stream) { return step_one(h, io, stream, false); }

extern "C" int cn_set_arbitration(cn_handle h, int mode)
{
    if (!h) return fail(CN_ERR_ARG, "cn_set_arbitration: null handle");
    if (mode != CN_ARB_AUTO && mode != CN_ARB_OLDEST_FIRST && mode != CN_ARB_FAIR)
        return fail(CN_ERR_ARG, "cn_set_arbitration: mode must be CN_ARB_AUTO (0), CN_ARB_OLDEST_FIRST (1) or CN_ARB_FAIR (2)");
    h->arbitration = mode;
    return CN_OK;
}

extern "C" int cn_set_group_envs(cn_handle h, int64_t total_envs)
{
    if (!h || total_envs < 0) return fail(CN_ERR_ARG, "cn_set_group_envs: null handle or negative count");
    h->group_envs = total_envs;
    return CN_OK;
}

extern "C" int cn_get_arbitration(cn_handle h)
{
    if (!h) return fail(CN_ERR_ARG, "cn_get_arbitration: null handle");
    const bool fair = cn_world_has_fair(h->world) && cn_fair_launch(launch_facts(h, false));
    return fair ? CN_ARB_FAIR : CN_ARB_OLDEST_FIRST;
}

extern "C" int cn_step_multi(int n, const cn_handle* handles, const cn_step_io* ios, void* const* streams)
{
    if (n < 0 || (n > 0 && (!handles || !ios || !streams))) return fail(CN_ERR_ARG, "cn_step_multi: null argument");
    bool overlapped = false;        // more than one handle in the call: their launches are meant to overlap (CN_ARB_AUTO -> oldest-first)
    for (int i = 1; i < n; ++i) overlapped = overlapped || handles[i] != handles[0];
    for (int i = 0; i < n; ++i) {
        const int rc = step_one(handles[i], &ios[i], streams[i], overlapped);
        if (rc != CN_OK) return rc;
    }
    return CN_OK;
}

// ---- cn_step_group_*: J handles' environments in ONE launch ----------------------------------------------------------------------------
// Job j rides in the grid's z dimension and reads row j of a device table where cn_step's kernel reads its kernel-argument segment
// (env_kernel_body, JOBS).  cn_step_group_create marshals the rows exactly as step_one / cn_reset + launch() do and uploads them once:
// the step table is never written again; the reset table only by cn_step_group_reset, ahead of its own launch on the same stream.
struct cn_step_group_s {
    int n = 0, device = 0, kernel = 0;      // jobs; the handles' device; index into cn_group_kernel_info
    std::vector<cn_handle> handles;
    char* d_tables = nullptr;               // [2][n] rows, CN_JOB_ROW_BYTES apart: the step table, then the reset table
    char* reset_rows = nullptr;             // the reset table as the device holds it (pinned host memory: the source of an async copy)
    hipEvent_t copied = nullptr;            // behind the last such copy: the host rows are not touched before it
    bool copy_pending = false;
    unsigned grid_x = 0, threads = 64;
    size_t lds = 0;
};

static void destroy_group(cn_step_group_s* g)
{
    if (!g) return;
    DeviceScope scope(g->device);
    (void)hipFree(g->d_tables); (void)hipHostFree(g->reset_rows);
    if (g->copied) (void)hipEventDestroy(g->copied);
    delete g;
}

extern "C" int cn_step_group_create(int n, const cn_handle* handles, const cn_step_io* ios, cn_step_group_handle* out)
{
    if (n < 1 || n > CN_STEP_GROUP_MAX)
        return fail(CN_ERR_ARG, "cn_step_group_create: " + std::to_string(n) + " jobs; a group holds 1 ... " + std::to_string(CN_STEP_GROUP_MAX));
    if (!handles || !ios || !out) return fail(CN_ERR_ARG, "cn_step_group_create: null argument");
    auto job = [](int j) { return "cn_step_group_create: job " + std::to_string(j) + ": "; };
    int64_t total = 0;
    for (int j = 0; j < n; ++j) {
        const cn_env_s* h = handles[j];
        const cn_step_io& io = ios[j];
        if (!h) return fail(CN_ERR_ARG, job(j) + "null handle");
        if (!io.action || !io.obs || !io.reward || !io.done) return fail(CN_ERR_ARG, job(j) + "null action, obs, reward or done");
        if (io.auto_reset == 1)
            return fail(CN_ERR_ARG, job(j) + "auto_reset 1 (reset inside the same call) has no group kernel; use 0 or 2");
        if (h->kp.timing || h->kp.ablate) return fail(CN_ERR_ARG, job(j) + "the handle has stage timing or an ablation mask set");
        if (h->device != handles[0]->device)
            return fail(CN_ERR_ARG, job(j) + "on device " + std::to_string(h->device) + ", job 0 on device " + std::to_string(handles[0]->device));
        for (int i = 0; i < j; ++i)
            if (handles[i] == h) return fail(CN_ERR_ARG, job(j) + "the same handle as job " + std::to_string(i));
        total += h->cfg.n_envs;
    }
    const cn_env_s* h0 = handles[0];
    const int kernel = cn_select_group_kernel(h0->world, total, h0->n_cus, h0->x2);
    for (int j = 1; j < n; ++j) {
        const cn_env_s* h = handles[j];
        const int kj = cn_select_group_kernel(h->world, total, h->n_cus, h->x2);
        if (h->world != h0->world || kj != kernel)
            return fail(CN_ERR_CONFIG, job(j) + "its group kernel is " + cn_group_kernel_info[kj].name + ", job 0's is " +
                                       cn_group_kernel_info[kernel].name + "; one launch runs one kernel");
    }
    const CnKernelInfo& ki = cn_group_kernel_info[kernel];
    const bool x2 = ki.geometry == CN_GEO_X2;
    std::unique_ptr<cn_step_group_s, void (*)(cn_step_group_s*)> guard(new cn_step_group_s(), destroy_group);
    cn_step_group_s* g = guard.get();
    g->n = n; g->device = h0->device; g->kernel = kernel; g->handles.assign(handles, handles + n);
    g->threads = x2 ? 128 : 64;
    const size_t row = CN_JOB_ROW_BYTES;
    std::vector<char> step_rows((size_t)n * row, 0);
    DeviceScope scope(g->device);
    CN_HIPCHK(fail, hipHostMalloc(&g->reset_rows, (size_t)n * row));
    CN_HIPCHK(fail, hipEventCreateWithFlags(&g->copied, hipEventDisableTiming));
    memset(g->reset_rows, 0, (size_t)n * row);
    for (int j = 0; j < n; ++j) {
        const cn_env_s* h = handles[j];
        const cn_step_io& io = ios[j];
        const size_t lds = ki.compact ? h->lds_shape : h->lds;
        CnKParams kp = h->kp;       // step_one
        kp.mode = CN_MODE_STEP; kp.auto_reset = io.auto_reset;
        kp.action = io.action; kp.step_counter = io.step_counter; kp.obs = io.obs; kp.final_obs = io.final_obs;
        kp.obs_f64 = io.obs_f64; kp.reward = io.reward; kp.done = io.done; kp.topk_idx = io.topk_idx;
        if (x2) kp.wave_lds = (int32_t)((lds + 15) & ~(size_t)15);      // launch()
        memcpy(&step_rows[(size_t)j * row], &kp, sizeof(kp));
        CnKParams kr = h->kp;       // cn_reset
        kr.mode = CN_MODE_RESET; kr.mask = nullptr; kr.obs = io.obs; kr.obs_f64 = io.obs_f64;
        if (x2) kr.wave_lds = kp.wave_lds;
        memcpy(g->reset_rows + (size_t)j * row, &kr, sizeof(kr));
        const size_t need = x2 ? (size_t)kp.wave_lds + 256 : lds;
        if (need > g->lds) g->lds = need;
        if ((unsigned)h->cfg.n_envs > g->grid_x) g->grid_x = (unsigned)h->cfg.n_envs;
    }
    CN_HIPCHK(fail, hipMalloc(&g->d_tables, 2 * (size_t)n * row));      // (hipMalloc: 256-byte aligned)
    CN_HIPCHK(fail, hipMemcpy(g->d_tables, step_rows.data(), step_rows.size(), hipMemcpyHostToDevice));
    CN_HIPCHK(fail, hipMemcpy(g->d_tables + (size_t)n * row, g->reset_rows, (size_t)n * row, hipMemcpyHostToDevice));
    if (g->lds > 64 * 1024)
        CN_HIPCHK(fail, hipFuncSetAttribute((const void*)kGroupFn[kernel], hipFuncAttributeMaxDynamicSharedMemorySize, (int)g->lds));
    *out = guard.release();
    return CN_OK;
}

static int group_launch(cn_step_group_s* g, const char* table, void* stream)
{
    hipLaunchKernelGGL(kGroupFn[g->kernel], dim3(g->grid_x, 1, (unsigned)g->n), dim3(g->threads), g->lds, (hipStream_t)stream, (const CnKParams*)table);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_step_group_step(cn_step_group_handle g, void* stream)
{
    if (!g) return fail(CN_ERR_ARG, "cn_step_group_step: null group");
    DeviceScope scope(g->device);
    return group_launch(g, g->d_tables, stream);
}

extern "C" int cn_step_group_reset(cn_step_group_handle g, const uint8_t* const* masks, void* stream)
{
    if (!g) return fail(CN_ERR_ARG, "cn_step_group_reset: null group");
    DeviceScope scope(g->device);
    const size_t row = CN_JOB_ROW_BYTES, bytes = (size_t)g->n * row;
    auto mask_at = [&](int j) { return g->reset_rows + (size_t)j * row + offsetof(CnKParams, mask); };
    bool changed = false;
    for (int j = 0; j < g->n && !changed; ++j) {
        const uint8_t* had;
        memcpy(&had, mask_at(j), sizeof(had));
        changed = had != (masks ? masks[j] : nullptr);
    }
    if (changed) {
        // the masks' addresses go into the rows ahead of the launch, on its stream: behind every earlier launch of the group there
        if (g->copy_pending) CN_HIPCHK(fail, hipEventSynchronize(g->copied));
        for (int j = 0; j < g->n; ++j) { const uint8_t* m = masks ? masks[j] : nullptr; memcpy(mask_at(j), &m, sizeof(m)); }
        CN_HIPCHK(fail, hipMemcpyAsync(g->d_tables + bytes, g->reset_rows, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
        CN_HIPCHK(fail, hipEventRecord(g->copied, (hipStream_t)stream));
        g->copy_pending = true;
    }
    return group_launch(g, g->d_tables + bytes, stream);
}

extern "C" int cn_step_group_jobs(cn_step_group_handle g) { return g ? g->n : fail(CN_ERR_ARG, "cn_step_group_jobs: null group"); }

extern "C" const char* cn_step_group_kernel_name(cn_step_group_handle g)
{
    if (!g) { fail(CN_ERR_ARG, "cn_step_group_kernel_name: null group"); return nullptr; }
    return cn_group_kernel_info[g->kernel].name;
}

extern "C" void cn_step_group_destroy(cn_step_group_handle g) { destroy_group(g); }

extern "C" int cn_observe_external(cn_handle h, const cn_external_io* io, void* stream)
{
    if (!h || !io || !io->ranges || !io->odom || !io->obs || !io->reward || !io->done)
        return fail(CN_ERR_ARG, "cn_observe_external: null argument");
    CnKParams kp = h->kp;
    if (io->phase < 0 || io->phase > 7 || (io->phase && io->is_reset))
        return fail(CN_ERR_ARG, "cn_observe_external: phase is a mask of CN_PHASE_* and only applies to the step flow");
    if ((io->phase & CN_PHASE_REWARD) && !(io->phase & CN_PHASE_GET_STATE) && !io->obs_f64)
        return fail(CN_ERR_ARG, "cn_observe_external: CN_PHASE_REWARD alone reads the float64 state (obs_f64)");
    kp.mode = io->is_reset ? CN_MODE_EXT_RESET : CN_MODE_EXT_STEP;
    kp.ext_phase = io->phase;
    kp.ext_ranges = io->ranges; kp.ext_odom = io->odom; kp.step_counter = io->step_counter;
    kp.obs = io->obs; kp.obs_f64 = io->obs_f64; kp.reward = io->reward; kp.done = io->done; kp.topk_idx = io->topk_idx;
    return launch(h, kp, (hipStream_t)stream);
}

// cn_step_sequence / cn_rollout_policy: the handle's argument block for n_steps next-step-reset periods into the caller's slots
template <typename IO>      // cn_sequence_io, cn_policy_io: the same member names
static CnKParams roll_params(cn_handle h, const IO* io)
{
    CnKParams kp = h->kp;
    kp.mode = CN_MODE_STEP; kp.auto_reset = 2;
    kp.action = io->action; kp.step_counter = nullptr; kp.final_obs = nullptr; kp.obs_f64 = nullptr;
    kp.obs = io->obs; kp.reward = io->reward; kp.done = io->done; kp.topk_idx = io->topk_idx;
    kp.roll_steps = io->n_steps; kp.roll_action_in_stride = io->action_stride; kp.roll_obs_stride = io->obs_stride;
    kp.roll_reward_stride = io->reward_stride; kp.roll_done_stride = io->done_stride; kp.roll_topk_stride = io->topk_stride;
    return kp;
}
template <typename IO>
static bool roll_null(const IO* io) { return !io || !io->action || !io->obs || !io->reward || !io->done; }
template <typename IO>
static bool roll_negative(const IO* io)
{
    return io->n_steps < 0 || io->action_stride < 0 || io->obs_stride < 0 || io->reward_stride < 0 || io->done_stride < 0 || io->topk_stride < 0;
}

extern "C" int cn_step_sequence(cn_handle h, const cn_sequence_io* io, void* stream)
{
    if (!h || roll_null(io)) return fail(CN_ERR_ARG, "cn_step_sequence: null argument");
    if (roll_negative(io)) return fail(CN_ERR_ARG, "cn_step_sequence: negative step count or stride");
    if (io->n_steps == 0) return CN_OK;
    CnKParams kp = roll_params(h, io);
    DeviceScope scope(h->device);
    const KernelChoice kc = kernel_of(h, CN_FORM_SEQUENCE);
    hipLaunchKernelGGL(kc.fn, dim3(h->cfg.n_envs), dim3(64), lds_of(h, kc), (hipStream_t)stream, kp);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_rollout_policy(cn_handle h, const cn_actor_weights* w, const cn_policy_io* io, void* stream)
{
    if (!h || !w || roll_null(io) || !io->obs0 || !w->w1p || !w->b1 || !w->w2p || !w->b2 || !w->w3 || !w->b3)
        return fail(CN_ERR_ARG, "cn_rollout_policy: null argument");
    if (!h->pol_lds)
        return fail(CN_ERR_CONFIG, "cn_rollout_policy: not even 8 environments of this shape fit one CU's LDS (160 KiB)");
    const int D = h->D;      // 366 + 4 K, or 363 / 370 at 360 rays for the two older layouts
    if (w->hidden != 256 || w->obs_dim != D || w->obs_dim_padded != ((D + 31) & ~31))
        return fail(CN_ERR_CONFIG, "cn_rollout_policy: the actor must be cn_actor_pack_weights' layout for this handle's observation width (hidden 256, obs_dim_padded = obs_dim rounded up to 32)");
    if (roll_negative(io)) return fail(CN_ERR_ARG, "cn_rollout_policy: negative step count or stride");
    if (io->n_steps == 0) return CN_OK;
    CnKParams kp = roll_params(h, io);
    kp.pol_w1p = w->w1p; kp.pol_b1 = w->b1; kp.pol_w2p = w->w2p; kp.pol_b2 = w->b2; kp.pol_w3 = w->w3; kp.pol_b3 = w->b3;
    kp.pol_obs0 = io->obs0; kp.pol_seed = io->seed; kp.pol_counter = io->counter;
    kp.pol_max_v = io->max_v; kp.pol_max_w = io->max_w; kp.pol_sigma = io->sigma;
    kp.pol_D = D; kp.pol_Dp = w->obs_dim_padded; kp.pol_wave_lds = (int32_t)h->pol_wave_lds;
    kp.pol_envs = h->pol_envs; kp.pol_act_off = (int32_t)h->pol_act_off;
    DeviceScope scope(h->device);
    cn_kernel_fn fn = kernel_of(h, CN_FORM_POLICY).fn;
    hipLaunchKernelGGL(fn, dim3((h->cfg.n_envs + h->pol_envs - 1) / h->pol_envs), dim3(64 * h->pol_envs), h->pol_lds, (hipStream_t)stream, kp);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_get_counters(cn_handle h, int32_t* out, void* stream)
{
    if (!h || !out) return fail(CN_ERR_ARG, "cn_get_counters: null argument");
    int N = h->cfg.n_envs;
    DeviceScope scope(h->device);
    hipLaunchKernelGGL(cn_gather_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->kp,
                       (float*)nullptr, (float*)nullptr, out);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_get_returns(cn_handle h, float* last_return, float* running_return, void* stream)
{
    if (!h) return fail(CN_ERR_ARG, "cn_get_returns: null handle");
    int N = h->cfg.n_envs;
    DeviceScope scope(h->device);
    hipLaunchKernelGGL(cn_gather_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->kp, last_return,
                       running_return, (int32_t*)nullptr);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_debug_env(cn_handle h, int env, double* scalars, double* robot_ped, double* tracks, int32_t* ints)
{
    if (!h || env < 0 || env >= h->cfg.n_envs) return fail(CN_ERR_ARG, "cn_debug_env: bad argument");
    DeviceScope scope(h->device);
    CN_HIPCHK(fail, hipDeviceSynchronize());
    const int P = h->cfg.n_peds;
    std::vector<double> sd(CN_SD_COUNT);
    const char* rec = h->d_state + (size_t)env * h->stride;
    CN_HIPCHK(fail, hipMemcpy(sd.data(), rec + CN_ST_OFF_SD, CN_SD_COUNT * 8, hipMemcpyDeviceToHost));
    if (scalars) memcpy(scalars, sd.data(), CN_SD_COUNT * 8);
    if (robot_ped) {
        memcpy(robot_ped, sd.data(), 5 * 8);
        if (P > 0) {
            CN_HIPCHK(fail, hipMemcpy(robot_ped + 5, rec + CN_ST_OFF_PED_P, (size_t)P * 32, hipMemcpyDeviceToHost));   // ped_p | ped_v
        }
    }
    if (tracks)
        CN_HIPCHK(fail, hipMemcpy(tracks, h->d_trk + (size_t)env * CN_TF_COUNT * h->trk_cap, CN_TF_COUNT * h->trk_cap * 8,
                         hipMemcpyDeviceToHost));
    if (ints) CN_HIPCHK(fail, hipMemcpy(ints, rec + CN_ST_OFF_SI, CN_SI_COUNT * 4, hipMemcpyDeviceToHost));
    return CN_OK;
}

// snapshot layout (include/crowdnav.h): cn_snapshot_header | sd | si | ped_p | ped_v | trk | ped_init | ped_preset | ped_aux
// One section: N rows of `width` bytes, `pitch` bytes apart on the device (a field of the env records) or dense (pitch 0: an array of
// its own; of a wide handle's d_trk the N tables, not the scratch column behind them).  Width 0 (no pedestrians): nothing to copy.
struct SnapSection { void* dev; size_t pitch, width; std::vector<double>* host_copy; };
static std::vector<SnapSection> snapshot_sections(cn_handle h)
{
    const size_t P = h->cfg.n_peds, S = h->stride;
    char* st = h->d_state;
    return {{st + CN_ST_OFF_SD, S, CN_SD_COUNT * 8, nullptr},     {st + CN_ST_OFF_SI, S, CN_SI_COUNT * 4, nullptr},
            {st + CN_ST_OFF_PED_P, S, P * 16, nullptr},           {st + CN_ST_OFF_PED_V(P), S, P * 16, nullptr},
            {h->d_trk, 0, (size_t)CN_TF_COUNT * h->trk_cap * 8, nullptr},
            {h->d_ped_init, 0, P * 16, &h->ped_init},             // (cn_reset re-uploads the host copy: a restore refreshes it)
            {h->d_ped_preset, 0, P * 16, nullptr},                {h->d_ped_aux, 0, P * 24, nullptr}};
}
// every section to (restore = false) or from (true) the payload at `q`
static int snapshot_copy(cn_handle h, char* q, bool restore)
{
    const size_t N = h->cfg.n_envs;
    for (const SnapSection& s : snapshot_sections(h)) {
        if (!s.width) continue;
        if (restore && s.host_copy) s.host_copy->assign((const double*)q, (const double*)(q + N * s.width));
        const hipMemcpyKind kind = restore ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
        void* dst = restore ? s.dev : (void*)q;
        const void* src = restore ? (const void*)q : s.dev;
        if (s.pitch) CN_HIPCHK(fail, hipMemcpy2D(dst, restore ? s.pitch : s.width, src, restore ? s.width : s.pitch, s.width, N, kind));
        else CN_HIPCHK(fail, hipMemcpy(dst, src, N * s.width, kind));
        q += N * s.width;
    }
    return CN_OK;
}
static size_t snapshot_payload(cn_handle h)
{
    size_t row = 0;
    for (const SnapSection& s : snapshot_sections(h)) row += s.width;
    return row * h->cfg.n_envs;
}
extern "C" size_t cn_snapshot_size(cn_handle h)
{
    if (!h) return 0;
    return sizeof(cn_snapshot_header) + snapshot_payload(h);
}

static void fill_header(cn_handle h, cn_snapshot_header* hd)
{
    memset(hd, 0, sizeof(*hd));
    hd->magic = CN_SNAPSHOT_MAGIC; hd->abi_version = CN_ABI_VERSION; hd->header_bytes = (int32_t)sizeof(cn_snapshot_header);
    hd->sd_count = CN_SD_COUNT; hd->si_count = CN_SI_COUNT; hd->tf_count = CN_TF_COUNT; hd->track_capacity = h->trk_cap;
    hd->total_bytes = sizeof(cn_snapshot_header) + snapshot_payload(h);
    hd->config = h->cfg;
}

extern "C" int cn_snapshot(cn_handle h, void* buf, size_t size)
{
    if (!h || !buf) return fail(CN_ERR_ARG, "cn_snapshot: null argument");
    if (size < cn_snapshot_size(h)) return fail(CN_ERR_SIZE, "cn_snapshot: buffer too small");
    DeviceScope scope(h->device);
    CN_HIPCHK(fail, hipDeviceSynchronize());
    cn_snapshot_header hd;
    fill_header(h, &hd);
    memcpy(buf, &hd, sizeof(hd));
    return snapshot_copy(h, (char*)buf + sizeof(hd), false);
}

// first field of the two configurations that differs (nullptr: identical)
static const char* config_mismatch(const cn_config& a, const cn_config& b)
{
#define CN_CMP(f) if (memcmp(&a.f, &b.f, sizeof(a.f)) != 0) return #f;
    CN_CMP(n_envs) CN_CMP(n_peds) CN_CMP(n_rays) CN_CMP(k_obstacles) CN_CMP(max_steps) CN_CMP(ped_mode) CN_CMP(dt_ms)
    CN_CMP(scan_latency_ms) CN_CMP(settle_ms) CN_CMP(ped_cycle_ms) CN_CMP(ped_stagger_ms) CN_CMP(track_capacity) CN_CMP(obs_layout)
    CN_CMP(geos_untyped_empty) CN_CMP(ped_contact) CN_CMP(risk_mode) CN_CMP(py2_round) CN_CMP(sf_tick_ms) CN_CMP(scan_f32) CN_CMP(waypoint_reward)
    CN_CMP(env_index_base) CN_CMP(seed)
    CN_CMP(room_half) CN_CMP(ped_radius) CN_CMP(ped_vmax) CN_CMP(robot_clearance) CN_CMP(lidar_min) CN_CMP(lidar_max) CN_CMP(lidar_span)
    CN_CMP(lidar_offset_x) CN_CMP(max_scan_range) CN_CMP(min_scan_range) CN_CMP(goal_x) CN_CMP(goal_y) CN_CMP(start_x) CN_CMP(start_y)
    CN_CMP(spawn_x) CN_CMP(spawn_y) CN_CMP(spawn_yaw) CN_CMP(waypoint_radius) CN_CMP(goal_eps)
    CN_CMP(sf_tau) CN_CMP(sf_A) CN_CMP(sf_B) CN_CMP(sf_wall_A) CN_CMP(sf_wall_B) CN_CMP(sf_goal_eps) CN_CMP(wheel_accel) CN_CMP(wheel_separation)
#undef CN_CMP
    return nullptr;
}

extern "C" int cn_restore(cn_handle h, const void* buf, size_t size)
{
    if (!h || !buf) return fail(CN_ERR_ARG, "cn_restore: null argument");
    if (size < sizeof(cn_snapshot_header)) return fail(CN_ERR_SIZE, "cn_restore: buffer smaller than a snapshot header");
    cn_snapshot_header hd;
    memcpy(&hd, buf, sizeof(hd));
    if (hd.magic != CN_SNAPSHOT_MAGIC) return fail(CN_ERR_ARG, "cn_restore: not a libcrowdnav snapshot (bad magic)");
    if (hd.abi_version != CN_ABI_VERSION || hd.header_bytes != (int32_t)sizeof(cn_snapshot_header))
        return fail(CN_ERR_CONFIG, "cn_restore: snapshot written by ABI version " + std::to_string(hd.abi_version) +
                                   ", this library is ABI " + std::to_string(CN_ABI_VERSION));
    if (hd.sd_count != CN_SD_COUNT || hd.si_count != CN_SI_COUNT || hd.tf_count != CN_TF_COUNT || hd.track_capacity != h->trk_cap)
        return fail(CN_ERR_CONFIG, "cn_restore: snapshot record layout (sd / si / track fields, tracker slots) differs from this handle's");
    if (const char* f = config_mismatch(hd.config, h->cfg))
        return fail(CN_ERR_CONFIG, std::string("cn_restore: the snapshot was taken under another configuration: cn_config.") + f +
                                   " differs (a state only means something under the configuration that produced it)");
    if (hd.total_bytes != cn_snapshot_size(h) || size < hd.total_bytes) return fail(CN_ERR_SIZE, "cn_restore: truncated snapshot");
    // the payload's records, before anything is synchronised or copied: a refused blob leaves the handle as it was
    {
        const size_t N = h->cfg.n_envs, P = h->cfg.n_peds;
        const char* q = (const char*)buf + sizeof(hd);
        CnRecordSections sec;
        sec.sd = (const double*)q; q += N * CN_SD_COUNT * 8;
        sec.si = (const int32_t*)q; q += N * CN_SI_COUNT * 4;
        sec.ped_p = (const double*)q; q += N * P * 16;
        sec.ped_v = (const double*)q; q += N * P * 16;
        sec.trk = (const double*)q;
        const CnRecordVerdict v = cn_check_records(h->cfg, h->trk_cap, h->max_conf, (int)N, sec);
        if (!v.ok) {
            char text[160];
            cn_record_verdict_text(v, text, sizeof(text));
            return fail(CN_ERR_CONFIG, std::string("cn_restore: the snapshot holds a record no run produces: ") + text +
                                       " (csrc/crowdnav_snapshot_check.h states the ranges); nothing was restored");
        }
    }
    DeviceScope scope(h->device);
    CN_HIPCHK(fail, hipDeviceSynchronize());
    return snapshot_copy(h, (char*)buf + sizeof(hd), true);      // (only read from)
}
