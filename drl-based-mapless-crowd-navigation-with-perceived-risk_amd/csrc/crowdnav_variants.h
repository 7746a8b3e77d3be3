// crowdnav_variants.h -- the one table of the kernels that take CnKParams: which world (class of configurations cn_create accepts)
// gets which kernel for which call.  crowdnav_kernel.hip expands it to the kernels' definitions and their compile units,
// crowdnav_abi.hip to their declarations, the function table and the dynamic-LDS attribute lists, and cn_select_kernel() below is
// the selection every launch and cn_kernel_name go through.  Plain C++: no HIP, no device (tests/test_kernel_table.py compiles it
// with g++ and walks the selection on the CPU).
//
// To add a world: add ONE row to CN_WORLDS (its position is its index, and the rows' order is the kernels' definition order inside
// each compile unit) and give cn_world_index() the fact that leads to it.  Definitions, compile units, declarations, attribute lists
// and selection follow from the row; tests/test_kernel_table.py wants the new names in its own statement of the table.
//
// A row:  X(ID,  LAYOUT, GT, SIM, WIDE, SHAPE,  BOUNDS, COMPACT,  STEP,  SAME_HAS, SAME,  EXT_HAS, EXT,  SEQ, SEQ_TU,  POL, POL_TU, POL_BOUND)
//   ID                   CN_W_<ID> is the world's index
//   LAYOUT ... SHAPE     the template facts of env_kernel_body / sequence_body / policy_sequence_body (SIM: 1 contact ticks, 2 social
//                        force with the pair matrix, 3 wheel ramp, 4 dense social force; SHAPE: 0 generic, 360, 720)
//   BOUNDS               launch bounds of the step and sequence kernels (the same-call reset and external kernels: one plain wave)
//   COMPACT              step / sequence / policy kernels use the compact LDS layout (launched with the handle's lds_shape)
//   STEP, SEQ, POL       kernel names; SEQ_TU / POL_TU: the compile unit (csrc/build.sh, CN_TU) of that kernel -- every one-step
//                        kernel is in unit 1; POL_BOUND: the policy kernel's workgroup bound
//   SAME_HAS, EXT_HAS    OWN: the row defines the kernel named next; USE: it launches another row's; NONE: the world has no such
//                        form (external /scan + /odom in gt mode) -- the name is then a placeholder
#pragma once
#include <stdint.h>
#include "../../include/crowdnav.h"

#define CN_WORLDS(X) \
    X(PLAIN,  0, false, 0, false, 0,   CN_HOT_BOUNDS,         false, cn_env_kernel,        OWN, cn_env_kernel_same,        OWN,  cn_env_kernel_ext,      cn_env_kernel_seq,        2, cn_policy_kernel,        2, 64 * POL_ENVS) \
    X(S360,   0, false, 0, false, 360, CN_HOT_BOUNDS,         false, cn_env_kernel_s360,   USE, cn_env_kernel_same,        USE,  cn_env_kernel_ext,      cn_env_kernel_seq_s360,   2, cn_policy_kernel_s360,   2, 64 * POL_ENVS) \
    X(S720,   0, false, 0, false, 720, CN_S720_BOUNDS,        true,  cn_env_kernel_s720,   USE, cn_env_kernel_same,        USE,  cn_env_kernel_ext,      cn_env_kernel_seq_s720,   2, cn_policy_kernel_s720,   4, 64 * POL_ENVS) \
    X(GT,     0, true,  0, false, 0,   __launch_bounds__(64), false, cn_env_kernel_gt,     OWN, cn_env_kernel_gt_same,     NONE, none,                   cn_env_kernel_gt_seq,     2, cn_policy_kernel_gt,     2, 64 * POL_ENVS) \
    X(WIDE,   0, false, 0, true,  0,   __launch_bounds__(64), false, cn_env_kernel_wide,   OWN, cn_env_kernel_wide_same,   OWN,  cn_env_kernel_wide_ext, cn_env_kernel_seq_wide,   2, cn_policy_kernel_wide,   2, 64 * POL_ENVS) \
    X(SF,     0, false, 2, false, 0,   __launch_bounds__(64), false, cn_env_kernel_sf,     OWN, cn_env_kernel_sf_same,     USE,  cn_env_kernel_ext,      cn_env_kernel_seq_sf,     3, cn_policy_kernel_sf,     4, 64 * POL_ENVS) \
    X(SFD,    0, false, 4, false, 0,   __launch_bounds__(64), false, cn_env_kernel_sfd,    OWN, cn_env_kernel_sfd_same,    USE,  cn_env_kernel_ext,      cn_env_kernel_seq_sfd,    3, cn_policy_kernel_sfd,    4, 64 * POL_ENVS) \
    X(WA,     0, false, 3, false, 0,   __launch_bounds__(64), false, cn_env_kernel_wa,     OWN, cn_env_kernel_wa_same,     USE,  cn_env_kernel_ext,      cn_env_kernel_seq_wa,     3, cn_policy_kernel_wa,     4, 64 * POL_ENVS) \
    X(GT_SF,  0, true,  2, false, 0,   __launch_bounds__(64), false, cn_env_kernel_gt_sf,  OWN, cn_env_kernel_gt_sf_same,  NONE, none,                   cn_env_kernel_gt_seq_sf,  3, cn_policy_kernel_gt_sf,  4, 64 * POL_ENVS) \
    X(GT_SFD, 0, true,  4, false, 0,   __launch_bounds__(64), false, cn_env_kernel_gt_sfd, OWN, cn_env_kernel_gt_sfd_same, NONE, none,                   cn_env_kernel_gt_seq_sfd, 3, cn_policy_kernel_gt_sfd, 4, 64 * POL_ENVS) \
    X(GT_WA,  0, true,  3, false, 0,   __launch_bounds__(64), false, cn_env_kernel_gt_wa,  OWN, cn_env_kernel_gt_wa_same,  NONE, none,                   cn_env_kernel_gt_seq_wa,  3, cn_policy_kernel_gt_wa,  4, 64 * POL_ENVS) \
    X(CT,     0, false, 1, false, 0,   __launch_bounds__(64), false, cn_env_kernel_ct,     OWN, cn_env_kernel_ct_same,     USE,  cn_env_kernel_ext,      cn_env_kernel_seq_ct,     5, cn_policy_kernel_ct,     5, 64 * POL_ENVS) \
    X(GT_CT,  0, true,  1, false, 0,   __launch_bounds__(64), false, cn_env_kernel_gt_ct,  OWN, cn_env_kernel_gt_ct_same,  NONE, none,                   cn_env_kernel_gt_seq_ct,  5, cn_policy_kernel_gt_ct,  5, 64 * POL_ENVS) \
    X(ORIG,   1, false, 0, false, 0,   __launch_bounds__(64), false, cn_env_kernel_orig,   OWN, cn_env_kernel_orig_same,   OWN,  cn_env_kernel_orig_ext, cn_env_kernel_seq_orig,   5, cn_policy_kernel_orig,   5, 64 * POL_ENVS) \
    X(RW,     2, false, 0, false, 0,   __launch_bounds__(64), false, cn_env_kernel_rw,     OWN, cn_env_kernel_rw_same,     OWN,  cn_env_kernel_rw_ext,   cn_env_kernel_seq_rw,     5, cn_policy_kernel_rw,     5, 64 * 8)

// The step kernels only the three plain tracker worlds (PLAIN, S360, S720) have: the fair-arbitration forms and the headline shape's
// launch geometries.  Their wrappers are written out in crowdnav_kernel.hip (unit 1); listed here once for everything else.
//   X(NAME, COMPACT, GEOMETRY)     GEOMETRY: ONE wave per workgroup, W4 = several environments per workgroup, X2 = two waves per environment
#define CN_HEADLINE_KERNELS(X) \
    X(cn_env_kernel_fair,         false, ONE) \
    X(cn_env_kernel_fair_s360,    false, ONE) \
    X(cn_env_kernel_s360_w4,      false, W4) \
    X(cn_env_kernel_fair_s360_w4, false, W4) \
    X(cn_env_kernel_s360_x2,      false, X2) \
    X(cn_env_kernel_fair_s720,    true,  ONE)

// ---- the flat kernel lists: CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) once per kernel; the user defines CN_KERNEL around each use ------
#define CN_HAS_OWN(...) __VA_ARGS__
#define CN_HAS_USE(...)
#define CN_HAS_NONE(...)
#define CN_ROW_STEP_SEQ_(ID, LAYOUT, GT, SIM, WIDE, SHAPE, BOUNDS, COMPACT, STEP, SAME_HAS, SAME, EXT_HAS, EXT, SEQ, SEQ_TU, POL, POL_TU, POL_BOUND) \
    CN_KERNEL(STEP, 1, COMPACT, ONE) CN_HAS_##SAME_HAS(CN_KERNEL(SAME, 1, false, ONE)) CN_HAS_##EXT_HAS(CN_KERNEL(EXT, 1, false, ONE)) CN_KERNEL(SEQ, SEQ_TU, COMPACT, ONE)
#define CN_ROW_POLICY_(ID, LAYOUT, GT, SIM, WIDE, SHAPE, BOUNDS, COMPACT, STEP, SAME_HAS, SAME, EXT_HAS, EXT, SEQ, SEQ_TU, POL, POL_TU, POL_BOUND) \
    CN_KERNEL(POL, POL_TU, COMPACT, ONE)
#define CN_HEADLINE_(NAME, COMPACT, GEOMETRY) CN_KERNEL(NAME, 1, COMPACT, GEOMETRY)
// every kernel launched with cn_create's dynamic LDS size (step, same-call reset, external, sequence), and the policy kernels
#define CN_DYNAMIC_LDS_KERNELS CN_WORLDS(CN_ROW_STEP_SEQ_) CN_HEADLINE_KERNELS(CN_HEADLINE_)
#define CN_POLICY_KERNELS CN_WORLDS(CN_ROW_POLICY_)

enum { CN_GEO_ONE = 0, CN_GEO_W4 = 1, CN_GEO_X2 = 2 };
#define CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) CN_K_##NAME,
enum {      // a kernel's index: [0, CN_K_N_DYNAMIC) the dynamic-LDS kernels, [CN_K_N_DYNAMIC, CN_K_COUNT) the policy kernels
    CN_DYNAMIC_LDS_KERNELS
    CN_K_N_DYNAMIC, CN_K_BEFORE_POLICY_ = CN_K_N_DYNAMIC - 1,
    CN_POLICY_KERNELS
    CN_K_COUNT, CN_K_none = -1
};
#undef CN_KERNEL
static_assert(CN_K_N_DYNAMIC == 53 && CN_K_COUNT - CN_K_N_DYNAMIC == 15, "53 step / sequence kernels and 15 policy kernels");

struct CnKernelInfo { const char* name; int tu; bool compact; int geometry; };
#define CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) {#NAME, TU, COMPACT, CN_GEO_##GEOMETRY},
static constexpr CnKernelInfo cn_kernel_info[CN_K_COUNT] = { CN_DYNAMIC_LDS_KERNELS CN_POLICY_KERNELS };
#undef CN_KERNEL

// ---- worlds ------------------------------------------------------------------------------------------------------------------------
#define CN_ROW_ID_(ID, ...) CN_W_##ID,
enum { CN_WORLDS(CN_ROW_ID_) CN_W_COUNT };
struct CnWorld { int step, same, ext, seq, pol; };      // kernel indices; ext: CN_K_none in gt mode
#define CN_ROW_WORLD_(ID, LAYOUT, GT, SIM, WIDE, SHAPE, BOUNDS, COMPACT, STEP, SAME_HAS, SAME, EXT_HAS, EXT, SEQ, SEQ_TU, POL, POL_TU, POL_BOUND) \
    {CN_K_##STEP, CN_K_##SAME, CN_K_##EXT, CN_K_##SEQ, CN_K_##POL},
static constexpr CnWorld cn_worlds[CN_W_COUNT] = { CN_WORLDS(CN_ROW_WORLD_) };

// The world of a configuration cn_create accepted (its refusals make these facts exclusive where the order does not): the older
// observation layouts, the wide tracker table, the wheel ramp, dense social force (sf without the pair matrix, up to 128
// pedestrians), social force, contact ticks -- each of the last four in both risk modes -- plain gt, and the plain tracker world by shape.
static inline int cn_world_index(int obs_layout, bool wide, bool gt, bool wa, bool sfd, bool sf, bool ct, bool shape360, bool shape720)
{
    if (obs_layout == CN_LAYOUT_REALWORLD) return CN_W_RW;
    if (obs_layout == CN_LAYOUT_ORIGINAL) return CN_W_ORIG;
    if (wide) return CN_W_WIDE;
    if (wa) return gt ? CN_W_GT_WA : CN_W_WA;
    if (sfd) return gt ? CN_W_GT_SFD : CN_W_SFD;
    if (sf) return gt ? CN_W_GT_SF : CN_W_SF;
    if (ct) return gt ? CN_W_GT_CT : CN_W_CT;
    if (gt) return CN_W_GT;
    return shape360 ? CN_W_S360 : shape720 ? CN_W_S720 : CN_W_PLAIN;
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------
// cn_kernel_name's `what`, less 4 (a cn_step_multi launch: CN_FORM_STEP with CnLaunchFacts::overlapped)
enum { CN_FORM_STEP = 0, CN_FORM_SAME = 1, CN_FORM_SEQUENCE = 2, CN_FORM_EXTERNAL = 3, CN_FORM_POLICY = 5 };
struct CnLaunchFacts {
    int arbitration;            // CN_ARB_*
    bool overlapped;            // one of several handles' launches in a cn_step_multi
    int n_cus;                  // compute units of the device (0: unknown)
    int64_t n_envs, group_envs; // this handle's environments; cn_set_group_envs (0 = alone)
    int x2;                     // CN_X2: -1 unset (by grid size), 0 / 1
    int wpb;                    // environments per workgroup of the _w4 kernels (CN_WPB); 0 = one
};
static inline bool cn_world_has_fair(int world) { return world == CN_W_PLAIN || world == CN_W_S360 || world == CN_W_S720; }
// Does a cn_step launch use fair arbitration (where the world has a fair kernel)?  CN_ARB_AUTO: from two wavefronts per SIMD.
static inline bool cn_fair_launch(const CnLaunchFacts& f)
{
    if (f.arbitration == CN_ARB_FAIR) return true;
    if (f.arbitration == CN_ARB_OLDEST_FIRST || f.overlapped) return false;
    return f.n_cus > 0 && f.n_envs >= 8 * (int64_t)f.n_cus;
}
// The kernel (index into cn_kernel_info) a call of `form` on a handle of `world` launches; CN_K_none: the world has no such form.
static inline int cn_select_kernel(int world, int form, const CnLaunchFacts& f)
{
    const CnWorld& w = cn_worlds[world];
    switch (form) {
    case CN_FORM_SAME: return w.same;
    case CN_FORM_EXTERNAL: return w.ext;
    case CN_FORM_SEQUENCE: return w.seq;
    case CN_FORM_POLICY: return w.pol;
    }
    if (!cn_world_has_fair(world)) return w.step;
    const bool fair = cn_fair_launch(f);
    if (world == CN_W_S360 && f.n_cus > 0) {
        const int64_t resident = f.group_envs > f.n_envs ? f.group_envs : f.n_envs;
        // small grids: two wavefronts per environment while all of them fit at two per SIMD
        if (f.x2 == 1 || (f.x2 < 0 && resident <= 8 * (int64_t)f.n_cus)) return CN_K_cn_env_kernel_s360_x2;
        // the whole launch resident at once: several environments per workgroup
        if (f.wpb && resident <= 16 * (int64_t)f.n_cus) return fair ? CN_K_cn_env_kernel_fair_s360_w4 : CN_K_cn_env_kernel_s360_w4;
    }
    if (!fair) return w.step;
    return world == CN_W_S360 ? CN_K_cn_env_kernel_fair_s360 : world == CN_W_S720 ? CN_K_cn_env_kernel_fair_s720 : CN_K_cn_env_kernel_fair;
}

// ---- the group kernels: J handles' environments in ONE launch (cn_step_group_*) -----------------------------------------------------
// A list of its own, beside the 53 + 15 above: every world's STEP kernel as <STEP>_grp(const CnKParams* jobs) -- job blockIdx.z reads
// row z of a device table where the kernels above read their kernel-argument segment -- with the row's BOUNDS, and the headline
// shape's two-wavefront geometry.  csrc/crowdnav_step_group.hip compiles them (the group-only section of crowdnav_kernel.hip); TU 0
// below says "none of that file's units 1-5".  A world's group kernel has the world's index; the _x2_grp kernel follows the rows.
#define CN_ROW_GROUP_(ID, LAYOUT, GT, SIM, WIDE, SHAPE, BOUNDS, COMPACT, STEP, SAME_HAS, SAME, EXT_HAS, EXT, SEQ, SEQ_TU, POL, POL_TU, POL_BOUND) \
    CN_KERNEL(STEP##_grp, 0, COMPACT, ONE)
#define CN_GROUP_KERNELS CN_WORLDS(CN_ROW_GROUP_) CN_KERNEL(cn_env_kernel_s360_x2_grp, 0, false, X2)
#define CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) CN_G_##NAME,
enum { CN_GROUP_KERNELS CN_G_COUNT };
#undef CN_KERNEL
static_assert(CN_G_COUNT == CN_W_COUNT + 1 && CN_G_COUNT == 16, "one group kernel per world and the headline shape's x2 form");
#define CN_KERNEL(NAME, TU, COMPACT, GEOMETRY) {#NAME, TU, COMPACT, CN_GEO_##GEOMETRY},
static constexpr CnKernelInfo cn_group_kernel_info[CN_G_COUNT] = { CN_GROUP_KERNELS };
#undef CN_KERNEL
// The kernel (index into cn_group_kernel_info) a group of handles of `world` launches.  total_envs: the environments of all its jobs --
// cn_select_kernel's x2 rule with resident = their sum; x2: the handles' CN_X2 (-1 unset, 0 / 1).
static inline int cn_select_group_kernel(int world, int64_t total_envs, int n_cus, int x2)
{
    if (world == CN_W_S360 && (x2 == 1 || (x2 < 0 && total_envs <= 8 * (int64_t)n_cus))) return CN_G_cn_env_kernel_s360_x2_grp;
    return world;
}
