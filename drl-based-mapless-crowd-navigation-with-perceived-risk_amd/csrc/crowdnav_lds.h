// crowdnav_lds.h -- the LDS map of an environment's working set.  Every size is written once, as a macro
// below.  cn_lds_map composes them into offsets, overlays and the total: cn_create (crowdnav_abi.hip) sizes every launch from it
// and tests/test_lds_map.py walks it on the CPU (plain C++17, so a g++ program can).  env_kernel_body (crowdnav_kernel.hip) runs
// one pointer over the same macros in the same order.  LDS accesses past the allocation do not fault -- they read zeros or are
// dropped -- which is why the carve and the size must not be two pieces of arithmetic.
#pragma once
#include "crowdnav_kernel.h"

#if defined(__HIPCC__)
#define CN_LDS_FN __host__ __device__ __forceinline__
#else
#define CN_LDS_FN inline
#endif
#define CN_NMASK 13        /* bit-word masks kept in LDS: M_COUNT of crowdnav_kernel.hip's enum (static_assert there) */

// The shapes that have kernels compiled for them (_s360 / _s720): BASELINE configs[1] and configs[4] with cn_create's max_conf,
// tracker slots and near-list placement for them.  The kernels assume these six values; cn_create picks them for nothing else.
struct CnShape { int R, P, K, max_conf, trk_cap, near_sep; };
enum { CN_SHAPE_360 = 0, CN_SHAPE_720, CN_SHAPE_COUNT };
constexpr CnShape cn_shapes[CN_SHAPE_COUNT] = { {360, 20, 8, 91, 32, 1}, {720, 100, 8, 181, 64, 0} };

// Byte offsets from the working set's base, and sizes.  The base must be 16-byte aligned (the kernels' dynamic LDS is declared so
// and every per-wave stride is rounded to 16): rw is aligned as an offset, the kernel aligns the address.  The sub-arrays of a region are typed views the kernel
// forms itself.
//   region A (offset 0, szA): end points in integer thousandths | the LDS tracker table | compact: the pedestrians' velocities
//   region B (offset szA, szB): gradients + alias sources | bbox staging (64 doubles) | confirmed objects (szC), then cpv [64], the
//                               observation tail [8 + 4 K], kidx [CN_MAX_K] | the near-pedestrian list when it has no region of its own
struct CnLdsMap {
    size_t szA, szB, szC;
    size_t w64, wbase, ped, pedv, nearp;    // bit words [CN_NMASK][Wn], wbase [3][Wn], positions, velocities, near list [P + 1][4]
    size_t rw;                              // 16-byte aligned: the real-world layout's lists (12 bytes per ray), behind everything else
    size_t total;                           // what a launch asks for (a multiple of 16); 1 << 30: the compact layout does not fit
};
// The sizes.  They are macros, not functions, so that env_kernel_body's carve -- a running pointer over exactly these expressions --
// compiles to the code it always did: every carve formed from cn_lds_map's struct moved the generic kernels' register allocation
// (a policy kernel gained VGPR spills) and measured the same-call kernel 0.5 % slower.  n = rays - 1, Wn = 64-ray words, mc = max_conf;
// CMP: the 720-ray shape kernels' compact layout (int16 end points, 12-byte confirmed objects, velocities overlaid on region A,
// which is idle whenever the simulator runs); slots: tracker slots in LDS (0 for a wide table, which lives in HBM).
#define CN_LDS_WORDS(n) (((n) + 63) >> 6)
#define CN_LDS_SZ_PTS(CMP, n) ((size_t)(((CMP) ? 6 : 10) * (n) + 7) & ~(size_t)7)
#define CN_LDS_SZ_TRK(slots) (8 * (size_t)(CN_TF_COUNT * (slots)))
#define CN_LDS_SZ_GRAD(n) ((size_t)(6 * (n) + 7) & ~(size_t)7)
#define CN_LDS_SZ_CONF(CMP, mc) ((CMP) ? ((12 * (mc) + 7) & ~(size_t)7) : 32 * (mc))
#define CN_LDS_SZ_CTAIL(K) (8 * 64 + 8 * (size_t)(8 + 4 * (K)) + 4 * (size_t)CN_MAX_K)     /* cpv [64], tail [8 + 4 K], kidx */
#define CN_LDS_SZ_STAGE (8 * 64)
#define CN_LDS_SZ_W64(Wn) (8 * (size_t)(CN_NMASK * (Wn)))
#define CN_LDS_SZ_WBASE(Wn) (8 * (size_t)((3 * (Wn) + 1) / 2))
#define CN_LDS_SZ_PED(P) (8 * (size_t)(2 * (P) + 2))
#define CN_LDS_SZ_NEAR(P) (32 * (size_t)((P) + 1))
#define CN_LDS_SZ_RW(n) (12 * (size_t)(n) + 16)

CN_LDS_FN CnLdsMap cn_lds_map(int n, int P, int K, int max_conf, int trk_slots, int near_sep, bool compact, bool realworld)
{
    CnLdsMap m;
    const size_t mc = (size_t)max_conf, pts = CN_LDS_SZ_PTS(compact, n), trk = CN_LDS_SZ_TRK(trk_slots), grad = CN_LDS_SZ_GRAD(n);
    const int Wn = CN_LDS_WORDS(n);
    m.szA = pts > trk ? pts : trk;
    m.szC = CN_LDS_SZ_CONF(compact, mc);
    const size_t conf = m.szC + CN_LDS_SZ_CTAIL(K);
    m.szB = grad > conf ? grad : conf;
    if (m.szB < CN_LDS_SZ_STAGE) m.szB = CN_LDS_SZ_STAGE;
    if (!near_sep && m.szB < CN_LDS_SZ_NEAR(P)) m.szB = CN_LDS_SZ_NEAR(P);
    m.w64 = m.szA + m.szB;
    m.wbase = m.w64 + CN_LDS_SZ_W64(Wn);
    m.ped = m.wbase + CN_LDS_SZ_WBASE(Wn);
    m.pedv = compact ? 0 : m.ped + CN_LDS_SZ_PED(P);
    size_t end = m.ped + (compact ? 1 : 2) * CN_LDS_SZ_PED(P);
    m.nearp = near_sep ? end : m.szA;       // overlaid: the ray loop's own, and region B is dead until the gradients are written
    if (near_sep) end += CN_LDS_SZ_NEAR(P);
    m.rw = (end + 15) & ~(size_t)15;
    if (realworld) end = m.rw + CN_LDS_SZ_RW(n);
    m.total = compact && CN_LDS_SZ_PED(P) > m.szA ? (size_t)1 << 30 : (end + 15) & ~(size_t)15;
    return m;
}

// The near-pedestrian list gets its own region when that costs no resident wavefront (160 KiB of LDS, 16 wave slots per CU) --
// measured 1.5 % faster than sharing region B with the gradients -- and is overlaid on region B otherwise (100 pedestrians x 720
// rays: 8 instead of 7 wavefronts per CU).
inline int cn_lds_trk_slots(int trk_cap) { return trk_cap > CN_MAX_TRACKS ? 0 : trk_cap; }
inline int cn_lds_waves_per_cu(size_t lds) { const size_t w = (160 * 1024) / (lds ? lds : 1); return (int)(w > 16 ? 16 : w); }
inline int cn_lds_near_separate(int R, int P, int K, int max_conf, int trk_cap)
{
    const int ts = cn_lds_trk_slots(trk_cap);
    return cn_lds_waves_per_cu(cn_lds_map(R - 1, P, K, max_conf, ts, 1, false, false).total) ==
           cn_lds_waves_per_cu(cn_lds_map(R - 1, P, K, max_conf, ts, 0, false, false).total);
}
// What the simulators may use of regions A + B in every non-compact layout (szA >= 10 n, szB >= 6 n): cn_create's documented limits
// for ped_contact and the social-force pair matrix are in terms of this, not of a particular layout's larger regions.
constexpr size_t cn_lds_sim_scratch(int R) { return 16 * (size_t)(R - 1); }
