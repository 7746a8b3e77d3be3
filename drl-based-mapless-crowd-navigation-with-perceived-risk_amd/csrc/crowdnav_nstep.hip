// crowdnav_nstep.hip -- cn_nstep_record (include/crowdnav.h): cn_pop_record's job with n-step rows -- the returns accumulate in a
// pending store on the device and a row reaches the ring when it spans n_step steps or its episode ends -- in two launches whatever
// the number of members and the window: the two kernels, then the entry points that launch them (errors go to cn_last_error).
// The shape is crowdnav_pop_record.hip's: member = blockIdx.z, its job a row of a table in device memory that
// cn_nstep_record_create uploads once; `launch` travels by value.  The scan, the episode log and the keep functor are
// crowdnav_record.h's, so the log's float64 sums keep their one order; the members' checks are crowdnav_record_host.h's.  A unit of
// its own, so that every other unit keeps its instruction stream.
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "crowdnav_host.h"
#include "crowdnav_record.h"
#include "crowdnav_record_host.h"

// a member's job: cn_pop_record's row (its `slot` is not used: an environment row may emit several ring rows), then the window
struct CnNstepJob {
    CnPopRecordJob rec;
    float *ps, *pa, *pret;                        // the pending store: [n][W][D], [n][W][2], [n][W]
    int32_t *count, *clock;                       // [n]
    int4* desc;                                   // [n], launch A -> launch B: {first ring slot or -1, rows emitted or -1 = not kept, pre-call count, clock}
    float w[CN_NSTEP_MAX];                        // w[k] = cn_nstep_discount(gamma, k), k < W
    int32_t W, reserved;
};

// ret + w r: the float32 product and the float32 sum, each rounded on its own (no FMA)
__device__ __forceinline__ float cn_nstep_add(float ret, float w, float r)
{
#pragma clang fp contract(off)
    const float term = w * r;
    return ret + term;
}
// tau mod W for any int tau (a clock restored by a caller is not trusted to be non-negative)
__device__ __forceinline__ int cn_nstep_slot(int tau, int W) { const int t = tau % W; return t < 0 ? t + W : t; }

// Launch A, grid (1, 1, P) x 1024: member z's plan.  Thread t owns the rows i = t (mod 1024): it updates their pending returns, counts
// the ring rows they emit, scans the counts into first slots and leaves the descriptor; then the ring's position and fill level, the
// episode log with the same keep flags, and resetting <- done behind a workgroup barrier, as cn_pop_record_scan_kernel.  Of what
// launch B reads, only the returns of entries that were already pending are written here, and B wants them updated.
extern "C" __global__ void __launch_bounds__(1024) cn_nstep_plan_kernel(const CnNstepJob* __restrict__ table, float launch)
{
    __shared__ int wsum[16];
    __shared__ double red[5][16];
    const CnNstepJob& jb = table[blockIdx.z];
    const CnPopRecordJob& rj = jb.rec;
    const int n = rj.n, W = jb.W;
    if (n <= 0) return;                                        // (workgroup-uniform)
    const CnKeepNotResetting keep{rj.resetting};
    const int64_t cap = rj.ring.capacity, pos = *rj.ring.pos_dev, size = *rj.ring.size_dev;
    int64_t carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        int m = 0, c0 = 0, k0 = 0, kept = 0;
        if (i < n) {
            c0 = min(max(jb.count[i], 0), W - 1);              // (a restored count is not trusted either: the loop below stays inside the row)
            k0 = jb.clock[i];
            kept = keep(i);
            if (kept) {
                const float r = rj.reward[i];
                const int fin = rj.done[i] != 0;
                float* ret = jb.pret + (size_t)i * W;
                for (int k = 1; k <= c0; ++k) {                // the entry of age k lies in slot (clock - k) mod W
                    const int s = cn_nstep_slot(k0 - k, W);
                    ret[s] = cn_nstep_add(ret[s], jb.w[k], r);
                }
                m = fin ? c0 + 1 : (c0 + 1 == W ? 1 : 0);
                jb.count[i] = fin ? 0 : c0 + 1 - m;
                jb.clock[i] = fin ? 0 : k0 + 1;
            }
        }
        int tot;
        const int c = cn_block_scan_1024(m, wsum, tot);
        if (i < n) jb.desc[i] = make_int4(m > 0 ? (int)((pos + carry + c - m) % cap) : -1, kept ? m : -1, c0, k0);
        carry += tot;
    }
    if (threadIdx.x == 0) {
        *rj.ring.pos_dev = (pos + carry) % cap;
        *rj.ring.size_dev = size + carry < cap ? size + carry : cap;
    }
    if (rj.state) cn_episode_log_body(rj.log, rj.done, CnEpisodeFromState{rj.state, rj.state_stride}, keep, launch, n, wsum, red);
    else cn_episode_log_body(rj.log, rj.done, CnEpisodeFromArrays{rj.counters, CN_COUNTER_COLS, rj.last_return}, keep, launch, n, wsum, red);
    __syncthreads();
    const uint8_t* __restrict__ done = rj.done;
    uint8_t* resetting = rj.resetting;
    for (int i = threadIdx.x; i < n; i += 1024) resetting[i] = done[i] != 0;
}

// one ring row: s [D] from `s`, s2 [D] from `s2`, then the four scalars' lanes
__device__ __forceinline__ void cn_nstep_ring_row(const cn_replay_ring& ring, int64_t sl, const float* s, const float* a, float ret,
                                                  const float* __restrict__ s2, float d)
{
    const int D = ring.obs_dim;
    float* __restrict__ ds = ring.s + (size_t)sl * D;
    float* __restrict__ ds2 = ring.s2 + (size_t)sl * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) { ds[c] = s[c]; ds2[c] = s2[c]; }
    if (threadIdx.x < 2) ring.a[(size_t)sl * 2 + threadIdx.x] = a[threadIdx.x];
    if (threadIdx.x == 2) ring.r[sl] = ret;
    if (threadIdx.x == 3) ring.d[sl] = d;
}

// Launch B, grid (max n_p, W, P) x 256.  Workgroup (e, 0, z): the new entry of row e, from prev into its ring slot (the episode
// ended, or W = 1) or into its slot of the store -- free, since at most W - 1 entries were pending --, then prev <- obs for the row,
// kept or not; thread t copies the columns c = t (mod 256) in every loop, so it overwrites in prev only what it has itself read.
// Workgroup (e, j >= 1, z): the pending entry q = j - 1 (oldest first), if the call emits it, from the store into ring slot first + q.
extern "C" __global__ void __launch_bounds__(256) cn_nstep_copy_kernel(const CnNstepJob* __restrict__ table)
{
    const CnNstepJob& jb = table[blockIdx.z];
    const CnPopRecordJob& rj = jb.rec;
    const int e = blockIdx.x, j = blockIdx.y;
    if (e >= rj.n) return;                                     // (workgroup-uniform, as every branch below)
    const int W = jb.W, D = rj.ring.obs_dim;
    const int4 ds = jb.desc[e];
    const int first = ds.x, m = ds.y, c0 = ds.z, k0 = ds.w;
    const int64_t cap = rj.ring.capacity;
    const float* __restrict__ obs = rj.obs + (size_t)e * D;
    const float d = rj.done[e] ? 1.f : 0.f;
    if (j == 0) {
        float* prev = rj.prev + (size_t)e * D;
        if (m > c0) {                                          // kept and emitted with the older entries: the last of its m rows
            cn_nstep_ring_row(rj.ring, (first + (int64_t)c0) % cap, prev, rj.action + (size_t)e * 2, rj.reward[e], obs, d);
        } else if (m >= 0) {                                   // kept and pending
            const size_t at = (size_t)e * W + cn_nstep_slot(k0, W);
            float* __restrict__ s = jb.ps + at * D;
            for (int c = threadIdx.x; c < D; c += blockDim.x) s[c] = prev[c];
            if (threadIdx.x < 2) jb.pa[at * 2 + threadIdx.x] = rj.action[(size_t)e * 2 + threadIdx.x];
            if (threadIdx.x == 2) jb.pret[at] = rj.reward[e];
        }
        for (int c = threadIdx.x; c < D; c += blockDim.x) prev[c] = obs[c];
        return;
    }
    const int q = j - 1;
    if (q >= c0 || q >= m) return;                             // (m = -1: not kept)
    const size_t at = (size_t)e * W + cn_nstep_slot(k0 - c0 + q, W);
    cn_nstep_ring_row(rj.ring, (first + (int64_t)q) % cap, jb.ps + at * D, jb.pa + at * 2, jb.pret[at], obs, d);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct cn_nstep_record_s {
    int device = 0, P = 0, W = 1, max_n = 0;               // max_n: the widest member's rows, launch B's grid x (0: nothing to launch)
    void* mem = nullptr;                                   // one allocation: the table, then every member's descriptors, flags and store
    const CnNstepJob* jobs = nullptr;
    std::vector<uint8_t*> resetting;
    std::vector<cn_nstep_pending> pending;
    cn_nstep_record_s() = default;
    cn_nstep_record_s(const cn_nstep_record_s&) = delete;
    ~cn_nstep_record_s() { if (mem) { DeviceScope scope(device); (void)hipFree(mem); } }
};

extern "C" float cn_nstep_discount(float gamma, int k)
{
    double acc = 1.0;
    for (int i = 0; i < k; ++i) acc *= (double)gamma;
    return (float)acc;
}

extern "C" int cn_nstep_record_create(const cn_nstep_member* members, int n_members, int n_step, int obs_dim, int device,
                                      cn_nstep_record_handle* out)
{
    const std::string f("cn_nstep_record_create");
    if (int rc = cn_record_check_call(f, members, out, n_members, obs_dim)) return rc;
    if (n_step < 1 || n_step > CN_NSTEP_MAX) return fail(CN_ERR_ARG, f + ": n_step must be 1 ... 16");
    const int P = n_members, W = n_step;
    std::vector<CnRecordNamed> written;
    int max_n = 0;
    for (int p = 0; p < P; ++p) {
        if (int rc = cn_record_check_member(f, members[p].rec, p, obs_dim, W, written)) return rc;
        const float g = members[p].gamma;
        if (!std::isfinite(g) || !(g > 0.f) || g > 1.f)
            return fail(CN_ERR_ARG, f + ": member " + std::to_string(p) + ": gamma is " + std::to_string(g) + ", not a finite value in (0, 1]");
        max_n = std::max(max_n, (int)members[p].rec.n);
    }
    std::unique_ptr<cn_nstep_record_s> h(new (std::nothrow) cn_nstep_record_s());
    if (!h) return fail(CN_ERR_ARG, f + ": out of memory");
    int dev = device;
    if (dev < 0) CN_HIPCHK(fail, hipGetDevice(&dev));
    h->device = dev; h->P = P; h->W = W; h->max_n = max_n;
    DeviceScope scope(dev);
    // [jobs P] rounded up to 256 bytes, then per member desc [n] int4, resetting [n] bytes, count [n], clock [n], ret [n][W], a [n][W][2],
    // s [n][W][D], each rounded up to 16 bytes.  The allocation is zeroed and the table uploaded by a blocking copy behind it: the flags
    // and the store are zero whatever stream the first call runs on.
    const auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t tab = (sizeof(CnNstepJob) * P + 255) & ~(size_t)255;
    size_t total = tab;
    std::vector<size_t> off[7];
    for (int p = 0; p < P; ++p) {
        const size_t n = (size_t)members[p].rec.n;
        const size_t bytes[7] = {sizeof(int4) * n, n, sizeof(int32_t) * n, sizeof(int32_t) * n, sizeof(float) * n * W,
                                 sizeof(float) * n * W * 2, sizeof(float) * n * W * (size_t)obs_dim};
        for (int k = 0; k < 7; ++k) { off[k].push_back(total); total += up16(bytes[k]); }
    }
    CN_HIPCHK(fail, hipMalloc(&h->mem, total));
    CN_HIPCHK(fail, hipMemset(h->mem, 0, total));
    std::vector<CnNstepJob> hj(P);
    h->resetting.resize(P); h->pending.resize(P);
    char* base = (char*)h->mem;
    for (int p = 0; p < P; ++p) {
        const cn_pop_record_member& m = members[p].rec;
        CnNstepJob& j = hj[p];
        CnPopRecordJob& r = j.rec;
        r.ring = m.ring; r.log = m.log;
        r.state = m.env ? m.env->d_state : nullptr; r.state_stride = m.env ? (int64_t)m.env->stride : 0;
        r.counters = m.counters; r.last_return = m.last_return;
        r.prev = m.prev; r.obs = m.obs; r.action = m.action; r.reward = m.reward; r.done = m.done;
        r.resetting = h->resetting[p] = (uint8_t*)(base + off[1][p]);
        r.slot = nullptr; r.n = m.n; r.reserved = 0;
        j.desc = (int4*)(base + off[0][p]);
        j.count = (int32_t*)(base + off[2][p]); j.clock = (int32_t*)(base + off[3][p]);
        j.pret = (float*)(base + off[4][p]); j.pa = (float*)(base + off[5][p]); j.ps = (float*)(base + off[6][p]);
        for (int k = 0; k < CN_NSTEP_MAX; ++k) j.w[k] = k < W ? cn_nstep_discount(members[p].gamma, k) : 0.f;
        j.W = W; j.reserved = 0;
        h->pending[p] = cn_nstep_pending{j.ps, j.pa, j.pret, j.count, j.clock, m.n, W, obs_dim, 0};
    }
    CN_HIPCHK(fail, hipMemcpy(h->mem, hj.data(), sizeof(CnNstepJob) * P, hipMemcpyHostToDevice));
    CN_HIPCHK(fail, hipDeviceSynchronize());
    h->jobs = (const CnNstepJob*)h->mem;
    *out = h.release();
    return CN_OK;
}
extern "C" void cn_nstep_record_destroy(cn_nstep_record_handle h) { delete h; }
extern "C" int cn_nstep_record_members(cn_nstep_record_handle h) { return h ? h->P : 0; }

static bool nstep_member_ok(cn_nstep_record_handle h, int member, const char* f)
{
    if (!h) { (void)fail(CN_ERR_ARG, std::string(f) + ": null handle"); return false; }
    if (member < 0 || member >= h->P) {
        (void)fail(CN_ERR_ARG, std::string(f) + ": member " + std::to_string(member) + " out of range (the handle has " + std::to_string(h->P) + ")");
        return false;
    }
    return true;
}
extern "C" uint8_t* cn_nstep_record_resetting(cn_nstep_record_handle h, int member)
{
    return nstep_member_ok(h, member, "cn_nstep_record_resetting") ? h->resetting[member] : nullptr;
}
extern "C" int cn_nstep_record_pending(cn_nstep_record_handle h, int member, cn_nstep_pending* out)
{
    if (!nstep_member_ok(h, member, "cn_nstep_record_pending")) return CN_ERR_ARG;
    if (!out) return fail(CN_ERR_ARG, "cn_nstep_record_pending: out is null");
    *out = h->pending[member];
    return CN_OK;
}

extern "C" int cn_nstep_record(cn_nstep_record_handle h, float launch, void* stream)
{
    if (!h) return fail(CN_ERR_ARG, "cn_nstep_record: null handle");
    if (h->max_n == 0) return CN_OK;
    DeviceScope scope(h->device);
    hipLaunchKernelGGL(cn_nstep_plan_kernel, dim3(1, 1, h->P), dim3(1024), 0, (hipStream_t)stream, h->jobs, launch);
    hipLaunchKernelGGL(cn_nstep_copy_kernel, dim3(h->max_n, h->W, h->P), dim3(256), 0, (hipStream_t)stream, h->jobs);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}
