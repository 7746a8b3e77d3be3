// crowdnav_actor.hip -- the TD3 actor outside the step loop: its kernels (gfx950) and their entry points of the C-ABI
// (include/crowdnav.h), each kernel next to the host code that launches it:
//   cn_policy_tail                 heads, exploration noise and clip on ready logits
//   cn_actor_pack_weights          the packed weight layout the matrix cores consume
//   cn_actor_forward               Actor.forward + Agent.act's noise and clip, one launch
//   cn_actor_pop_*                 a population's actors: every member's forward in one launch, their re-pack in one more
// The tile itself -- actor_layer, actor_tile -- is crowdnav_actor.h, shared with the policy kernels of crowdnav_kernel.hip
// (cn_rollout_policy).  Errors go to the environment's channel, cn_last_error.
#include <string.h>
#include <algorithm>
#include <memory>
#include <mutex>
#include <new>

#include "crowdnav_actor.h"
#include "crowdnav_host.h"

// ---- policy tail of the TD3 actor (the caller of the hot path) ---------------------------
// One launch instead of ~10 elementwise ones: action heads sigmoid(l0)*max_v / tanh(l1)*max_w (TD3:103-104),
// Gaussian exploration noise N(0, sigma) (TD3:67-78, 209-211) from a counter-based RNG, clip to
// v in [0, max_v], w in [-max_w, max_w] (TD3:214-215).
extern "C" __global__ void cn_policy_tail_kernel(const float* __restrict__ logits, float* __restrict__ action, int n,
                                                 float max_v, float max_w, float sigma, uint64_t seed, uint64_t counter)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float l0 = logits[2 * i], l1 = logits[2 * i + 1];
    float v = max_v / (1.0f + __expf(-l0));
    float w = max_w * tanhf(l1);
    if (sigma > 0.0f) {
        uint64_t h = cn_mix64(seed ^ cn_mix64(counter));
        h = cn_mix64(h ^ (uint64_t)(uint32_t)i);
        float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777217.0f);   // (0, 1]
        float u2 = (float)(uint32_t)((h >> 8) & 0xffffffu) * (1.0f / 16777216.0f);
        float r = sqrtf(-2.0f * __logf(u1)), s_, c_;
        __sincosf(6.28318530718f * u2, &s_, &c_);
        v += sigma * r * c_;
        w += sigma * r * s_;
    }
    action[2 * i] = fminf(fmaxf(v, 0.0f), max_v);
    action[2 * i + 1] = fminf(fmaxf(w, -max_w), max_w);
}

extern "C" int cn_policy_tail(const float* logits, float* action, int n, float max_v, float max_w, float sigma,
                              uint64_t seed, uint64_t counter, int device, void* stream)
{
    if (!logits || !action || n < 0) return fail(CN_ERR_ARG, "cn_policy_tail: bad argument");
    if (n == 0) return CN_OK;
    int dev = device;
    if (dev < 0) CN_HIPCHK(fail, hipGetDevice(&dev));
    DeviceScope scope(dev);
    hipLaunchKernelGGL(cn_policy_tail_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, logits, action, n,
                       max_v, max_w, sigma, seed, counter);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" __global__ void cn_actor_pack_kernel(const float* __restrict__ wt, int K, float* __restrict__ packed)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;        // index into `packed`
    if (idx >= K * ACT_H) return;
    const int j = idx & 3, lane = (idx >> 2) & 63, q = (idx >> 8) & 3, w = (idx >> 10) & 7, b = idx >> 13;
    const int k = 32 * b + 4 * (2 * q + (j >> 1)) + (lane >> 4), c = 32 * w + 2 * (lane & 15) + (j & 1);
    packed[idx] = wt[(size_t)k * ACT_H + c];
}

extern "C" int cn_actor_pack_weights(const float* wt, int k_rows, float* packed, int device, void* stream)
{
    if (!wt || !packed || wt == packed) return fail(CN_ERR_ARG, "cn_actor_pack_weights: null or aliasing argument");
    if (k_rows < 32 || (k_rows & 31)) return fail(CN_ERR_CONFIG, "cn_actor_pack_weights: k_rows must be a positive multiple of 32");
    int dev = device;
    if (dev < 0) CN_HIPCHK(fail, hipGetDevice(&dev));
    DeviceScope scope(dev);
    const int total = k_rows * 256;
    hipLaunchKernelGGL(cn_actor_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, wt, k_rows, packed);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

// ---- cn_actor_forward: the whole actor in one launch, a tile of 16 rows per workgroup (actor_tile, crowdnav_actor.h) -------------
#ifdef CN_TIMING
// profiling build: s_memtime stamps of workgroup b's wave 0 at [b][8] (tools/actor_timing.py).  Only cn_actor_kernel asks for them
// (actor_tile's STAMP): the slot is the workgroup's x, which the members of cn_actor_pop_kernel and the policy kernels' periods share.
__device__ long long* cn_actor_timing = nullptr;
extern "C" int cn_debug_set_actor_timing(long long* dev_buf)
{
    return hipMemcpyToSymbol(HIP_SYMBOL(cn_actor_timing), &dev_buf, sizeof(dev_buf)) == hipSuccess ? 0 : -4;
}
template <> __device__ __forceinline__ void actor_stamp<true>(int k)
{
    if (cn_actor_timing && threadIdx.x == 0) cn_actor_timing[(size_t)blockIdx.x * 8 + k] = (long long)__builtin_amdgcn_s_memtime();
}
#endif
extern "C" __global__ void __launch_bounds__(ACT_THREADS) cn_actor_kernel(const float* __restrict__ obs, int n, int D, int Dp,
        const float* __restrict__ W1T, const float* __restrict__ b1, const float* __restrict__ W2T,
        const float* __restrict__ b2, const float* __restrict__ W3, const float* __restrict__ b3,
        float* __restrict__ action, float max_v, float max_w, float sigma, uint64_t seed, uint64_t counter)
{
    extern __shared__ __attribute__((aligned(16))) float act_sm[];
    const int row0 = blockIdx.x * ACT_M;
    actor_tile<ACT_THREADS / 64, true>(obs + (size_t)row0 * D, min(ACT_M, n - row0), row0, D, Dp, W1T, b1, W2T, b2, W3, b3,
                                       action + 2 * (size_t)row0, nullptr, max_v, max_w, sigma, seed, counter, act_sm);
}

// An actor kernel whose tile exceeds 64 KiB: raise its dynamic-LDS limit to a CU's 160 KiB on the current device.  hipFuncSetAttribute
// is per device: once per ordinal (attr_set: the kernel's own 64 flags), under a lock.  (Declared in crowdnav_host.h: cn_ddpg_act's
// kernel, crowdnav_ddpg.hip, runs the same tile.)
int allow_full_lds(const void* kernel, int dev, bool* attr_set)
{
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (dev >= 64 || !attr_set[dev]) {
        CN_HIPCHK(fail, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if (dev < 64) attr_set[dev] = true;
    }
    return CN_OK;
}

extern "C" int cn_actor_forward(const cn_actor_weights* w, const float* obs, float* action, int n, float max_v, float max_w,
                                float sigma, uint64_t seed, uint64_t counter, int device, void* stream)
{
    if (!w || !obs || !action || n < 0 || !w->w1p || !w->b1 || !w->w2p || !w->b2 || !w->w3 || !w->b3)
        return fail(CN_ERR_ARG, "cn_actor_forward: null argument");
    if (w->hidden != 256 || w->obs_dim < 1 || w->obs_dim_padded < w->obs_dim || (w->obs_dim_padded & 31))
        return fail(CN_ERR_CONFIG, "cn_actor_forward: hidden must be 256 and obs_dim_padded a multiple of 32 (the packed layout of cn_actor_pack_weights)");
    if (n == 0) return CN_OK;
    const int Dp = w->obs_dim_padded;
    const size_t lds = actor_tile_bytes(Dp);
    if (lds > 160 * 1024) return fail(CN_ERR_CONFIG, "cn_actor_forward: observation too wide for one LDS tile");
    int dev = device;
    if (dev < 0) CN_HIPCHK(fail, hipGetDevice(&dev));
    DeviceScope scope(dev);
    if (lds > 64 * 1024) { static bool attr_set[64] = {false}; const int rc = allow_full_lds((const void*)cn_actor_kernel, dev, attr_set); if (rc != CN_OK) return rc; }
    hipLaunchKernelGGL(cn_actor_kernel, dim3((n + 15) / 16), dim3(512), lds, (hipStream_t)stream, obs, n, w->obs_dim, Dp,
                       w->w1p, w->b1, w->w2p, w->b2, w->w3, w->b3, action, max_v, max_w, sigma, seed, counter);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

// ---- a population's actors: P members' cn_actor_forward in ONE launch, their re-pack in one more (cn_actor_pop_*) --------------
// Member = blockIdx.z, its job a row of a table in device memory that cn_actor_pop_create uploads once (workgroup-uniform: scalar
// loads); the members' call counters change with every call and travel BY VALUE in the kernel-argument segment (64 x 8 bytes), so a
// call copies nothing to the device.  The grid's x is the widest member's tile count: a workgroup beyond its own member's rows
// leaves before the first barrier (the test is workgroup-uniform).  Everything else is actor_tile with the row WITHIN the member --
// the tile, the noise key (seed_p, counter_p, row) and therefore every bit of the output are cn_actor_kernel's for that member.
// One tile is 42 KB of LDS at 398 inputs: tiles of different members share a CU, which P launches in series on one stream never do.
extern "C" __global__ void __launch_bounds__(ACT_THREADS) cn_actor_pop_kernel(const CnActorPopJob* __restrict__ table, int D, int Dp,
                                                                              int add_noise, CnActorPopCounters ctr)
{
    extern __shared__ __attribute__((aligned(16))) float act_sm[];
    const CnActorPopJob& jb = table[blockIdx.z];
    const int n = jb.n, row0 = blockIdx.x * ACT_M;
    if (row0 >= n) return;
    actor_tile<ACT_THREADS / 64>(jb.obs + (size_t)row0 * D, min(ACT_M, n - row0), row0, D, Dp, jb.w1p, jb.b1, jb.w2p, jb.b2, jb.w3, jb.b3,
                                 jb.action + 2 * (size_t)row0, nullptr, jb.max_v, jb.max_w, add_noise ? jb.sigma : 0.0f, jb.seed,
                                 ctr.c[blockIdx.z], act_sm);
}

// cn_actor_pack_kernel's layout for every member and both layers in one launch, read straight from the nn.Linear storages
// W[c][k] ([256][K_in] row-major: the transpose that cn_actor_pack_weights' caller stages first never exists).  One thread per packed
// element; grid (Dp, 2 layers, P) x 256 threads; layer 1 pads k >= D with zeros, so every element of both buffers is written.
// Pure data movement, once per weight update: neighbouring threads read W 4 K_in bytes apart (about 0.4 MB per member, uncoalesced,
// out of L2 after the update that wrote it) and write coalesced.  A tile transposed through LDS would mend the read; it is not worth
// the machinery for a launch whose cost is its latency.
extern "C" __global__ void __launch_bounds__(256) cn_actor_pop_pack_kernel(const CnActorPopPackJob* __restrict__ table, int D, int Dp)
{
    const CnActorPopPackJob& jb = table[blockIdx.z];
    const int layer = blockIdx.y;
    const int K = layer ? ACT_H : Dp, K_in = layer ? ACT_H : D;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;        // index into the packed buffer
    if (idx >= K * ACT_H) return;
    const float* __restrict__ W = layer ? jb.w2 : jb.w1;
    float* __restrict__ packed = layer ? jb.w2p : jb.w1p;
    const int j = idx & 3, lane = (idx >> 2) & 63, q = (idx >> 8) & 3, w = (idx >> 10) & 7, b = idx >> 13;
    const int k = 32 * b + 4 * (2 * q + (j >> 1)) + (lane >> 4), c = 32 * w + 2 * (lane & 15) + (j & 1);
    packed[idx] = k < K_in ? W[(size_t)c * K_in + k] : 0.0f;
}


struct cn_actor_pop_s {
    int device = 0, P = 0, D = 0, Dp = 0, tiles = 0;      // tiles: the widest member's, the grid's x (0: nothing to launch)
    size_t lds = 0;
    void* mem = nullptr;                                   // one allocation: the two tables, then every member's w1p and w2p
    const CnActorPopJob* jobs = nullptr;
    const CnActorPopPackJob* pack = nullptr;
    std::vector<cn_actor_weights> weights;
    cn_actor_pop_s() = default;
    cn_actor_pop_s(const cn_actor_pop_s&) = delete;
    ~cn_actor_pop_s() { if (mem) { DeviceScope scope(device); (void)hipFree(mem); } }
};

extern "C" int cn_actor_pop_create(const cn_actor_pop_member* members, int n_members, int obs_dim, int device, cn_actor_pop_handle* out)
{
    const std::string f("cn_actor_pop_create");
    if (!members) return fail(CN_ERR_ARG, f + ": members is null");
    if (!out) return fail(CN_ERR_ARG, f + ": out is null");
    if (n_members < 1 || n_members > CN_ACTOR_POP_MAX) return fail(CN_ERR_ARG, f + ": n_members must be 1 ... 64");
    if (obs_dim < 1) return fail(CN_ERR_CONFIG, f + ": obs_dim must be at least 1");
    const int64_t Dp64 = ((int64_t)obs_dim + 31) / 32 * 32;
    const size_t lds = actor_tile_bytes((size_t)Dp64);       // cn_actor_forward's tile
    const int P = n_members, D = obs_dim, Dp = (int)Dp64;
    if (lds > 160 * 1024) return fail(CN_ERR_CONFIG, f + ": obs_dim: observation too wide for one LDS tile");
    int tiles = 0;
    for (int p = 0; p < P; ++p) {
        const cn_actor_pop_member& m = members[p];
        const std::string who = ": member " + std::to_string(p) + ": ";
        const float* const ps[6] = {m.actor.w1, m.actor.b1, m.actor.w2, m.actor.b2, m.actor.w3, m.actor.b3};
        static const char* const pn[6] = {"actor.w1", "actor.b1", "actor.w2", "actor.b2", "actor.w3", "actor.b3"};
        for (int i = 0; i < 6; ++i)
            if (!ps[i]) return fail(CN_ERR_ARG, f + who + pn[i] + " is null");
        if (m.n < 0) return fail(CN_ERR_ARG, f + who + "n is negative");
        if (m.n > 0 && !m.obs) return fail(CN_ERR_ARG, f + who + "obs is null");
        if (m.n > 0 && !m.action) return fail(CN_ERR_ARG, f + who + "action is null");
        tiles = std::max(tiles, (int)(((int64_t)m.n + 15) / 16));
    }
    std::unique_ptr<cn_actor_pop_s> h(new (std::nothrow) cn_actor_pop_s());
    if (!h) return fail(CN_ERR_ARG, f + ": out of memory");
    int dev = device;
    if (dev < 0) CN_HIPCHK(fail, hipGetDevice(&dev));
    h->device = dev; h->P = P; h->D = D; h->Dp = Dp; h->tiles = tiles; h->lds = lds;
    DeviceScope scope(dev);
    // [jobs P][pack jobs P] rounded up to 256 bytes, then per member w1p [Dp][256] and w2p [256][256] (16-byte loads: both sizes are
    // multiples of 1 KB)
    const size_t n1 = (size_t)Dp * 256, n2 = (size_t)256 * 256;
    const size_t tab = (sizeof(CnActorPopJob) * P + sizeof(CnActorPopPackJob) * P + 255) & ~(size_t)255;
    CN_HIPCHK(fail, hipMalloc(&h->mem, tab + sizeof(float) * (n1 + n2) * P));
    CnActorPopJob* jobs = (CnActorPopJob*)h->mem;
    CnActorPopPackJob* pack = (CnActorPopPackJob*)(jobs + P);
    float* wbuf = (float*)((char*)h->mem + tab);
    std::vector<CnActorPopJob> hj(P);
    std::vector<CnActorPopPackJob> hp(P);
    h->weights.resize(P);
    for (int p = 0; p < P; ++p) {
        const cn_actor_pop_member& m = members[p];
        float* w1p = wbuf + (size_t)p * (n1 + n2);
        float* w2p = w1p + n1;
        hj[p] = CnActorPopJob{m.obs, w1p, m.actor.b1, w2p, m.actor.b2, m.actor.w3, m.actor.b3, m.action, m.n, m.max_v, m.max_w, m.sigma, m.seed};
        hp[p] = CnActorPopPackJob{m.actor.w1, m.actor.w2, w1p, w2p};
        h->weights[p] = cn_actor_weights{w1p, m.actor.b1, w2p, m.actor.b2, m.actor.w3, m.actor.b3, D, Dp, 256, 0};
    }
    CN_HIPCHK(fail, hipMemcpy(jobs, hj.data(), sizeof(CnActorPopJob) * P, hipMemcpyHostToDevice));
    CN_HIPCHK(fail, hipMemcpy(pack, hp.data(), sizeof(CnActorPopPackJob) * P, hipMemcpyHostToDevice));
    h->jobs = jobs; h->pack = pack;
    if (lds > 64 * 1024) { static bool attr_set[64] = {false}; const int rc = allow_full_lds((const void*)cn_actor_pop_kernel, dev, attr_set); if (rc != CN_OK) return rc; }
    *out = h.release();
    return CN_OK;
}
extern "C" void cn_actor_pop_destroy(cn_actor_pop_handle h) { delete h; }
extern "C" int cn_actor_pop_members(cn_actor_pop_handle h) { return h ? h->P : 0; }

extern "C" int cn_actor_pop_pack(cn_actor_pop_handle h, void* stream)
{
    if (!h) return fail(CN_ERR_ARG, "cn_actor_pop_pack: null handle");
    DeviceScope scope(h->device);
    // x covers the larger layer: Dp blocks of 256 elements for layer 1, 256 for layer 2
    hipLaunchKernelGGL(cn_actor_pop_pack_kernel, dim3(std::max(h->Dp, 256), 2, h->P), dim3(256), 0, (hipStream_t)stream, h->pack, h->D, h->Dp);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_actor_pop_forward(cn_actor_pop_handle h, const uint64_t* counters, int add_noise, void* stream)
{
    if (!h) return fail(CN_ERR_ARG, "cn_actor_pop_forward: null handle");
    if (!counters) return fail(CN_ERR_ARG, "cn_actor_pop_forward: counters is null");
    if (h->tiles == 0) return CN_OK;
    CnActorPopCounters ctr;
    memset(&ctr, 0, sizeof(ctr));
    memcpy(ctr.c, counters, sizeof(uint64_t) * h->P);
    DeviceScope scope(h->device);
    hipLaunchKernelGGL(cn_actor_pop_kernel, dim3(h->tiles, 1, h->P), dim3(512), h->lds, (hipStream_t)stream, h->jobs, h->D, h->Dp,
                       add_noise ? 1 : 0, ctr);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_actor_pop_weights(cn_actor_pop_handle h, int member, cn_actor_weights* out)
{
    if (!h) return fail(CN_ERR_ARG, "cn_actor_pop_weights: null handle");
    if (!out) return fail(CN_ERR_ARG, "cn_actor_pop_weights: out is null");
    if (member < 0 || member >= h->P) return fail(CN_ERR_ARG, "cn_actor_pop_weights: member " + std::to_string(member) + " out of range (the handle has " + std::to_string(h->P) + ")");
    *out = h->weights[member];
    return CN_OK;
}
