// crowdnav_record.h -- the collection loop's bookkeeping on the device: the bodies of cn_replay_write's and cn_episode_log_add's
// kernels (crowdnav_replay.hip, one member per launch) and of cn_pop_record's (crowdnav_pop_record.hip, member = blockIdx.z).  Both
// instantiate the SAME text, which is what makes the population's recorder equal the solo calls bit for bit: the slots, the order of
// the float64 sums and every conversion exist once.  What differs between the two is where a row's inputs come from, and that is a
// functor: the keep flag (a byte array or NULL / the inverse of `resetting`) and the episode record (the [n][14] counters and the
// returns that cn_get_counters / cn_get_returns gathered / the environment's state records themselves).
// A header of its own rather than part of crowdnav_device.h: the step kernels' units include that one and keep compiling from
// unchanged text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/crowdnav.h"
#include "crowdnav_kernel.h"

// inclusive scan of one int per thread over a 1024-thread workgroup (wave scans + a scan of the 16 wave totals)
__device__ __forceinline__ int cn_block_scan_1024(int v, int* __restrict__ wsum, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(v, d, 64); if (lane >= d) v += u; }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { const int x = wsum[w]; if (w < wave) before += x; tot += x; }
    __syncthreads();
    total = tot;
    return v + before;
}

// ---- where a row's keep flag comes from ----------------------------------------------------------------------------------------
struct CnKeepBytes {            // cn_replay_write: keep[i] != 0, NULL = all rows
    const uint8_t* __restrict__ keep;
    __device__ __forceinline__ int operator()(int i) const { return keep ? (keep[i] != 0) : 1; }
};
struct CnKeepNotResetting {     // cn_pop_record: the rows whose environment is not in its reset launch
    const uint8_t* resetting;
    __device__ __forceinline__ int operator()(int i) const { return resetting[i] == 0; }
};

// slots of the kept rows, in row order; the ring's position and fill level move at the end (one workgroup: they are read first)
template <class Keep>
__device__ __forceinline__ void cn_replay_slot_body(const Keep keep, int n, int64_t cap, int64_t* pos_dev, int64_t* size_dev,
                                                    int32_t* __restrict__ slot, int* __restrict__ wsum)
{
    const int64_t pos = *pos_dev, size = *size_dev;
    int64_t carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const int k = i < n ? keep(i) : 0;
        int tot;
        const int c = cn_block_scan_1024(k, wsum, tot);
        if (i < n) slot[i] = k ? (int32_t)((pos + carry + c - 1) % cap) : -1;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        *pos_dev = (pos + carry) % cap;
        *size_dev = size + carry < cap ? size + carry : cap;
    }
}

// row i (one 256-thread workgroup) into its slot
__device__ __forceinline__ void cn_replay_copy_body(const cn_replay_ring& ring, const float* ps, const float* pa, const float* pr,
                                                    const float* ps2, const uint8_t* done, const int32_t* slot, int i)
{
    const int D = ring.obs_dim;
    const int32_t sl = slot[i];
    if (sl < 0) return;
    const float* __restrict__ s = ps + (size_t)i * D;
    const float* __restrict__ s2 = ps2 + (size_t)i * D;
    float* __restrict__ ds = ring.s + (size_t)sl * D;
    float* __restrict__ ds2 = ring.s2 + (size_t)sl * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) { ds[c] = s[c]; ds2[c] = s2[c]; }
    if (threadIdx.x < 2) ring.a[(size_t)sl * 2 + threadIdx.x] = pa[(size_t)i * 2 + threadIdx.x];
    if (threadIdx.x == 2) ring.r[sl] = pr[i];
    if (threadIdx.x == 3) ring.d[sl] = done[i] ? 1.f : 0.f;
}

// ---- where a finished episode's record comes from ------------------------------------------------------------------------------
struct CnEpisodeRow { float success, failure, ret, steps, ego, social, obst; };
struct CnEpisodeFromArrays {    // cn_episode_log_add: the counter columns 4, 5, 13, 10, 11, 12 and last_return
    const int32_t* __restrict__ counters; int cols; const float* __restrict__ ret;
    __device__ __forceinline__ CnEpisodeRow operator()(int i) const
    {
        const int32_t* __restrict__ cr = counters + (size_t)i * cols;
        return CnEpisodeRow{(float)cr[4], (float)cr[5], ret[i], (float)cr[13], (float)cr[10], (float)cr[11], (float)cr[12]};
    }
};
struct CnEpisodeFromState {     // cn_pop_record with an environment: cn_gather_kernel's reads and conversions, then the same widening
    const char* __restrict__ state; int64_t stride;
    __device__ __forceinline__ CnEpisodeRow operator()(int i) const
    {
        const char* rec = state + (size_t)i * (size_t)stride;
        const double* __restrict__ sd = (const double*)(rec + CN_ST_OFF_SD);
        const int* __restrict__ si = (const int*)(rec + CN_ST_OFF_SI);
        return CnEpisodeRow{(float)si[CN_SI_SUCCESS], (float)si[CN_SI_FAILURE], (float)sd[CN_SD_LAST_RETURN],
                            (float)(int32_t)sd[CN_SD_LAST_EP_STEPS], (float)(int32_t)sd[CN_SD_LAST_EGO_VIOL],
                            (float)(int32_t)sd[CN_SD_LAST_SOCIAL_VIOL], (float)(int32_t)sd[CN_SD_LAST_OBST_STEPS]};
    }
};

// the finished episodes' rows and the running totals, one 1024-thread workgroup; trans(i): row i is a transition (tot_dev[4])
template <class Src, class Trans>
__device__ __forceinline__ void cn_episode_log_body(const cn_episode_log& log, const uint8_t* __restrict__ done, const Src src,
                                                    const Trans trans, float launch, int n, int* __restrict__ wsum, double (*red)[16])
{
    const int64_t n0 = *log.n_dev;
    int64_t carry = 0;
    double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const int k = i < n ? (done[i] != 0) : 0;
        int tot;
        const int c = cn_block_scan_1024(k, wsum, tot);
        if (i < n) {
            if (k) {
                const CnEpisodeRow e = src(i);
                const int64_t at = n0 + carry + c - 1;
                if (at < log.max_rows) {
                    float* __restrict__ row = log.rows + (size_t)at * 8;
                    row[0] = e.success; row[1] = e.failure; row[2] = e.ret; row[3] = e.steps;
                    row[4] = e.ego; row[5] = e.social; row[6] = e.obst; row[7] = launch;
                }
                t[0] += 1.0; t[1] += (double)e.success; t[2] += (double)e.ret; t[3] += (double)e.steps;
            }
            if (trans(i)) t[4] += 1.0;
        }
        carry += tot;
    }
    // totals: lanes, then wavefronts, in a fixed order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        double v = t[q];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) red[q][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) v += red[threadIdx.x][w];
        log.tot_dev[threadIdx.x] += v;
    }
    if (threadIdx.x == 0) *log.n_dev = n0 + carry;
}

// cn_pop_record's job table: one row per member in device memory, written once by cn_pop_record_create
struct CnPopRecordJob {
    cn_replay_ring ring;
    cn_episode_log log;
    const char* state; int64_t state_stride;      // the member's environment records, or NULL: then counters / last_return
    const int32_t* counters; const float* last_return;
    float* prev; const float *obs, *action, *reward;
    const uint8_t* done;
    uint8_t* resetting;                           // [n], the handle's
    int32_t* slot;                                // [n], the handle's
    int32_t n, reserved;
};
