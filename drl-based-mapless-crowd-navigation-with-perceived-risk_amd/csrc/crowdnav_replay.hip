// crowdnav_replay.hip -- the collection loop's bookkeeping for one learner, and the replay draw without an update: cn_replay_write,
// cn_episode_log_add, cn_replay_sample_indices, cn_replay_sample_shared (include/crowdnav.h): five small kernels and their entry points.  Errors go to
// the learners' channel (cn_td3_last_error, crowdnav_learner.h).  The bodies of the write and log kernels are crowdnav_record.h's,
// shared with cn_pop_record's kernels (crowdnav_pop_record.hip) so that both are the same text; the row draw is
// crowdnav_learner_device.h's, the one td3_prep_kernel and dqn_prep_kernel gather by.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crowdnav.h"
#include "crowdnav_learner.h"
#include "crowdnav_learner_device.h"
#include "crowdnav_record.h"

namespace {
// the rows an update with (seed, counter, mode) gathers, without the update: cn_replay_sample_indices
__global__ void __launch_bounds__(256) cn_replay_indices_kernel(uint64_t seed, unsigned long long cnt, int B, const int64_t* size_dev, int mode,
                                                                int64_t* __restrict__ rows)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < B) rows[m] = (int64_t)cn_replay_row(seed, cnt, m, size_dev, mode);
}
// ... and the {ring, row} pairs a shared update of member `self` would gather: cn_replay_sample_shared.  One wavefront per batch row,
// lane q reading ring q's live size, as the first wavefront of td3_prep_shared_kernel does.
__global__ void __launch_bounds__(64) cn_replay_shared_kernel(uint64_t seed, unsigned long long cnt, const int64_t* const* __restrict__ size_dev,
                                                              int P, int self, int mode, int64_t* __restrict__ rows)
{
    const int m = blockIdx.x, lane = threadIdx.x;
    unsigned long long n = 0;
    if (lane < P) { const int64_t live = *size_dev[lane]; n = live > 0 ? (unsigned long long)live : 0ull; }
    const CnSharedRow at = cn_replay_row_shared(seed, cnt, m, n, P, self, mode);
    if (lane == 0) { rows[2 * (size_t)m] = (int64_t)at.ring; rows[2 * (size_t)m + 1] = (int64_t)at.row; }
}
__global__ void __launch_bounds__(1024) cn_replay_slot_kernel(const uint8_t* __restrict__ keep, int n, int64_t cap, int64_t* pos_dev,
                                                              int64_t* size_dev, int32_t* __restrict__ slot)
{
    __shared__ int wsum[16];
    cn_replay_slot_body(CnKeepBytes{keep}, n, cap, pos_dev, size_dev, slot, wsum);
}
struct ReplayCopyArgs { cn_replay_ring ring; const float *s, *a, *r, *s2; const uint8_t* done; const int32_t* slot; };
__global__ void __launch_bounds__(256) cn_replay_copy_kernel(ReplayCopyArgs p)
{
    cn_replay_copy_body(p.ring, p.s, p.a, p.r, p.s2, p.done, p.slot, blockIdx.x);
}
// the finished episodes' rows and the running totals, one workgroup
struct EpisodeLogArgs { cn_episode_log log; const uint8_t* done; const int32_t* counters; int cols; const float* ret; const uint8_t* trans; float launch; int n; };
__global__ void __launch_bounds__(1024) cn_episode_log_kernel(EpisodeLogArgs p)
{
    __shared__ int wsum[16];
    __shared__ double red[5][16];
    cn_episode_log_body(p.log, p.done, CnEpisodeFromArrays{p.counters, p.cols, p.ret}, CnKeepBytes{p.trans}, p.launch, p.n, wsum, red);
}
}  // namespace

extern "C" int cn_replay_sample_indices(uint64_t seed, uint64_t counter, int B, const int64_t* size_dev, int mode, int64_t* rows_dev,
                                        int device, void* stream)
{
    if (!size_dev || !rows_dev) return td3_fail(CN_ERR_ARG, "cn_replay_sample_indices: null argument");
    if (B < 1) return td3_fail(CN_ERR_ARG, "cn_replay_sample_indices: B < 1");
    if (mode != CN_SAMPLE_WITH_REPLACEMENT && mode != CN_SAMPLE_DISTINCT)
        return td3_fail(CN_ERR_ARG, "cn_replay_sample_indices: mode must be CN_SAMPLE_WITH_REPLACEMENT (0) or CN_SAMPLE_DISTINCT (1)");
    DeviceScope scope(device);
    hipLaunchKernelGGL(cn_replay_indices_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, (unsigned long long)counter, B,
                       size_dev, mode, rows_dev);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_replay_sample_shared(uint64_t seed, uint64_t counter, int B, const int64_t* const* size_dev_table, int P, int self, int mode,
                                       int64_t* rows_dev, int device, void* stream)
{
    if (!size_dev_table || !rows_dev) return td3_fail(CN_ERR_ARG, "cn_replay_sample_shared: null argument");
    if (B < 1) return td3_fail(CN_ERR_ARG, "cn_replay_sample_shared: B < 1");
    if (P < 1 || P > 64) return td3_fail(CN_ERR_ARG, "cn_replay_sample_shared: P must be 1 ... 64");
    if (self < 0 || self >= P) return td3_fail(CN_ERR_ARG, "cn_replay_sample_shared: self must be 0 ... P - 1");
    if (mode != CN_SAMPLE_WITH_REPLACEMENT && mode != CN_SAMPLE_DISTINCT)
        return td3_fail(CN_ERR_ARG, "cn_replay_sample_shared: mode must be CN_SAMPLE_WITH_REPLACEMENT (0) or CN_SAMPLE_DISTINCT (1)");
    DeviceScope scope(device);
    hipLaunchKernelGGL(cn_replay_shared_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, seed, (unsigned long long)counter, size_dev_table, P, self,
                       mode, rows_dev);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_replay_write(const cn_replay_ring* ring, const float* s, const float* a, const float* r, const float* s2,
                               const uint8_t* done, const uint8_t* keep, int n, int32_t* slot_scratch, int device, void* stream)
{
    if (!ring || !s || !a || !r || !s2 || !done || !slot_scratch) return td3_fail(CN_ERR_ARG, "cn_replay_write: null argument");
    if (!ring->s || !ring->a || !ring->r || !ring->s2 || !ring->d || !ring->pos_dev || !ring->size_dev || ring->capacity < 1 || ring->obs_dim < 1)
        return td3_fail(CN_ERR_ARG, "cn_replay_write: incomplete ring");
    if (n < 1) return td3_fail(CN_ERR_ARG, "cn_replay_write: n < 1");
    if ((int64_t)n > ring->capacity) return td3_fail(CN_ERR_ARG, "cn_replay_write: more rows than the ring holds (two rows of one call would share a slot)");
    DeviceScope scope(device);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cn_replay_slot_kernel, dim3(1), dim3(1024), 0, st, keep, n, ring->capacity, ring->pos_dev, ring->size_dev, slot_scratch);
    ReplayCopyArgs ca;
    ca.ring = *ring; ca.s = s; ca.a = a; ca.r = r; ca.s2 = s2; ca.done = done; ca.slot = slot_scratch;
    hipLaunchKernelGGL(cn_replay_copy_kernel, dim3(n), dim3(256), 0, st, ca);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_episode_log_add(const cn_episode_log* log, const uint8_t* done, const int32_t* counters, int counter_cols,
                                  const float* last_return, const uint8_t* transitions, float launch, int n, int device, void* stream)
{
    if (!log || !log->rows || !log->n_dev || !log->tot_dev || !done || !counters || !last_return || !transitions)
        return td3_fail(CN_ERR_ARG, "cn_episode_log_add: null argument");
    if (n < 1 || counter_cols < 14 || log->max_rows < 0) return td3_fail(CN_ERR_ARG, "cn_episode_log_add: n < 1, fewer than 14 counter columns or max_rows < 0");
    DeviceScope scope(device);
    EpisodeLogArgs ea;
    ea.log = *log; ea.done = done; ea.counters = counters; ea.cols = counter_cols; ea.ret = last_return; ea.trans = transitions; ea.launch = launch; ea.n = n;
    hipLaunchKernelGGL(cn_episode_log_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ea);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}
