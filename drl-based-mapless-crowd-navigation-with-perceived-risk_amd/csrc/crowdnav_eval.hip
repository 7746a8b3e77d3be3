// crowdnav_eval.hip -- cn_eval_* (include/crowdnav.h): the evaluation of J jobs (one greedy actor in one world each) on the device --
// the three kernels (reset, record, finish), then the entry points that launch them (they read an environment handle's state records:
// crowdnav_host.h; errors go to cn_last_error).  The episode log's body is crowdnav_record.h's, the text cn_episode_log_add's kernel
// is made of, instantiated on the `counted` bytes: that is what makes a job's log equal the solo call bit for bit.
// Job = blockIdx.z, its row of a table in device memory that cn_eval_create uploads once (workgroup-uniform: scalar loads, as
// cn_pop_record's); `launch` changes with every call and travels by value.  No atomics: every job's outputs belong to its own
// workgroup.  A unit of its own, so that every other unit keeps its instruction stream.
#include <memory>
#include <new>

#include "crowdnav_host.h"
#include "crowdnav_record.h"

// cn_eval's job table: one row per job in device memory, written once by cn_eval_create
struct CnEvalJob {
    cn_episode_log log;
    const char* state; int64_t state_stride;      // the job's environment records, or NULL: then counters / last_return
    const int32_t* counters; const float* last_return;
    const uint8_t* done;
    int32_t* finished;                            // [n], the handle's: episodes counted per environment
    uint8_t* counted;                             // [n], the handle's scratch
    int32_t n, quota, group, reserved;
};

#define CN_EVAL_SUMS 10                           // the columns of sums[j] that receive something (10, 11 stay 0)

// grid (1, 1, J) x 1024
extern "C" __global__ void __launch_bounds__(1024) cn_eval_reset_kernel(const CnEvalJob* __restrict__ table, cn_eval_state* st)
{
    const int z = blockIdx.z;
    const CnEvalJob& jb = table[z];
    const int n = jb.n;
    int32_t* finished = jb.finished;
    for (int i = threadIdx.x; i < n; i += 1024) finished[i] = 0;
    if (threadIdx.x < CN_EVAL_COLS) st->sums[z][threadIdx.x] = 0.0;
    if (threadIdx.x < 5) jb.log.tot_dev[threadIdx.x] = 0.0;
    if (threadIdx.x == 0) { st->remaining[z] = n; *jb.log.n_dev = 0; }
}

// the ten sums of one job's counted rows, in cn_episode_log_body's order: thread-strided partials, the xor butterfly, the 16 waves
template <class Src>
__device__ __forceinline__ void cn_eval_sums_body(const uint8_t* counted, const Src src, int n, double* sums, double (*red)[16])
{
    double t[CN_EVAL_SUMS];
#pragma unroll
    for (int q = 0; q < CN_EVAL_SUMS; ++q) t[q] = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        if (!counted[i]) continue;
        const CnEpisodeRow e = src(i);
        t[0] += 1.0; t[1] += (double)e.success; t[2] += (double)e.failure;
        if (e.success == 0.f && e.failure == 0.f) t[3] += 1.0;
        t[4] += (double)e.ret; t[5] += (double)e.steps;
        if (e.obst > 0.f) {                      // a score exists only where an obstacle was present (the reference divides by zero there)
            t[6] += 1.0 - (double)e.ego / (double)e.obst;
            t[7] += 1.0 - (double)e.social / (double)e.obst;
            t[8] += 1.0;
        }
        if (e.success != 0.f) t[9] += (double)e.steps;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < CN_EVAL_SUMS; ++q) {
        double v = t[q];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) red[q][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < CN_EVAL_SUMS) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) v += red[threadIdx.x][w];
        sums[threadIdx.x] += v;
    }
}

// grid (1, 1, J) x 1024: job z's counted flags, its cn_episode_log_kernel on them, its sums, then finished += counted and remaining.
// Thread t reads and writes finished and counted of rows i = t (mod 1024) only; the barriers between the passes order the rest.
extern "C" __global__ void __launch_bounds__(1024) cn_eval_record_kernel(const CnEvalJob* __restrict__ table, cn_eval_state* st, float launch)
{
    __shared__ int wsum[16];
    __shared__ double red[CN_EVAL_SUMS][16];
    const int z = blockIdx.z;
    const CnEvalJob& jb = table[z];
    const int n = jb.n, quota = jb.quota;
    if (n <= 0 || st->remaining[z] == 0) return;               // (workgroup-uniform: remaining is written after the last barrier only)
    const uint8_t* __restrict__ done = jb.done;
    int32_t* finished = jb.finished;
    uint8_t* counted = jb.counted;
    for (int i = threadIdx.x; i < n; i += 1024) counted[i] = done[i] != 0 && finished[i] < quota;
    __syncthreads();
    const CnKeepBytes trans{counted};
    if (jb.state) {
        const CnEpisodeFromState src{jb.state, jb.state_stride};
        cn_episode_log_body(jb.log, counted, src, trans, launch, n, wsum, red);
        __syncthreads();                                       // the log's totals were read from red
        cn_eval_sums_body(counted, src, n, st->sums[z], red);
    } else {
        const CnEpisodeFromArrays src{jb.counters, CN_COUNTER_COLS, jb.last_return};
        cn_episode_log_body(jb.log, counted, src, trans, launch, n, wsum, red);
        __syncthreads();
        cn_eval_sums_body(counted, src, n, st->sums[z], red);
    }
    int below = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int32_t f = finished[i] + (counted[i] != 0);
        finished[i] = f;
        below += f < quota;
    }
    int total;
    (void)cn_block_scan_1024(below, wsum, total);
    if (threadIdx.x == 0) st->remaining[z] = total;
}

// one workgroup of 64 threads: thread j the summary of job j, then thread g the fitness of group g
extern "C" __global__ void __launch_bounds__(64) cn_eval_finish_kernel(const CnEvalJob* __restrict__ table, cn_eval_state* st, int J, int G,
                                                                       int col, float* fitness_dev)
{
    __shared__ float val[CN_EVAL_MAX];
    __shared__ int grp[CN_EVAL_MAX];
    const int t = threadIdx.x;
    if (t < J) {
        const double* s = st->sums[t];
        const float out[8] = {(float)s[0], (float)(s[1] / s[0]), (float)(s[2] / s[0]), (float)(s[3] / s[0]), (float)(s[4] / s[0]),
                              (float)(s[5] / s[0]), (float)(s[6] / s[8]), (float)(s[7] / s[8])};
#pragma unroll
        for (int k = 0; k < 8; ++k) st->summary[t][k] = out[k];
        val[t] = col == 1 ? out[1] : out[4];
        grp[t] = table[t].group;
    }
    __syncthreads();
    if (t < G) {
        double acc = 0.0, cnt = 0.0;
        for (int j = 0; j < J; ++j)
            if (grp[j] == t) { acc += (double)val[j]; cnt += 1.0; }
        const float f = (float)(acc / cnt);                    // a group without jobs: 0 / 0
        st->fitness[t] = f;
        if (fitness_dev) fitness_dev[t] = f;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct cn_eval_s {
    int device = 0, J = 0, G = 0, max_n = 0;               // max_n: the widest job's rows (0: cn_eval_record has nothing to launch)
    void* mem = nullptr;                                   // one allocation: the table, the state, then every job's finished and counted
    const CnEvalJob* jobs = nullptr;
    cn_eval_state* state = nullptr;
    cn_eval_s() = default;
    cn_eval_s(const cn_eval_s&) = delete;
    ~cn_eval_s() { if (mem) { DeviceScope scope(device); (void)hipFree(mem); } }
};

extern "C" int cn_eval_create(const cn_eval_job* jobs, int n_jobs, int n_groups, int device, cn_eval_handle* out)
{
    const std::string f("cn_eval_create");
    if (!jobs) return fail(CN_ERR_ARG, f + ": jobs is null");
    if (!out) return fail(CN_ERR_ARG, f + ": out is null");
    if (n_jobs < 1 || n_jobs > CN_EVAL_MAX) return fail(CN_ERR_ARG, f + ": n_jobs must be 1 ... 64");
    if (n_groups < 1 || n_groups > CN_EVAL_MAX) return fail(CN_ERR_ARG, f + ": n_groups must be 1 ... 64");
    const int J = n_jobs;
    struct Named { const void* ptr; const char* name; int job; };
    std::vector<Named> written;                            // what a launch writes, per job: no two jobs may share any of it
    int max_n = 0;
    for (int j = 0; j < J; ++j) {
        const cn_eval_job& m = jobs[j];
        const std::string who = ": job " + std::to_string(j) + ": ";
        if (m.group < 0 || m.group >= n_groups)
            return fail(CN_ERR_ARG, f + who + "group is " + std::to_string(m.group) + ", outside 0 ... " + std::to_string(n_groups - 1));
        if (m.n < 0) return fail(CN_ERR_ARG, f + who + "n is negative");
        if (m.quota < 1) return fail(CN_ERR_ARG, f + who + "quota must be at least 1");
        if (m.n > 0) {
            if (!m.done) return fail(CN_ERR_ARG, f + who + "done is null");
            if (!m.env && !(m.counters && m.last_return))
                return fail(CN_ERR_ARG, f + who + "neither env nor both counters and last_return are given");
        }
        if (m.env && m.n != m.env->cfg.n_envs)
            return fail(CN_ERR_ARG, f + who + "n is " + std::to_string(m.n) + " but env has n_envs " + std::to_string(m.env->cfg.n_envs));
        if (!m.log.rows || !m.log.n_dev || !m.log.tot_dev) return fail(CN_ERR_ARG, f + who + "incomplete log");
        if (m.log.max_rows < 0) return fail(CN_ERR_ARG, f + who + "log.max_rows is negative");
        const Named mine[3] = {{m.log.rows, "log.rows", j}, {m.log.n_dev, "log.n_dev", j}, {m.log.tot_dev, "log.tot_dev", j}};
        for (const Named& x : mine)
            for (const Named& y : written)
                if (y.ptr == x.ptr)
                    return fail(CN_ERR_CONFIG, f + who + x.name + " is also job " + std::to_string(y.job) + "'s " + y.name +
                                               " (they would race inside a launch)");
        written.insert(written.end(), mine, mine + 3);
        if (m.n > max_n) max_n = m.n;
    }
    std::unique_ptr<cn_eval_s> h(new (std::nothrow) cn_eval_s());
    if (!h) return fail(CN_ERR_ARG, f + ": out of memory");
    int dev = device;
    if (dev < 0) CN_HIPCHK(fail, hipGetDevice(&dev));
    h->device = dev; h->J = J; h->G = n_groups; h->max_n = max_n;
    DeviceScope scope(dev);
    // [jobs J] and [state], each rounded up to 256 bytes, then per job finished [n] int32 and counted [n] bytes, each rounded up to 16
    // bytes.  The whole image is made on the host and uploaded by one blocking copy: the state is what cn_eval_reset leaves whatever
    // stream the first call runs on.
    const size_t tab = (sizeof(CnEvalJob) * J + 255) & ~(size_t)255;
    const size_t sta = (sizeof(cn_eval_state) + 255) & ~(size_t)255;
    size_t total = tab + sta;
    std::vector<size_t> off_fin(J), off_cnt(J);
    for (int j = 0; j < J; ++j) {
        off_fin[j] = total; total += (sizeof(int32_t) * (size_t)jobs[j].n + 15) & ~(size_t)15;
        off_cnt[j] = total; total += ((size_t)jobs[j].n + 15) & ~(size_t)15;
    }
    CN_HIPCHK(fail, hipMalloc(&h->mem, total));
    std::vector<char> image(total, 0);
    CnEvalJob* hj = (CnEvalJob*)image.data();
    cn_eval_state* hs = (cn_eval_state*)(image.data() + tab);
    for (int j = 0; j < J; ++j) {
        const cn_eval_job& m = jobs[j];
        CnEvalJob& d = hj[j];
        d.log = m.log;
        d.state = m.env ? m.env->d_state : nullptr; d.state_stride = m.env ? (int64_t)m.env->stride : 0;
        d.counters = m.counters; d.last_return = m.last_return; d.done = m.done;
        d.finished = (int32_t*)((char*)h->mem + off_fin[j]);
        d.counted = (uint8_t*)h->mem + off_cnt[j];
        d.n = m.n; d.quota = m.quota; d.group = m.group; d.reserved = 0;
        hs->remaining[j] = m.n;
    }
    CN_HIPCHK(fail, hipMemcpy(h->mem, image.data(), total, hipMemcpyHostToDevice));
    h->jobs = (const CnEvalJob*)h->mem;
    h->state = (cn_eval_state*)((char*)h->mem + tab);
    *out = h.release();
    return CN_OK;
}
extern "C" void cn_eval_destroy(cn_eval_handle h) { delete h; }
extern "C" int cn_eval_jobs(cn_eval_handle h) { return h ? h->J : 0; }
extern "C" const cn_eval_state* cn_eval_state_dev(cn_eval_handle h) { return h ? h->state : nullptr; }

extern "C" int cn_eval_reset(cn_eval_handle h, void* stream)
{
    if (!h) return fail(CN_ERR_ARG, "cn_eval_reset: null handle");
    DeviceScope scope(h->device);
    hipLaunchKernelGGL(cn_eval_reset_kernel, dim3(1, 1, h->J), dim3(1024), 0, (hipStream_t)stream, h->jobs, h->state);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_eval_record(cn_eval_handle h, float launch, void* stream)
{
    if (!h) return fail(CN_ERR_ARG, "cn_eval_record: null handle");
    if (h->max_n == 0) return CN_OK;
    DeviceScope scope(h->device);
    hipLaunchKernelGGL(cn_eval_record_kernel, dim3(1, 1, h->J), dim3(1024), 0, (hipStream_t)stream, h->jobs, h->state, launch);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_eval_finish(cn_eval_handle h, int metric, float* fitness_dev, void* stream)
{
    if (!h) return fail(CN_ERR_ARG, "cn_eval_finish: null handle");
    if (metric != CN_EVAL_SUCCESS_RATE && metric != CN_EVAL_MEAN_RETURN)
        return fail(CN_ERR_ARG, "cn_eval_finish: metric is " + std::to_string(metric) + ", neither CN_EVAL_SUCCESS_RATE (0) nor CN_EVAL_MEAN_RETURN (1)");
    DeviceScope scope(h->device);
    hipLaunchKernelGGL(cn_eval_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, h->jobs, h->state, h->J, h->G,
                       metric == CN_EVAL_SUCCESS_RATE ? 1 : 4, fitness_dev);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}
