// crowdnav_pop_record.hip -- cn_pop_record (include/crowdnav.h): a population's transitions and finished episodes in two launches
// whatever the number of members -- the two kernels, then the entry points that launch them (they read an environment handle's state
// records: crowdnav_host.h; errors go to cn_last_error).  The bodies are crowdnav_record.h's, the text cn_replay_write's and
// cn_episode_log_add's kernels are made of.
// Member = blockIdx.z, its job a row of a table in device memory that cn_pop_record_create uploads once (workgroup-uniform: scalar
// loads, as cn_actor_pop_kernel's); `launch` changes with every call and travels by value.  A unit of its own, so that the units of
// the step kernels and of the learners keep their instruction streams.
#include <algorithm>
#include <memory>
#include <new>

#include "crowdnav_host.h"
#include "crowdnav_record.h"
#include "crowdnav_record_host.h"

// Launch A, grid (1, 1, P) x 1024: member z's cn_replay_slot_kernel with keep = !resetting, then its cn_episode_log_kernel with the
// same flags as `transitions`, then resetting <- done.  Thread t reads and writes the flags of rows i = t (mod 1024) only, and the
// scans end in a workgroup barrier, so the flags are read by both bodies before they are overwritten.
extern "C" __global__ void __launch_bounds__(1024) cn_pop_record_scan_kernel(const CnPopRecordJob* __restrict__ table, float launch)
{
    __shared__ int wsum[16];
    __shared__ double red[5][16];
    const CnPopRecordJob& jb = table[blockIdx.z];
    const int n = jb.n;
    if (n <= 0) return;                                        // (workgroup-uniform)
    const CnKeepNotResetting keep{jb.resetting};
    cn_replay_slot_body(keep, n, jb.ring.capacity, jb.ring.pos_dev, jb.ring.size_dev, jb.slot, wsum);
    if (jb.state) cn_episode_log_body(jb.log, jb.done, CnEpisodeFromState{jb.state, jb.state_stride}, keep, launch, n, wsum, red);
    else cn_episode_log_body(jb.log, jb.done, CnEpisodeFromArrays{jb.counters, CN_COUNTER_COLS, jb.last_return}, keep, launch, n, wsum, red);
    __syncthreads();
    const uint8_t* __restrict__ done = jb.done;
    uint8_t* resetting = jb.resetting;
    for (int i = threadIdx.x; i < n; i += 1024) resetting[i] = done[i] != 0;
}

// Launch B, grid (max n_p, 1, P) x 256: row x of member z into its slot (cn_replay_copy_kernel's body with s = prev, s2 = obs), then
// prev <- obs for that row, kept or not.  Thread t copies the columns c = t (mod 256) in both loops, so it overwrites in prev only
// what it has itself already read.
extern "C" __global__ void __launch_bounds__(256) cn_pop_record_copy_kernel(const CnPopRecordJob* __restrict__ table)
{
    const CnPopRecordJob& jb = table[blockIdx.z];
    const int i = blockIdx.x;
    if (i >= jb.n) return;                                     // (workgroup-uniform)
    cn_replay_copy_body(jb.ring, jb.prev, jb.action, jb.reward, jb.obs, jb.done, jb.slot, i);
    const int D = jb.ring.obs_dim;
    const float* __restrict__ obs = jb.obs + (size_t)i * D;
    float* prev = jb.prev + (size_t)i * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) prev[c] = obs[c];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct cn_pop_record_s {
    int device = 0, P = 0, max_n = 0;                      // max_n: the widest member's rows, launch B's grid x (0: nothing to launch)
    void* mem = nullptr;                                   // one allocation: the table, then every member's slot scratch and resetting bytes
    const CnPopRecordJob* jobs = nullptr;
    std::vector<uint8_t*> resetting;
    cn_pop_record_s() = default;
    cn_pop_record_s(const cn_pop_record_s&) = delete;
    ~cn_pop_record_s() { if (mem) { DeviceScope scope(device); (void)hipFree(mem); } }
};

extern "C" int cn_pop_record_create(const cn_pop_record_member* members, int n_members, int obs_dim, int device, cn_pop_record_handle* out)
{
    const std::string f("cn_pop_record_create");
    if (int rc = cn_record_check_call(f, members, out, n_members, obs_dim)) return rc;
    const int P = n_members;
    std::vector<CnRecordNamed> written;                    // what a launch writes, per member: no two members may share any of it
    int max_n = 0;
    for (int p = 0; p < P; ++p) {
        if (int rc = cn_record_check_member(f, members[p], p, obs_dim, 1, written)) return rc;
        max_n = std::max(max_n, (int)members[p].n);
    }
    std::unique_ptr<cn_pop_record_s> h(new (std::nothrow) cn_pop_record_s());
    if (!h) return fail(CN_ERR_ARG, f + ": out of memory");
    int dev = device;
    if (dev < 0) CN_HIPCHK(fail, hipGetDevice(&dev));
    h->device = dev; h->P = P; h->max_n = max_n;
    DeviceScope scope(dev);
    // [jobs P] rounded up to 256 bytes, then per member slot [n] int32 and resetting [n] bytes, each rounded up to 16 bytes.  The whole
    // image is made on the host and uploaded by one blocking copy: the flags are zero whatever stream the first call runs on.
    const size_t tab = (sizeof(CnPopRecordJob) * P + 255) & ~(size_t)255;
    size_t total = tab;
    std::vector<size_t> off_slot(P), off_flag(P);
    for (int p = 0; p < P; ++p) {
        off_slot[p] = total; total += (sizeof(int32_t) * (size_t)members[p].n + 15) & ~(size_t)15;
        off_flag[p] = total; total += ((size_t)members[p].n + 15) & ~(size_t)15;
    }
    CN_HIPCHK(fail, hipMalloc(&h->mem, total));
    std::vector<char> image(total, 0);
    CnPopRecordJob* hj = (CnPopRecordJob*)image.data();
    h->resetting.resize(P);
    for (int p = 0; p < P; ++p) {
        const cn_pop_record_member& m = members[p];
        CnPopRecordJob& j = hj[p];
        j.ring = m.ring; j.log = m.log;
        j.state = m.env ? m.env->d_state : nullptr; j.state_stride = m.env ? (int64_t)m.env->stride : 0;
        j.counters = m.counters; j.last_return = m.last_return;
        j.prev = m.prev; j.obs = m.obs; j.action = m.action; j.reward = m.reward; j.done = m.done;
        j.resetting = h->resetting[p] = (uint8_t*)h->mem + off_flag[p];
        j.slot = (int32_t*)((char*)h->mem + off_slot[p]);
        j.n = m.n; j.reserved = 0;
    }
    CN_HIPCHK(fail, hipMemcpy(h->mem, image.data(), total, hipMemcpyHostToDevice));
    h->jobs = (const CnPopRecordJob*)h->mem;
    *out = h.release();
    return CN_OK;
}
extern "C" void cn_pop_record_destroy(cn_pop_record_handle h) { delete h; }
extern "C" int cn_pop_record_members(cn_pop_record_handle h) { return h ? h->P : 0; }

extern "C" uint8_t* cn_pop_record_resetting(cn_pop_record_handle h, int member)
{
    if (!h) { (void)fail(CN_ERR_ARG, "cn_pop_record_resetting: null handle"); return nullptr; }
    if (member < 0 || member >= h->P) {
        (void)fail(CN_ERR_ARG, "cn_pop_record_resetting: member " + std::to_string(member) + " out of range (the handle has " + std::to_string(h->P) + ")");
        return nullptr;
    }
    return h->resetting[member];
}

extern "C" int cn_pop_record(cn_pop_record_handle h, float launch, void* stream)
{
    if (!h) return fail(CN_ERR_ARG, "cn_pop_record: null handle");
    if (h->max_n == 0) return CN_OK;
    DeviceScope scope(h->device);
    hipLaunchKernelGGL(cn_pop_record_scan_kernel, dim3(1, 1, h->P), dim3(1024), 0, (hipStream_t)stream, h->jobs, launch);
    hipLaunchKernelGGL(cn_pop_record_copy_kernel, dim3(h->max_n, 1, h->P), dim3(256), 0, (hipStream_t)stream, h->jobs);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}
