// crowdnav_state.hip -- a fused learner's whole state as one blob in device memory, out and in by ONE launch each (gfx950).
//
// The statement and the blob's layout: include/crowdnav.h (cn_td3_state_*, cn_td3_pop_state_*).  What a handle's state IS comes from
// the unit that owns the handle, as a list of live tensors in segment order (crowdnav_state.h: StateView); this file lays the blob
// out from that list, keeps the header and the directory as a device image, and flattens list and image into a table of jobs, a
// workgroup each: at most CHUNK words copied between a live address and an offset into the caller's blob.  The table is built once
// per handle, on first use; a save or a load is then one launch of state_copy_kernel over it, whatever the number of members.
//   save   image -> blob (header, directory); every segment -> blob, the padding behind it zeroed; a population's hyper-parameters
//          from the first place the update reads each of them
//   load   every segment <- blob; each hyper-parameter to EVERY place the update reads it
// One launch rather than one per tensor: a member has 77 segments, most of them a few hundred bytes (biases, the tick's scalars), so
// per-tensor copies are launch-bound (P = 8: 616 launches), and one launch is also what makes the save one graph node at one point of
// the stream.  The copy's body is td3_pbt_copy_kernel's (crowdnav_td3.hip): 16-byte accesses where source and destination reach a
// 16-byte boundary together, single words before, after and otherwise.  No job's destination overlaps another's.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/crowdnav.h"
#include "crowdnav_learner.h"
#include "crowdnav_state.h"

namespace {
enum { CHUNK = 4096 };                             // words per job: four 16-byte accesses per thread of a 256-thread workgroup
enum { DIR_SAVE = 1, DIR_LOAD = 2 };
struct StateJob {
    char* live;                                    // the handle's side
    uint64_t off;                                  // the blob's side, from its start
    uint32_t words;                                // <= CHUNK
    uint32_t zero;                                 // save: words of padding to zero behind the copy (the last piece of a segment)
    uint32_t dirs;                                 // DIR_SAVE | DIR_LOAD: when this job runs
    uint32_t reserved;
};
size_t round16(size_t x) { return (x + 15) / 16 * 16; }
}  // namespace

struct StateTable {
    int device = 0, njobs = 0;
    void* dev = nullptr;                           // one allocation: the image, then the jobs
    const StateJob* jobs = nullptr;
    std::vector<char> image;                       // header + directory, as a save writes them and a load expects them
    std::vector<const void*> live;                 // per segment
    size_t total = 0;
};
void state_table_free(StateTable* t)
{
    if (!t) return;
    if (t->dev) { DeviceScope scope(t->device); (void)hipFree(t->dev); }
    delete t;
}

// grid (jobs) x 256.  load = 0: live -> blob; 1: blob -> live.
__global__ __launch_bounds__(256) void state_copy_kernel(const StateJob* jobs, char* blob, int load)
{
    const StateJob j = jobs[blockIdx.x];
    if (!(j.dirs & (load ? DIR_LOAD : DIR_SAVE))) return;
    float* lp = (float*)j.live;
    float* bp = (float*)(blob + j.off);
    const float* sp = load ? bp : lp;
    float* dp = load ? lp : bp;
    const size_t n = j.words, tid = threadIdx.x, stride = 256;
    const uintptr_t sa = (uintptr_t)sp, da = (uintptr_t)dp;
    size_t head = n;
    if (((sa ^ da) & 15) == 0) head = std::min(n, (size_t)(((16 - (sa & 15)) & 15) / 4));
    const size_t n4 = (n - head) / 4;
    for (size_t i = tid; i < head; i += stride) dp[i] = sp[i];
    const float4* s4 = (const float4*)(sp + head);
    float4* d4 = (float4*)(dp + head);
    for (size_t i = tid; i < n4; i += stride) d4[i] = s4[i];
    for (size_t i = head + 4 * n4 + tid; i < n; i += stride) dp[i] = sp[i];
    if (!load) for (size_t i = tid; i < j.zero; i += stride) dp[n + i] = 0.f;
}

namespace {
// The handle's table, built on first use.  Null on an error (text in cn_td3_last_error).
template <class Hd, class View>
StateTable* state_table(const char* fn, Hd h, View view)
{
    StateView v;
    view(h, false, v);
    if (*v.table) return *v.table;
    const std::string f(fn);
    view(h, true, v);
    std::unique_ptr<StateTable> t(new (std::nothrow) StateTable());
    if (!t) { td3_fail(CN_ERR_ARG, f + ": out of memory"); return nullptr; }
    t->device = v.device;
    const size_t nseg = v.seg.size(), image_bytes = sizeof(cn_state_header) + nseg * sizeof(cn_state_segment);
    static_assert(sizeof(cn_state_header) % 16 == 0 && sizeof(cn_state_segment) % 16 == 0, "the payload starts on a 16-byte boundary");
    t->image.assign(image_bytes, 0);
    cn_state_segment* dir = (cn_state_segment*)(t->image.data() + sizeof(cn_state_header));
    size_t off = image_bytes;
    for (size_t i = 0; i < nseg; ++i) {
        const StateSeg& s = v.seg[i];
        dir[i].member = s.member; dir[i].kind = s.kind; dir[i].index = s.index; dir[i].reserved = 0;
        dir[i].offset = off; dir[i].bytes = (uint64_t)s.words * 4;
        off += round16((size_t)s.words * 4);
        t->live.push_back(s.live);
    }
    t->total = off;
    cn_state_header* hd = (cn_state_header*)t->image.data();
    hd->magic = CN_STATE_MAGIC; hd->version = CN_STATE_VERSION; hd->family = v.family; hd->n_members = v.P; hd->obs_dim = v.obs_dim;
    hd->hidden = v.hidden; hd->batch = v.batch; hd->pbt_bound = v.pbt_bound; hd->n_segments = (int32_t)nseg; hd->total_bytes = off;
    // the jobs: the image (save only; its live side is filled in below), then the segments in pieces of CHUNK words
    std::vector<StateJob> jobs;
    auto pieces = [&](char* live, uint64_t at, size_t words, size_t bytes_padded, uint32_t dirs) {
        for (size_t w = 0; w < words; w += CHUNK) {
            const size_t n = std::min<size_t>(CHUNK, words - w);
            const bool last = w + n == words;
            jobs.push_back({live + 4 * w, at + 4 * w, (uint32_t)n, last ? (uint32_t)(bytes_padded / 4 - words) : 0u, dirs, 0u});
        }
    };
    pieces(nullptr, 0, image_bytes / 4, image_bytes, DIR_SAVE);
    const size_t image_jobs = jobs.size();
    for (size_t i = 0; i < nseg; ++i) {
        const StateSeg& s = v.seg[i];
        const size_t padded = round16((size_t)s.words * 4);
        if (s.live) { pieces((char*)s.live, dir[i].offset, s.words, padded, DIR_SAVE | DIR_LOAD); continue; }
        // a population's hyper-parameters: word k of the segment <-> the places that hold hyper-parameter k of this member
        for (int k = 0; k < (int)s.words; ++k) {
            bool first = true;
            for (const StateScatter& sc : v.scatter) {
                if (sc.member != s.member || sc.hyper != k) continue;
                const bool pad = first && k + 1 == (int)s.words;
                jobs.push_back({(char*)sc.live, dir[i].offset + 4 * (uint64_t)k, 1u, pad ? (uint32_t)(padded / 4 - s.words) : 0u,
                                (uint32_t)(first ? DIR_SAVE | DIR_LOAD : DIR_LOAD), 0u});
                first = false;
            }
            if (first) { td3_fail(CN_ERR_ARG, f + ": a hyper-parameter that no table holds"); return nullptr; }      // (never)
        }
    }
    DeviceScope scope(v.device);
    const size_t jobs_at = round16(image_bytes);
    hipError_t e = hipMalloc(&t->dev, jobs_at + jobs.size() * sizeof(StateJob));
    if (e != hipSuccess) { td3_fail(CN_ERR_HIP, f + ": hipMalloc: " + hipGetErrorString(e)); return nullptr; }
    for (size_t i = 0; i < image_jobs; ++i) jobs[i].live += (uintptr_t)t->dev;
    e = hipMemcpy(t->dev, t->image.data(), image_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)t->dev + jobs_at, jobs.data(), jobs.size() * sizeof(StateJob), hipMemcpyHostToDevice);
    if (e != hipSuccess) { td3_fail(CN_ERR_HIP, f + ": hipMemcpy: " + hipGetErrorString(e)); state_table_free(t.release()); return nullptr; }
    t->jobs = (const StateJob*)((char*)t->dev + jobs_at); t->njobs = (int)jobs.size();
    *v.table = t.release();
    return *v.table;
}

// what the blob at blob_dev says of itself against what this handle writes; nothing is written before this returns CN_OK
int check_blob(const std::string& f, const StateTable* t, const void* blob_dev, hipStream_t st)
{
    hipError_t e = hipStreamSynchronize(st);
    std::vector<char> got(t->image.size());
    if (e == hipSuccess) e = hipMemcpy(got.data(), blob_dev, got.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": reading the header: " + hipGetErrorString(e));
    const cn_state_header &a = *(const cn_state_header*)got.data(), &b = *(const cn_state_header*)t->image.data();
    if (a.magic != b.magic) return td3_fail(CN_ERR_ARG, f + ": wrong magic (not a state blob)");
    if (a.version != b.version) return td3_fail(CN_ERR_ARG, f + ": format version " + std::to_string(a.version) + ", this library reads " + std::to_string(b.version));
    const char* differs = a.family != b.family ? "family" : a.n_members != b.n_members ? "n_members" : a.obs_dim != b.obs_dim ? "obs_dim"
        : a.hidden != b.hidden ? "hidden" : a.batch != b.batch ? "batch" : a.pbt_bound != b.pbt_bound ? "pbt_bound"
        : a.n_segments != b.n_segments ? "n_segments" : a.total_bytes != b.total_bytes ? "total_bytes" : nullptr;
    if (differs) return td3_fail(CN_ERR_CONFIG, f + ": the blob's " + differs + " differs from the handle's");
    if (memcmp(got.data(), t->image.data(), got.size()) != 0) return td3_fail(CN_ERR_CONFIG, f + ": a directory entry differs from the handle's");
    return CN_OK;
}

template <class Hd, class View>
int state_move(const char* fn, Hd h, View view, void* blob_dev, size_t bytes, void* stream, int load)
{
    const std::string f(fn);
    if (!h || !blob_dev) return td3_fail(CN_ERR_ARG, f + ": null " + (h ? "blob_dev" : "handle"));
    if ((uintptr_t)blob_dev & 3) return td3_fail(CN_ERR_ARG, f + ": blob_dev must be 4-byte aligned");
    const StateTable* t = state_table(fn, h, view);
    if (!t) return CN_ERR_HIP;
    if (bytes != t->total) return td3_fail(CN_ERR_ARG, f + ": bytes = " + std::to_string(bytes) + ", this handle's state is " + std::to_string(t->total));
    DeviceScope scope(t->device);
    hipStream_t st = (hipStream_t)stream;
    if (load) if (const int rc = check_blob(f, t, blob_dev, st)) return rc;
    hipLaunchKernelGGL(state_copy_kernel, dim3(t->njobs), dim3(256), 0, st, t->jobs, (char*)blob_dev, load);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}
template <class Hd, class View>
const void* state_segment(const char* fn, Hd h, View view, int i, cn_state_segment* out)
{
    if (!h) { td3_fail(CN_ERR_ARG, std::string(fn) + ": null handle"); return nullptr; }
    const StateTable* t = state_table(fn, h, view);
    if (!t || i < 0 || (size_t)i >= t->live.size()) return nullptr;
    if (out) *out = ((const cn_state_segment*)(t->image.data() + sizeof(cn_state_header)))[i];
    return t->live[i];
}
template <class Hd, class View>
size_t state_size(const char* fn, Hd h, View view)
{
    if (!h) { td3_fail(CN_ERR_ARG, std::string(fn) + ": null handle"); return 0; }
    const StateTable* t = state_table(fn, h, view);
    return t ? t->total : 0;
}
}  // namespace

extern "C" size_t cn_td3_state_size(cn_td3_handle h) { return state_size("cn_td3_state_size", h, td3_state_view); }
extern "C" int cn_td3_state_save(cn_td3_handle h, void* blob_dev, size_t bytes, void* stream)
{
    return state_move("cn_td3_state_save", h, td3_state_view, blob_dev, bytes, stream, 0);
}
extern "C" int cn_td3_state_load(cn_td3_handle h, const void* blob_dev, size_t bytes, void* stream)
{
    return state_move("cn_td3_state_load", h, td3_state_view, const_cast<void*>(blob_dev), bytes, stream, 1);
}
extern "C" const void* cn_td3_state_segment_dev(cn_td3_handle h, int i, cn_state_segment* seg_out)
{
    return state_segment("cn_td3_state_segment_dev", h, td3_state_view, i, seg_out);
}
extern "C" size_t cn_td3_pop_state_size(cn_td3_pop_handle h) { return state_size("cn_td3_pop_state_size", h, td3_pop_state_view); }
extern "C" int cn_td3_pop_state_save(cn_td3_pop_handle h, void* blob_dev, size_t bytes, void* stream)
{
    return state_move("cn_td3_pop_state_save", h, td3_pop_state_view, blob_dev, bytes, stream, 0);
}
extern "C" int cn_td3_pop_state_load(cn_td3_pop_handle h, const void* blob_dev, size_t bytes, void* stream)
{
    return state_move("cn_td3_pop_state_load", h, td3_pop_state_view, const_cast<void*>(blob_dev), bytes, stream, 1);
}
extern "C" const void* cn_td3_pop_state_segment_dev(cn_td3_pop_handle h, int i, cn_state_segment* seg_out)
{
    return state_segment("cn_td3_pop_state_segment_dev", h, td3_pop_state_view, i, seg_out);
}
