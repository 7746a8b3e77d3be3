// crowdnav_pop_record.hip -- the kernels of cn_pop_record (include/crowdnav.h): a population's transitions and finished episodes in
// two launches whatever the number of members.  The entry points are in crowdnav_abi.hip (they know an environment handle's state
// records); the bodies are crowdnav_record.h's, the text cn_replay_write's and cn_episode_log_add's kernels are made of.
// Member = blockIdx.z, its job a row of a table in device memory that cn_pop_record_create uploads once (workgroup-uniform: scalar
// loads, as cn_actor_pop_kernel's); `launch` changes with every call and travels by value.  A unit of its own, so that the units of
// the step kernels and of the learners keep their instruction streams.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crowdnav_record.h"

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
