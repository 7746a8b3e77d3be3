// crowdnav_host.h -- what the host sides of libcrowdnav.so share (host code only): the device scope, the HIP check, the environment
// handle and the environment's error channel.  The library has three error channels -- cn_last_error (crowdnav_abi.hip; the actor's
// and the population recorder's entry points report there too), cn_td3_last_error (crowdnav_gemm.hip: every fused learner's, declared in crowdnav_learner.h), cn_tab_last_error
// (crowdnav_tab.hip) -- and every entry point reports to one of them through that channel's fail function.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

#include "crowdnav_kernel.h"

// RAII: run on the handle's device even if the calling thread's current device is another one
struct DeviceScope {
    int prev = -1, want;
    explicit DeviceScope(int dev) : want(dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != want) (void)hipSetDevice(want); }
    ~DeviceScope() { if (prev >= 0 && prev != want) (void)hipSetDevice(prev); }
};

// a HIP call that must succeed: otherwise return CN_ERR_HIP through FAIL, the fail function of the caller's error channel
#define CN_HIPCHK(FAIL, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return FAIL(CN_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// the environment's error channel: the thread's cn_last_error() string (crowdnav_abi.hip); returns `code`
__attribute__((visibility("hidden"))) int fail(int code, const std::string& msg);

// an actor-tile kernel whose tile exceeds 64 KiB: its dynamic-LDS limit raised to a CU's 160 KiB on `dev` (crowdnav_actor.hip)
__attribute__((visibility("hidden"))) int allow_full_lds(const void* kernel, int dev, bool* attr_set);

struct cn_env_s {
    cn_config cfg;
    int device;
    int D, max_conf, trk_cap;
    bool wide = false;                // trk_cap > CN_MAX_TRACKS: the tracker table stays in HBM (the _wide kernels)
    int world = 0;                    // CN_W_*: this configuration's row of CN_WORLDS (crowdnav_variants.h)
    size_t lds;
    CnKParams kp;        // template with state/table pointers filled in
    double *d_lidar = nullptr, *d_poly = nullptr, *d_ped_init = nullptr, *d_ped_preset = nullptr, *d_trk = nullptr;
    double* d_ped_aux = nullptr;      // [N, P, 3] ped_mode 2: goal x, goal y, goal counter
    char* d_state = nullptr;          // N per-env records (crowdnav_kernel.h: sd | si | ped_p | ped_v | pad), `stride` bytes apart
    size_t stride;
    std::vector<double> ped_init;
    int arbitration = CN_ARB_AUTO;    // cn_set_arbitration
    int n_cus = 0;                    // compute units of `device` (CN_ARB_AUTO: fair from 2 wavefronts per SIMD = 8 x n_cus envs)
    size_t lds_shape = 0;             // dynamic LDS of the _s720 kernels (compact layout); 0 = this handle has none
    size_t pol_wave_lds = 0, pol_lds = 0;   // cn_rollout_policy: bytes between the environments' LDS working sets of a workgroup; the workgroup's total (0 = does not fit)
    int pol_envs = 0;                 // ... environments per workgroup: 16, or 8 where 16 working sets do not fit one CU's LDS
    size_t pol_act_off = 0;           // ... byte offset of the workgroup's actions (past the working sets and the actor tile)
    int64_t group_envs = 0;           // cn_set_group_envs: environments in flight together with this handle's (0 = alone)
    int x2 = -1;                      // cn_env_kernel_s360_x2 (two wavefronts per environment): -1 = by grid size, 0 / 1 = CN_X2 override
    int wpb4 = 0;                     // 4: the 360-ray step kernels run four environments per workgroup (launches of at most one round of wavefronts); 0: one
    bool shape360 = false;            // the headline shape (360 rays, 20 pedestrians, K = 8 and cn_create's sizes for it): the _s360 kernels
    bool shape720 = false;            // BASELINE configs[4] (720 rays, 100 pedestrians, K = 8): the _s720 kernels
};
