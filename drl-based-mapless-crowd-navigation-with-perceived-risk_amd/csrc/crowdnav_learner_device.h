// crowdnav_learner_device.h -- device code that more than one unit of the fused learners uses (gfx950): the MFMA operand vectors and
// their edge loads (the GEMM kernels, crowdnav_gemm.hip; the act kernels of crowdnav_dqn.hip and crowdnav_sac.hip), the 16-row layer
// those two act kernels share, the soft update, and the replay-row draw (td3_prep_kernel, dqn_prep_kernel, cn_replay_indices_kernel;
// over the union of a population's rings: td3_prep_shared_kernel, cn_replay_shared_kernel).
// Everything here is __device__ __forceinline__: no kernel is defined in a header.  A header of its own rather than part of
// crowdnav_device.h: the step kernels' units include that one and keep compiling from unchanged text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crowdnav.h"
#include "crowdnav_device.h"

typedef float f32x4_t __attribute__((ext_vector_type(4)));
// target <- target (1 - tau) + local tau (TD3:297-299)
__device__ __forceinline__ float td3_soft(float target, float local, float tau) { return target * (1.f - tau) + local * tau; }

// vectors that are only 4-byte aligned (a row of 398 floats starts on an 8-byte boundary at best): global_load_dwordx2 / x4
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2u_t __attribute__((ext_vector_type(2), aligned(4)));
typedef float f32x4u_t __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ f32x4_t td3_ld4(const float* __restrict__ p, int c, int n)     // p[c .. c + 3], zero at and past n
{
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (c < n) v[0] = p[c];
    if (c + 1 < n) v[1] = p[c + 1];
    if (c + 2 < n) v[2] = p[c + 2];
    if (c + 3 < n) v[3] = p[c + 3];
    return v;
}
__device__ __forceinline__ f32x2_t td3_ld2(const float* __restrict__ p, int c, int n)
{
    f32x2_t v = {0.f, 0.f};
    if (c < n) v[0] = p[c];
    if (c + 1 < n) v[1] = p[c + 1];
    return v;
}
#define TD3_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
// MFMA 16x16x4 operand / result layout, lane l: a = A[row l & 15][k l >> 4], b = B[k l >> 4][col l & 15], acc[q] = C[row 4 (l >> 4) + q][col l & 15]

// out[r][n] = relu(sum_k A[r][k] W[n][k] + b[n]) for the workgroup's 16 rows, units n < Hp (zero from H on); lane (li, lk) feeds
// A[li][16 t + 4 lk + e] and W[n0 + li][the same k] to MFMA e of block t, as td3_fwd_kernel does
__device__ __forceinline__ void dqn_act_layer(const float* arow, int K, const float* __restrict__ W, const float* __restrict__ b, int H,
                                              float* out, int Hp, int wave, int li, int lk)
{
    const int nb = (K + 15) >> 4;
    for (int nt = wave; nt < (Hp >> 4); nt += 4) {
        const int n0 = nt * 16;
        const float* __restrict__ wrow = W + (size_t)min(n0 + li, H - 1) * K;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        const int nfull = K >> 4;
        // full blocks of 16 inputs, 8 in flight (the loads of a block do not wait for the MFMAs of the one before), then the ragged one
        for (int t0 = 0; t0 < nfull; t0 += 8) {
            f32x4_t av[8], bv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = 16 * min(t0 + u, nfull - 1) + 4 * lk;          // (past the end: loaded, not used)
                av[u] = *(const f32x4u_t*)(arow + k); bv[u] = *(const f32x4u_t*)(wrow + k);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (t0 + u < nfull) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = TD3_MFMA(av[u][e], bv[u][e], acc);
                }
        }
        if (nfull < nb) {
            const int k = 16 * nfull + 4 * lk;
            const f32x4_t av = td3_ld4(arow, k, K), bv = td3_ld4(wrow, k, K);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = TD3_MFMA(av[e], bv[e], acc);
        }
        const int nn = n0 + li;
        const float bias = nn < H ? b[nn] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(4 * lk + q) * Hp + nn] = nn < H ? fmaxf(acc[q] + bias, 0.f) : 0.f;
    }
}

// Replay sampling WITHOUT replacement (CN_SAMPLE_DISTINCT; the statement is in include/crowdnav.h next to cn_td3_batch_dev): row m of
// update `cnt` is a keyed bijection of [0, n) evaluated at m mod n -- a four-round Feistel network on Z_a x Z_b (a = ceil(sqrt n),
// b = ceil(n / a)), walked along its cycle until it lands below n.  Nothing here depends on another row, and with a workgroup-uniform
// m every value is uniform.  Sums are exact: (L + h) mod a is taken as (L + h mod a) mod a, never wrapped at 2^64 first (a wrapped
// sum would not be a rotation of Z_a).  n >= 1; a <= 3037000500, so t * t, a * b and L * b + R stay below 2^64.
__device__ __forceinline__ uint64_t cn_replay_row_distinct(uint64_t seed, uint64_t cnt, uint64_t m, uint64_t n)
{
    uint64_t r = 0;                                // floor(sqrt(n - 1)), bit by bit: a = r + 1 is the least integer with a * a >= n
    for (uint64_t bit = 1ull << 31; bit; bit >>= 1) { const uint64_t t = r | bit; if (t * t <= n - 1) r = t; }
    const uint64_t a = r + 1, b = (n + a - 1) / a;
    const uint64_t K = cn_mix64(seed ^ cn_mix64(cnt ^ 0x9E3779B97F4A7C15ull));
    const uint64_t k0 = cn_mix64(K ^ 1ull), k1 = cn_mix64(K ^ 2ull), k2 = cn_mix64(K ^ 3ull), k3 = cn_mix64(K ^ 4ull);
    uint64_t x = m % n;
    for (int pass = 0; pass < 64; ++pass) {
        uint64_t L = x / b, R = x % b;
        L += cn_mix64(k0 ^ R) % a; if (L >= a) L -= a;
        R += cn_mix64(k1 ^ L) % b; if (R >= b) R -= b;
        L += cn_mix64(k2 ^ R) % a; if (L >= a) L -= a;
        R += cn_mix64(k3 ^ L) % b; if (R >= b) R -= b;
        x = L * b + R;
        if (x < n) return x;
    }
    return x % n;                                  // (never expected: a pass lands at or above n with probability <= 1/4)
}
// row of batch row m of update `cnt` among `size` >= 1 live rows: the draw with replacement, or the bijection above (mode: the
// handle's, CN_SAMPLE_*)
__device__ __forceinline__ size_t cn_replay_row_of(uint64_t seed, unsigned long long cnt, int m, unsigned long long size, int mode)
{
    if (mode == CN_SAMPLE_DISTINCT) return (size_t)cn_replay_row_distinct(seed, cnt, (uint64_t)(uint32_t)m, size);
    return (size_t)(cn_mix64(cn_mix64(seed ^ cn_mix64(cnt)) ^ (uint64_t)(uint32_t)m) % size);
}
// ... of one ring, whose live size is read here
__device__ __forceinline__ size_t cn_replay_row(uint64_t seed, unsigned long long cnt, int m, const int64_t* size_dev, int mode)
{
    const unsigned long long size = (unsigned long long)(*size_dev > 0 ? *size_dev : 1);
    return cn_replay_row_of(seed, cnt, m, size, mode);
}

// The shared replay source (CN_REPLAY_SHARED; the statement is in include/crowdnav.h next to cn_td3_pop_update): batch row m of member
// `self` is drawn from the union of P <= 64 rings laid end to end.  ONE whole wavefront calls this, lane q holding n = ring q's live
// size (0 for a negative size and in the lanes at and above P).  The prefix sums are a shuffle scan (integers: the order is free), the
// total leaves the vector registers so that the draw stays wavefront-uniform, a ballot finds the ring.  Every lane returns the same
// {ring, row}.  (Lanes at and above P hold the total as their prefix: they pass the test only when a lane below P does.)
struct CnSharedRow { int ring; unsigned long long row; };
__device__ __forceinline__ CnSharedRow cn_replay_row_shared(uint64_t seed, unsigned long long cnt, int m, unsigned long long n, int P, int self, int mode)
{
    const int lane = (int)(threadIdx.x & 63u);
    unsigned long long incl = n;                   // pre_{lane + 1}
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, (unsigned)d, 64);
        if (lane >= d) incl += up;
    }
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(incl & 0xffffffffull), P - 1);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(incl >> 32), P - 1);
    const unsigned long long total = ((unsigned long long)hi << 32) | lo;
    const unsigned long long x = cn_replay_row_of(seed, cnt, m, total > 0 ? total : 1ull, mode);
    const unsigned long long below = __ballot(x < incl);
    CnSharedRow out = {self, 0ull};                // every ring empty
    if (below) {
        out.ring = __ffsll((long long)below) - 1;
        out.row = x - __shfl(incl - n, out.ring, 64);
    }
    return out;
}
