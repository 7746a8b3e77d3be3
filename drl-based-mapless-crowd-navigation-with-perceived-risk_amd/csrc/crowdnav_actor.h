// crowdnav_actor.h -- the fused TD3 actor's tile (device code): 3 x Linear(256) + ReLU + output stage in ONE launch (the caller of
// the hot path, A33).  Shared by crowdnav_actor.hip (cn_actor_kernel, cn_actor_pop_kernel), the policy kernels of
// crowdnav_kernel.hip (cn_rollout_policy; units 2, 4 and 5) and crowdnav_ddpg.hip (cn_ddpg_act_kernel: the tile with DDPG's noise).
#pragma once
#include <type_traits>
#include "crowdnav_device.h"

// Actor.forward (TD3:96-106) + Agent.act's noise and clip (TD3:209-215) for a tile of 16 environments per workgroup,
// on the f32-input matrix cores: v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain, same precision as the
// reference's fp32 PyTorch actor).  Lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15].
// Round 3: every wave runs the FULL K range of its own 256 / NW columns (NW = 8 waves: two interleaved column tiles per wave,
// col = 32 wave + 2 j + t, one 8-byte load of the K-major weights feeds both MFMAs), so there are no K-split partial sums
// to park in LDS and re-add: the tile needs X [16][Dp + 1] and one hidden buffer [16][257] -- 42 KB instead of 108 KB, 512
// threads instead of 1024 -- which is what lets an actor workgroup sit on a CU NEXT TO a dozen environment wavefronts
// (rollout_groups: one group's actor overlaps the others' env steps; before, it had to wait for 108 KB of LDS to drain).
// Activations never leave LDS; weights stream from L2 (670 KB, shared by all tiles).
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define ACT_H 256
#define ACT_M 16
#define ACT_THREADS 512            /* cn_actor_kernel: 8 waves */
// A tile's LDS: X [16][Dp + 1] (layer 2 reuses it), then H [16][257].  actor_tile carves it with these leading dimensions and every
// launch asks for actor_tile_bytes (in size_t: an observation too wide for a tile is refused, not wrapped).
#define ACT_LDX(Dp) ((Dp) + 1)
#define ACT_LDH (ACT_H + 1)
__host__ __device__ constexpr size_t actor_tile_bytes(size_t Dp) { return sizeof(float) * ACT_M * (ACT_LDX(Dp) + ACT_LDH); }

// Weights arrive PACKED in the order the matrix cores consume them (cn_actor_pack_kernel, crowdnav_actor.hip): for a
// layer with K inputs (a multiple of 32) and 256 outputs, block b = 8 k-steps of 4, wave w = 32 columns, q = a pair of k-steps,
//   P[((((b 8 + w) 4 + q) 64 + lane) 4 + j] = W^T[k = 32 b + 4 (2 q + (j >> 1)) + (lane >> 4)][c = 32 w + 2 (lane & 15) + (j & 1)]
// so a lane's operands for one block are FOUR 16-byte loads 1 KB apart and a wave's are 4 KB contiguous.  With the K-major
// layout the same operands were eight 8-byte loads (16 lanes x 8 B on each of 4 rows per instruction); tools/micro/l2_stream.hip:
// a workgroup streaming a shared 688 KB array out of L2 gets 70-73 GB/s with global_load_dwordx2 and 114-139 GB/s with
// dwordx4 -- and the tile's two layers ran at exactly that dwordx2 pace (19.5 B/clk per CU in both), whatever the prefetch depth.
#define ACT_U 8                    /* k-steps per pipelined block */
struct ActW { float4 v[ACT_U / 2]; };
// A lane's operands of block `blk`: uniform base (SGPR pair, advanced per block on the scalar unit) + this lane's 32-bit
// offset + an immediate -- global_load_dwordx4 v, v_off, s[base] offset:1024 i -- so the loop has no 64-bit vector address
// arithmetic (with a per-lane pointer every load cost a v_add_co / v_addc pair and their s_nop).
struct ActWPtr { const float4* base; unsigned off; };
__device__ __forceinline__ void actor_wload(ActW& w, const ActWPtr bp, int blk)
{
    const float4* q = bp.base + (size_t)blk * (8 * 4 * 64);
#pragma unroll
    for (int i = 0; i < ACT_U / 2; ++i) w.v[i] = q[bp.off + (unsigned)(i * 64)];
}
__device__ __forceinline__ ActWPtr actor_wptr(const float* __restrict__ WP, int wave, int lane)
{
    return ActWPtr{reinterpret_cast<const float4*>(WP) + (size_t)wave * (4 * 64), (unsigned)lane};
}

// One layer for this wave's 32 columns (two interleaved 16-column tiles: col = 32 wave + 2 j + t):
// out[r][c] = relu(sum_k A[r][k] W^T[k][c] + bias[c]), K a multiple of 32, k ascending.  `first`: the weights of block 0,
// requested by the caller BEFORE the barrier that releases A (their L2 round trip overlaps the staging / the previous layer's
// tail).  The loop keeps the NEXT block -- its weights from L2 AND its A operands from LDS -- in flight while this block's 16
// MFMAs issue, and its body is BRANCH-FREE on purpose: with `if (blk + 2 < nblk) load` in it the compiler's s_waitcnt counting
// merged the "loaded" and "not loaded" paths and waited for the block it had just requested.  The last pair re-requests the
// final block instead (clamped, never skipped).
struct ActA { float a[ACT_U]; };
__device__ __forceinline__ void actor_aload(ActA& x, const float* ap, int k0)
{
#pragma unroll
    for (int u = 0; u < ACT_U; ++u) x.a[u] = ap[k0 + 4 * u];
}
// FINAL (the second hidden layer): the activations are not written back -- linear3 (TD3:101) is folded into the epilogue: every
// lane multiplies its 4 rows x 2 columns of relu(h2) by linear3's weights of those columns, a DPP scan sums the 16 lanes
// (= 32 columns) of each row group, and lane 15 of the group leaves the wave's partial logits in out[(wave 16 + row) 2 + o];
// the caller adds the eight waves in wave order.  (Before: 16 x 256 activations through LDS, a barrier, 8 k LDS reads.)
__device__ __forceinline__ float actor_row_sum(float v)      // inclusive scan over the 16 lanes of a DPP row: lane 15 = the sum
{
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false));   // row_shr:1
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, false));   // row_shr:2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, false));   // row_shr:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, false));   // row_shr:8
    return v;
}
template <bool FINAL = false>
__device__ __forceinline__ void actor_layer(const float* __restrict__ A, int lda, int K, const float* __restrict__ WP,
                                            const float* __restrict__ bias, float* __restrict__ out, int ldo, int wave, int lane,
                                            const ActW& first, const float* __restrict__ W3 = nullptr)
{
    const int ai = lane & 15, ak = lane >> 4;
    const int colb = 32 * wave + 2 * ai;
    float w3[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (FINAL) { w3[0] = W3[colb]; w3[1] = W3[colb + 1]; w3[2] = W3[ACT_H + colb]; w3[3] = W3[ACT_H + colb + 1]; }
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    const float* ap = A + ai * lda + ak;
    const ActWPtr bp = actor_wptr(WP, wave, lane);
    // two register blocks, ping-pong: block b's MFMAs run on one while the other receives block b + 1 (a copy `cur = nxt` at the
    // end of an iteration would wait for the loads it is supposed to hide).  The scheduling barriers keep the compiler from
    // sinking the loads below the MFMAs.  (A ring of four blocks, three requests ahead, measured the same 17.5 us: layer 1 7 %
    // faster, layer 2 10 % slower for its longer ramp -- the loads are not latency-bound any more.)
    ActW w0 = first, w1;
    ActA a0, a1;
    const int nblk = K / (4 * ACT_U);
    auto mma = [&](const ActW& w, const ActA& x) {
#pragma unroll
        for (int i = 0; i < ACT_U / 2; ++i) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.a[2 * i], w.v[i].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.a[2 * i], w.v[i].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.a[2 * i + 1], w.v[i].z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.a[2 * i + 1], w.v[i].w, acc1, 0, 0, 0);
        }
    };
    actor_aload(a0, ap, 0);
    int blk = 0;
#ifndef ACT_ABLATE
#define ACT_ABLATE 0        /* experiments only: 1 = no weight loads in the loop, 2 = no A loads, 3 = neither */
#endif
    if (ACT_ABLATE & 1) w1 = w0;
    if (ACT_ABLATE & 2) a1 = a0;
    for (; blk + 1 < nblk; blk += 2) {
        if (!(ACT_ABLATE & 1)) actor_wload(w1, bp, blk + 1);
        if (!(ACT_ABLATE & 2)) actor_aload(a1, ap, (blk + 1) * 4 * ACT_U);
        __builtin_amdgcn_sched_barrier(0);
        mma(w0, a0);
        __builtin_amdgcn_sched_barrier(0);
        const int nb = min(blk + 2, nblk - 1);
        if (!(ACT_ABLATE & 1)) actor_wload(w0, bp, nb);
        if (!(ACT_ABLATE & 2)) actor_aload(a0, ap, nb * 4 * ACT_U);
        __builtin_amdgcn_sched_barrier(0);
        mma(w1, a1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (blk < nblk) mma(w0, a0);                        // odd block count: the last pair left block nblk - 1 in w0 / a0
    const int rowb = ak * 4;                            // C/D: col = lane & 15, row = (lane >> 4) * 4 + reg
    const float bv0 = bias[colb], bv1 = bias[colb + 1];
    if constexpr (!FINAL) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            out[(rowb + r) * ldo + colb] = fmaxf(acc0[r] + bv0, 0.f);
            out[(rowb + r) * ldo + colb + 1] = fmaxf(acc1[r] + bv1, 0.f);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float h0 = fmaxf(acc0[r] + bv0, 0.f), h1 = fmaxf(acc1[r] + bv1, 0.f);
            const float l0 = actor_row_sum(fmaf(h1, w3[1], h0 * w3[0]));
            const float l1 = actor_row_sum(fmaf(h1, w3[3], h0 * w3[2]));
            if (ai == 15) { out[(wave * ACT_M + rowb + r) * 2] = l0; out[(wave * ACT_M + rowb + r) * 2 + 1] = l1; }
        }
    }
}

// One tile of 16 environments through the actor (TD3:96-106 + 209-215), by the NW waves of a workgroup (all of its threads must
// call this).  obs / action: the tile's first row; n_live: rows of the tile that exist; act_sm: actor_tile_bytes(Dp) of
// LDS.  Ends with the actions in global memory (the caller synchronises before anyone reads them).
// `active` (wave-uniform): the policy kernel's workgroups have 16 waves; the eight that do not take part in the tile only keep
// the barrier count.  action2: a second copy of the actions (LDS, or NULL).
// STAMP (cn_actor_kernel alone): the eight actor_stamp points are time stamps in the profiling build, which specialises
// actor_stamp<true> (crowdnav_actor.hip), and nothing anywhere else.
// NOISE: what the output stage adds to a head's value before the clip.  void: TD3's Gaussian term (sigma, seed, counter).  Otherwise
// a type with `float operator()(float head, int row, int o, bool live) const`, called by the 32 threads (tile row i, output o) with
// row = row0 + i and live = the row exists, whose result is clipped and stored (cn_ddpg_act_kernel: the Ornstein-Uhlenbeck term);
// sigma, seed and counter are not read then.  The choice is made by `if constexpr` inside the one body, not by splitting the tile into
// functions: the compiler simplifies a function before it inlines it, and a split tile came out of every kernel with other address
// arithmetic or another register allocation than the whole one.
template <bool STAMP> __device__ __forceinline__ void actor_stamp(int k) {}
template <int NW, bool STAMP = false, class NOISE = void>        // NW = 8 (the packed weight layout is laid out for 8 waves x 32 columns)
__device__ __forceinline__ void actor_tile(const float* __restrict__ obs, int n_live, int row0, int D, int Dp,
        const float* __restrict__ W1T, const float* __restrict__ b1, const float* __restrict__ W2T,
        const float* __restrict__ b2, const float* __restrict__ W3, const float* __restrict__ b3,
        float* __restrict__ action, float* action2, float max_v, float max_w, float sigma, uint64_t seed, uint64_t counter,
        float* act_sm, const bool active = true, const int tid_in = -1, const NOISE* noise = nullptr)
{
    static_assert(NW == 8, "packed weights: 8 waves x 32 columns");
    const int ldx = ACT_LDX(Dp), ldh = ACT_LDH;
    float* X = act_sm;                 // [16][Dp + 1]; layer 2 writes its output here (the observations are dead by then)
    float* H = X + ACT_M * ldx;        // [16][257] hidden activations of layer 1
    const int tid = tid_in >= 0 ? tid_in : (int)threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    ActW w1, w2;
    actor_stamp<STAMP>(0);
    if (active) {
    actor_wload(w1, actor_wptr(W1T, wave, lane), 0);                   // in flight while the observations are staged
    // Staging the tile: rows by wave, coalesced.  Every load of a chunk (8 x 64 columns of each of the wave's rows) is issued
    // before the first store: written as `X[c] = src[c]` the loop paid one L2 round trip per 64 columns, in series -- 7 to 14 of
    // them, half of the tile's latency.
    constexpr int RPW = ACT_M / NW, CH = 8;
    for (int c0 = 0; c0 < Dp; c0 += 64 * CH) {
        float v[RPW][CH];
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const int r = wave + q * NW;
            const float* src = obs + (size_t)r * D;
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = c0 + lane + 64 * j;
                v[q][j] = (r < n_live && c < D) ? src[c] : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const int r = wave + q * NW;
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = c0 + lane + 64 * j;
                if (c < Dp) X[r * ldx + c] = v[q][j];
            }
        }
    }
    }
    actor_stamp<STAMP>(1);
    __syncthreads();
    actor_stamp<STAMP>(2);
    if (active) {
    actor_layer(X, ldx, Dp, W1T, b1, H, ldh, wave, lane, w1);
    actor_wload(w2, actor_wptr(W2T, wave, lane), 0);                   // ... and while the slowest wave finishes layer 1
    }
    actor_stamp<STAMP>(3);
    __syncthreads();
    actor_stamp<STAMP>(4);
    float* PL = X;                     // [8 waves][16 rows][2]: the waves' partial logits (the observations are dead by now)
    if (active) actor_layer<true>(H, ldh, ACT_H, W2T, b2, PL, 0, wave, lane, w2, W3);
    actor_stamp<STAMP>(5);
    __syncthreads();
    actor_stamp<STAMP>(6);
    if (tid < 2 * ACT_M)
    {   // heads, exploration noise, clip: thread = (env i, output o)
        const int i = tid >> 1, o = tid & 1, part = 0;
        float logit = b3[o];
#pragma unroll
        for (int w = 0; w < NW; ++w) logit += PL[(w * ACT_M + i) * 2 + o];
        const int e = row0 + i;
        float val = (o == 0) ? max_v / (1.0f + __expf(-logit)) : max_w * tanhf(logit);
        if constexpr (std::is_void<NOISE>::value) {
        if (sigma > 0.0f) {   // same generator as cn_policy_tail_kernel: keyed by (seed, counter, env row)
            uint64_t hh = cn_mix64(seed ^ cn_mix64(counter));
            hh = cn_mix64(hh ^ (uint64_t)(uint32_t)e);
            float u1 = ((float)(uint32_t)(hh >> 40) + 1.0f) * (1.0f / 16777217.0f);
            float u2 = (float)(uint32_t)((hh >> 8) & 0xffffffu) * (1.0f / 16777216.0f);
            float rr_ = sqrtf(-2.0f * __logf(u1)), s_, c_;
            __sincosf(6.28318530718f * u2, &s_, &c_);
            val += sigma * rr_ * ((o == 0) ? c_ : s_);
        }
        } else val = (*noise)(val, e, o, i < n_live);
        val = (o == 0) ? fminf(fmaxf(val, 0.0f), max_v) : fminf(fmaxf(val, -max_w), max_w);
        if (part == 0 && i < n_live) {
            action[2 * (size_t)i + o] = val;
            if (action2) action2[2 * (size_t)i + o] = val;
        }
    }
    actor_stamp<STAMP>(7);
}
