// crowdnav_gemm.hip -- the kernels that every fused learner launches (gfx950), and the only unit that defines or instantiates them:
// the three MFMA GEMM kernels F / G / H in their GATE / POP instantiations with the tick that rides in F, and td3_prep_kernel (the
// replay sample and gather) with td3_prep_shared_kernel, a population's gather from all members' rings.  The other units reach them
// through the launchers at the end of this file (crowdnav_learner.h declares them next to the argument structs): TD3 and its population (crowdnav_td3.hip), DDPG (crowdnav_ddpg.hip), SAC (crowdnav_sac.hip)
// launch the GATE = false instantiations, DQN (crowdnav_dqn.hip) alone GATE = true, the population alone POP = true.
// The learners' error channel (cn_td3_last_error) is defined here too.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>

#include "../../include/crowdnav.h"
#include "crowdnav_device.h"
#include "crowdnav_learner.h"
#include "crowdnav_learner_device.h"

namespace {

thread_local std::string g_td3_err;

// ---- the three GEMM kernels ---------------------------------------------------------------------------------------------
// C[i][j] = sum_r A(i, r) B(r, j) on v_mfma_f32_16x16x4_f32.  These layers are tiny (batch 128 x 256 units x 400 inputs =
// 26 MFLOP) and latency-bound, so the shape is: many small workgroups (a 16 x 16 / 16 x 32 / 32 x 32 tile of C each), the
// reduction split over the workgroup's four wavefronts, every operand loaded from global memory STRAIGHT into the MFMA operand
// registers as 8 / 16-byte vectors along the direction that is contiguous in memory -- no LDS staging, no barrier before the
// single one of the cross-wavefront sum.  What makes that possible: the order in which a reduction's terms are fed to the
// matrix core is free as long as both operands use the same order (F), and an operand whose contiguous direction is the OUTPUT
// index can feed several accumulators from one vector (G: two, H: two x two).  (Rounds 3-4 staged 32 x 32 tiles through LDS in
// 128-deep chunks, 32 workgroups a network: 9-13 us a launch, now 4-6.)
//   F  forward          i = row m, j = unit n, r = input k :  A = X[m][k],  B = W[n][k],   C = act(acc + bias[n])
//   G  backward (data)  i = row m, j = input k, r = unit n :  A = dY[m][n], B = W[n][k],   C = acc * [mask[m][k] > 0]
//   H  backward (weights) + Adam   i = unit n, j = input k, r = row m :  A = dY[m][n], B = X[m][k],  W[n][k] <- Adam(acc);
//      the workgroups of the first j-tile also reduce dY over the rows and step the bias
// one thread: advance the update counter and the Adam step counters, publish this update's bias corrections.  Runs inside a forward
// launch (a kernel of its own cost a full launch, ~4.6 us, for six scalar operations): after td3_prep_kernel, which reads the
// counter, and before the first kernel that reads the corrections (td3_critic_head_bwd_kernel).
__device__ __forceinline__ void td3_tick(const TickArgs& p)
{
    *p.counter += 1ull;
    p.steps[0] += 1.f;
    const double c1 = p.pw[0] * (double)p.beta1, c2 = p.pw[1] * (double)p.beta2;
    p.pw[0] = c1; p.pw[1] = c2;
    p.adam[0] = p.lr_critic / (float)(1.0 - c1);
    p.adam[1] = sqrtf((float)(1.0 - c2));
    if (p.do_actor) {
        p.steps[1] += 1.f;
        const double a1 = p.pw[2] * (double)p.beta1, a2 = p.pw[3] * (double)p.beta2;
        p.pw[2] = a1; p.pw[3] = a2;
        p.adam[2] = p.lr_actor / (float)(1.0 - a1);
        p.adam[3] = sqrtf((float)(1.0 - a2));
    }
}
template <bool POP> struct td3_args { typedef GemmArgs type; };
template <> struct td3_args<true> { typedef PopGemmArgs type; };

// F: a 16 x 16 tile per workgroup; the reduction in blocks of 16 inputs, block t = wavefront t mod 4.  Lane (li, lk) loads
// X[i0 + li][16 t + 4 lk ..+3] and W[j0 + li][the same]: component e of the two vectors is the pair the lane feeds to MFMA e of
// the block (k = 16 t + 4 lk + e on both sides).
#define TD3_FKB 8          /* blocks a wavefront has in flight (16 dwordx4 loads) */
// GATE = true (DQN's second chunk): the launch does nothing while *args.rms_gate == 0
// POP = true (a population; td3_dgrad_kernel and td3_wgrad_kernel have the same parameter): args is a PopGemmArgs -- the job comes
// from the table in device memory, and every member ticks once, in the first workgroup of its first job.  One body for both, so a
// member's tile is the same arithmetic in the same order as a solo handle's.
template <bool GATE, bool POP = false>
__global__ void __launch_bounds__(256) td3_fwd_kernel(typename td3_args<POP>::type args)
{
    if constexpr (GATE) { if (*args.rms_gate == 0) return; }
    const GemmJob& jb = args.job[blockIdx.z];
    const int I = jb.I, J = jb.J, R = jb.R;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    if constexpr (POP) {
        if (args.do_tick && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z % args.njobs == 0 && threadIdx.x == 0) td3_tick(args.tick[blockIdx.z / args.njobs]);
    } else {
        if (args.do_tick && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) td3_tick(args.tick);
    }
    if (i0 >= I || j0 >= J) return;
    __shared__ float red[4][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const float* __restrict__ arow = jb.A + (size_t)min(i0 + li, I - 1) * jb.lda;       // (rows past the edge: loaded, never stored)
    const float* __restrict__ brow = jb.B + (size_t)min(j0 + li, J - 1) * jb.ldb;
    const int nfull = R >> 4;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    const float pbias = jb.bias[min(j0 + li, J - 1)];
    const bool ragged = (R & 15) && (nfull & 3) == wave;          // the last, partial block: loaded first, multiplied last
    f32x4_t ta = {0.f, 0.f, 0.f, 0.f}, tb = {0.f, 0.f, 0.f, 0.f};
    if (ragged) { ta = td3_ld4(arow, 16 * nfull + 4 * lk, R); tb = td3_ld4(brow, 16 * nfull + 4 * lk, R); }
    // the policy head of this tile's 16 rows: the hidden units in runs of 4, run c of every 16 = (wavefront c >> 2, lane group c & 3)
    const bool head = jb.hd_h2 != nullptr;
    __shared__ float hred[4][2][16];
    float hp0 = 0.f, hp1 = 0.f, wa0 = 0.f, wa1 = 0.f;
    if (head) {
        const int HH = jb.hd_H;
        const float* __restrict__ hrow = jb.hd_h2 + (size_t)min(i0 + li, I - 1) * HH;
        const float* __restrict__ w3 = jb.hd_W3;
        wa0 = brow[R]; wa1 = brow[R + 1];
        if ((HH & 3) == 0) {
#pragma unroll 4
            for (int n = 4 * (4 * wave + lk); n < HH; n += 64) {
                const f32x4_t hv = *(const f32x4u_t*)(hrow + n), u0 = *(const f32x4u_t*)(w3 + n), u1 = *(const f32x4u_t*)(w3 + HH + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) { hp0 = fmaf(hv[e], u0[e], hp0); hp1 = fmaf(hv[e], u1[e], hp1); }
            }
        } else {
            for (int n = 4 * (4 * wave + lk); n < HH; n += 64) {
                const f32x4_t hv = td3_ld4(hrow, n, HH), u0 = td3_ld4(w3, n, HH), u1 = td3_ld4(w3 + HH, n, HH);
#pragma unroll
                for (int e = 0; e < 4; ++e) { hp0 = fmaf(hv[e], u0[e], hp0); hp1 = fmaf(hv[e], u1[e], hp1); }
            }
        }
    }
    for (int t0 = wave; t0 < nfull; t0 += 4 * TD3_FKB) {
        f32x4_t av[TD3_FKB], bv[TD3_FKB];
#pragma unroll
        for (int u = 0; u < TD3_FKB; ++u) {
            const int t = min(t0 + 4 * u, nfull - 1);         // (past the end: a block that is loaded and not used)
            av[u] = *(const f32x4u_t*)(arow + 16 * t + 4 * lk);
            bv[u] = *(const f32x4u_t*)(brow + 16 * t + 4 * lk);
        }
#pragma unroll
        for (int u = 0; u < TD3_FKB; ++u) {
            if (t0 + 4 * u < nfull) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = TD3_MFMA(av[u][e], bv[u][e], acc);
            }
        }
    }
    if (ragged) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = TD3_MFMA(ta[e], tb[e], acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[wave][q][lane] = acc[q];
    if (head) {
        hp0 += __shfl_xor(hp0, 16, 64); hp0 += __shfl_xor(hp0, 32, 64);
        hp1 += __shfl_xor(hp1, 16, 64); hp1 += __shfl_xor(hp1, 32, 64);
        if (lk == 0) { hred[wave][0][li] = hp0; hred[wave][1][li] = hp1; }
    }
    __syncthreads();
    const int q = wave, i = i0 + 4 * lk + q, j = j0 + li;      // thread -> one element of the tile
    const bool in = i < I && j < J;
    float y = ((red[0][q][lane] + red[1][q][lane]) + red[2][q][lane]) + red[3][q][lane];
    if (head && in) {
        const int r = 4 * lk + q;
        const float lg0 = (((hred[0][0][r] + hred[1][0][r]) + hred[2][0][r]) + hred[3][0][r]) + jb.hd_b3[0];
        const float lg1 = (((hred[0][1][r] + hred[1][1][r]) + hred[2][1][r]) + hred[3][1][r]) + jb.hd_b3[1];
        float a0 = jb.hd_max_v / (1.f + expf(-lg0)), a1 = jb.hd_max_w * tanhf(lg1);
        if (jb.hd_noise) { a0 += jb.hd_noise[2 * i]; a1 += jb.hd_noise[2 * i + 1]; }
        if (jb.hd_logits && blockIdx.x == 0 && li == 0) { jb.hd_logits[2 * i] = lg0; jb.hd_logits[2 * i + 1] = lg1; }
        y = fmaf(a1, wa1, fmaf(a0, wa0, y));
    }
    y += pbias;
    if (jb.relu) y = fmaxf(y, 0.f);
    if (in) {
        const size_t o = (size_t)i * jb.ldc + j;
        jb.C[o] = y;
        if (jb.dz_out) jb.dz_out[o] = y > 0.f ? -jb.dz_w3[j] / jb.dz_rows : 0.f;
    }
    if (jb.qp_out) {                                // (uniform) this tile's share of q[i]: the 16 lanes of a row, then tile x's slot
        float pq = in ? y * jb.qp_w3[j] : 0.f;
        pq += __shfl_xor(pq, 1, 64); pq += __shfl_xor(pq, 2, 64); pq += __shfl_xor(pq, 4, 64); pq += __shfl_xor(pq, 8, 64);
        if (li == 0 && i < I) jb.qp_out[(size_t)i * jb.qp_nt + blockIdx.x] = blockIdx.x == 0 ? pq + jb.qp_b3[0] : pq;
    }
}

// G: a 16 x 32 tile per workgroup.  dY's rows are contiguous along the reduction (as in F), W's along the OUTPUT: lane (li, lk)
// loads W[16 t + 4 lk + e][j0 + 2 li, + 1] for e = 0..3 -- two accumulators, columns j0 + 2 c and j0 + 2 c + 1.
#define TD3_GKB 4
template <bool GATE, bool POP = false>
__global__ void __launch_bounds__(256) td3_dgrad_kernel(typename td3_args<POP>::type args)
{
    if constexpr (GATE) { if (*args.rms_gate == 0) return; }
    const GemmJob& jb = args.job[blockIdx.z];
    const int I = jb.I, J = jb.J, R = jb.R;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 32;
    if (i0 >= I || j0 >= J) return;
    __shared__ float red[4][8][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const float* __restrict__ arow = jb.A + (size_t)min(i0 + li, I - 1) * jb.lda;
    const float* __restrict__ B = jb.B;
    const int jc = j0 + 2 * li;
    const int nb = (R + 15) >> 4;
    const bool inner = j0 + 32 <= J;               // (uniform) no ragged edge along j
    f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float pmask[2];                                // the ReLU mask of this thread's two elements, requested before the reduction
#pragma unroll
    for (int c = 0; c < 2; ++c) { const int i = i0 + 4 * lk + wave, j = jc + c; pmask[c] = (i < I && j < J) ? jb.mask[(size_t)i * jb.ldc + j] : 0.f; }
    float pdw[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    if (jb.da_out) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (jc + c < J) { pdw[c][0] = jb.da_w[(size_t)(jc + c) * jb.da_ld]; pdw[c][1] = jb.da_w[(size_t)(jc + c) * jb.da_ld + 1]; }
    }
    // head-backward mode: this lane's row of dq (14 loads in flight with the operands')
    const bool hb = jb.hb_h2 != nullptr;
    __shared__ float dqs[16];
    float dq_li = 0.f;
    if (hb) arow = jb.hb_h2 + (size_t)min(i0 + li, I - 1) * jb.lda;
    if (hb && (blockIdx.x == 0 || (wave == 0 && lk == 0))) {      // (the first column tile needs dq in every lane: it stores dz2)
        const int m = min(i0 + li, I - 1);
        float qs[3] = {0.f, 0.f, 0.f};             // this critic, the two target critics (DDPG: one)
        const int nq = jb.hb_single ? 2 : 3;
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            if (n >= nq) break;
            const float* __restrict__ pp = jb.hb_qpart + ((size_t)(n == 0 ? jb.hb_net : 1 + n) * I + m) * jb.hb_qnt;
            float a_ = 0.f;
            int t = 0;
#pragma unroll 4
            for (; t + 4 <= jb.hb_qnt; t += 4) { const f32x4_t v = *(const f32x4u_t*)(pp + t); a_ += (v[0] + v[1]) + (v[2] + v[3]); }
            for (; t < jb.hb_qnt; ++t) a_ += pp[t];
            qs[n] = a_;
        }
        const float y = jb.hb_r[m] + (1.f - jb.hb_d[m]) * jb.hb_gamma * (jb.hb_single ? qs[1] : fminf(qs[1], qs[2]));
        dq_li = 2.f * (qs[0] - y) / (float)I;
        if (wave == 0 && lk == 0) {
            dqs[li] = dq_li;
            if (blockIdx.x == 0 && i0 + li < I) jb.hb_dq[i0 + li] = dq_li;
        }
    }
    const bool ab = jb.ab_h2 != nullptr;
    float dl0 = 0.f, dl1 = 0.f;
    if (ab) {
        const int m = min(i0 + li, I - 1);
        float da[2];
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const float* __restrict__ pp = jb.ab_dapart + ((size_t)2 * m + o) * jb.ab_dant;
            float a_ = 0.f;
            int t = 0;
#pragma unroll 2
            for (; t + 4 <= jb.ab_dant; t += 4) { const f32x4_t v = *(const f32x4u_t*)(pp + t); a_ += (v[0] + v[1]) + (v[2] + v[3]); }
            for (; t < jb.ab_dant; ++t) a_ += pp[t];
            da[o] = a_;
        }
        const float lg0 = jb.ab_logits[2 * m], lg1 = jb.ab_logits[2 * m + 1];
        const float s_ = 1.f / (1.f + expf(-lg0)), th = tanhf(lg1);
        dl0 = da[0] * (jb.ab_max_v * s_ * (1.f - s_));
        dl1 = da[1] * (jb.ab_max_w * (1.f - th * th));
        if (blockIdx.x == 0 && wave == 0 && lk == 0 && i0 + li < I) { jb.ab_dl[2 * (i0 + li)] = dl0; jb.ab_dl[2 * (i0 + li) + 1] = dl1; }
        arow = jb.ab_h2 + (size_t)m * jb.lda;
    }
    for (int t0 = wave; t0 < nb; t0 += 4 * TD3_GKB) {
        f32x4_t av[TD3_GKB];
        f32x2_t bv[TD3_GKB][4];
#pragma unroll
        for (int u = 0; u < TD3_GKB; ++u) {
            const int t = t0 + 4 * u, k = 16 * t + 4 * lk;
            if (t < nb && inner && 16 * t + 16 <= R) {
                av[u] = *(const f32x4u_t*)(arow + k);
                if (hb) {
                    const f32x4_t wv = *(const f32x4u_t*)(jb.hb_w3 + k);
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[u][e] = av[u][e] > 0.f ? wv[e] : 0.f;
                }
                if (ab) {
                    const f32x4_t w0 = *(const f32x4u_t*)(jb.ab_w3 + k), w1 = *(const f32x4u_t*)(jb.ab_w3 + R + k);
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[u][e] = av[u][e] > 0.f ? fmaf(dl1, w1[e], dl0 * w0[e]) : 0.f;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[u][e] = *(const f32x2u_t*)(B + (size_t)(k + e) * jb.ldb + jc);
            } else if (t < nb) {
                av[u] = td3_ld4(arow, k, R);
                if (hb) {
                    const f32x4_t wv = td3_ld4(jb.hb_w3, k, R);
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[u][e] = av[u][e] > 0.f ? wv[e] : 0.f;
                }
                if (ab) {
                    const f32x4_t w0 = td3_ld4(jb.ab_w3, k, R), w1 = td3_ld4(jb.ab_w3 + R, k, R);
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[u][e] = av[u][e] > 0.f ? fmaf(dl1, w1[e], dl0 * w0[e]) : 0.f;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[u][e] = k + e < R ? td3_ld2(B + (size_t)(k + e) * jb.ldb, jc, J) : f32x2_t{0.f, 0.f};
            } else {
                av[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[u][e] = f32x2_t{0.f, 0.f};
            }
        }
#pragma unroll
        for (int u = 0; u < TD3_GKB; ++u) {
            if (t0 + 4 * u < nb) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc0 = TD3_MFMA(av[u][e], bv[u][e][0], acc0); acc1 = TD3_MFMA(av[u][e], bv[u][e][1], acc1); }
            }
        }
        if ((hb || ab) && blockIdx.x == 0 && i0 + li < I) {      // dz2 = A, for the weight-gradient launch
            const float sc = hb ? dq_li : 1.f;
            float* __restrict__ zb = (hb ? jb.hb_dz2 : jb.ab_dz2) + (size_t)(i0 + li) * jb.lda;
#pragma unroll
            for (int u = 0; u < TD3_GKB; ++u) {
                const int t = t0 + 4 * u, k = 16 * t + 4 * lk;
                if (t >= nb) continue;
                float* __restrict__ zr = zb + k;
                if (k + 4 <= R) *(f32x4u_t*)zr = av[u] * sc;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (k + e < R) zr[e] = av[u][e] * sc;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { red[wave][q][lane] = acc0[q]; red[wave][4 + q][lane] = acc1[q]; }
    __syncthreads();
    const int q = wave, i = i0 + 4 * lk + q;
    const float rowscale = hb ? dqs[4 * lk + q] : 1.f;
    float dv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int j = jc + c;
        const float d = (((red[0][4 * c + q][lane] + red[1][4 * c + q][lane]) + red[2][4 * c + q][lane]) + red[3][4 * c + q][lane]) * rowscale;
        dv[c] = (i < I && j < J && pmask[c] > 0.f) ? d : 0.f;
        if (i < I && j < J) jb.C[(size_t)i * jb.ldc + j] = dv[c];
    }
    if (jb.da_out) {                                // (uniform)
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            float pa = fmaf(dv[1], pdw[1][o], dv[0] * pdw[0][o]);
            pa += __shfl_xor(pa, 1, 64); pa += __shfl_xor(pa, 2, 64); pa += __shfl_xor(pa, 4, 64); pa += __shfl_xor(pa, 8, 64);
            if (li == 0 && i < I) jb.da_out[((size_t)2 * i + o) * jb.da_nt + blockIdx.x] = pa;
        }
    }
}

// H: a 32 x 32 tile per workgroup, the batch rows split over the four wavefronts in steps of 4 (step s = wavefront s mod 4).
// Both operands are contiguous along their output index: lane (li, lk) loads dY[4 s + lk][i0 + 2 li, + 1] and
// X[4 s + lk][j0 + 2 li, + 1] -- 2 x 2 accumulators, acc[a][b] = the (rows i0 + 2 r + a) x (columns j0 + 2 c + b) sub-lattice.
// RMS = false: Adam (TD3, DDPG); RMS = true: RMSprop without momentum (DQN, Keras 2's RMSprop.get_updates:
// a = rho a + (1 - rho) g^2, p -= lr g / (sqrt(a) + eps), the accumulator in jb.m / jb.bm; no target copy, no loss).
#define TD3_HKS 8          /* steps a wavefront has in flight (16 dwordx2 loads, 32 MFMAs) */
template <bool RMS, bool POP = false>
__global__ void __launch_bounds__(256) td3_wgrad_kernel(typename td3_args<POP>::type args)
{
    const GemmJob& jb = args.job[blockIdx.z];
    const int I = jb.I, J = jb.J, R = jb.R;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    if (i0 >= I || j0 >= J) return;
    if constexpr (RMS) { if (*args.rms_gate == 0) return; }
    __shared__ float red[4][16][64];
    __shared__ float bred[4][4][32];
    __shared__ float lred[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const float* __restrict__ A = jb.A;
    const float* __restrict__ B = jb.B;
    const int ic = i0 + 2 * li, jc = j0 + 2 * li;
    const int ns = (R + 3) >> 2;
    // a lane's pair of rows / columns: 2 = both inside, 1 = only the first (odd extents), 0 = past the edge (a ragged tile: the lane
    // loads a pair that IS inside and its products are never stored).  Pairs that straddle the edge take the element-wise path.
    const int amode = ic + 1 < I ? 2 : ic < I ? 1 : 0, bmode = jc + 1 < J ? 2 : jc < J ? 1 : 0;
    const bool vec = __all(bmode != 1) && J >= 2;       // (an odd last ROW of the tile -- or I = 1, the linear3 jobs -- loads one element)
    const int jcv = bmode == 2 ? jc : 0;
    const float adam0 = RMS ? 0.f : jb.adam[0], adam1 = RMS ? 0.f : jb.adam[1];
    f32x4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float bs0 = 0.f, bs1 = 0.f;                    // sums of dY over this lane's rows (the bias gradient, first j-tile only)
    float ls0 = 0.f;                               // ... and of dY[.][0]^2 (loss_out)
    // the Adam step's operands of this thread's four elements, requested now: their round trip overlaps the reduction's
    float pm[4], pv[4], pw[4], pt[4];
#pragma unroll
    for (int z = 0; z < 4; ++z) {
        const int i = i0 + (tid >> 5) + 8 * z, j = j0 + (tid & 31);
        const bool in = i < I && j < J;
        const size_t o = in ? (size_t)i * jb.ldc + j : 0;
        pm[z] = in ? jb.m[o] : 0.f; pv[z] = (!RMS && in) ? jb.v[o] : 0.f; pw[z] = in ? jb.C[o] : 0.f;
        pt[z] = (!RMS && in && jb.tgt) ? jb.tgt[o] : 0.f;
    }
    for (int s0 = wave; s0 < ns; s0 += 4 * TD3_HKS) {
        f32x2_t av[TD3_HKS], bv[TD3_HKS];
#pragma unroll
        for (int u = 0; u < TD3_HKS; ++u) {
            const int s = s0 + 4 * u, k = 4 * s + lk;
            if (s < ns && vec && 4 * s + 4 <= R) {
                av[u] = f32x2_t{0.f, 0.f};
                if (amode == 2) av[u] = *(const f32x2u_t*)(A + (size_t)k * jb.lda + ic);
                else if (amode == 1) av[u][0] = A[(size_t)k * jb.lda + ic];
                bv[u] = *(const f32x2u_t*)(B + (size_t)k * jb.ldb + jcv);
            } else if (s < ns && k < R) {
                av[u] = td3_ld2(A + (size_t)k * jb.lda, ic, I);
                bv[u] = td3_ld2(B + (size_t)k * jb.ldb, jc, J);
            } else { av[u] = f32x2_t{0.f, 0.f}; bv[u] = f32x2_t{0.f, 0.f}; }
        }
#pragma unroll
        for (int u = 0; u < TD3_HKS; ++u) {
            if (s0 + 4 * u < ns) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = TD3_MFMA(av[u][a], bv[u][b], acc[a][b]);
                bs0 += av[u][0]; bs1 += av[u][1]; ls0 = fmaf(av[u][0], av[u][0], ls0);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[wave][(2 * a + b) * 4 + q][lane] = acc[a][b][q];
    bred[wave][lk][2 * li] = bs0; bred[wave][lk][2 * li + 1] = bs1;
    if (li == 0) lred[wave][lk] = ls0;
    __syncthreads();
    if (!RMS && jb.loss_out && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        float l_ = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int k = 0; k < 4; ++k) l_ += lred[w][k];
        jb.loss_out[0] = l_ * (0.25f * (float)R);
    }
    // thread -> four elements of the tile, 32 consecutive columns per half-wavefront: row ii = 2 (4 g + q) + a, column jj = 2 c + b
#pragma unroll
    for (int z = 0; z < 4; ++z) {
        const int ii = (tid >> 5) + 8 * z, jj = tid & 31;
        const int a = ii & 1, g = ii >> 3, q = (ii >> 1) & 3, c = jj >> 1, b = jj & 1;
        const int slot = (2 * a + b) * 4 + q, l = 16 * g + c;
        const int i = i0 + ii, j = j0 + jj;
        if (i >= I || j >= J) continue;
        const float gsum = ((red[0][slot][l] + red[1][slot][l]) + red[2][slot][l]) + red[3][slot][l];
        const size_t o = (size_t)i * jb.ldc + j;
        if constexpr (RMS) {
            const float a = args.rms_rho * pm[z] + (1.f - args.rms_rho) * (gsum * gsum);
            jb.m[o] = a;
            jb.C[o] = pw[z] - args.rms_lr * gsum / (sqrtf(a) + args.rms_eps);
            continue;
        }
        const float m = args.beta1 * pm[z] + (1.f - args.beta1) * gsum;
        const float v = args.beta2 * pv[z] + (1.f - args.beta2) * gsum * gsum;
        jb.m[o] = m; jb.v[o] = v;
        const float w = pw[z] - adam0 * m / (sqrtf(v) / adam1 + args.eps);
        jb.C[o] = w;
        if (jb.tgt) jb.tgt[o] = td3_soft(pt[z], w, args.tau);
    }
    if (blockIdx.x == 0 && tid < 32 && i0 + tid < I && jb.bparam) {
        const int i = i0 + tid;
        float gsum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int k = 0; k < 4; ++k) gsum += bred[w][k][tid];
        if constexpr (RMS) {
            const float a = args.rms_rho * jb.bm[i] + (1.f - args.rms_rho) * (gsum * gsum);
            jb.bm[i] = a;
            jb.bparam[i] = jb.bparam[i] - args.rms_lr * gsum / (sqrtf(a) + args.rms_eps);
            return;
        }
        const float m = args.beta1 * jb.bm[i] + (1.f - args.beta1) * gsum;
        const float v = args.beta2 * jb.bv[i] + (1.f - args.beta2) * gsum * gsum;
        jb.bm[i] = m; jb.bv[i] = v;
        const float b = jb.bparam[i] - adam0 * m / (sqrtf(v) / adam1 + args.eps);
        jb.bparam[i] = b;
        if (jb.btgt) jb.btgt[i] = td3_soft(jb.btgt[i], b, args.tau);
    }
}

// POP = true (a population): grid (B, P), member blockIdx.y's arguments from a table in device memory (one table per sampling mode)
template <bool POP> struct td3_prep_in { typedef PrepArgs type; typedef const PrepArgs view; };
template <> struct td3_prep_in<true> { typedef const PrepArgs* type; typedef const PrepArgs& view; };
__device__ __forceinline__ const PrepArgs& td3_prep_of(const PrepArgs& p) { return p; }
__device__ __forceinline__ const PrepArgs& td3_prep_of(const PrepArgs* table) { return table[blockIdx.y]; }
template <bool POP = false>
__global__ void __launch_bounds__(256) td3_prep_kernel(typename td3_prep_in<POP>::type in)
{
    typename td3_prep_in<POP>::view p = td3_prep_of(in);
    const int m = blockIdx.x, tid = threadIdx.x, Dc = p.D + 2;
    const unsigned long long cnt = *p.counter;       // (advanced by td3_tick inside a later launch on the stream)
    size_t row = (size_t)m;
    if (p.size_dev) row = cn_replay_row(p.seed, cnt, m, p.size_dev, p.mode);
    const float* s = p.rs + row * (size_t)p.D;
    const float* s2 = p.rs2 + row * (size_t)p.D;
    for (int c = tid; c < p.D; c += blockDim.x) {
        p.xs[(size_t)m * Dc + c] = s[c];
        p.x2[(size_t)m * Dc + c] = s2[c];
    }
    if (tid < 2) {
        p.xs[(size_t)m * Dc + p.D + tid] = p.ra[row * 2 + tid];
    }
    if (tid < 2 && p.noise) {
        float z;
        if (p.noise_in) z = p.noise_in[(size_t)m * 2 + tid];
        else {   // Box-Muller on a counter-based pair, keyed by (seed, update counter, row)
            const uint64_t h = cn_mix64(cn_mix64(p.seed ^ cn_mix64(cnt ^ 0x5bd1e995u)) ^ (uint64_t)(uint32_t)m);
            const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777217.0f);
            const float u2 = (float)(uint32_t)((h >> 8) & 0xffffffu) * (1.0f / 16777216.0f);
            const float rr = sqrtf(-2.0f * logf(u1));
            z = tid == 0 ? rr * cosf(6.28318530718f * u2) : rr * sinf(6.28318530718f * u2);
        }
        p.noise[(size_t)m * 2 + tid] = fminf(fmaxf(z * p.noise_std, -p.noise_clip), p.noise_clip);     // TD3:241-242
    }
    if (tid == 2) p.r[m] = p.rr[row];
    if (tid == 3) p.d[m] = p.rd[row];
}
// A population whose members draw from ALL members' rings (CN_REPLAY_SHARED; the statement: include/crowdnav.h).  Grid (B, P) over the
// same tables as td3_prep_kernel<true>: the outputs, counter, seed and noise parameters of row p = blockIdx.y, the ring of row q*.  The
// first wavefront reads the P live sizes (lane q: ring q's), finds {q*, row} (cn_replay_row_shared) and hands it to the other three
// through LDS; lane 0 also writes it to src [P][B][2].  The gather and the noise are td3_prep_kernel's.
__global__ void __launch_bounds__(256) td3_prep_shared_kernel(PrepSharedArgs in)
{
    __shared__ unsigned long long pick[2];
    const PrepArgs& p = in.table[blockIdx.y];
    const int m = blockIdx.x, tid = threadIdx.x, Dc = p.D + 2, P = in.P;
    const unsigned long long cnt = *p.counter;
    if (tid < 64) {
        unsigned long long n = 0;
        if (tid < P) { const int64_t live = *in.table[tid].size_dev; n = live > 0 ? (unsigned long long)live : 0ull; }
        const CnSharedRow at = cn_replay_row_shared(p.seed, cnt, m, n, P, (int)blockIdx.y, p.mode);
        if (tid == 0) {
            pick[0] = (unsigned long long)at.ring; pick[1] = at.row;
            int64_t* out = in.src + ((size_t)blockIdx.y * gridDim.x + m) * 2;
            out[0] = (int64_t)at.ring; out[1] = (int64_t)at.row;
        }
    }
    __syncthreads();
    const PrepArgs& from = in.table[pick[0]];
    const size_t row = (size_t)pick[1];
    const float* s = from.rs + row * (size_t)p.D;
    const float* s2 = from.rs2 + row * (size_t)p.D;
    for (int c = tid; c < p.D; c += blockDim.x) {
        p.xs[(size_t)m * Dc + c] = s[c];
        p.x2[(size_t)m * Dc + c] = s2[c];
    }
    if (tid < 2) {
        p.xs[(size_t)m * Dc + p.D + tid] = from.ra[row * 2 + tid];
        const uint64_t h = cn_mix64(cn_mix64(p.seed ^ cn_mix64(cnt ^ 0x5bd1e995u)) ^ (uint64_t)(uint32_t)m);      // as td3_prep_kernel
        const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777217.0f);
        const float u2 = (float)(uint32_t)((h >> 8) & 0xffffffu) * (1.0f / 16777216.0f);
        const float rr = sqrtf(-2.0f * logf(u1));
        const float z = tid == 0 ? rr * cosf(6.28318530718f * u2) : rr * sinf(6.28318530718f * u2);
        p.noise[(size_t)m * 2 + tid] = fminf(fmaxf(z * p.noise_std, -p.noise_clip), p.noise_clip);
    }
    if (tid == 2) p.r[m] = from.rr[row];
    if (tid == 3) p.d[m] = from.rd[row];
}
// The actor-loss chain -mean Q1(s, pi(s)) (TD3:268-269) has no kernel of its own: its first link (d/dh2 of the critic) is
// td3_fwd_kernel's dz epilogue; through the critic's first layer to the action (the two action columns of W1) = per-tile partial
// sums in td3_dgrad_kernel's da epilogue; through the heads' derivatives and the actor's linear3 = the same kernel's ab mode on
// the next launch; dW3a = dl^T h2a = a two-row job of td3_wgrad_kernel.  (Rounds 3-4: td3_dlogit_kernel, one wavefront per row,
// 4.8 us, and td3_actor_head_bwd_kernel, 9 us; the critics had td3_q_head_kernel and td3_critic_head_bwd_kernel.)

}  // namespace

// ---- the learners' error channel (crowdnav_learner.h) ------------------------------------------------------------------------------
int td3_fail(int code, const std::string& msg) { g_td3_err = msg; return code; }
extern "C" const char* cn_td3_last_error(void) { return g_td3_err.c_str(); }

// ---- the launchers (crowdnav_learner.h) ----------------------------------------------------------------------------------------------
dim3 gemm_grid(int mode, const GemmJob* jobs, int njobs)
{
    constexpr int TI[3] = {16, 16, 32}, TJ[3] = {16, 32, 32};      // the kernels' tiles of C: F 16 x 16, G 16 x 32, H 32 x 32
    int gx = 0, gy = 0;
    for (int z = 0; z < njobs; ++z) {
        const int x_ = (jobs[z].J + TJ[mode] - 1) / TJ[mode], y_ = (jobs[z].I + TI[mode] - 1) / TI[mode];
        gx = x_ > gx ? x_ : gx; gy = y_ > gy ? y_ : gy;
    }
    return dim3(gx, gy, 1);
}
// One launch on the caller's own argument struct.  hipLaunchKernelGGL would hand `args` to the kernel's host stub by value: a copy of
// up to 2.6 KB (GemmArgs) per launch, which an update whose unit also held the kernels (stub inlined) never made.  This is the stub's
// own call; like hipLaunchKernelGGL it leaves the error to the caller's hipGetLastError.
template <class Args>
static void launch(void (*kernel)(Args), dim3 grid, const Args& args, hipStream_t st)
{
    void* argv[1] = {const_cast<Args*>(&args)};
    (void)hipLaunchKernel((const void*)kernel, grid, dim3(256), argv, 0, st);
}
void launch_gemm(int mode, bool gate, const GemmArgs& ga, int njobs, hipStream_t st)
{
    dim3 grid = gemm_grid(mode, ga.job, njobs);
    grid.z = njobs;
    if (mode == GEMM_F) launch(gate ? td3_fwd_kernel<true> : td3_fwd_kernel<false>, grid, ga, st);
    else if (mode == GEMM_G) launch(gate ? td3_dgrad_kernel<true> : td3_dgrad_kernel<false>, grid, ga, st);
    else launch(gate ? td3_wgrad_kernel<true> : td3_wgrad_kernel<false>, grid, ga, st);
}
void launch_gemm_pop(int mode, const PopGemmArgs& ga, dim3 grid, hipStream_t st)
{
    if (mode == GEMM_F) launch(td3_fwd_kernel<false, true>, grid, ga, st);
    else if (mode == GEMM_G) launch(td3_dgrad_kernel<false, true>, grid, ga, st);
    else launch(td3_wgrad_kernel<false, true>, grid, ga, st);
}
void launch_prep(const PrepArgs& pa, hipStream_t st) { launch(td3_prep_kernel<false>, dim3(pa.B), pa, st); }
void launch_prep_pop(const PrepArgs* table, int B, int P, hipStream_t st) { launch(td3_prep_kernel<true>, dim3(B, P), table, st); }
void launch_prep_shared(const PrepArgs* table, int64_t* src, int B, int P, hipStream_t st)
{
    launch(td3_prep_shared_kernel, dim3(B, P), PrepSharedArgs{table, src, P}, st);
}
