// crowdnav_td3.hip -- the TD3 update (td3.py:225-285 of the reference: Agent.learn) as a short chain of HIP kernels (gfx950).
//
// The caller of the hot path.  A vectorised environment makes the learner the bottleneck: through PyTorch one
// update is ~150 small kernels (1.2 ms as a hipGraph at batch 128).  Here the same arithmetic is 7 launches for the critic
// step and 5 more when the actor and the targets move (rounds 3-4: 10 + 11), all float32 like the reference:
//   prep        sample the replay on the device (counter-based indices and target-policy noise), gather [s|a], [s2|.], r, d
//   gemm F      Y = act(X W^T + b) on the f32 matrix cores (v_mfma_f32_16x16x4_f32), up to four networks per launch;
//               optional: the policy's last layer + heads evaluated in place of X's action columns, the critic's last layer
//               as per-tile partial sums of the activation just written, the first link of the actor-loss chain
//   gemm G      dX = (dY W) (.) [H > 0]   (back-propagation through a ReLU layer); optional: dY evaluated, not read -- the TD
//               target + MSE gradient + linear3 backward of a critic, or the heads' derivatives + linear3 backward of the actor;
//               the action gradient's partial sums
//   gemm H      dW = dY^T X folded into the Adam step of W (and of b) and the soft update of the target's copy: the gradient
//               never exists in memory; linear3's gradients are one- and two-row jobs of the same launch
// Launch order: prep | actor_t L1 (+ actor L1) | L2 (+ L2) | critics L1 (target actions from the head) | critics L2 (+ q partials,
// tick) | G (dq, dz2 evaluated) | H (six jobs)   and, every policy_delay-th update:  q1 L1 on (s, pi(s)) | q1 L2 (+ dz) | G (+ da
// partials) | G (dl, dz2a evaluated) | H (three jobs).
// The parameters are the caller's (PyTorch nn.Linear storages, weight [out][in]); Adam's moments and step counters live here.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <memory>
#include <new>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/crowdnav.h"
#include "crowdnav_device.h"
#include "crowdnav_host.h"
#include "crowdnav_record.h"

typedef float f32x4_t __attribute__((ext_vector_type(4)));

namespace {

thread_local std::string g_td3_err;
int td3_fail(int code, const std::string& msg) { g_td3_err = msg; return code; }

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
enum { GEMM_F = 0, GEMM_G = 1, GEMM_H = 2 };
// one thread: advance the update counter and the Adam step counters, publish this update's bias corrections.  Runs inside a forward
// launch (a kernel of its own cost a full launch, ~4.6 us, for six scalar operations): after td3_prep_kernel, which reads the
// counter, and before the first kernel that reads the corrections (td3_critic_head_bwd_kernel).
struct TickArgs {
    float* adam;                                   // [2 optimizers][2]: lr / (1 - beta1^t), sqrt(1 - beta2^t)
    float* steps;                                  // [2] step counters (critics, actor)
    double* pw;                                    // [2 optimizers][2]: beta1^t, beta2^t as running products (powf was most of this thread's time)
    unsigned long long* counter;                   // update counter (keys the sampling)
    int do_actor; float lr_critic, lr_actor, beta1, beta2;
};
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
struct GemmJob {
    const float* A; const float* B; float* C;      // H: C = the weight being stepped
    const float* bias;                             // F: bias[n]
    const float* mask;                             // G: activation the ReLU mask is taken from (same shape / ld as C)
    float* m; float* v;                            // H: Adam moments of the weight
    float* bparam; float* bm; float* bv;           // H: bias and its moments
    const float* adam;                             // H: {lr / (1 - beta1^t), sqrt(1 - beta2^t)} of this optimizer (device)
    int I, J, R;                                   // extents of i, j, r
    int lda, ldb, ldc;
    int relu;
    // F, optional: the first link of the actor-loss chain written next to the activation it is masked by (TD3:268-269,
    // -mean Q1(s, pi(s))): dz_out[m][n] = -(1 / dz_rows) dz_w3[n] [y > 0]  (was a kernel of its own: one more launch)
    const float* dz_w3; float* dz_out; float dz_rows;
    // H, optional (actor updates): the target network's copy of the weight / bias, soft-updated from the value just stepped
    // (TD3:287-299; was an 18-tensor launch of its own at the end of the update)
    float* tgt; float* btgt;
    // F, optional: the LAST TWO columns of A are not read but evaluated here -- they are a policy's action on the row,
    // Actor.forward's last layer and heads (TD3:101-105) on the policy's second hidden activation hd_h2 [I][hd_H]:
    //   logits = hd_h2 hd_W3^T + hd_b3,  action = (sigmoid max_v, tanh max_w) (+ hd_noise: the clipped target-policy noise, not
    //   re-clipped to the action bounds, TD3:244-247);  R counts the columns before them, B's row has R + 2.
    // Their share of the product is rank 2 and is added after the cross-wavefront sum.  (Was a launch of its own that wrote the
    // actions into A.)  hd_logits [I][2], optional: the logits, kept for the backward pass (written by the first column tile).
    const float* hd_h2; const float* hd_W3; const float* hd_b3; const float* hd_noise; float* hd_logits;
    int hd_H; float hd_max_v, hd_max_w;
    // F, optional: Critic.forward's last layer on the activation this job writes, q = C . qp_w3 + qp_b3 (TD3:139), as partial sums
    // over the tile's 16 units: qp_out[i * qp_nt + column tile] (the bias rides in tile 0; the consumer adds the tiles in order)
    const float* qp_w3; const float* qp_b3; float* qp_out; int qp_nt;
    // G, optional: the next link of the actor-loss chain, through the critic's first layer to the action: partial sums over the
    // tile's 32 units of C[i][j] da_w[j * da_ld + o], o = 0, 1 (the two action columns of W1): da_out[(2 i + o) * da_nt + column tile]
    const float* da_w; float* da_out; int da_ld, da_nt;
    // G, optional: A is not read but evaluated -- it is the gradient at a critic's second hidden layer (TD3:249-260),
    //   A[m][k] = dq[m] hb_w3[k] [hb_h2[m][k] > 0],   dq[m] = 2 (q[m] - y[m]) / I,   y = r + (1 - d) gamma min(q1_t, q2_t)[m],
    // q of network hb_net and of the two targets (networks 2, 3) from td3_fwd_kernel's per-tile partial sums hb_qpart.  dq scales a
    // whole row, so the reduction runs on hb_w3 (.) [h2 > 0] and the epilogue multiplies.  The first column tile also writes what
    // the weight-gradient launch needs: hb_dq [I] (linear3's gradient = dq^T h2: a job of that launch) and hb_dz2 [I][R] = A.
    // (Was td3_critic_head_bwd_kernel: a launch between the forward pass and this one.)
    // hb_single != 0 (DDPG, ddpg.py:223-225): ONE target network, y = r + (1 - d) gamma q_t with q_t = network 2's partial sums;
    // network 3's are not read.
    const float* hb_h2; const float* hb_w3; const float* hb_qpart; const float* hb_r; const float* hb_d;
    float* hb_dq; float* hb_dz2; int hb_qnt, hb_net; float hb_gamma; int hb_single;
    // G, optional, the ACTOR's counterpart (TD3:268-269, -mean Q1(s, pi(s)) arriving at the policy's second hidden layer):
    //   A[m][k] = (dl[m][0] ab_w3[k] + dl[m][1] ab_w3[R + k]) [ab_h2[m][k] > 0],   dl[m][o] = da[m][o] (max_v s (1 - s), max_w (1 - t^2)),
    // da from this kernel's own per-tile partial sums of the launch before (ab_dapart), s / t from the policy's logits.  The first
    // column tile writes ab_dl [I][2] (linear3's gradient = dl^T h2: a two-row job of the weight-gradient launch) and ab_dz2 = A.
    // (Was td3_actor_head_bwd_kernel.)
    const float* ab_h2; const float* ab_w3; const float* ab_dapart; const float* ab_logits;
    float* ab_dl; float* ab_dz2; int ab_dant; float ab_max_v, ab_max_w;
    // H, optional: A is one column (I = 1) of per-row loss gradients dq; loss_out[0] = mean squared TD error = (R / 4) sum dq^2
    float* loss_out;
};
// (rms_*: the RMSprop instantiation of the weight-gradient kernel, td3_wgrad_kernel<true>, alone reads them -- appended after the
// fields the Adam kernels read, so those keep their kernel-argument offsets)
struct GemmArgs {
    GemmJob job[6]; float beta1, beta2, eps, tau; TickArgs tick; int do_tick;
    const int* rms_gate;                           // RMSprop: the launch steps nothing while *rms_gate == 0 (device)
    float rms_lr, rms_rho, rms_eps;
};
static_assert(sizeof(GemmArgs) <= 4096, "GemmArgs travels in the kernarg segment (4 KB)");
// The population form (cn_td3_pop_update): P members' jobs do not fit the kernarg segment, so they lie in device memory, built once
// when the handle is created: job[member * njobs + z] is job z of the launch for that member (blockIdx.z walks it), tick[member] its
// tick's arguments.  What differs between members travels in the job (its pointers, the Adam constants' pointer, hb_gamma) or in the
// tick's arguments; the four scalars here are the ones the members must agree in.
struct PopGemmArgs { const GemmJob* job; const TickArgs* tick; int njobs; float beta1, beta2, eps, tau; int do_tick; };
template <bool POP> struct td3_args { typedef GemmArgs type; };
template <> struct td3_args<true> { typedef PopGemmArgs type; };
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


// ---- small kernels ------------------------------------------------------------------------------------------------------
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
// ring row of batch row m of update `cnt`: the draw with replacement, or the bijection above (mode: the handle's, CN_SAMPLE_*)
__device__ __forceinline__ size_t cn_replay_row(uint64_t seed, unsigned long long cnt, int m, const int64_t* size_dev, int mode)
{
    const unsigned long long size = (unsigned long long)(*size_dev > 0 ? *size_dev : 1);
    if (mode == CN_SAMPLE_DISTINCT) return (size_t)cn_replay_row_distinct(seed, cnt, (uint64_t)(uint32_t)m, size);
    return (size_t)(cn_mix64(cn_mix64(seed ^ cn_mix64(cnt)) ^ (uint64_t)(uint32_t)m) % size);
}
// the rows an update with (seed, counter, mode) gathers, without the update: cn_replay_sample_indices
__global__ void __launch_bounds__(256) cn_replay_indices_kernel(uint64_t seed, unsigned long long cnt, int B, const int64_t* size_dev, int mode,
                                                                int64_t* __restrict__ rows)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < B) rows[m] = (int64_t)cn_replay_row(seed, cnt, m, size_dev, mode);
}
struct PrepArgs {
    const float *rs, *ra, *rr, *rs2, *rd;          // replay ring (rows `obs_dim` / 2 / 1 wide) or the explicit batch
    const float* noise_in;                         // explicit target-policy noise [B][2] (unit variance, before the clip) or null
    const int64_t* size_dev;                       // live replay size (device) or null = the rows ARE the batch
    float *xs, *x2, *r, *d, *noise;                // outputs: [B][D + 2] x 2, [B], [B], [B][2] (noise null: none drawn, DDPG)
    const unsigned long long* counter;             // update counter (keys the sampling; advanced by td3_tick)
    uint64_t seed;
    int B, D;
    float noise_std, noise_clip;
    int mode;                                      // CN_SAMPLE_*: how the replay rows are drawn
};
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
__device__ __forceinline__ float td3_wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// The actor-loss chain -mean Q1(s, pi(s)) (TD3:268-269) has no kernel of its own: its first link (d/dh2 of the critic) is
// td3_fwd_kernel's dz epilogue; through the critic's first layer to the action (the two action columns of W1) = per-tile partial
// sums in td3_dgrad_kernel's da epilogue; through the heads' derivatives and the actor's linear3 = the same kernel's ab mode on
// the next launch; dW3a = dl^T h2a = a two-row job of td3_wgrad_kernel.  (Rounds 3-4: td3_dlogit_kernel, one wavefront per row,
// 4.8 us, and td3_actor_head_bwd_kernel, 9 us; the critics had td3_q_head_kernel and td3_critic_head_bwd_kernel.)
// ---- the collection loop's bookkeeping (cn_replay_write, cn_episode_log_add) --------------------------------------------------
// (bodies: crowdnav_record.h, shared with cn_pop_record's kernels -- crowdnav_pop_record.hip -- so that both are the same text)
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

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {
// A learner's workspace is ONE device allocation that the handle's layout(Pool&) describes once, as a take(field, n) per buffer.
// learner_create runs it twice: with base == nullptr it only sums (the size hipMalloc gets), then it assigns the fields -- so the
// size cannot disagree with the carve-up.  Every field is aligned for its own type, wherever it stands.
struct Pool {
    char* base;
    size_t size = 0;
    template <class T> void take(T*& field, size_t n)
    {
        size = (size + alignof(T) - 1) / alignof(T) * alignof(T);
        if (base) field = (T*)(base + size);
        size += n * sizeof(T);
    }
};
// elements of tensor j of {w1, b1, w2, b2, w3, b3} of Linear(in1, H) - Linear(H, H) - Linear(H, out3)
size_t param_count(int in1, int out3, int H, int j)
{
    const size_t h = (size_t)H;
    switch (j) { case 0: return h * in1; case 1: return h; case 2: return h * h; case 3: return h; case 4: return out3 * h; default: return out3; }
}
bool mlp_ok(const cn_td3_mlp& n) { return n.w1 && n.b1 && n.w2 && n.b2 && n.w3 && n.b3; }
int check_mlps(const char* fn, std::initializer_list<const cn_td3_mlp*> nets)
{
    for (const cn_td3_mlp* n : nets) if (!mlp_ok(*n)) return td3_fail(CN_ERR_ARG, std::string(fn) + ": null parameter pointer");
    return CN_OK;
}

// What the three handles share.  It owns the pool: deleting the handle frees it, on every path.
struct Learner {
    int device = 0, B = 0, D = 0, H = 0;
    void* pool = nullptr;          // one allocation for the whole workspace
    float* loss = nullptr;
    unsigned long long* counter = nullptr;         // update counter (keys the sampling)
    int sample_mode = CN_SAMPLE_WITH_REPLACEMENT;  // cn_*_set_replay_sample: read on the host when an update is enqueued
    Learner() = default;
    Learner(const Learner&) = delete;
    ~Learner() { if (pool) { DeviceScope scope(device); (void)hipFree(pool); } }
    int start(const char*) { return CN_OK; }       // what create still has to write into the zeroed pool: nothing by default
};
// cn_*_create after the checks of the configuration: Hd = the handle (cfg, layout(Pool&), start(fn)), fn = the name in the error texts
template <class Hd, class Cfg>
int learner_create(const char* fn, const Cfg& c, int device, Hd** out)
{
    const std::string f(fn);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return td3_fail(CN_ERR_NO_DEVICE, f + ": no HIP device (libcrowdnav has no CPU fallback)");
    if (device < 0 || device >= ndev) return td3_fail(CN_ERR_ARG, f + ": bad device ordinal");
    DeviceScope scope(device);
    std::unique_ptr<Hd> h(new (std::nothrow) Hd());
    if (!h) return td3_fail(CN_ERR_ARG, f + ": out of memory");
    h->cfg = c; h->device = device; h->B = c.batch; h->D = c.obs_dim; h->H = c.hidden;
    Pool count{nullptr};
    h->layout(count);
    hipError_t e = hipMalloc(&h->pool, count.size);
    if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMalloc: " + hipGetErrorString(e));
    e = hipMemset(h->pool, 0, count.size);
    if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMemset: " + hipGetErrorString(e));
    Pool assign{(char*)h->pool};
    h->layout(assign);
    if (const int rc = h->start(fn)) return rc;
    *out = h.release();
    return CN_OK;
}
// cn_*_update's argument checks: a handle, and either an explicit batch with its five arrays or a replay ring in the configuration
template <class Hd, class Batch>
int check_update(const char* fn, const Hd* h, const Batch* batch)
{
    if (!h) return td3_fail(CN_ERR_ARG, std::string(fn) + ": null handle");
    const auto& c = h->cfg;
    if (!batch && (!c.replay_s || !c.replay_a || !c.replay_r || !c.replay_s2 || !c.replay_d || !c.replay_size_dev))
        return td3_fail(CN_ERR_ARG, std::string(fn) + ": no explicit batch and no replay ring in the configuration");
    if (batch && (!batch->s || !batch->a || !batch->r || !batch->s2 || !batch->d)) return td3_fail(CN_ERR_ARG, std::string(fn) + ": null batch pointer");
    return CN_OK;
}

// cn_*_set_replay_sample: the mode of the updates enqueued from now on (a captured update keeps the kernel arguments it was captured with)
int set_replay_sample(const char* fn, Learner* h, int mode)
{
    if (!h) return td3_fail(CN_ERR_ARG, std::string(fn) + ": null handle");
    if (mode != CN_SAMPLE_WITH_REPLACEMENT && mode != CN_SAMPLE_DISTINCT)
        return td3_fail(CN_ERR_ARG, std::string(fn) + ": mode must be CN_SAMPLE_WITH_REPLACEMENT (0) or CN_SAMPLE_DISTINCT (1); the handle keeps its mode");
    h->sample_mode = mode;
    return CN_OK;
}

// What the TD3 and the DDPG handle share: the gathered batch, the two policies' activations, the actor-loss chain and Adam's state.
struct ActorCritic : Learner {
    float *xs, *x2, *r, *d, *noise, *logits;       // batch (noise: TD3 alone, null in a DDPG handle)
    float *t_h1, *t_h2, *a_h1, *a_h2;              // target actor on s2, actor on s
    float *qpart, *dapart;                         // partial sums of the critics' outputs [.][B][qnt] and of the action gradient [B][2][dant]
    float* dl;                                     // the actor's loss gradient: dlogit [B][2]
    float* adam;                                   // [2 optimizers: critic(s), actor][2]
    float* steps;                                  // [2]
    double* pw;                                    // [4] running products beta^t
    float* mom[3][6][2];                           // Adam moments: actor, critic (, second critic) x {w1, b1, w2, b2, w3, b3} x {m, v}
    int qnt() const { return (H + 15) / 16; }
    int dant() const { return (H + 31) / 32; }
    void take_moments(Pool& p, int nets)
    {
        for (int net = 0; net < nets; ++net) for (int j = 0; j < 6; ++j) for (int k = 0; k < 2; ++k)
            p.take(mom[net][j][k], param_count(net == 0 ? D : D + 2, net == 0 ? 2 : 1, H, j));
    }
    int start(const char* fn)
    {
        const double one[4] = {1.0, 1.0, 1.0, 1.0};
        const hipError_t e = hipMemcpy(pw, one, sizeof(one), hipMemcpyHostToDevice);
        return e == hipSuccess ? CN_OK : td3_fail(CN_ERR_HIP, std::string(fn) + ": hipMemcpy: " + hipGetErrorString(e));
    }
};
// the batch td3_prep_kernel gathered for the last update: written by that launch only, read (never written) by the GEMMs after it
const float* batch_dev(const ActorCritic* h, int what)
{
    if (!h) return nullptr;
    switch (what) { case 0: return h->xs; case 1: return h->x2; case 2: return h->r; case 3: return h->d; case 4: return h->noise; default: return nullptr; }
}
// td3_prep_kernel's arguments: the rows of the explicit batch, or a sample of the configuration's replay ring
template <class Cfg>
PrepArgs prep_args(const ActorCritic& h, const Cfg& c, const cn_td3_batch* batch)
{
    PrepArgs pa;
    memset(&pa, 0, sizeof(pa));
    if (batch) { pa.rs = batch->s; pa.ra = batch->a; pa.rr = batch->r; pa.rs2 = batch->s2; pa.rd = batch->d; pa.noise_in = batch->target_noise; }
    else { pa.rs = c.replay_s; pa.ra = c.replay_a; pa.rr = c.replay_r; pa.rs2 = c.replay_s2; pa.rd = c.replay_d; pa.size_dev = c.replay_size_dev; }
    pa.xs = h.xs; pa.x2 = h.x2; pa.r = h.r; pa.d = h.d; pa.noise = h.noise; pa.counter = h.counter;
    pa.seed = c.seed; pa.B = h.B; pa.D = h.D; pa.mode = h.sample_mode;
    return pa;
}
// the part of GemmArgs (zeroed by the caller) that no launch of an update changes: Adam's constants and the tick's arguments
template <class Cfg>
void adam_args(GemmArgs& ga, const ActorCritic& h, const Cfg& c, int do_actor)
{
    ga.beta1 = c.beta1; ga.beta2 = c.beta2; ga.eps = c.eps; ga.tau = c.tau;
    ga.tick.adam = h.adam; ga.tick.steps = h.steps; ga.tick.pw = h.pw; ga.tick.counter = h.counter; ga.tick.do_actor = do_actor;
    ga.tick.lr_critic = c.lr_critic; ga.tick.lr_actor = c.lr_actor; ga.tick.beta1 = c.beta1; ga.tick.beta2 = c.beta2;
}

// ---- the GemmJob builders of the three updates: every field they do not name is zero -------------------------------------------
// F: Y [I][J] = act(X [I][K] W^T + b)
void fwd_job(GemmJob& j, const float* X, int I, int ldx, int K, const float* W, const float* b, float* Y, int J, int relu)
{
    memset(&j, 0, sizeof(j));
    j.A = X; j.B = W; j.C = Y; j.bias = b; j.I = I; j.J = J; j.R = K; j.lda = ldx; j.ldb = K; j.ldc = J; j.relu = relu;
}
// F, on top of fwd_job: the last two columns of X are policy `pol`'s action on the row, evaluated from its second hidden activation h2
void head_job(GemmJob& j, int D, int H, const float* h2, const cn_td3_mlp& pol, const float* noise, float* logits, float max_v, float max_w)
{
    j.R = D; j.hd_h2 = h2; j.hd_W3 = pol.w3; j.hd_b3 = pol.b3; j.hd_noise = noise; j.hd_logits = logits; j.hd_H = H; j.hd_max_v = max_v; j.hd_max_w = max_w;
}
// G: dX [I][J] = (dY [I][R] W) (.) [mask > 0]
void dgrad_job(GemmJob& j, const float* dY, int I, int R, const float* W, const float* mask, float* dX, int J)
{
    memset(&j, 0, sizeof(j));
    j.A = dY; j.B = W; j.C = dX; j.mask = mask; j.I = I; j.J = J; j.R = R; j.lda = R; j.ldb = J; j.ldc = J;
}
// G through a critic's second layer with dY evaluated (hb_*): the TD target from q partial-sum slot `net` and the target slots
void critic_bwd_job(GemmJob& j, const ActorCritic& h, const cn_td3_mlp& crit, const float* h1, const float* h2, int net, int single, float gamma,
                    float* dq, float* dz2, float* dz1)
{
    dgrad_job(j, h2, h.B, h.H, crit.w2, h1, dz1, h.H);
    j.hb_h2 = h2; j.hb_w3 = crit.w3; j.hb_qpart = h.qpart; j.hb_qnt = h.qnt(); j.hb_net = net; j.hb_single = single; j.hb_r = h.r; j.hb_d = h.d;
    j.hb_gamma = gamma; j.hb_dq = dq; j.hb_dz2 = dz2;
}
// G through the actor's second layer with dY evaluated (ab_*): the heads' derivatives on the action gradient's partial sums
void actor_bwd_job(GemmJob& j, const ActorCritic& h, const cn_td3_mlp& actor, float max_v, float max_w, float* dz2, float* dz1)
{
    dgrad_job(j, h.a_h2, h.B, h.H, actor.w2, h.a_h1, dz1, h.H);
    j.ab_h2 = h.a_h2; j.ab_w3 = actor.w3; j.ab_dapart = h.dapart; j.ab_dant = h.dant(); j.ab_logits = h.logits;
    j.ab_max_v = max_v; j.ab_max_w = max_w; j.ab_dl = h.dl; j.ab_dz2 = dz2;
}
// H: W [I][J] stepped by dY^T [I][R] X [R][J], its bias by the row sums of dY^T; st = the optimizer's state of W, then of the bias,
// {m, v} each (RMSprop: the accumulator and null); adam = the optimizer's bias corrections; tgt / btgt = the target's copies, or null
void wgrad_job(GemmJob& j, const float* dY, int I, const float* X, int ldx, int J, int R, float* W, float* bparam, float* const (*st)[2],
               const float* adam = nullptr, float* tgt = nullptr, float* btgt = nullptr)
{
    memset(&j, 0, sizeof(j));
    j.A = dY; j.B = X; j.C = W; j.I = I; j.J = J; j.R = R; j.lda = I; j.ldb = ldx; j.ldc = J;
    j.m = st[0][0]; j.v = st[0][1]; j.bparam = bparam; j.bm = st[1][0]; j.bv = st[1][1]; j.adam = adam; j.tgt = tgt; j.btgt = btgt;
}
template <int MODE, bool GATE = false>
void launch_gemm(const GemmArgs& ga, int njobs, hipStream_t st)
{
    constexpr int TI = MODE == GEMM_H ? 32 : 16, TJ = MODE == GEMM_F ? 16 : 32;      // the kernel's tile of C
    int gx = 0, gy = 0;
    for (int z = 0; z < njobs; ++z) { const int x_ = (ga.job[z].J + TJ - 1) / TJ, y_ = (ga.job[z].I + TI - 1) / TI; gx = x_ > gx ? x_ : gx; gy = y_ > gy ? y_ : gy; }
    if (MODE == GEMM_F) hipLaunchKernelGGL(td3_fwd_kernel<GATE>, dim3(gx, gy, njobs), dim3(256), 0, st, ga);
    else if (MODE == GEMM_G) hipLaunchKernelGGL(td3_dgrad_kernel<GATE>, dim3(gx, gy, njobs), dim3(256), 0, st, ga);
    else hipLaunchKernelGGL(td3_wgrad_kernel<GATE>, dim3(gx, gy, njobs), dim3(256), 0, st, ga);
}
}  // namespace

extern "C" const char* cn_td3_last_error(void) { return g_td3_err.c_str(); }

// ---- TD3 --------------------------------------------------------------------------------------------------------------------
struct cn_td3_s : ActorCritic {
    cn_td3_config cfg;
    float *c_h1[4], *c_h2[4];               // q1, q2, q1_t, q2_t
    float *dq[2];                           // the critics' loss gradients per row (td3_dgrad_kernel's head-backward mode)
    float *dz2[2], *dz1[2];
    void layout(Pool& p)
    {
        const size_t b = B, Dc = D + 2, h = H;
        p.take(counter, 1); p.take(pw, 4);
        p.take(xs, b * Dc); p.take(x2, b * Dc); p.take(r, b); p.take(d, b); p.take(noise, 2 * b); p.take(logits, 2 * b);
        p.take(t_h1, b * h); p.take(t_h2, b * h);
        for (int z = 0; z < 4; ++z) { p.take(c_h1[z], b * h); p.take(c_h2[z], b * h); }
        p.take(qpart, 4 * b * qnt()); p.take(dapart, 2 * b * dant()); p.take(dq[0], b); p.take(dq[1], b); p.take(dl, 2 * b);
        p.take(a_h1, b * h); p.take(a_h2, b * h);
        for (int z = 0; z < 2; ++z) { p.take(dz2[z], b * h); p.take(dz1[z], b * h); }
        p.take(loss, 1); p.take(adam, 4); p.take(steps, 2);
        take_moments(p, 3);
    }
};

extern "C" int cn_td3_create(const cn_td3_config* cfg, int device, cn_td3_handle* out)
{
    if (!cfg || !out) return td3_fail(CN_ERR_ARG, "cn_td3_create: null argument");
    const cn_td3_config& c = *cfg;
    if (c.obs_dim < 1 || c.hidden < 1 || c.batch < 1 || c.batch > 4096 || c.hidden > 4096 || c.policy_delay < 1)
        return td3_fail(CN_ERR_CONFIG, "cn_td3_create: obs_dim / hidden / batch / policy_delay out of range");
    if (const int rc = check_mlps("cn_td3_create", {&c.actor, &c.actor_t, &c.q1, &c.q1_t, &c.q2, &c.q2_t})) return rc;
    return learner_create("cn_td3_create", c, device, out);
}
extern "C" void cn_td3_destroy(cn_td3_handle h) { delete h; }
extern "C" const float* cn_td3_loss_dev(cn_td3_handle h) { return h ? h->loss : nullptr; }
extern "C" const float* cn_td3_batch_dev(cn_td3_handle h, int what) { return batch_dev(h, what); }
extern "C" int cn_td3_set_replay_sample(cn_td3_handle h, int mode) { return set_replay_sample("cn_td3_set_replay_sample", h, mode); }

// The launches of one update, in order, handed to `em`: em.prep(PrepArgs), then em.gemm<MODE>(GemmArgs, njobs) per GEMM launch.
// cn_td3_update's emitter launches them as they come; a population's records them once, when the handle is created.
template <class Emit>
void td3_chain(const cn_td3_s* h, int do_actor, const cn_td3_batch* batch, Emit& em)
{
    const cn_td3_config& c = h->cfg;
    const int B = h->B, D = h->D, Dc = D + 2, H = h->H, qnt = h->qnt();
    // 0. sample / gather, noise, Adam constants
    PrepArgs pa = prep_args(*h, c, batch);
    pa.noise_std = c.noise_std; pa.noise_clip = c.noise_clip;
    em.prep(pa);
    GemmArgs ga;
    memset(&ga, 0, sizeof(ga));
    adam_args(ga, *h, c, do_actor ? 1 : 0);
    // 1-2. the target actor's hidden layers on s2 (TD3:238).  On actor updates the policy's own hidden layers on s (TD3:268; they
    // read the actor, which the critic step does not touch) ride in the same two launches as a second job.
    const int na = do_actor ? 2 : 1;
    fwd_job(ga.job[0], h->x2, B, Dc, D, c.actor_t.w1, c.actor_t.b1, h->t_h1, H, 1);
    fwd_job(ga.job[1], h->xs, B, Dc, D, c.actor.w1, c.actor.b1, h->a_h1, H, 1);
    em.template gemm<GEMM_F>(ga, na);
    fwd_job(ga.job[0], h->t_h1, B, H, H, c.actor_t.w2, c.actor_t.b2, h->t_h2, H, 1);
    fwd_job(ga.job[1], h->a_h1, B, H, H, c.actor.w2, c.actor.b2, h->a_h2, H, 1);
    em.template gemm<GEMM_F>(ga, na);
    // (3, the policies' last layer and heads, runs inside the launches that consume the actions: 4 and 13)
    // 4-6. the four critics forward: q1, q2 on (s, a); q1_t, q2_t on (s2, a2)
    const cn_td3_mlp* crit[4] = {&c.q1, &c.q2, &c.q1_t, &c.q2_t};
    for (int z = 0; z < 4; ++z) fwd_job(ga.job[z], z < 2 ? h->xs : h->x2, B, Dc, Dc, crit[z]->w1, crit[z]->b1, h->c_h1[z], H, 1);
    for (int z = 2; z < 4; ++z) head_job(ga.job[z], D, H, h->t_h2, c.actor_t, h->noise, nullptr, c.max_v, c.max_w);      // a2 = pi_t(s2) + clipped noise
    em.template gemm<GEMM_F>(ga, 4);
    // 5-6. ... their second layers, and the last (q = h2 . W3 + b3) as per-tile partial sums in the same epilogue; the tick too
    for (int z = 0; z < 4; ++z) {
        fwd_job(ga.job[z], h->c_h1[z], B, H, H, crit[z]->w2, crit[z]->b2, h->c_h2[z], H, 1);
        ga.job[z].qp_w3 = crit[z]->w3; ga.job[z].qp_b3 = crit[z]->b3; ga.job[z].qp_out = h->qpart + (size_t)z * B * qnt; ga.job[z].qp_nt = qnt;
    }
    ga.do_tick = 1;
    em.template gemm<GEMM_F>(ga, 4);
    ga.do_tick = 0;
    // 7-8. TD target, MSE gradient (per row, evaluated where it is consumed) and through the second hidden layer:
    // dz1 = (dz2 W2) (.) [h1 > 0], dz2 = dq W3 (.) [h2 > 0]   (W2, W3 are read here, stepped in 9)
    for (int z = 0; z < 2; ++z) critic_bwd_job(ga.job[z], *h, *crit[z], h->c_h1[z], h->c_h2[z], z, 0, c.gamma, h->dq[z], h->dz2[z], h->dz1[z]);
    em.template gemm<GEMM_G>(ga, 2);
    // 9. weight gradients folded into Adam: W2, b2, W1, b1 of both critics, and linear3 (dW3 = dq^T h2, db3 = sum dq: one-row jobs);
    // on actor updates the target critics follow in the same epilogue (nothing reads them again in this update)
    for (int z = 0; z < 2; ++z) {
        const cn_td3_mlp none = {}, &t = do_actor ? *crit[2 + z] : none;
        wgrad_job(ga.job[z], h->dz2[z], H, h->c_h1[z], H, H, B, crit[z]->w2, crit[z]->b2, &h->mom[1 + z][2], h->adam, t.w2, t.b2);
        wgrad_job(ga.job[2 + z], h->dz1[z], H, h->xs, Dc, Dc, B, crit[z]->w1, crit[z]->b1, &h->mom[1 + z][0], h->adam, t.w1, t.b1);
        wgrad_job(ga.job[4 + z], h->dq[z], 1, h->c_h2[z], H, H, B, crit[z]->w3, crit[z]->b3, &h->mom[1 + z][4], h->adam, t.w3, t.b3);
    }
    ga.job[4].loss_out = h->loss;                                 // the first critic's MSE: what Agent.learn returns
    em.template gemm<GEMM_H>(ga, 6);
    if (do_actor) {
        // (10-11, the policy's hidden layers on s, ran inside launches 1-2; 12, its head, runs inside 13)
        // 13-14. the UPDATED first critic on (s, pi(s)) (TD3:268)
        fwd_job(ga.job[0], h->xs, B, Dc, Dc, c.q1.w1, c.q1.b1, h->c_h1[0], H, 1);    // (xs's own action columns are not read: head_job)
        head_job(ga.job[0], D, H, h->a_h2, c.actor, nullptr, h->logits, c.max_v, c.max_w);        // pi(s)
        em.template gemm<GEMM_F>(ga, 1);
        fwd_job(ga.job[0], h->c_h1[0], B, H, H, c.q1.w2, c.q1.b2, h->c_h2[0], H, 1);
        ga.job[0].dz_w3 = c.q1.w3; ga.job[0].dz_out = h->dz2[0]; ga.job[0].dz_rows = (float)B;      // 15. -mean Q's gradient at h2, in the epilogue
        em.template gemm<GEMM_F>(ga, 1);
        // 16-17. ... back to the action, through the heads, linear3 of the actor + Adam
        dgrad_job(ga.job[0], h->dz2[0], B, H, c.q1.w2, h->c_h1[0], h->dz1[0], H);
        ga.job[0].da_w = c.q1.w1 + D; ga.job[0].da_ld = Dc; ga.job[0].da_out = h->dapart; ga.job[0].da_nt = h->dant();     // the action columns of W1
        em.template gemm<GEMM_G>(ga, 1);
        // 17-19. through the heads' derivatives and the actor's hidden layers (the heads' part evaluated inside the backward GEMM,
        // linear3's gradient dl^T h2 as a two-row job of the weight-gradient launch)
        actor_bwd_job(ga.job[0], *h, c.actor, c.max_v, c.max_w, h->dz2[1], h->dz1[1]);
        em.template gemm<GEMM_G>(ga, 1);
        wgrad_job(ga.job[0], h->dz2[1], H, h->a_h1, H, H, B, c.actor.w2, c.actor.b2, &h->mom[0][2], h->adam + 2, c.actor_t.w2, c.actor_t.b2);
        wgrad_job(ga.job[1], h->dz1[1], H, h->xs, Dc, D, B, c.actor.w1, c.actor.b1, &h->mom[0][0], h->adam + 2, c.actor_t.w1, c.actor_t.b1);
        wgrad_job(ga.job[2], h->dl, 2, h->a_h2, H, H, B, c.actor.w3, c.actor.b3, &h->mom[0][4], h->adam + 2, c.actor_t.w3, c.actor_t.b3);
        em.template gemm<GEMM_H>(ga, 3);
        // (20, the soft updates of the three targets, ran in the Adam epilogues of 7, 9, 17 and 19)
    }
}
namespace {
struct Td3LaunchNow {                              // cn_td3_update: every launch goes to the stream as the chain names it
    hipStream_t st;
    void prep(const PrepArgs& pa) { hipLaunchKernelGGL(td3_prep_kernel<false>, dim3(pa.B), dim3(256), 0, st, pa); }
    template <int MODE> void gemm(const GemmArgs& ga, int njobs) { launch_gemm<MODE>(ga, njobs, st); }
};
}  // namespace

extern "C" int cn_td3_update(cn_td3_handle h, int do_actor, const cn_td3_batch* batch, void* stream)
{
    if (const int rc = check_update("cn_td3_update", h, batch)) return rc;
    DeviceScope scope(h->device);
    Td3LaunchNow em{(hipStream_t)stream};
    td3_chain(h, do_actor, batch, em);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

// ---- a population of TD3 learners: P members' updates in the 7 (+ 5) launches of one --------------------------------------------
// Member p's jobs are what td3_chain gives for a solo handle of cfgs[p]; they ride in the grid's z dimension (z = p * njobs + job)
// of the kernels' POP = true instantiations, which read them from tables in device memory.  A handle's pointers never change, so the
// tables of both chains (do_actor 0 / 1) and of both sampling modes are built and uploaded once, in cn_td3_pop_create;
// cn_td3_pop_update only enqueues.
namespace {
struct PopStep { int mode, njobs, do_tick, gx, gy; size_t first; };      // one GEMM launch: its jobs are table[first + p * njobs + z]
struct Td3Record {                                 // td3_chain's emitter at create time: keeps what a solo update would have launched
    struct Step { int mode, njobs, do_tick; GemmJob job[6]; };
    PrepArgs pa;
    TickArgs tick;
    Step step[12];
    int n = 0;
    void prep(const PrepArgs& p) { pa = p; }
    template <int MODE> void gemm(const GemmArgs& ga, int njobs)
    {
        if (n >= 12 || njobs > 6) return;             // (an update is at most 11 GEMM launches of at most 6 jobs)
        Step& s = step[n++];
        s.mode = MODE; s.njobs = njobs; s.do_tick = ga.do_tick; tick = ga.tick;
        for (int z = 0; z < njobs; ++z) s.job[z] = ga.job[z];
    }
};
}  // namespace
struct cn_td3_pop_s {
    int device = 0, P = 0, B = 0;
    int sample_mode = CN_SAMPLE_WITH_REPLACEMENT;
    float beta1 = 0.f, beta2 = 0.f, eps = 0.f, tau = 0.f;
    std::vector<std::unique_ptr<cn_td3_s>> mem;    // the members' workspaces and Adam state: solo handles that are never updated alone
    void* tables = nullptr;                        // one allocation: losses [P], prep tables [2 modes][P], tick tables [2 chains][P], jobs
    float* loss = nullptr;
    const PrepArgs* prep[2] = {nullptr, nullptr};
    const TickArgs* tick[2] = {nullptr, nullptr};
    const GemmJob* jobs = nullptr;
    std::vector<PopStep> chain[2];
    cn_td3_pop_s() = default;
    cn_td3_pop_s(const cn_td3_pop_s&) = delete;
    ~cn_td3_pop_s() { if (tables) { DeviceScope scope(device); (void)hipFree(tables); } }
};

extern "C" int cn_td3_pop_create(const cn_td3_config* cfgs, int n_members, int device, cn_td3_pop_handle* out)
{
    const std::string f("cn_td3_pop_create");
    if (!cfgs || !out) return td3_fail(CN_ERR_ARG, f + ": null argument");
    if (n_members < 1 || n_members > 64) return td3_fail(CN_ERR_ARG, f + ": n_members must be 1 ... 64");
    const int P = n_members;
    const cn_td3_config& c0 = cfgs[0];
    struct Named { const float* p; int member; const char* what; };
    std::vector<Named> named;
    for (int p = 0; p < P; ++p) {
        const cn_td3_config& c = cfgs[p];
        const std::string who = "member " + std::to_string(p);
        if (c.obs_dim < 1 || c.hidden < 1 || c.batch < 1 || c.batch > 4096 || c.hidden > 4096 || c.policy_delay < 1)
            return td3_fail(CN_ERR_CONFIG, f + ": " + who + ": obs_dim / hidden / batch / policy_delay out of range");
        // the grid and the launch-level scalars are one for all members
        const char* differs = c.obs_dim != c0.obs_dim ? "obs_dim" : c.hidden != c0.hidden ? "hidden" : c.batch != c0.batch ? "batch"
            : c.policy_delay != c0.policy_delay ? "policy_delay" : c.beta1 != c0.beta1 ? "beta1" : c.beta2 != c0.beta2 ? "beta2"
            : c.eps != c0.eps ? "eps" : c.tau != c0.tau ? "tau" : c.max_v != c0.max_v ? "max_v" : c.max_w != c0.max_w ? "max_w" : nullptr;
        if (differs) return td3_fail(CN_ERR_CONFIG, f + ": " + who + " differs from member 0 in " + differs + " (the members share it)");
        if (!mlp_ok(c.actor) || !mlp_ok(c.actor_t) || !mlp_ok(c.q1) || !mlp_ok(c.q1_t) || !mlp_ok(c.q2) || !mlp_ok(c.q2_t))
            return td3_fail(CN_ERR_ARG, f + ": " + who + ": null parameter pointer");
        if (!c.replay_s || !c.replay_a || !c.replay_r || !c.replay_s2 || !c.replay_d || !c.replay_size_dev)
            return td3_fail(CN_ERR_ARG, f + ": " + who + ": no replay ring in the configuration (a population has no explicit-batch form)");
        const cn_td3_mlp* nets[6] = {&c.actor, &c.actor_t, &c.q1, &c.q1_t, &c.q2, &c.q2_t};
        static const char* const netn[6] = {"actor", "actor_t", "q1", "q1_t", "q2", "q2_t"};
        for (int n = 0; n < 6; ++n)
            for (const float* t : {nets[n]->w1, nets[n]->b1, nets[n]->w2, nets[n]->b2, nets[n]->w3, nets[n]->b3}) named.push_back({t, p, netn[n]});
    }
    // two members stepping one tensor would race inside a launch: every parameter tensor belongs to one member
    std::sort(named.begin(), named.end(), [](const Named& a, const Named& b) { return a.p != b.p ? a.p < b.p : a.member < b.member; });
    for (size_t i = 1; i < named.size(); ++i)
        if (named[i].p == named[i - 1].p && named[i].member != named[i - 1].member)
            return td3_fail(CN_ERR_CONFIG, f + ": members " + std::to_string(named[i - 1].member) + " (" + named[i - 1].what + ") and " +
                            std::to_string(named[i].member) + " (" + named[i].what + ") name the same parameter tensor");
    std::unique_ptr<cn_td3_pop_s> h(new (std::nothrow) cn_td3_pop_s());
    if (!h) return td3_fail(CN_ERR_ARG, f + ": out of memory");
    h->device = device; h->P = P; h->B = c0.batch;
    h->beta1 = c0.beta1; h->beta2 = c0.beta2; h->eps = c0.eps; h->tau = c0.tau;
    for (int p = 0; p < P; ++p) {
        cn_td3_s* m = nullptr;
        if (const int rc = learner_create(f.c_str(), cfgs[p], device, &m)) return rc;
        h->mem.emplace_back(m);
    }
    DeviceScope scope(device);
    // record what a solo update of every member would launch, for both chains (GEMMs, tick); the job tables' size follows from it
    std::vector<Td3Record> rec[2];
    size_t njobs_all = 0;
    for (int a = 0; a < 2; ++a) {
        rec[a].resize(P);
        for (int p = 0; p < P; ++p) td3_chain(h->mem[p].get(), a, nullptr, rec[a][p]);
        for (int k = 0; k < rec[a][0].n; ++k) njobs_all += (size_t)P * rec[a][0].step[k].njobs;
    }
    Pool count{nullptr};
    float* loss = nullptr; PrepArgs* prep[2] = {nullptr, nullptr}; TickArgs* tick[2] = {nullptr, nullptr}; GemmJob* jobs = nullptr;
    auto layout = [&](Pool& pl) {
        pl.take(loss, (size_t)P);
        for (int q = 0; q < 2; ++q) pl.take(prep[q], (size_t)P);
        for (int q = 0; q < 2; ++q) pl.take(tick[q], (size_t)P);
        pl.take(jobs, njobs_all);
    };
    layout(count);
    hipError_t e = hipMalloc(&h->tables, count.size);
    if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMalloc: " + hipGetErrorString(e));
    e = hipMemset(h->tables, 0, count.size);
    if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMemset: " + hipGetErrorString(e));
    Pool assign{(char*)h->tables};
    layout(assign);
    // the losses lie side by side: a member writes pop loss [p], not its own handle's (recorded again below, with that pointer)
    std::vector<PrepArgs> hprep((size_t)2 * P);
    std::vector<TickArgs> htick((size_t)2 * P);
    std::vector<GemmJob> hjobs(njobs_all);
    size_t first = 0;
    for (int a = 0; a < 2; ++a) {
        for (int p = 0; p < P; ++p) {
            cn_td3_s* m = h->mem[p].get();
            m->loss = loss + p;
            for (int mode : {CN_SAMPLE_DISTINCT, CN_SAMPLE_WITH_REPLACEMENT}) {      // (ends on the mode a fresh handle has)
                m->sample_mode = mode;
                rec[a][p].n = 0;
                td3_chain(m, a, nullptr, rec[a][p]);
                hprep[(size_t)mode * P + p] = rec[a][p].pa;
            }
            htick[(size_t)a * P + p] = rec[a][p].tick;
        }
        for (int k = 0; k < rec[a][0].n; ++k) {
            const Td3Record::Step& s0 = rec[a][0].step[k];
            constexpr int TI[3] = {16, 16, 32}, TJ[3] = {16, 32, 32};      // the kernels' tiles of C (launch_gemm)
            PopStep ps{s0.mode, s0.njobs, s0.do_tick, 0, 0, first};
            for (int z = 0; z < s0.njobs; ++z) {
                const int x_ = (s0.job[z].J + TJ[s0.mode] - 1) / TJ[s0.mode], y_ = (s0.job[z].I + TI[s0.mode] - 1) / TI[s0.mode];
                ps.gx = x_ > ps.gx ? x_ : ps.gx; ps.gy = y_ > ps.gy ? y_ : ps.gy;
            }
            if (first + (size_t)P * s0.njobs > hjobs.size()) return td3_fail(CN_ERR_ARG, f + ": job table size");      // (never: counted above)
            for (int p = 0; p < P; ++p)
                for (int z = 0; z < s0.njobs; ++z) hjobs[first + (size_t)p * s0.njobs + z] = rec[a][p].step[k].job[z];
            first += (size_t)P * s0.njobs;
            h->chain[a].push_back(ps);
        }
    }
    static_assert(CN_SAMPLE_WITH_REPLACEMENT == 0 && CN_SAMPLE_DISTINCT == 1, "the prep tables are indexed by the mode");
    for (int q = 0; q < 2; ++q) {
        e = hipMemcpy(prep[q], hprep.data() + (size_t)q * P, sizeof(PrepArgs) * P, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(tick[q], htick.data() + (size_t)q * P, sizeof(TickArgs) * P, hipMemcpyHostToDevice);
        if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMemcpy: " + hipGetErrorString(e));
        h->prep[q] = prep[q]; h->tick[q] = tick[q];
    }
    e = hipMemcpy(jobs, hjobs.data(), sizeof(GemmJob) * hjobs.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMemcpy: " + hipGetErrorString(e));
    h->loss = loss; h->jobs = jobs;
    *out = h.release();
    return CN_OK;
}
extern "C" void cn_td3_pop_destroy(cn_td3_pop_handle h) { delete h; }
extern "C" int cn_td3_pop_members(cn_td3_pop_handle h) { return h ? h->P : 0; }
extern "C" const float* cn_td3_pop_loss_dev(cn_td3_pop_handle h) { return h ? h->loss : nullptr; }
extern "C" const float* cn_td3_pop_batch_dev(cn_td3_pop_handle h, int member, int what)
{
    return (h && member >= 0 && member < h->P) ? batch_dev(h->mem[member].get(), what) : nullptr;
}
extern "C" int cn_td3_pop_set_replay_sample(cn_td3_pop_handle h, int mode)
{
    if (!h) return td3_fail(CN_ERR_ARG, "cn_td3_pop_set_replay_sample: null handle");
    if (mode != CN_SAMPLE_WITH_REPLACEMENT && mode != CN_SAMPLE_DISTINCT)
        return td3_fail(CN_ERR_ARG, "cn_td3_pop_set_replay_sample: mode must be CN_SAMPLE_WITH_REPLACEMENT (0) or CN_SAMPLE_DISTINCT (1); the handle keeps its mode");
    h->sample_mode = mode;
    return CN_OK;
}

extern "C" int cn_td3_pop_update(cn_td3_pop_handle h, int do_actor, void* stream)
{
    if (!h) return td3_fail(CN_ERR_ARG, "cn_td3_pop_update: null handle");
    DeviceScope scope(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int a = do_actor ? 1 : 0;
    hipLaunchKernelGGL(td3_prep_kernel<true>, dim3(h->B, h->P), dim3(256), 0, st, h->prep[h->sample_mode]);
    for (const PopStep& s : h->chain[a]) {
        const PopGemmArgs ga{h->jobs + s.first, h->tick[a], s.njobs, h->beta1, h->beta2, h->eps, h->tau, s.do_tick};
        const dim3 grid(s.gx, s.gy, h->P * s.njobs);
        if (s.mode == GEMM_F) hipLaunchKernelGGL((td3_fwd_kernel<false, true>), grid, dim3(256), 0, st, ga);
        else if (s.mode == GEMM_G) hipLaunchKernelGGL((td3_dgrad_kernel<false, true>), grid, dim3(256), 0, st, ga);
        else hipLaunchKernelGGL((td3_wgrad_kernel<false, true>), grid, dim3(256), 0, st, ga);
    }
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

// ---- DDPG (ddpg.py:198-243 of the reference: Agent.learn) on the same three GEMM kernels -----------------------------------
// One critic and its target, no policy delay, no target-policy noise.  The actor loss -mean Q(s, pi(s)) is back-propagated
// BEFORE the critic's step (ddpg.py:226-238), so both gradients are taken at the pre-update weights and the two branches share
// launches.  8 launches:  prep | actor_t L1 (+ actor L1) | L2 (+ L2) | critic_t L1 on (s2, pi_t(s2)), critic L1 on (s, a) and on
// (s, pi(s)) | their L2 (+ q partials of critic_t and critic, dz on the pi(s) branch, tick) | G (critic: dq, dz2 evaluated;
// pi(s) branch: da partials) | G (actor: dl, dz2a evaluated) | H (six jobs: critic and actor W1 / W2 / W3 + Adam + soft updates).
struct cn_ddpg_s : ActorCritic {
    cn_ddpg_config cfg;
    float *c_h1[3], *c_h2[3];                // critic on (s, a), critic on (s, pi(s)), critic_t on (s2, pi_t(s2)); q partials: slots 0 and 2
    float* dq;
    float *dz2c, *dz1c, *dz2p, *dz1p, *dz2a, *dz1a;   // critic step, pi(s) branch through the critic, actor
    void layout(Pool& p)
    {
        const size_t b = B, Dc = D + 2, h = H;
        p.take(counter, 1); p.take(pw, 4);
        p.take(xs, b * Dc); p.take(x2, b * Dc); p.take(r, b); p.take(d, b); p.take(logits, 2 * b);
        p.take(t_h1, b * h); p.take(t_h2, b * h); p.take(a_h1, b * h); p.take(a_h2, b * h);
        for (int z = 0; z < 3; ++z) { p.take(c_h1[z], b * h); p.take(c_h2[z], b * h); }
        for (float** f : {&dz2c, &dz1c, &dz2p, &dz1p, &dz2a, &dz1a}) p.take(*f, b * h);
        p.take(qpart, 3 * b * qnt()); p.take(dapart, 2 * b * dant()); p.take(dq, b); p.take(dl, 2 * b);
        p.take(loss, 1); p.take(adam, 4); p.take(steps, 2);
        take_moments(p, 2);
    }
};

extern "C" int cn_ddpg_create(const cn_ddpg_config* cfg, int device, cn_ddpg_handle* out)
{
    if (!cfg || !out) return td3_fail(CN_ERR_ARG, "cn_ddpg_create: null argument");
    const cn_ddpg_config& c = *cfg;
    if (c.obs_dim < 1 || c.hidden < 1 || c.batch < 1 || c.batch > 4096 || c.hidden > 4096)
        return td3_fail(CN_ERR_CONFIG, "cn_ddpg_create: obs_dim / hidden / batch out of range");
    if (const int rc = check_mlps("cn_ddpg_create", {&c.actor, &c.actor_t, &c.critic, &c.critic_t})) return rc;
    return learner_create("cn_ddpg_create", c, device, out);
}
extern "C" void cn_ddpg_destroy(cn_ddpg_handle h) { delete h; }
extern "C" const float* cn_ddpg_loss_dev(cn_ddpg_handle h) { return h ? h->loss : nullptr; }
extern "C" const float* cn_ddpg_batch_dev(cn_ddpg_handle h, int what) { return batch_dev(h, what); }     // no target noise (what 4: NULL)
extern "C" int cn_ddpg_set_replay_sample(cn_ddpg_handle h, int mode) { return set_replay_sample("cn_ddpg_set_replay_sample", h, mode); }

extern "C" int cn_ddpg_update(cn_ddpg_handle h, const cn_td3_batch* batch, void* stream)
{
    if (const int rc = check_update("cn_ddpg_update", h, batch)) return rc;
    if (batch && batch->target_noise) return td3_fail(CN_ERR_ARG, "cn_ddpg_update: DDPG has no target-policy noise (batch->target_noise must be NULL)");
    const cn_ddpg_config& c = h->cfg;
    DeviceScope scope(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int B = h->B, D = h->D, Dc = D + 2, H = h->H, qnt = h->qnt();
    // 1. sample / gather (ddpg.py:208-214); no noise is drawn
    const PrepArgs pa = prep_args(*h, c, batch);
    hipLaunchKernelGGL(td3_prep_kernel<false>, dim3(B), dim3(256), 0, st, pa);
    GemmArgs ga;
    memset(&ga, 0, sizeof(ga));
    adam_args(ga, *h, c, 1);                        // both optimizers step on every update
    // 2-3. actor_t's hidden layers on s2 (ddpg.py:219), actor's on s (:216)
    fwd_job(ga.job[0], h->x2, B, Dc, D, c.actor_t.w1, c.actor_t.b1, h->t_h1, H, 1);
    fwd_job(ga.job[1], h->xs, B, Dc, D, c.actor.w1, c.actor.b1, h->a_h1, H, 1);
    launch_gemm<GEMM_F>(ga, 2, st);
    fwd_job(ga.job[0], h->t_h1, B, H, H, c.actor_t.w2, c.actor_t.b2, h->t_h2, H, 1);
    fwd_job(ga.job[1], h->a_h1, B, H, H, c.actor.w2, c.actor.b2, h->a_h2, H, 1);
    launch_gemm<GEMM_F>(ga, 2, st);
    // 4. the critics' first layers: critic on (s, a) (:229), critic on (s, pi(s)) (:216, the logits kept for the heads' backward),
    // critic_t on (s2, pi_t(s2)) (:220) -- the policies' last layers and heads evaluated in place of the action columns, no noise
    fwd_job(ga.job[0], h->xs, B, Dc, Dc, c.critic.w1, c.critic.b1, h->c_h1[0], H, 1);
    fwd_job(ga.job[1], h->xs, B, Dc, Dc, c.critic.w1, c.critic.b1, h->c_h1[1], H, 1);
    head_job(ga.job[1], D, H, h->a_h2, c.actor, nullptr, h->logits, c.max_v, c.max_w);
    fwd_job(ga.job[2], h->x2, B, Dc, Dc, c.critic_t.w1, c.critic_t.b1, h->c_h1[2], H, 1);
    head_job(ga.job[2], D, H, h->t_h2, c.actor_t, nullptr, nullptr, c.max_v, c.max_w);
    launch_gemm<GEMM_F>(ga, 3, st);
    // 5. their second layers; q = h2 . W3 + b3 as per-tile partial sums of critic (slot 0) and critic_t (slot 2); on the pi(s)
    // branch the first link of -mean Q (:217): dz = -(1 / B) W3 [h2 > 0]; the tick
    fwd_job(ga.job[0], h->c_h1[0], B, H, H, c.critic.w2, c.critic.b2, h->c_h2[0], H, 1);
    ga.job[0].qp_w3 = c.critic.w3; ga.job[0].qp_b3 = c.critic.b3; ga.job[0].qp_out = h->qpart; ga.job[0].qp_nt = qnt;
    fwd_job(ga.job[1], h->c_h1[1], B, H, H, c.critic.w2, c.critic.b2, h->c_h2[1], H, 1);
    ga.job[1].dz_w3 = c.critic.w3; ga.job[1].dz_out = h->dz2p; ga.job[1].dz_rows = (float)B;
    fwd_job(ga.job[2], h->c_h1[2], B, H, H, c.critic_t.w2, c.critic_t.b2, h->c_h2[2], H, 1);
    ga.job[2].qp_w3 = c.critic_t.w3; ga.job[2].qp_b3 = c.critic_t.b3; ga.job[2].qp_out = h->qpart + (size_t)2 * B * qnt; ga.job[2].qp_nt = qnt;
    ga.do_tick = 1;
    launch_gemm<GEMM_F>(ga, 3, st);
    ga.do_tick = 0;
    // 6. both through the PRE-update critic: the TD target y = r + (1 - d) gamma q_t (:221-222, one target), the MSE gradient
    // (:230) and dz1 = (dz2 W2) [h1 > 0]; the pi(s) branch on to the action (the two action columns of W1)
    critic_bwd_job(ga.job[0], *h, c.critic, h->c_h1[0], h->c_h2[0], 0, 1, c.gamma, h->dq, h->dz2c, h->dz1c);
    dgrad_job(ga.job[1], h->dz2p, B, H, c.critic.w2, h->c_h1[1], h->dz1p, H);
    ga.job[1].da_w = c.critic.w1 + D; ga.job[1].da_ld = Dc; ga.job[1].da_out = h->dapart; ga.job[1].da_nt = h->dant();
    launch_gemm<GEMM_G>(ga, 2, st);
    // 7. the actor: through the heads' derivatives and its second hidden layer
    actor_bwd_job(ga.job[0], *h, c.actor, c.max_v, c.max_w, h->dz2a, h->dz1a);
    launch_gemm<GEMM_G>(ga, 1, st);
    // 8. weight gradients folded into both Adam steps (:233-238) and the soft updates of both targets (:241-242, from the
    // stepped weights); linear3's gradients are the one- / two-row jobs; loss_out = the critic's MSE
    wgrad_job(ga.job[0], h->dz2c, H, h->c_h1[0], H, H, B, c.critic.w2, c.critic.b2, &h->mom[1][2], h->adam, c.critic_t.w2, c.critic_t.b2);
    wgrad_job(ga.job[1], h->dz1c, H, h->xs, Dc, Dc, B, c.critic.w1, c.critic.b1, &h->mom[1][0], h->adam, c.critic_t.w1, c.critic_t.b1);
    wgrad_job(ga.job[2], h->dq, 1, h->c_h2[0], H, H, B, c.critic.w3, c.critic.b3, &h->mom[1][4], h->adam, c.critic_t.w3, c.critic_t.b3);
    ga.job[2].loss_out = h->loss;
    wgrad_job(ga.job[3], h->dz2a, H, h->a_h1, H, H, B, c.actor.w2, c.actor.b2, &h->mom[0][2], h->adam + 2, c.actor_t.w2, c.actor_t.b2);
    wgrad_job(ga.job[4], h->dz1a, H, h->xs, Dc, D, B, c.actor.w1, c.actor.b1, &h->mom[0][0], h->adam + 2, c.actor_t.w1, c.actor_t.b1);
    wgrad_job(ga.job[5], h->dl, 2, h->a_h2, H, H, B, c.actor.w3, c.actor.b3, &h->mom[0][4], h->adam + 2, c.actor_t.w3, c.actor_t.b3);
    launch_gemm<GEMM_H>(ga, 6, st);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

// ---- DQN (deepq.py of the reference: learnOnMiniBatch, selectAction) -----------------------------------------------------------
// The update (deepq.py:219-266 with memory.py:22-28 and Keras's fit(batch_size = 64, epochs = 1, shuffle)), 16 launches:
//   prep   sample B rows (with replacement, td3_prep_kernel's hash), gather [s; s2] as 2B stacked rows; one extra workgroup lays
//          out X_batch (sample m's s, then its s2 when final: 64 + F rows), draws the shuffle, marks chunk 1 (the first B shuffled
//          rows) and chunk 2 (the F after them), and publishes the gates
//   F x 3  online net L1 / L2 / L3 on the 2B rows, target net on the B s2 rows (its result is read only after the first copy)
//   T      Y and dq of chunk 1 (rows outside the chunk: dq = 0); the loss
//   G x 2, H   backward, weight gradients folded into RMSprop (td3_wgrad_kernel<true>; gate: the update is live)
//   F x 3, T, G x 2, H   chunk 2 on the stepped weights against the same Y: all seven return at once on the device when F = 0
//   (every GEMM here is a GATE = true instantiation; the TD3 / DDPG launches use GATE = false, the parent's instructions)
//   copy   the hard target copy when this update is the target_every-th, and the update counter
namespace {
struct DqnPrepArgs {
    const float *rs, *rr, *rs2, *rd;               // replay ring / explicit batch: s, s2 rows `ld` floats apart
    const float* ra;                               // replay: actions [.][2], the index in column 0 (or null)
    const int32_t* a_in;                           // explicit batch: action indices [B] (or null)
    const int32_t* perm_in;                        // explicit shuffle of the B + F X_batch rows, or null = drawn here
    const int64_t* size_dev;                       // live replay size, or null = the rows ARE the batch
    float *x, *r, *d; int32_t* a;                  // [2B][ld], [B], [B], [B]
    int32_t *chunk, *flags;                        // [2B], [8]
    const unsigned long long* counter; unsigned long long* kcur;
    uint64_t seed;
    int B, ld, D, learn_start, target_every;
    int mode;                                      // CN_SAMPLE_*
};
__device__ __forceinline__ size_t dqn_row(const DqnPrepArgs& p, int m, unsigned long long cnt)
{
    if (!p.size_dev) return (size_t)m;
    return cn_replay_row(p.seed, cnt, m, p.size_dev, p.mode);
}
__global__ void __launch_bounds__(256) dqn_prep_kernel(DqnPrepArgs p)
{
    const int B = p.B, tid = threadIdx.x;
    const unsigned long long cnt = *p.counter;
    if ((int)blockIdx.x < 2 * B) {                 // gather one stacked row
        const int g = blockIdx.x, m = g < B ? g : g - B;
        const size_t row = dqn_row(p, m, cnt);
        const float* src = (g < B ? p.rs : p.rs2) + row * (size_t)p.ld;
        float* dst = p.x + (size_t)g * p.ld;
        for (int c = tid; c < p.D; c += blockDim.x) dst[c] = src[c];
        if (g < B && tid == 0) {
            p.r[m] = p.rr[row]; p.d[m] = p.rd[row];
            p.a[m] = p.a_in ? p.a_in[m] : (int32_t)p.ra[row * 2];
        }
        return;
    }
    // the plan (the last workgroup), in LDS: perm, order and the shuffle's draws as int16 [2B] each, the final flags [B]
    extern __shared__ __align__(8) unsigned char dqn_plan_lds[];
    int16_t* perm = (int16_t*)dqn_plan_lds;
    int16_t* order = perm + 2 * B;
    int16_t* jr = order + 2 * B;
    uint8_t* fin = (uint8_t*)(jr + 2 * B);
    __shared__ int n_rows;
    const bool live = !p.size_dev || *p.size_dev > (int64_t)p.learn_start;
    for (int m = tid; m < B; m += blockDim.x) fin[m] = p.rd[dqn_row(p, m, cnt)] != 0.f ? 1 : 0;
    for (int g = tid; g < 2 * B; g += blockDim.x) p.chunk[g] = 0;
    __syncthreads();
    if (tid == 0) {                                // X_batch order (deepq.py:248-262): s_m, then s2_m when final
        int n = 0;
        for (int m = 0; m < B; ++m) { order[n++] = (int16_t)m; if (fin[m]) order[n++] = (int16_t)(B + m); }
        n_rows = n;
    }
    __syncthreads();
    const int n = n_rows, F = n - B;
    if (p.perm_in) { for (int i = tid; i < n; i += blockDim.x) perm[i] = (int16_t)p.perm_in[i]; }
    else {                                         // Fisher-Yates keyed by (seed, update counter): draws in parallel, swaps in order
        for (int i = tid; i < n; i += blockDim.x) {
            const uint64_t h = cn_mix64(cn_mix64(p.seed ^ cn_mix64(cnt ^ 0x3c6ef372fe94f82bull)) ^ (uint64_t)(uint32_t)i);
            perm[i] = (int16_t)i;
            jr[i] = (int16_t)(h % (uint64_t)(i + 1));
        }
        __syncthreads();
        if (tid == 0)
            for (int i = n - 1; i > 0; --i) { const int j = jr[i]; const int16_t t = perm[i]; perm[i] = perm[j]; perm[j] = t; }
    }
    __syncthreads();
    if (live)
        for (int i = tid; i < n; i += blockDim.x) {
            const int xr = perm[i];
            if (xr >= 0 && xr < n) p.chunk[order[xr]] = i < B ? 1 : 2;
        }
    if (tid != 0) return;
    *p.kcur = cnt;
    p.flags[0] = live ? 1 : 0;
    p.flags[1] = (live && F > 0) ? 1 : 0;
    p.flags[2] = F;
    p.flags[3] = cnt >= (unsigned long long)p.target_every ? 1 : 0;            // Q' = the target net after the first copy
    p.flags[4] = (live && (cnt + 1ull) % (unsigned long long)p.target_every == 0ull) ? 1 : 0;
}
// Y (deepq.py:240-262, once, before either step) and dq = 2 (q - Y) / (3 n_chunk) of the rows of chunk `which` (Keras mse: the mean
// over the 3 outputs, then over the chunk's rows); one workgroup.  which == 1 also writes Y and the chunk's loss.
struct DqnTargetArgs {
    const float *q, *tq, *r, *d; const int32_t *a, *chunk, *flags;   // q: this chunk's forward (chunk 1: the pre-step Q)
    float *Y, *dq, *loss;
    float gamma; int B, which;
};
__global__ void __launch_bounds__(256) dqn_target_kernel(DqnTargetArgs p)
{
    __shared__ float red[256];
    if (p.flags[p.which - 1] == 0) {               // nothing to step: not live yet (chunk 1), or F = 0 (chunk 2)
        if (p.which == 2 && threadIdx.x == 0) p.loss[1] = 0.f;
        return;
    }
    const int B = p.B, F = p.flags[2];
    const float n = p.which == 1 ? (float)B : (float)(F > 0 ? F : 1);
    float ls = 0.f;
    for (int g = threadIdx.x; g < 2 * B; g += blockDim.x) {
        const float* q = p.q + (size_t)g * 3;
        float y[3];
        if (p.which == 1) {
            const int m = g < B ? g : g - B;
            if (g < B) {
                const float* qn = p.flags[3] ? p.tq + (size_t)m * 3 : p.q + (size_t)(B + m) * 3;
                const float mx = fmaxf(fmaxf(qn[0], qn[1]), qn[2]);
                const float t = p.d[m] != 0.f ? p.r[m] : p.r[m] + p.gamma * mx;
                y[0] = q[0]; y[1] = q[1]; y[2] = q[2];
                const int a = p.a[m];
                if (a >= 0 && a < 3) y[a] = t;
            } else {
                y[0] = y[1] = y[2] = p.r[m];           // a final sample's extra row: [r, r, r]
            }
#pragma unroll
            for (int o = 0; o < 3; ++o) p.Y[(size_t)g * 3 + o] = y[o];
        } else {
#pragma unroll
            for (int o = 0; o < 3; ++o) y[o] = p.Y[(size_t)g * 3 + o];
        }
        const bool in = p.chunk[g] == p.which;
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const float e = q[o] - y[o];
            p.dq[(size_t)g * 3 + o] = in ? 2.f * e / (3.f * n) : 0.f;
            if (in) ls = fmaf(e, e, ls);
        }
    }
    red[threadIdx.x] = ls;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) p.loss[p.which - 1] = red[0] / (3.f * n);
}
// the hard copy online -> target (deepq.py:136-148) when flags[4] is set; the update counter
struct DqnCopyArgs { const float* src[6]; float* dst[6]; long long n[6]; const int32_t* flags; unsigned long long* counter; const unsigned long long* kcur; };
__global__ void __launch_bounds__(256) dqn_copy_kernel(DqnCopyArgs p)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.flags[0]) *p.counter = *p.kcur + 1ull;
    if (!p.flags[4]) return;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (int t = 0; t < 6; ++t)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n[t]; i += stride) p.dst[t][i] = p.src[t][i];
}

// Action selection (start_dqn_training.py:103-104: getQValues, selectAction) for 16 rows per workgroup: both hidden layers on the
// f32 matrix cores with the activations in LDS (hidden padded to a multiple of 32 with zero units), the 3-way head, argmax with
// ties to the lowest index (np.argmax), and the epsilon draw keyed by (seed, counter, row).
struct DqnActArgs {
    const float* obs; int64_t ld; int n, D, H, Hp;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    double eps0, disc, eps_min; const int64_t* episodes_dev;
    uint64_t seed, counter;
    int32_t* action; float* twist; float* q;
};
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
__global__ void __launch_bounds__(256) dqn_act_kernel(DqnActArgs p)
{
    extern __shared__ float dqn_lds[];
    float* h1 = dqn_lds;
    float* h2 = dqn_lds + 16 * p.Hp;
    __shared__ float qs[16][3];
    __shared__ double eps_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.x * 16;
    if (tid == 0) {       // the epsilon of the episode under way: start_dqn_training.py:89-90 applied once per episode begun
        double e = p.eps0;
        if (p.episodes_dev && p.disc < 1.0) {
            const long long E = *p.episodes_dev;
            // (bounded: eps_min > 0 and disc < 1 end the loop after log(eps_min / eps0) / log(disc) steps; the cap only guards
            // against a discount so close to 1 that the schedule would take longer than any run has episodes)
            for (long long k = 0; k <= E && k < (1ll << 22) && e > p.eps_min; ++k) e *= p.disc;
        }
        eps_s = e;
    }
    dqn_act_layer(p.obs + (size_t)min(i0 + li, p.n - 1) * p.ld, p.D, p.w1, p.b1, p.H, h1, p.Hp, wave, li, lk);
    __syncthreads();
    dqn_act_layer(h1 + li * p.Hp, p.H, p.w2, p.b2, p.H, h2, p.Hp, wave, li, lk);      // (h1's row in LDS; the reduction over its H units)
    __syncthreads();
    if (tid < 192) {      // q[r][o] = h2[r] . W3[o] + b3[o]: 4 lanes per (row, output), units n = part mod 4
        const int r = tid / 12, o = (tid % 12) >> 2, part = tid & 3;
        const float* __restrict__ w = p.w3 + (size_t)o * p.H;
        float s = 0.f;
        for (int nn = part; nn < p.H; nn += 4) s = fmaf(h2[r * p.Hp + nn], w[nn], s);
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
        if (part == 0) qs[r][o] = s + p.b3[o];
    }
    __syncthreads();
    if (tid < 16 && i0 + tid < p.n) {
        const int i = i0 + tid;
        const float q0 = qs[tid][0], q1 = qs[tid][1], q2 = qs[tid][2];
        int best = 0; float bq = q0;
        if (q1 > bq) { best = 1; bq = q1; }
        if (q2 > bq) { best = 2; }
        const uint64_t h = cn_mix64(cn_mix64(p.seed ^ cn_mix64(p.counter ^ 0x2545f4914f6cdd1dull)) ^ (uint64_t)(uint32_t)i);
        const double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);             // random.random(): 53 bits in [0, 1)
        const uint64_t h2_ = cn_mix64(h ^ 0x9e3779b97f4a7c15ull);
        const int pick = (int)(((h2_ >> 32) * 3ull) >> 32);                           // np.random.randint(0, 3)
        const int act = u < eps_s ? pick : best;
        p.action[i] = act;
        // environment_stage_1_original.py:412-425: (0.22, 0), (0.22, 2.0), (0.22, -2.0)
        p.twist[2 * i] = 0.22f; p.twist[2 * i + 1] = act == 0 ? 0.f : act == 1 ? 2.0f : -2.0f;
        if (p.q) { p.q[3 * i] = q0; p.q[3 * i + 1] = q1; p.q[3 * i + 2] = q2; }
    }
}
}  // namespace

struct cn_dqn_s : Learner {
    cn_dqn_config cfg;
    float *x, *r, *d, *h1, *h2, *th1, *th2, *q, *q2, *tq, *Y, *dq, *dz2, *dz1;   // q: pre-step Q, q2: chunk 2's
    int32_t *a, *chunk, *flags;
    unsigned long long* kcur;
    float* acc[6][2];                              // RMSprop accumulators of w1, b1, w2, b2, w3, b3 ([.][1]: null, Adam's second moment)
    size_t params(int j) const { return param_count(D, 3, H, j); }
    void layout(Pool& p)
    {
        const size_t b = B, ld = cfg.obs_ld, h = H;
        p.take(counter, 1); p.take(kcur, 1);
        p.take(x, 2 * b * ld); p.take(r, b); p.take(d, b);
        p.take(h1, 2 * b * h); p.take(h2, 2 * b * h); p.take(th1, b * h); p.take(th2, b * h);
        p.take(q, 2 * b * 3); p.take(Y, 2 * b * 3); p.take(dq, 2 * b * 3); p.take(q2, 2 * b * 3); p.take(tq, b * 3);
        p.take(dz2, 2 * b * h); p.take(dz1, 2 * b * h); p.take(loss, 2);
        p.take(a, b); p.take(chunk, 2 * b); p.take(flags, 8);
        for (int j = 0; j < 6; ++j) p.take(acc[j][0], params(j));
    }
};

extern "C" int cn_dqn_create(const cn_dqn_config* cfg, int device, cn_dqn_handle* out)
{
    if (!cfg || !out) return td3_fail(CN_ERR_ARG, "cn_dqn_create: null argument");
    const cn_dqn_config& c = *cfg;
    if (c.obs_dim < 1 || c.obs_ld < c.obs_dim || c.hidden < 1 || c.hidden > 4096 || c.batch < 1 || c.batch > 4096 || c.target_every < 1 || c.learn_start < 0)
        return td3_fail(CN_ERR_CONFIG, "cn_dqn_create: obs_dim / obs_ld / hidden / batch / target_every / learn_start out of range");
    if (const int rc = check_mlps("cn_dqn_create", {&c.q, &c.q_t})) return rc;
    return learner_create("cn_dqn_create", c, device, out);
}
extern "C" void cn_dqn_destroy(cn_dqn_handle h) { delete h; }
extern "C" const float* cn_dqn_loss_dev(cn_dqn_handle h) { return h ? h->loss : nullptr; }
extern "C" int cn_dqn_set_replay_sample(cn_dqn_handle h, int mode) { return set_replay_sample("cn_dqn_set_replay_sample", h, mode); }

extern "C" const void* cn_dqn_batch_dev(cn_dqn_handle h, int what)
{
    if (!h) return nullptr;
    switch (what) {
        case 0: return h->x; case 1: return h->r; case 2: return h->d; case 3: return h->a; case 4: return h->chunk;
        case 5: return h->flags; case 6: return h->Y; case 7: return h->q; case 8: return h->counter; default: return nullptr;
    }
}

extern "C" int cn_dqn_update(cn_dqn_handle h, const cn_dqn_batch* batch, void* stream)
{
    if (const int rc = check_update("cn_dqn_update", h, batch)) return rc;
    const cn_dqn_config& c = h->cfg;
    DeviceScope scope(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int B = h->B, D = h->D, ld = c.obs_ld, H = h->H;
    DqnPrepArgs pa;
    memset(&pa, 0, sizeof(pa));
    if (batch) { pa.rs = batch->s; pa.rs2 = batch->s2; pa.rr = batch->r; pa.rd = batch->d; pa.a_in = batch->a; pa.perm_in = batch->perm; }
    else { pa.rs = c.replay_s; pa.rs2 = c.replay_s2; pa.rr = c.replay_r; pa.rd = c.replay_d; pa.ra = c.replay_a; pa.size_dev = c.replay_size_dev; }
    pa.x = h->x; pa.r = h->r; pa.d = h->d; pa.a = h->a; pa.chunk = h->chunk; pa.flags = h->flags;
    pa.counter = h->counter; pa.kcur = h->kcur; pa.seed = c.seed; pa.B = B; pa.ld = ld; pa.D = D;
    pa.learn_start = c.learn_start; pa.target_every = c.target_every; pa.mode = h->sample_mode;
    hipLaunchKernelGGL(dqn_prep_kernel, dim3(2 * B + 1), dim3(256), (size_t)(13 * B + 8) / 8 * 8, st, pa);

    GemmArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.rms_lr = c.lr; ga.rms_rho = c.rho; ga.rms_eps = c.eps;
    // every GEMM of a chunk is gated on the device (the launches of chunk 2 return at once when F = 0; all of them while the replay
    // path waits for learn_start)
    auto forward = [&](int chunk) {               // online net on the 2B stacked rows (+ chunk 1: the target net on the B s2 rows)
        const int nj = chunk == 1 ? 2 : 1;
        float* q = chunk == 1 ? h->q : h->q2;
        ga.rms_gate = h->flags + (chunk - 1);
        fwd_job(ga.job[0], h->x, 2 * B, ld, D, c.q.w1, c.q.b1, h->h1, H, 1);
        fwd_job(ga.job[1], h->x + (size_t)B * ld, B, ld, D, c.q_t.w1, c.q_t.b1, h->th1, H, 1);
        launch_gemm<GEMM_F, true>(ga, nj, st);
        fwd_job(ga.job[0], h->h1, 2 * B, H, H, c.q.w2, c.q.b2, h->h2, H, 1);
        fwd_job(ga.job[1], h->th1, B, H, H, c.q_t.w2, c.q_t.b2, h->th2, H, 1);
        launch_gemm<GEMM_F, true>(ga, nj, st);
        fwd_job(ga.job[0], h->h2, 2 * B, H, H, c.q.w3, c.q.b3, q, 3, 0);
        fwd_job(ga.job[1], h->th2, B, H, H, c.q_t.w3, c.q_t.b3, h->tq, 3, 0);
        launch_gemm<GEMM_F, true>(ga, nj, st);
    };
    auto target = [&](int which) {
        DqnTargetArgs ta;
        ta.q = which == 1 ? h->q : h->q2; ta.tq = h->tq; ta.r = h->r; ta.d = h->d; ta.a = h->a; ta.chunk = h->chunk; ta.flags = h->flags;
        ta.Y = h->Y; ta.dq = h->dq; ta.loss = h->loss; ta.gamma = c.gamma; ta.B = B; ta.which = which;
        hipLaunchKernelGGL(dqn_target_kernel, dim3(1), dim3(256), 0, st, ta);
    };
    auto backward = [&](const int* gate) {        // dz2 = (dq W3) [h2 > 0], dz1 = (dz2 W2) [h1 > 0], then RMSprop of all six tensors
        ga.rms_gate = gate;
        dgrad_job(ga.job[0], h->dq, 2 * B, 3, c.q.w3, h->h2, h->dz2, H);
        launch_gemm<GEMM_G, true>(ga, 1, st);
        dgrad_job(ga.job[0], h->dz2, 2 * B, H, c.q.w2, h->h1, h->dz1, H);
        launch_gemm<GEMM_G, true>(ga, 1, st);
        wgrad_job(ga.job[0], h->dz2, H, h->h1, H, H, 2 * B, c.q.w2, c.q.b2, &h->acc[2]);
        wgrad_job(ga.job[1], h->dz1, H, h->x, ld, D, 2 * B, c.q.w1, c.q.b1, &h->acc[0]);
        wgrad_job(ga.job[2], h->dq, 3, h->h2, H, H, 2 * B, c.q.w3, c.q.b3, &h->acc[4]);
        launch_gemm<GEMM_H, true>(ga, 3, st);
    };
    // chunk 1 (its Y from the pre-step nets), then chunk 2 on the stepped weights (gated off on the device when F = 0)
    forward(1);
    target(1);
    backward(h->flags + 0);
    forward(2);
    target(2);
    backward(h->flags + 1);
    DqnCopyArgs ca;
    const float* src[6] = {c.q.w1, c.q.b1, c.q.w2, c.q.b2, c.q.w3, c.q.b3};
    float* dst[6] = {c.q_t.w1, c.q_t.b1, c.q_t.w2, c.q_t.b2, c.q_t.w3, c.q_t.b3};
    for (int j = 0; j < 6; ++j) { ca.src[j] = src[j]; ca.dst[j] = dst[j]; ca.n[j] = (long long)h->params(j); }
    ca.flags = h->flags; ca.counter = h->counter; ca.kcur = h->kcur;
    hipLaunchKernelGGL(dqn_copy_kernel, dim3(128), dim3(256), 0, st, ca);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_dqn_act(const cn_dqn_act_io* io, int device, void* stream)
{
    if (!io || !io->obs || !io->action || !io->twist) return td3_fail(CN_ERR_ARG, "cn_dqn_act: null argument");
    if (!mlp_ok(io->q)) return td3_fail(CN_ERR_ARG, "cn_dqn_act: null parameter pointer");
    if (io->n < 1 || io->obs_dim < 1 || io->obs_ld < io->obs_dim || io->hidden < 1 || io->hidden > 480)
        return td3_fail(CN_ERR_CONFIG, "cn_dqn_act: n / obs_dim / obs_ld / hidden out of range (hidden <= 480: two 16-row activations in 64 KB of LDS)");
    if (!(io->epsilon_discount >= 0.0 && io->epsilon_discount <= 1.0) || !(io->epsilon_min > 0.0))
        return td3_fail(CN_ERR_CONFIG, "cn_dqn_act: epsilon_discount outside [0, 1] or epsilon_min <= 0");
    DeviceScope scope(device);
    DqnActArgs p;
    p.obs = io->obs; p.ld = io->obs_ld; p.n = io->n; p.D = io->obs_dim; p.H = io->hidden; p.Hp = (io->hidden + 31) / 32 * 32;
    p.w1 = io->q.w1; p.b1 = io->q.b1; p.w2 = io->q.w2; p.b2 = io->q.b2; p.w3 = io->q.w3; p.b3 = io->q.b3;
    p.eps0 = io->epsilon; p.disc = io->epsilon_discount; p.eps_min = io->epsilon_min; p.episodes_dev = io->episodes_dev;
    p.seed = io->seed; p.counter = io->counter; p.action = io->action; p.twist = io->twist; p.q = io->q_out;
    const size_t lds = (size_t)2 * 16 * p.Hp * sizeof(float);
    hipLaunchKernelGGL(dqn_act_kernel, dim3((io->n + 15) / 16), dim3(256), lds, (hipStream_t)stream, p);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

// ---- SAC (sac.py of the reference: Agent.learn :231-290, Actor.evaluate :78-93, Agent.act :206-229) ----------------------------
// The three GEMM kernels above are used as they stand (their code paths, arguments and resources are the parent's); what SAC adds
// is row-wise and lives in kernels of its own.  The update, 10 launches (11 with the soft update as the reference wrote it):
//   prep    td3_prep_kernel: sample / gather [s | a], s2, r, d; the unit normal eps [B][2] (noise_std 1, no clip)
//   F       first layers of actor (s), Q (s, a), V (s), V_t (s2): four jobs
//   F       their second layers; Q(s, a), V(s), V_t(s2) as per-tile partial sums (qp_*)
//   head    sac_head_kernel: both heads, clamp, std, z = eps std + mean, t = tanh z, log_prob, the double squash; [s | a_new]; the tick
//   F, F    Q on (s, a_new), its output as partial sums
//   loss    sac_loss_kernel: the three losses, the per-row loss gradients dq, dv, d(mean, log_std), and the gradients at the three
//           second hidden layers (one output row per network: no reduction, so no GEMM)
//   G       through the second layers of Q, V and the actor: three jobs
//   H, H    weight gradients folded into the three Adam steps: Q and V (six jobs), the actor and its two heads (four jobs;
//           GemmArgs holds six)
//   pull    soft_update 0 only: V <- (1 - tau) V + tau V_t (sac.py:290 as written)
// Why not fewer: Q(s, a_new) needs the action, the action needs the trunk (F, F, head, F, F), every loss needs Q(s, a_new) or
// V_t(s2) (loss), and backward is G then H.  The head and the loss could ride in the GEMMs' epilogues as the hd_ / hb_ modes do
// for TD3 -- that means new branches inside td3_fwd_kernel / td3_dgrad_kernel, whose registers the TD3 and DDPG updates pay for;
// they are kept out of those kernels on purpose.  The ten weight-gradient jobs need two launches of a six-job GemmArgs.
// The three optimisers step on every update, so they share one step count; each has its own learning rate in the tick.
namespace {
enum { SAC_REC = 12 };     // per-row record: mean[2], log_std[2] (clamped), raw log_std[2], z[2], log_prob, Q(s, a_new), a_new[2]
struct SacHeadArgs {
    const float *h2, *mean_w, *mean_b, *ls_w, *ls_b, *eps, *xs;
    float *xn, *rec;
    int B, D, H, deterministic;
    float max_v, max_w, ls_min, ls_max, logp_eps;
    // the tick (block 0, thread 0)
    float* adam; float* steps; double* pw; unsigned long long* counter;
    float lr[3], beta1, beta2;
};
// one row's head: mean / log_std from the four dot products, then everything Actor.evaluate derives from them
__device__ __forceinline__ void sac_squash(float mean[2], const float lsraw[2], const float eps[2], int deterministic, float ls_min, float ls_max,
                                           float logp_eps, float max_v, float max_w, float* rec)
{
    float logp = 0.f, t[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float ls = fminf(fmaxf(lsraw[k], ls_min), ls_max);                    // SAC:72
        const float sd = expf(ls);
        const float z = deterministic ? mean[k] : eps[k] * sd + mean[k];            // Normal.sample: randn * std + mean, multiply then add
        t[k] = tanhf(z);
        const float dz = z - mean[k];
        // Normal.log_prob (torch.distributions): -(z - mean)^2 / (2 var) - log(std) - log(sqrt(2 pi));  SAC:86
        logp += -(dz * dz) / (2.f * (sd * sd)) - logf(sd) - 0.91893853320467274f - logf(1.f - t[k] * t[k] + logp_eps);
        rec[k] = mean[k]; rec[2 + k] = ls; rec[4 + k] = lsraw[k]; rec[6 + k] = z;
    }
    rec[8] = logp;
    rec[10] = max_v / (1.f + expf(-t[0]));                                           // SAC:90-91: the second squash
    rec[11] = max_w * tanhf(t[1]);
}
__global__ void __launch_bounds__(256) sac_head_kernel(SacHeadArgs p)
{
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, H = p.H, Dc = p.D + 2;
    if (m == 0 && tid == 0) {
        *p.counter += 1ull;
        p.steps[0] += 1.f;
        const double c1 = p.pw[0] * (double)p.beta1, c2 = p.pw[1] * (double)p.beta2;
        p.pw[0] = c1; p.pw[1] = c2;
#pragma unroll
        for (int o = 0; o < 3; ++o) { p.adam[2 * o] = p.lr[o] / (float)(1.0 - c1); p.adam[2 * o + 1] = sqrtf((float)(1.0 - c2)); }
    }
    __shared__ float red[4][4];
    const float* __restrict__ h = p.h2 + (size_t)m * H;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n = tid; n < H; n += 256) {
        const float hv = h[n];
        s[0] = fmaf(hv, p.mean_w[n], s[0]); s[1] = fmaf(hv, p.mean_w[H + n], s[1]);
        s[2] = fmaf(hv, p.ls_w[n], s[2]); s[3] = fmaf(hv, p.ls_w[H + n], s[3]);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) { s[o] = td3_wave_sum(s[o]); if (lane == 0) red[wave][o] = s[o]; }
    for (int c = tid; c < p.D; c += 256) p.xn[(size_t)m * Dc + c] = p.xs[(size_t)m * Dc + c];
    __syncthreads();
    if (tid == 0) {
        float d4[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) d4[o] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
        float mean[2] = {d4[0] + p.mean_b[0], d4[1] + p.mean_b[1]};
        const float lsraw[2] = {d4[2] + p.ls_b[0], d4[3] + p.ls_b[1]};
        const float eps[2] = {p.eps[2 * m], p.eps[2 * m + 1]};
        float* rec = p.rec + (size_t)m * SAC_REC;
        sac_squash(mean, lsraw, eps, p.deterministic, p.ls_min, p.ls_max, p.logp_eps, p.max_v, p.max_w, rec);
        rec[9] = 0.f;
        p.xn[(size_t)m * Dc + p.D] = rec[10]; p.xn[(size_t)m * Dc + p.D + 1] = rec[11];
    }
}
struct SacLossArgs {
    const float *qpart, *r, *d;                    // partial sums: slots 0 Q(s, a), 1 V(s), 2 V_t(s2), 3 Q(s, a_new)
    float* rec;
    const float *h2q, *h2v, *h2a, *w3q, *w3v, *mean_w, *ls_w;
    float *dq, *dv, *dl, *dz2q, *dz2v, *dz2a, *loss;
    int B, H, Hv, qnt, vnt, pnt;
    float gamma, ls_min, ls_max, mean_lambda, std_lambda, z_lambda;
};
struct SacRow { float q, v, vt, qn, y, logp, c; };
__device__ __forceinline__ float sac_psum(const float* __restrict__ pp, int nt) { float a = 0.f; for (int t = 0; t < nt; ++t) a += pp[t]; return a; }
__device__ __forceinline__ SacRow sac_row(const SacLossArgs& p, int m)
{
    SacRow w;
    const size_t B = p.B;
    const size_t slot = B * p.pnt;
    w.q = sac_psum(p.qpart + (size_t)m * p.qnt, p.qnt);
    w.v = sac_psum(p.qpart + slot + (size_t)m * p.vnt, p.vnt);
    w.vt = sac_psum(p.qpart + 2 * slot + (size_t)m * p.vnt, p.vnt);
    w.qn = sac_psum(p.qpart + 3 * slot + (size_t)m * p.qnt, p.qnt);
    w.y = p.r[m] + (1.f - p.d[m]) * p.gamma * w.vt;                 // SAC:258
    w.logp = p.rec[(size_t)m * SAC_REC + 8];
    w.c = w.logp - (w.qn - w.v);                                    // SAC:265-266: log_prob - log_prob_target, detached
    return w;
}
__global__ void __launch_bounds__(256) sac_loss_kernel(SacLossArgs p)
{
    const int m = blockIdx.x, tid = threadIdx.x, B = p.B, H = p.H;
    __shared__ float sh[8];
    __shared__ float lred[256][6];
    if (tid == 0) {
        const SacRow w = sac_row(p, m);
        float* rec = p.rec + (size_t)m * SAC_REC;
        rec[9] = w.qn;
        const float fb = (float)B;
        const float dq = 2.f * (w.q - w.y) / fb;                     // MSE(Q(s, a), y)                      SAC:259
        const float dv = 2.f * (w.v - (w.qn - w.logp)) / fb;         // MSE(V(s), Q(s, a_new) - log_prob)    SAC:262-263
        p.dq[m] = dq; p.dv[m] = dv;
        sh[0] = dq; sh[1] = dv;
        const float coef = w.c / fb;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float mean = rec[k], ls = rec[2 + k], raw = rec[4 + k], z = rec[6 + k];
            const float sd = expf(ls), var = sd * sd, dz = z - mean;
            // z is a value (Normal.sample, not rsample): log_prob reaches the actor through Normal.log_prob's mean and std only
            const float gm = coef * dz / var + p.mean_lambda * mean / fb;                                   // mean(mean^2) over [B][2]
            const bool inside = raw >= p.ls_min && raw <= p.ls_max;                                          // clamp's gradient mask
            const float gs = inside ? coef * (dz * dz / var - 1.f) + p.std_lambda * ls / fb : 0.f;
            p.dl[4 * m + k] = gm; p.dl[4 * m + 2 + k] = gs;
            sh[2 + k] = gm; sh[4 + k] = gs;
        }
    }
    __syncthreads();
    const float dq = sh[0], dv = sh[1], gm0 = sh[2], gm1 = sh[3], gs0 = sh[4], gs1 = sh[5];
    for (int k = tid; k < H; k += 256) {
        const size_t o = (size_t)m * H + k;
        p.dz2q[o] = p.h2q[o] > 0.f ? dq * p.w3q[k] : 0.f;
        p.dz2a[o] = p.h2a[o] > 0.f ? fmaf(gs1, p.ls_w[H + k], fmaf(gs0, p.ls_w[k], fmaf(gm1, p.mean_w[H + k], gm0 * p.mean_w[k]))) : 0.f;
    }
    for (int k = tid; k < p.Hv; k += 256) {
        const size_t o = (size_t)m * p.Hv + k;
        p.dz2v[o] = p.h2v[o] > 0.f ? dv * p.w3v[k] : 0.f;
    }
    if (m != 0) return;
    // the three losses: block 0 walks every row again (a few partial sums each), rows strided over the threads, fixed order
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < B; i += 256) {
        const SacRow w = sac_row(p, i);
        const float* rec = p.rec + (size_t)i * SAC_REC;
        const float eq = w.q - w.y, ev = w.v - (w.qn - w.logp);
        a[0] = fmaf(eq, eq, a[0]); a[1] = fmaf(ev, ev, a[1]); a[2] = fmaf(w.logp, w.c, a[2]);
        a[3] += rec[0] * rec[0] + rec[1] * rec[1]; a[4] += rec[2] * rec[2] + rec[3] * rec[3]; a[5] += rec[6] * rec[6] + rec[7] * rec[7];
    }
#pragma unroll
    for (int o = 0; o < 6; ++o) lred[tid][o] = a[o];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int o = 0; o < 6; ++o) lred[tid][o] += lred[tid + s][o];
        __syncthreads();
    }
    if (tid == 0) {
        const float fb = (float)B;
        p.loss[0] = lred[0][0] / fb;
        p.loss[1] = lred[0][1] / fb;
        p.loss[2] = lred[0][2] / fb + p.mean_lambda * lred[0][3] / (2.f * fb) + p.std_lambda * lred[0][4] / (2.f * fb) + p.z_lambda * lred[0][5] / fb;   // SAC:266-272
    }
}
// sac.py:290 as written: soft_update(local = V_t, target = V) -- V is pulled towards its frozen copy
struct SacPullArgs { float* v[6]; const float* vt[6]; long long n[6]; float tau; };
__global__ void __launch_bounds__(256) sac_pull_kernel(SacPullArgs p)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (int t = 0; t < 6; ++t)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n[t]; i += stride) p.v[t][i] = td3_soft(p.v[t][i], p.vt[t][i], p.tau);
}
// Agent.act (SAC:206-229) for 16 rows per workgroup: the trunk as dqn_act_kernel's, both heads, the sample, the double squash, the clip
struct SacActArgs {
    const float* obs; int64_t ld; int n, D, H, Hp, deterministic;
    cn_sac_actor a;
    float max_v, max_w, ls_min, ls_max;
    const float* eps_in; uint64_t seed, counter;
    float *twist, *mean, *log_std, *z;
};
__global__ void __launch_bounds__(256) sac_act_kernel(SacActArgs p)
{
    extern __shared__ float dqn_lds[];
    float* h1 = dqn_lds;
    float* h2 = dqn_lds + 16 * p.Hp;
    __shared__ float hs[16][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.x * 16;
    dqn_act_layer(p.obs + (size_t)min(i0 + li, p.n - 1) * p.ld, p.D, p.a.w1, p.a.b1, p.H, h1, p.Hp, wave, li, lk);
    __syncthreads();
    dqn_act_layer(h1 + li * p.Hp, p.H, p.a.w2, p.a.b2, p.H, h2, p.Hp, wave, li, lk);
    __syncthreads();
    {     // 16 rows x 4 head outputs x 4 lanes: units n = part mod 4
        const int r = tid >> 4, o = (tid & 15) >> 2, part = tid & 3;
        const float* __restrict__ w = (o < 2 ? p.a.mean_w : p.a.log_std_w) + (size_t)(o & 1) * p.H;
        float s = 0.f;
        for (int nn = part; nn < p.H; nn += 4) s = fmaf(h2[r * p.Hp + nn], w[nn], s);
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64);
        if (part == 0) hs[r][o] = s + (o < 2 ? p.a.mean_b[o] : p.a.log_std_b[o - 2]);
    }
    __syncthreads();
    if (tid < 16 && i0 + tid < p.n) {
        const int i = i0 + tid;
        float eps[2] = {0.f, 0.f};
        if (p.eps_in) { eps[0] = p.eps_in[2 * i]; eps[1] = p.eps_in[2 * i + 1]; }
        else if (!p.deterministic) {      // Box-Muller on a counter-based pair, keyed by (seed, call counter, row): td3_prep_kernel's draw
            const uint64_t h = cn_mix64(cn_mix64(p.seed ^ cn_mix64(p.counter ^ 0x5bd1e995u)) ^ (uint64_t)(uint32_t)i);
            const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777217.0f);
            const float u2 = (float)(uint32_t)((h >> 8) & 0xffffffu) * (1.0f / 16777216.0f);
            const float rr = sqrtf(-2.0f * logf(u1));
            eps[0] = rr * cosf(6.28318530718f * u2); eps[1] = rr * sinf(6.28318530718f * u2);
        }
        float mean[2] = {hs[tid][0], hs[tid][1]};
        const float lsraw[2] = {hs[tid][2], hs[tid][3]};
        float rec[SAC_REC];
        sac_squash(mean, lsraw, eps, p.deterministic, p.ls_min, p.ls_max, 1e-6f, p.max_v, p.max_w, rec);
        p.twist[2 * i] = fminf(fmaxf(rec[10], 0.f), p.max_v);                          // SAC:223-224
        p.twist[2 * i + 1] = fminf(fmaxf(rec[11], -p.max_w), p.max_w);
        if (p.mean) { p.mean[2 * i] = rec[0]; p.mean[2 * i + 1] = rec[1]; }
        if (p.log_std) { p.log_std[2 * i] = rec[2]; p.log_std[2 * i + 1] = rec[3]; }
        if (p.z) { p.z[2 * i] = rec[6]; p.z[2 * i + 1] = rec[7]; }
    }
}
}  // namespace

struct cn_sac_s : Learner {
    cn_sac_config cfg;
    int Hv = 0;
    float *xs, *x2, *xn, *r, *d, *eps, *rec;
    float *a_h1, *a_h2, *q_h1, *q_h2, *n_h1, *n_h2, *v_h1, *v_h2, *t_h1, *t_h2;     // actor, Q(s, a), Q(s, a_new), V, V_t
    float *qpart, *dq, *dv, *dl;
    float *dz2q, *dz1q, *dz2a, *dz1a, *dz2v, *dz1v;
    float *adam, *steps; double* pw;
    float* mom_a[8][2]; float* mom_q[6][2]; float* mom_v[6][2];
    int qnt() const { return (H + 15) / 16; }
    int vnt() const { return (Hv + 15) / 16; }
    int pnt() const { return qnt() > vnt() ? qnt() : vnt(); }      // a partial-sum slot is [B][pnt]
    void layout(Pool& p)
    {
        Hv = cfg.hidden_v;
        const size_t b = B, Dc = D + 2, h = H, hv = Hv;
        p.take(counter, 1); p.take(pw, 2);
        p.take(xs, b * Dc); p.take(x2, b * Dc); p.take(xn, b * Dc); p.take(r, b); p.take(d, b); p.take(eps, 2 * b); p.take(rec, SAC_REC * b);
        for (float** f : {&a_h1, &a_h2, &q_h1, &q_h2, &n_h1, &n_h2, &dz2q, &dz1q, &dz2a, &dz1a}) p.take(*f, b * h);
        for (float** f : {&v_h1, &v_h2, &t_h1, &t_h2, &dz2v, &dz1v}) p.take(*f, b * hv);
        p.take(qpart, 4 * b * pnt()); p.take(dq, b); p.take(dv, b); p.take(dl, 4 * b);
        p.take(loss, 3); p.take(adam, 6); p.take(steps, 1);
        const size_t na[8] = {h * D, h, h * h, h, 2 * h, 2, 2 * h, 2};
        for (int j = 0; j < 8; ++j) for (int k = 0; k < 2; ++k) p.take(mom_a[j][k], na[j]);
        for (int j = 0; j < 6; ++j) for (int k = 0; k < 2; ++k) { p.take(mom_q[j][k], param_count(D + 2, 1, H, j)); p.take(mom_v[j][k], param_count(D, 1, Hv, j)); }
    }
    int start(const char* fn)
    {
        const double one[2] = {1.0, 1.0};
        const hipError_t e = hipMemcpy(pw, one, sizeof(one), hipMemcpyHostToDevice);
        return e == hipSuccess ? CN_OK : td3_fail(CN_ERR_HIP, std::string(fn) + ": hipMemcpy: " + hipGetErrorString(e));
    }
};

namespace {
bool sac_actor_ok(const cn_sac_actor& a) { return a.w1 && a.b1 && a.w2 && a.b2 && a.mean_w && a.mean_b && a.log_std_w && a.log_std_b; }
}

extern "C" int cn_sac_create(const cn_sac_config* cfg, int device, cn_sac_handle* out)
{
    if (!cfg || !out) return td3_fail(CN_ERR_ARG, "cn_sac_create: null argument");
    const cn_sac_config& c = *cfg;
    if (c.obs_dim < 1 || c.hidden < 1 || c.hidden_v < 1 || c.batch < 1 || c.batch > 4096 || c.hidden > 4096 || c.hidden_v > 4096)
        return td3_fail(CN_ERR_CONFIG, "cn_sac_create: obs_dim / hidden / hidden_v / batch out of range");
    if (!(c.log_std_min <= c.log_std_max)) return td3_fail(CN_ERR_CONFIG, "cn_sac_create: log_std_min > log_std_max");
    if (c.soft_update != 0 && c.soft_update != 1) return td3_fail(CN_ERR_CONFIG, "cn_sac_create: soft_update must be 0 (as written) or 1 (intended)");
    if (!sac_actor_ok(c.actor)) return td3_fail(CN_ERR_ARG, "cn_sac_create: null parameter pointer");
    if (const int rc = check_mlps("cn_sac_create", {&c.q, &c.v, &c.v_t})) return rc;
    return learner_create("cn_sac_create", c, device, out);
}
extern "C" void cn_sac_destroy(cn_sac_handle h) { delete h; }
extern "C" const float* cn_sac_loss_dev(cn_sac_handle h) { return h ? h->loss : nullptr; }
extern "C" int cn_sac_set_replay_sample(cn_sac_handle h, int mode) { return set_replay_sample("cn_sac_set_replay_sample", h, mode); }
extern "C" const float* cn_sac_batch_dev(cn_sac_handle h, int what)
{
    if (!h) return nullptr;
    switch (what) {
        case 0: return h->xs; case 1: return h->x2; case 2: return h->r; case 3: return h->d; case 4: return h->eps;
        case 5: return h->rec; case 6: return h->dl; case 7: return h->dq; case 8: return h->dv; default: return nullptr;
    }
}

extern "C" int cn_sac_update(cn_sac_handle h, const cn_td3_batch* batch, void* stream)
{
    if (const int rc = check_update("cn_sac_update", h, batch)) return rc;
    const cn_sac_config& c = h->cfg;
    DeviceScope scope(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int B = h->B, D = h->D, Dc = D + 2, H = h->H, Hv = h->Hv, qnt = h->qnt(), vnt = h->vnt();
    const size_t slot = (size_t)B * h->pnt();
    // 1. sample / gather; eps = the unit normal (the explicit batch's target_noise, or td3_prep_kernel's keyed draw, scale 1, no clip)
    PrepArgs pa;
    memset(&pa, 0, sizeof(pa));
    if (batch) { pa.rs = batch->s; pa.ra = batch->a; pa.rr = batch->r; pa.rs2 = batch->s2; pa.rd = batch->d; pa.noise_in = batch->target_noise; }
    else { pa.rs = c.replay_s; pa.ra = c.replay_a; pa.rr = c.replay_r; pa.rs2 = c.replay_s2; pa.rd = c.replay_d; pa.size_dev = c.replay_size_dev; }
    pa.xs = h->xs; pa.x2 = h->x2; pa.r = h->r; pa.d = h->d; pa.noise = h->eps; pa.counter = h->counter;
    pa.seed = c.seed; pa.B = B; pa.D = D; pa.noise_std = 1.f; pa.noise_clip = 3.4e38f;       // (eps x 1, clipped at a bound no draw reaches)
    pa.mode = h->sample_mode;
    hipLaunchKernelGGL(td3_prep_kernel<false>, dim3(B), dim3(256), 0, st, pa);
    GemmArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.beta1 = c.beta1; ga.beta2 = c.beta2; ga.eps = c.eps; ga.tau = c.tau;
    // 2-3. every forward pass that does not need the new action, on the pre-update weights (SAC:253-257)
    fwd_job(ga.job[0], h->xs, B, Dc, D, c.actor.w1, c.actor.b1, h->a_h1, H, 1);
    fwd_job(ga.job[1], h->xs, B, Dc, Dc, c.q.w1, c.q.b1, h->q_h1, H, 1);
    fwd_job(ga.job[2], h->xs, B, Dc, D, c.v.w1, c.v.b1, h->v_h1, Hv, 1);
    fwd_job(ga.job[3], h->x2, B, Dc, D, c.v_t.w1, c.v_t.b1, h->t_h1, Hv, 1);
    launch_gemm<GEMM_F>(ga, 4, st);
    fwd_job(ga.job[0], h->a_h1, B, H, H, c.actor.w2, c.actor.b2, h->a_h2, H, 1);
    fwd_job(ga.job[1], h->q_h1, B, H, H, c.q.w2, c.q.b2, h->q_h2, H, 1);
    ga.job[1].qp_w3 = c.q.w3; ga.job[1].qp_b3 = c.q.b3; ga.job[1].qp_out = h->qpart; ga.job[1].qp_nt = qnt;
    fwd_job(ga.job[2], h->v_h1, B, Hv, Hv, c.v.w2, c.v.b2, h->v_h2, Hv, 1);
    ga.job[2].qp_w3 = c.v.w3; ga.job[2].qp_b3 = c.v.b3; ga.job[2].qp_out = h->qpart + slot; ga.job[2].qp_nt = vnt;
    fwd_job(ga.job[3], h->t_h1, B, Hv, Hv, c.v_t.w2, c.v_t.b2, h->t_h2, Hv, 1);
    ga.job[3].qp_w3 = c.v_t.w3; ga.job[3].qp_b3 = c.v_t.b3; ga.job[3].qp_out = h->qpart + 2 * slot; ga.job[3].qp_nt = vnt;
    launch_gemm<GEMM_F>(ga, 4, st);
    // 4. the heads (SAC:70-72, 80-91), [s | a_new], the tick
    SacHeadArgs ha;
    memset(&ha, 0, sizeof(ha));
    ha.h2 = h->a_h2; ha.mean_w = c.actor.mean_w; ha.mean_b = c.actor.mean_b; ha.ls_w = c.actor.log_std_w; ha.ls_b = c.actor.log_std_b;
    ha.eps = h->eps; ha.xs = h->xs; ha.xn = h->xn; ha.rec = h->rec; ha.B = B; ha.D = D; ha.H = H;
    ha.max_v = c.max_v; ha.max_w = c.max_w; ha.ls_min = c.log_std_min; ha.ls_max = c.log_std_max; ha.logp_eps = c.logp_eps;
    ha.adam = h->adam; ha.steps = h->steps; ha.pw = h->pw; ha.counter = h->counter;
    ha.lr[0] = c.lr_q; ha.lr[1] = c.lr_v; ha.lr[2] = c.lr_actor; ha.beta1 = c.beta1; ha.beta2 = c.beta2;
    hipLaunchKernelGGL(sac_head_kernel, dim3(B), dim3(256), 0, st, ha);
    // 5-6. Q(s, a_new) (SAC:261), still the pre-update Q
    fwd_job(ga.job[0], h->xn, B, Dc, Dc, c.q.w1, c.q.b1, h->n_h1, H, 1);
    launch_gemm<GEMM_F>(ga, 1, st);
    fwd_job(ga.job[0], h->n_h1, B, H, H, c.q.w2, c.q.b2, h->n_h2, H, 1);
    ga.job[0].qp_w3 = c.q.w3; ga.job[0].qp_b3 = c.q.b3; ga.job[0].qp_out = h->qpart + 3 * slot; ga.job[0].qp_nt = qnt;
    launch_gemm<GEMM_F>(ga, 1, st);
    // 7. losses and row gradients (SAC:258-272)
    SacLossArgs la;
    memset(&la, 0, sizeof(la));
    la.qpart = h->qpart; la.r = h->r; la.d = h->d; la.rec = h->rec; la.h2q = h->q_h2; la.h2v = h->v_h2; la.h2a = h->a_h2;
    la.w3q = c.q.w3; la.w3v = c.v.w3; la.mean_w = c.actor.mean_w; la.ls_w = c.actor.log_std_w;
    la.dq = h->dq; la.dv = h->dv; la.dl = h->dl; la.dz2q = h->dz2q; la.dz2v = h->dz2v; la.dz2a = h->dz2a; la.loss = h->loss;
    la.B = B; la.H = H; la.Hv = Hv; la.qnt = qnt; la.vnt = vnt; la.pnt = h->pnt(); la.gamma = c.gamma; la.ls_min = c.log_std_min; la.ls_max = c.log_std_max;
    la.mean_lambda = c.mean_lambda; la.std_lambda = c.std_lambda; la.z_lambda = c.z_lambda;
    hipLaunchKernelGGL(sac_loss_kernel, dim3(B), dim3(256), 0, st, la);
    // 8. through the three second layers
    dgrad_job(ga.job[0], h->dz2q, B, H, c.q.w2, h->q_h1, h->dz1q, H);
    dgrad_job(ga.job[1], h->dz2v, B, Hv, c.v.w2, h->v_h1, h->dz1v, Hv);
    dgrad_job(ga.job[2], h->dz2a, B, H, c.actor.w2, h->a_h1, h->dz1a, H);
    launch_gemm<GEMM_G>(ga, 3, st);
    // 9. Adam of Q, then of V (SAC:275-282); soft_update 1: V_t follows the stepped V in the same epilogue
    const cn_td3_mlp none = {}, &t = c.soft_update == 1 ? c.v_t : none;
    wgrad_job(ga.job[0], h->dz2q, H, h->q_h1, H, H, B, c.q.w2, c.q.b2, &h->mom_q[2], h->adam);
    wgrad_job(ga.job[1], h->dz1q, H, h->xs, Dc, Dc, B, c.q.w1, c.q.b1, &h->mom_q[0], h->adam);
    wgrad_job(ga.job[2], h->dq, 1, h->q_h2, H, H, B, c.q.w3, c.q.b3, &h->mom_q[4], h->adam);
    wgrad_job(ga.job[3], h->dz2v, Hv, h->v_h1, Hv, Hv, B, c.v.w2, c.v.b2, &h->mom_v[2], h->adam + 2, t.w2, t.b2);
    wgrad_job(ga.job[4], h->dz1v, Hv, h->xs, Dc, D, B, c.v.w1, c.v.b1, &h->mom_v[0], h->adam + 2, t.w1, t.b1);
    wgrad_job(ga.job[5], h->dv, 1, h->v_h2, Hv, Hv, B, c.v.w3, c.v.b3, &h->mom_v[4], h->adam + 2, t.w3, t.b3);
    launch_gemm<GEMM_H>(ga, 6, st);
    // 10. Adam of the actor (SAC:285-287): trunk and the two heads (two-row jobs on the columns of dl [B][4])
    wgrad_job(ga.job[0], h->dz2a, H, h->a_h1, H, H, B, c.actor.w2, c.actor.b2, &h->mom_a[2], h->adam + 4);
    wgrad_job(ga.job[1], h->dz1a, H, h->xs, Dc, D, B, c.actor.w1, c.actor.b1, &h->mom_a[0], h->adam + 4);
    wgrad_job(ga.job[2], h->dl, 2, h->a_h2, H, H, B, c.actor.mean_w, c.actor.mean_b, &h->mom_a[4], h->adam + 4);
    wgrad_job(ga.job[3], h->dl + 2, 2, h->a_h2, H, H, B, c.actor.log_std_w, c.actor.log_std_b, &h->mom_a[6], h->adam + 4);
    ga.job[2].lda = 4; ga.job[3].lda = 4;
    launch_gemm<GEMM_H>(ga, 4, st);
    if (c.soft_update == 0) {       // 11. SAC:290 as written
        SacPullArgs sp;
        float* v[6] = {c.v.w1, c.v.b1, c.v.w2, c.v.b2, c.v.w3, c.v.b3};
        const float* vt[6] = {c.v_t.w1, c.v_t.b1, c.v_t.w2, c.v_t.b2, c.v_t.w3, c.v_t.b3};
        for (int j = 0; j < 6; ++j) { sp.v[j] = v[j]; sp.vt[j] = vt[j]; sp.n[j] = (long long)param_count(D, 1, Hv, j); }
        sp.tau = c.tau;
        long long nmax = 1;
        for (int j = 0; j < 6; ++j) nmax = sp.n[j] > nmax ? sp.n[j] : nmax;
        const unsigned blocks = (unsigned)std::min<long long>(1024, (nmax + 1023) / 1024);      // grid-stride: four elements a thread
        hipLaunchKernelGGL(sac_pull_kernel, dim3(blocks), dim3(256), 0, st, sp);
    }
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

extern "C" int cn_sac_act(const cn_sac_act_io* io, int device, void* stream)
{
    if (!io || !io->obs || !io->twist) return td3_fail(CN_ERR_ARG, "cn_sac_act: null argument");
    if (!sac_actor_ok(io->actor)) return td3_fail(CN_ERR_ARG, "cn_sac_act: null parameter pointer");
    if (io->n < 1 || io->obs_dim < 1 || io->obs_ld < io->obs_dim || io->hidden < 1 || io->hidden > 480)
        return td3_fail(CN_ERR_CONFIG, "cn_sac_act: n / obs_dim / obs_ld / hidden out of range (hidden <= 480: two 16-row activations in 64 KB of LDS)");
    if (!(io->log_std_min <= io->log_std_max)) return td3_fail(CN_ERR_CONFIG, "cn_sac_act: log_std_min > log_std_max");
    DeviceScope scope(device);
    SacActArgs p;
    memset(&p, 0, sizeof(p));
    p.obs = io->obs; p.ld = io->obs_ld; p.n = io->n; p.D = io->obs_dim; p.H = io->hidden; p.Hp = (io->hidden + 31) / 32 * 32;
    p.deterministic = io->deterministic ? 1 : 0; p.a = io->actor;
    p.max_v = io->max_v; p.max_w = io->max_w; p.ls_min = io->log_std_min; p.ls_max = io->log_std_max;
    p.eps_in = io->eps; p.seed = io->seed; p.counter = io->counter;
    p.twist = io->twist; p.mean = io->mean; p.log_std = io->log_std; p.z = io->z;
    const size_t lds = (size_t)2 * 16 * p.Hp * sizeof(float);
    hipLaunchKernelGGL(sac_act_kernel, dim3((io->n + 15) / 16), dim3(256), lds, (hipStream_t)stream, p);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

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
