// crowdnav_learner.h -- what the units of the fused learners share (crowdnav_td3.hip, crowdnav_ddpg.hip, crowdnav_dqn.hip,
// crowdnav_sac.hip; crowdnav_replay.hip for the error channel).  Host code, apart from the argument structs that the kernels of
// crowdnav_gemm.hip read: those structs and the GEMM modes, the launchers that unit exports (no kernel is declared outside its
// file), the learners' error channel, the host scaffold of a handle (Pool, Learner, learner_create, the argument checks), what the
// TD3 and the DDPG handle share (ActorCritic), and the builders of a launch's GemmJobs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>

#include "../../include/crowdnav.h"
#include "crowdnav_host.h"

#pragma GCC visibility push(hidden)

// ---- the arguments of crowdnav_gemm.hip's kernels (what F, G and H compute: that file's design note) ----------------------------
enum { GEMM_F = 0, GEMM_G = 1, GEMM_H = 2 };
// the arguments of td3_tick, which rides in a forward launch: the update counter, the Adam step counters and bias corrections
struct TickArgs {
    float* adam;                                   // [2 optimizers][2]: lr / (1 - beta1^t), sqrt(1 - beta2^t)
    float* steps;                                  // [2] step counters (critics, actor)
    double* pw;                                    // [2 optimizers][2]: beta1^t, beta2^t as running products (powf was most of this thread's time)
    unsigned long long* counter;                   // update counter (keys the sampling)
    int do_actor; float lr_critic, lr_actor, beta1, beta2;
};
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
// td3_prep_shared_kernel's arguments: a population's prep table of the sampling mode, where {ring, row} of every batch row goes
// ([P][B][2]), and P
struct PrepSharedArgs { const PrepArgs* table; int64_t* src; int P; };

// ---- the launchers (crowdnav_gemm.hip): the mode is chosen on the host, once per launch ------------------------------------------
// grid x, y of a launch of `njobs` jobs in GEMM_F / G / H: the widest job's tiles of C.  The tile sizes are written there, once.
dim3 gemm_grid(int mode, const GemmJob* jobs, int njobs);
// a solo handle's launch: grid (gemm_grid, njobs) x 256.  gate: the GATE = true instantiation of F and G, the RMSprop one of H --
// DQN's launches, which do nothing while *ga.rms_gate == 0; TD3, DDPG and SAC pass false
void launch_gemm(int mode, bool gate, const GemmArgs& ga, int njobs, hipStream_t st);
// a population's launch (the POP = true instantiations): grid = (gemm_grid of one member's jobs, members x njobs)
void launch_gemm_pop(int mode, const PopGemmArgs& ga, dim3 grid, hipStream_t st);
// td3_prep_kernel: one workgroup per batch row; a population's on the grid (B, P) over a table of P PrepArgs in device memory
void launch_prep(const PrepArgs& pa, hipStream_t st);
void launch_prep_pop(const PrepArgs* table, int B, int P, hipStream_t st);
// td3_prep_shared_kernel on the same grid and table: every member's rows from the union of all members' rings (CN_REPLAY_SHARED)
void launch_prep_shared(const PrepArgs* table, int64_t* src, int B, int P, hipStream_t st);

// the learners' error channel: the thread's cn_td3_last_error() string (crowdnav_gemm.hip); returns `code`
int td3_fail(int code, const std::string& msg);

// ---- a handle's scaffold ---------------------------------------------------------------------------------------------------------
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
inline size_t param_count(int in1, int out3, int H, int j)
{
    const size_t h = (size_t)H;
    switch (j) { case 0: return h * in1; case 1: return h; case 2: return h * h; case 3: return h; case 4: return out3 * h; default: return out3; }
}
inline bool mlp_ok(const cn_td3_mlp& n) { return n.w1 && n.b1 && n.w2 && n.b2 && n.w3 && n.b3; }
inline int check_mlps(const char* fn, std::initializer_list<const cn_td3_mlp*> nets)
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

// cn_*_set_replay_sample, a solo handle's and the population's: the mode of the updates enqueued from now on (a captured update keeps
// the kernel arguments it was captured with)
template <class Hd>
int set_replay_sample(const char* fn, Hd* h, int mode)
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
inline const float* batch_dev(const ActorCritic* h, int what)
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
inline void fwd_job(GemmJob& j, const float* X, int I, int ldx, int K, const float* W, const float* b, float* Y, int J, int relu)
{
    memset(&j, 0, sizeof(j));
    j.A = X; j.B = W; j.C = Y; j.bias = b; j.I = I; j.J = J; j.R = K; j.lda = ldx; j.ldb = K; j.ldc = J; j.relu = relu;
}
// F, on top of fwd_job: the last two columns of X are policy `pol`'s action on the row, evaluated from its second hidden activation h2
inline void head_job(GemmJob& j, int D, int H, const float* h2, const cn_td3_mlp& pol, const float* noise, float* logits, float max_v, float max_w)
{
    j.R = D; j.hd_h2 = h2; j.hd_W3 = pol.w3; j.hd_b3 = pol.b3; j.hd_noise = noise; j.hd_logits = logits; j.hd_H = H; j.hd_max_v = max_v; j.hd_max_w = max_w;
}
// G: dX [I][J] = (dY [I][R] W) (.) [mask > 0]
inline void dgrad_job(GemmJob& j, const float* dY, int I, int R, const float* W, const float* mask, float* dX, int J)
{
    memset(&j, 0, sizeof(j));
    j.A = dY; j.B = W; j.C = dX; j.mask = mask; j.I = I; j.J = J; j.R = R; j.lda = R; j.ldb = J; j.ldc = J;
}
// G through a critic's second layer with dY evaluated (hb_*): the TD target from q partial-sum slot `net` and the target slots
inline void critic_bwd_job(GemmJob& j, const ActorCritic& h, const cn_td3_mlp& crit, const float* h1, const float* h2, int net, int single, float gamma,
                           float* dq, float* dz2, float* dz1)
{
    dgrad_job(j, h2, h.B, h.H, crit.w2, h1, dz1, h.H);
    j.hb_h2 = h2; j.hb_w3 = crit.w3; j.hb_qpart = h.qpart; j.hb_qnt = h.qnt(); j.hb_net = net; j.hb_single = single; j.hb_r = h.r; j.hb_d = h.d;
    j.hb_gamma = gamma; j.hb_dq = dq; j.hb_dz2 = dz2;
}
// G through the actor's second layer with dY evaluated (ab_*): the heads' derivatives on the action gradient's partial sums
inline void actor_bwd_job(GemmJob& j, const ActorCritic& h, const cn_td3_mlp& actor, float max_v, float max_w, float* dz2, float* dz1)
{
    dgrad_job(j, h.a_h2, h.B, h.H, actor.w2, h.a_h1, dz1, h.H);
    j.ab_h2 = h.a_h2; j.ab_w3 = actor.w3; j.ab_dapart = h.dapart; j.ab_dant = h.dant(); j.ab_logits = h.logits;
    j.ab_max_v = max_v; j.ab_max_w = max_w; j.ab_dl = h.dl; j.ab_dz2 = dz2;
}
// H: W [I][J] stepped by dY^T [I][R] X [R][J], its bias by the row sums of dY^T; st = the optimizer's state of W, then of the bias,
// {m, v} each (RMSprop: the accumulator and null); adam = the optimizer's bias corrections; tgt / btgt = the target's copies, or null
inline void wgrad_job(GemmJob& j, const float* dY, int I, const float* X, int ldx, int J, int R, float* W, float* bparam, float* const (*st)[2],
                      const float* adam = nullptr, float* tgt = nullptr, float* btgt = nullptr)
{
    memset(&j, 0, sizeof(j));
    j.A = dY; j.B = X; j.C = W; j.I = I; j.J = J; j.R = R; j.lda = I; j.ldb = ldx; j.ldc = J;
    j.m = st[0][0]; j.v = st[0][1]; j.bparam = bparam; j.bm = st[1][0]; j.bv = st[1][1]; j.adam = adam; j.tgt = tgt; j.btgt = btgt;
}

#pragma GCC visibility pop
