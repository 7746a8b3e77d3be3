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
// The kernels are crowdnav_gemm.hip's, reached through its launchers; the handle's scaffold and the job builders, which DDPG, DQN
// and SAC use as well, are crowdnav_learner.h.  This file is TD3 itself: the handle, the chain of launches, and the population --
// with the only two kernels defined here, population-based training's plan and copy (td3_pbt_plan_kernel, td3_pbt_copy_kernel).
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/crowdnav.h"
#include "crowdnav_device.h"
#include "crowdnav_learner.h"
#include "crowdnav_state.h"

namespace {
// The two emitters of td3_chain (after the handle): how the launches of one update, which the chain names in order, are used.
struct Td3LaunchNow {                              // cn_td3_update: every launch goes to the stream as the chain names it
    hipStream_t st;
    void prep(const PrepArgs& pa) { launch_prep(pa, st); }
    template <int MODE> void gemm(const GemmArgs& ga, int njobs) { launch_gemm(MODE, false, ga, njobs, st); }
};
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
// Population-based training's two launches (cn_td3_pop_exploit, at the end of this file; the statement: include/crowdnav.h).
enum { PBT_TENSORS = 36 + 36 + 3 };                // per member: the parameters, Adam's moments, and adam[4], steps[2], pw[4] of the tick
struct PbtTensor { float* p; uint32_t n, reserved; };                  // n floats at p (pw: 4 doubles = 8 floats)
struct PbtPlan { int32_t applied, n; int32_t dst[32], src[32]; };      // launch A's word to launch B: bottom[k] = dst[k] copies from src[k]
struct PbtPlanArgs {
    cn_td3_pbt_config cfg;
    cn_td3_pbt_state* state;
    PbtPlan* plan;
    double* last;                                  // [P][2]: the logs' {episodes, return sum} at the last applied call
    const double* const* tot;                      // [P]: the bound logs' tot_dev, or null
    PrepArgs* prep[2]; TickArgs* tick[2]; GemmJob* jobs;                // the update's tables, which hold the hyper-parameters by value
    const int* gamma_jobs; int n_gamma;            // [P][n_gamma]: where `jobs` holds member p's gamma
    const float* fitness;                          // [P] or null = from tot
    int P;
};
}  // namespace

// Launch A, one wavefront, thread p = member p: fitness, rank, plan; the state and the tables' hyper-parameters of the replaced.
__global__ __launch_bounds__(64) void td3_pbt_plan_kernel(const PbtPlanArgs a)
{
    __shared__ float fit[64];
    __shared__ int order[64];
    const int p = threadIdx.x, P = a.P, n = a.cfg.n_replace;
    const bool live = p < P;
    const uint64_t c = a.state->calls;
    float f = 0.f;
    double e_now = 0.0, r_now = 0.0;
    int few = 0;
    if (live) {
        if (a.fitness) f = a.fitness[p];
        else {
            e_now = a.tot[p][0]; r_now = a.tot[p][2];
            const double de = e_now - a.last[2 * p], dr = r_now - a.last[2 * p + 1];
            few = !(de >= (double)a.cfg.min_episodes);
            f = (float)(dr / de);
        }
    }
    if (__syncthreads_or(few)) {                   // skipped: the call counts and nothing else moves (every thread has read `calls`)
        if (p == 0) { a.state->calls = c + 1; a.plan->applied = 0; }
        return;
    }
    fit[p] = f;
    __syncthreads();
    int rank = 0;                                  // how many members stand before p: fitness descending, NaN last, then the index
    if (live) {
        const bool fn = f != f;
        for (int q = 0; q < P; ++q) {
            const float g = fit[q];
            const bool gn = g != g;
            const bool tie = (gn && fn) || (!gn && !fn && g == f);
            rank += ((!gn && fn) || (!gn && !fn && g > f) || (tie && q < p)) ? 1 : 0;
        }
        order[rank] = p;
    }
    __syncthreads();
    if (live) {
        const uint64_t K = cn_mix64(a.cfg.seed ^ cn_mix64(c));
        cn_td3_pbt_member& me = a.state->member[p];
        const int k = P - 1 - rank;                // p = bottom[k]
        me.fitness = f;
        if (k < n) {
            const int src = order[cn_mix64(K ^ (uint64_t)(k + 1)) % (uint64_t)n];
            a.plan->dst[k] = p; a.plan->src[k] = src;
            me.src = src; me.generation += 1;
            float v[CN_PBT_HYPERS];
            for (int j = 0; j < CN_PBT_HYPERS; ++j) {
                float x = a.state->member[src].hyper[j];
                if ((a.cfg.explore_mask >> j) & 1u) x = x * a.cfg.factor[cn_mix64(K ^ cn_mix64((uint64_t)(0x100 + 8 * p + j))) >> 63];
                x = fminf(fmaxf(x, a.cfg.lo[j]), a.cfg.hi[j]);
                me.hyper[j] = v[j] = x;
            }
            for (int q = 0; q < 2; ++q) {          // both chains' tick tables, both sampling modes' prep tables
                a.tick[q][p].lr_actor = v[CN_PBT_LR_ACTOR]; a.tick[q][p].lr_critic = v[CN_PBT_LR_CRITIC];
                a.prep[q][p].noise_std = v[CN_PBT_NOISE_STD]; a.prep[q][p].noise_clip = v[CN_PBT_NOISE_CLIP];
            }
            for (int g = 0; g < a.n_gamma; ++g) a.jobs[a.gamma_jobs[p * a.n_gamma + g]].hb_gamma = v[CN_PBT_GAMMA];
        } else {
            me.src = p;
        }
        if (!a.fitness) { a.last[2 * p] = e_now; a.last[2 * p + 1] = r_now; }
    }
    if (p == 0) { a.state->calls = c + 1; a.state->applied += 1; a.plan->applied = 1; a.plan->n = n; }
}

// Launch B, grid (chunks, PBT_TENSORS, n_replace): tensor y of member dst[z] <- that of src[z], bit for bit.  Any float count and any
// 4-byte alignment: 16-byte accesses where the two pointers reach a 16-byte boundary together, single floats before, after and otherwise.
__global__ __launch_bounds__(256) void td3_pbt_copy_kernel(const PbtPlan* plan, const PbtTensor* tens)
{
    if (!plan->applied) return;
    const PbtTensor s = tens[plan->src[blockIdx.z] * PBT_TENSORS + blockIdx.y], d = tens[plan->dst[blockIdx.z] * PBT_TENSORS + blockIdx.y];
    const float* sp = s.p;
    float* dp = d.p;
    const size_t n = d.n, tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const uintptr_t sa = (uintptr_t)sp, da = (uintptr_t)dp;
    size_t head = n;
    if (((sa ^ da) & 15) == 0) head = std::min(n, (size_t)(((16 - (sa & 15)) & 15) / 4));
    const size_t n4 = (n - head) / 4;
    for (size_t i = tid; i < head; i += stride) dp[i] = sp[i];
    const float4* s4 = (const float4*)(sp + head);
    float4* d4 = (float4*)(dp + head);
    for (size_t i = tid; i < n4; i += stride) d4[i] = s4[i];
    for (size_t i = head + 4 * n4 + tid; i < n; i += stride) dp[i] = sp[i];
}

// ---- TD3 --------------------------------------------------------------------------------------------------------------------
struct cn_td3_s : ActorCritic {
    cn_td3_config cfg;
    float *c_h1[4], *c_h2[4];               // q1, q2, q1_t, q2_t
    float *dq[2];                           // the critics' loss gradients per row (td3_dgrad_kernel's head-backward mode)
    float *dz2[2], *dz1[2];
    StateTable* state_tab = nullptr;        // cn_td3_state_*: built on first use (crowdnav_state.hip)
    ~cn_td3_s() { state_table_free(state_tab); }
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
// of the kernels' POP = true instantiations (crowdnav_gemm.hip), which read them from tables in device memory.  A handle's pointers never change, so the
// tables of both chains (do_actor 0 / 1) and of both sampling modes are built and uploaded once, in cn_td3_pop_create;
// cn_td3_pop_update only enqueues.
struct cn_td3_pop_s {
    int device = 0, P = 0, B = 0;
    int sample_mode = CN_SAMPLE_WITH_REPLACEMENT;
    int replay_source = CN_REPLAY_OWN;             // cn_td3_pop_set_replay_source: read on the host when an update is enqueued
    bool shared_ran = false;                       // a shared update was enqueued: batch_src holds its {ring, row}
    int64_t* batch_src = nullptr;                  // [P][B][2], written by td3_prep_shared_kernel alone
    float beta1 = 0.f, beta2 = 0.f, eps = 0.f, tau = 0.f;
    std::vector<std::unique_ptr<cn_td3_s>> mem;    // the members' workspaces and Adam state: solo handles that are never updated alone
    void* tables = nullptr;                        // one allocation: losses [P], prep tables [2 modes][P], tick tables [2 chains][P], jobs, batch_src
    float* loss = nullptr;
    const PrepArgs* prep[2] = {nullptr, nullptr};
    const TickArgs* tick[2] = {nullptr, nullptr};
    const GemmJob* jobs = nullptr;
    std::vector<PopStep> chain[2];
    // population-based training (cn_td3_pop_pbt_bind / cn_td3_pop_exploit, below)
    std::vector<int> gamma_jobs;                   // [P][n]: the indices into `jobs` where critic_bwd_job put member p's gamma, both chains
    void* pbt = nullptr;                           // one allocation at bind: state, plan, last, the tensor table, the gamma indices, the logs' totals
    cn_td3_pbt_config pbt_cfg;
    PbtPlanArgs pbt_args;                          // launch A's arguments but for the fitness; the device pointers never change after the bind
    const PbtTensor* pbt_tensors = nullptr;
    int pbt_chunks = 0;
    bool pbt_logs = false;
    StateTable* state_tab = nullptr;               // cn_td3_pop_state_*: built on first use, dropped by a bind (crowdnav_state.hip)
    cn_td3_pop_s() = default;
    cn_td3_pop_s(const cn_td3_pop_s&) = delete;
    ~cn_td3_pop_s()
    {
        state_table_free(state_tab);
        if (tables || pbt) { DeviceScope scope(device); (void)hipFree(tables); (void)hipFree(pbt); }
    }
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
    int64_t* batch_src = nullptr;
    auto layout = [&](Pool& pl) {
        pl.take(loss, (size_t)P);
        for (int q = 0; q < 2; ++q) pl.take(prep[q], (size_t)P);
        for (int q = 0; q < 2; ++q) pl.take(tick[q], (size_t)P);
        pl.take(jobs, njobs_all);
        pl.take(batch_src, (size_t)P * c0.batch * 2);
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
    struct GammaAt { int job0, njobs; };           // a job of member 0 that carries gamma, and its step's jobs per member
    std::vector<GammaAt> gamma_at;
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
            const dim3 g = gemm_grid(s0.mode, s0.job, s0.njobs);
            const PopStep ps{s0.mode, s0.njobs, s0.do_tick, (int)g.x, (int)g.y, first};
            if (first + (size_t)P * s0.njobs > hjobs.size()) return td3_fail(CN_ERR_ARG, f + ": job table size");      // (never: counted above)
            for (int p = 0; p < P; ++p)
                for (int z = 0; z < s0.njobs; ++z) hjobs[first + (size_t)p * s0.njobs + z] = rec[a][p].step[k].job[z];
            for (int z = 0; z < s0.njobs; ++z)                          // critic_bwd_job's jobs hold gamma by value: cn_td3_pop_exploit rewrites it
                if (s0.job[z].hb_h2) gamma_at.push_back({(int)first + z, s0.njobs});
            first += (size_t)P * s0.njobs;
            h->chain[a].push_back(ps);
        }
    }
    for (int p = 0; p < P; ++p)
        for (const GammaAt& g : gamma_at) h->gamma_jobs.push_back(g.job0 + p * g.njobs);
    static_assert(CN_SAMPLE_WITH_REPLACEMENT == 0 && CN_SAMPLE_DISTINCT == 1, "the prep tables are indexed by the mode");
    for (int q = 0; q < 2; ++q) {
        e = hipMemcpy(prep[q], hprep.data() + (size_t)q * P, sizeof(PrepArgs) * P, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(tick[q], htick.data() + (size_t)q * P, sizeof(TickArgs) * P, hipMemcpyHostToDevice);
        if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMemcpy: " + hipGetErrorString(e));
        h->prep[q] = prep[q]; h->tick[q] = tick[q];
    }
    e = hipMemcpy(jobs, hjobs.data(), sizeof(GemmJob) * hjobs.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMemcpy: " + hipGetErrorString(e));
    h->loss = loss; h->jobs = jobs; h->batch_src = batch_src;
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
extern "C" int cn_td3_pop_set_replay_sample(cn_td3_pop_handle h, int mode) { return set_replay_sample("cn_td3_pop_set_replay_sample", h, mode); }
extern "C" int cn_td3_pop_set_replay_source(cn_td3_pop_handle h, int source)
{
    if (!h) return td3_fail(CN_ERR_ARG, "cn_td3_pop_set_replay_source: null handle");
    if (source != CN_REPLAY_OWN && source != CN_REPLAY_SHARED)
        return td3_fail(CN_ERR_ARG, "cn_td3_pop_set_replay_source: source must be CN_REPLAY_OWN (0) or CN_REPLAY_SHARED (1); the handle keeps its source");
    h->replay_source = source;
    return CN_OK;
}
extern "C" const int64_t* cn_td3_pop_batch_src_dev(cn_td3_pop_handle h, int member)
{
    return (h && member >= 0 && member < h->P && h->shared_ran) ? h->batch_src + (size_t)member * h->B * 2 : nullptr;
}

extern "C" int cn_td3_pop_update(cn_td3_pop_handle h, int do_actor, void* stream)
{
    if (!h) return td3_fail(CN_ERR_ARG, "cn_td3_pop_update: null handle");
    DeviceScope scope(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int a = do_actor ? 1 : 0;
    if (h->replay_source == CN_REPLAY_SHARED) {    // the same tables; only this launch reads differently
        launch_prep_shared(h->prep[h->sample_mode], h->batch_src, h->B, h->P, st);
        h->shared_ran = true;
    } else launch_prep_pop(h->prep[h->sample_mode], h->B, h->P, st);
    for (const PopStep& s : h->chain[a]) {
        const PopGemmArgs ga{h->jobs + s.first, h->tick[a], s.njobs, h->beta1, h->beta2, h->eps, h->tau, s.do_tick};
        launch_gemm_pop(s.mode, ga, dim3(s.gx, s.gy, h->P * s.njobs), st);
    }
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

// ---- population-based training: exploit and explore on the device (the statement: include/crowdnav.h) ---------------------------
// The hyper-parameters a member trains with lie by value in the tables above; launch A rewrites them for the replaced members, launch
// B copies what the replaced take over.  Everything either launch reads is device memory that the bind laid out once.
extern "C" int cn_td3_pop_pbt_bind(cn_td3_pop_handle h, const cn_td3_pbt_config* cfg, const cn_episode_log* logs)
{
    const std::string f("cn_td3_pop_pbt_bind");
    if (!h || !cfg) return td3_fail(CN_ERR_ARG, f + ": null " + (h ? "cfg" : "handle"));
    const cn_td3_pbt_config& c = *cfg;
    const int P = h->P;
    if (c.n_replace < 1 || c.n_replace > P / 2)
        return td3_fail(CN_ERR_ARG, f + ": n_replace must be 1 ... n_members / 2 = " + std::to_string(P / 2) + " (the replaced and their sources are disjoint)");
    if (c.min_episodes < 1) return td3_fail(CN_ERR_ARG, f + ": min_episodes must be >= 1");
    for (int i = 0; i < 2; ++i)
        if (!std::isfinite(c.factor[i]) || !(c.factor[i] > 0.f)) return td3_fail(CN_ERR_ARG, f + ": factor[" + std::to_string(i) + "] must be finite and > 0");
    static const char* const hname[CN_PBT_HYPERS] = {"lr_actor", "lr_critic", "gamma", "noise_std", "noise_clip"};
    for (int k = 0; k < CN_PBT_HYPERS; ++k)
        if (!std::isfinite(c.lo[k]) || !std::isfinite(c.hi[k]) || c.lo[k] > c.hi[k])
            return td3_fail(CN_ERR_ARG, f + ": lo / hi of " + hname[k] + " must be finite with lo <= hi");
    if (c.explore_mask >> CN_PBT_HYPERS) return td3_fail(CN_ERR_ARG, f + ": explore_mask has bits at or above CN_PBT_HYPERS");
    if (logs)
        for (int p = 0; p < P; ++p)
            if (!logs[p].rows || !logs[p].n_dev || !logs[p].tot_dev || logs[p].max_rows < 0)
                return td3_fail(CN_ERR_ARG, f + ": member " + std::to_string(p) + ": incomplete log");
    std::vector<cn_td3_pbt_member> member((size_t)P);
    for (int p = 0; p < P; ++p) {
        const cn_td3_config& m = h->mem[p]->cfg;
        const float start[CN_PBT_HYPERS] = {m.lr_actor, m.lr_critic, m.gamma, m.noise_std, m.noise_clip};
        member[p].src = p; member[p].generation = 0; member[p].fitness = 0.f;
        for (int k = 0; k < CN_PBT_HYPERS; ++k) {
            if (!(start[k] >= c.lo[k] && start[k] <= c.hi[k]))
                return td3_fail(CN_ERR_CONFIG, f + ": member " + std::to_string(p) + ": " + hname[k] + " starts outside [lo, hi]");
            member[p].hyper[k] = start[k];
        }
    }
    DeviceScope scope(h->device);
    // the tensors a replaced member takes over, in one order for all members
    std::vector<PbtTensor> tens((size_t)P * PBT_TENSORS);
    uint32_t longest = 0;
    for (int p = 0; p < P; ++p) {
        cn_td3_s* m = h->mem[p].get();
        const cn_td3_mlp* nets[6] = {&m->cfg.actor, &m->cfg.actor_t, &m->cfg.q1, &m->cfg.q1_t, &m->cfg.q2, &m->cfg.q2_t};
        PbtTensor* t = tens.data() + (size_t)p * PBT_TENSORS;
        for (int net = 0; net < 6; ++net) {
            const float* w[6] = {nets[net]->w1, nets[net]->b1, nets[net]->w2, nets[net]->b2, nets[net]->w3, nets[net]->b3};
            for (int j = 0; j < 6; ++j) *t++ = {(float*)w[j], (uint32_t)param_count(net < 2 ? m->D : m->D + 2, net < 2 ? 2 : 1, m->H, j), 0};
        }
        for (int net = 0; net < 3; ++net) for (int j = 0; j < 6; ++j) for (int k = 0; k < 2; ++k)
            *t++ = {m->mom[net][j][k], (uint32_t)param_count(net == 0 ? m->D : m->D + 2, net == 0 ? 2 : 1, m->H, j), 0};
        *t++ = {m->adam, 4, 0}; *t++ = {m->steps, 2, 0}; *t++ = {(float*)m->pw, 8, 0};
        for (int j = 0; j < PBT_TENSORS; ++j) longest = std::max(longest, tens[(size_t)p * PBT_TENSORS + j].n);
    }
    const int n_gamma = (int)(h->gamma_jobs.size() / (size_t)P);
    std::vector<const double*> tot((size_t)P, nullptr);
    if (logs) for (int p = 0; p < P; ++p) tot[p] = logs[p].tot_dev;
    cn_td3_pbt_state* state = nullptr; PbtPlan* plan = nullptr; double* last = nullptr; const double** totd = nullptr;
    PbtTensor* tensd = nullptr; int* gammad = nullptr;
    auto layout = [&](Pool& pl) {
        pl.take(state, 1); pl.take(last, (size_t)2 * P); pl.take(totd, (size_t)P); pl.take(tensd, tens.size());
        pl.take(plan, 1); pl.take(gammad, h->gamma_jobs.size());
    };
    Pool count{nullptr};
    layout(count);
    void* block = nullptr;
    hipError_t e = hipMalloc(&block, count.size);
    if (e != hipSuccess) return td3_fail(CN_ERR_HIP, f + ": hipMalloc: " + hipGetErrorString(e));
    Pool assign{(char*)block};
    layout(assign);
    e = hipMemset(block, 0, count.size);
    if (e == hipSuccess) e = hipMemcpy(state->member, member.data(), sizeof(cn_td3_pbt_member) * P, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(totd, tot.data(), sizeof(double*) * P, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tensd, tens.data(), sizeof(PbtTensor) * tens.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(gammad, h->gamma_jobs.data(), sizeof(int) * h->gamma_jobs.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && h->pbt) {               // binding again starts over: the tables go back to what the members' configurations say
        e = hipDeviceSynchronize();
        std::vector<TickArgs> tk((size_t)P);
        std::vector<PrepArgs> pr((size_t)P);
        std::vector<GemmJob> jb(h->gamma_jobs.size());
        for (int q = 0; q < 2 && e == hipSuccess; ++q) {
            e = hipMemcpy(tk.data(), h->tick[q], sizeof(TickArgs) * P, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(pr.data(), h->prep[q], sizeof(PrepArgs) * P, hipMemcpyDeviceToHost);
            for (int p = 0; p < P; ++p) {
                const cn_td3_config& m = h->mem[p]->cfg;
                tk[p].lr_actor = m.lr_actor; tk[p].lr_critic = m.lr_critic; pr[p].noise_std = m.noise_std; pr[p].noise_clip = m.noise_clip;
            }
            if (e == hipSuccess) e = hipMemcpy((void*)h->tick[q], tk.data(), sizeof(TickArgs) * P, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy((void*)h->prep[q], pr.data(), sizeof(PrepArgs) * P, hipMemcpyHostToDevice);
        }
        for (size_t i = 0; i < h->gamma_jobs.size() && e == hipSuccess; ++i) {
            const float gamma = h->mem[i / (size_t)n_gamma]->cfg.gamma;
            e = hipMemcpy((char*)(h->jobs + h->gamma_jobs[i]) + offsetof(GemmJob, hb_gamma), &gamma, sizeof(float), hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) { (void)hipFree(block); return td3_fail(CN_ERR_HIP, f + ": " + hipGetErrorString(e)); }
    if (h->pbt) (void)hipFree(h->pbt);
    h->pbt = block;
    state_table_free(h->state_tab);                // the state blob gains (or moves) the PBT segments
    h->state_tab = nullptr;
    h->pbt_cfg = c; h->pbt_logs = logs != nullptr; h->pbt_tensors = tensd;
    h->pbt_chunks = (int)std::min<uint32_t>(64u, std::max<uint32_t>(1u, (longest + 4095u) / 4096u));
    PbtPlanArgs& a = h->pbt_args;
    memset(&a, 0, sizeof(a));
    a.cfg = c; a.state = state; a.plan = plan; a.last = last; a.tot = logs ? totd : nullptr;
    for (int q = 0; q < 2; ++q) { a.prep[q] = const_cast<PrepArgs*>(h->prep[q]); a.tick[q] = const_cast<TickArgs*>(h->tick[q]); }
    a.jobs = const_cast<GemmJob*>(h->jobs); a.gamma_jobs = gammad; a.n_gamma = n_gamma; a.P = P;
    return CN_OK;
}

extern "C" int cn_td3_pop_exploit(cn_td3_pop_handle h, const float* fitness_dev, void* stream)
{
    if (!h) return td3_fail(CN_ERR_ARG, "cn_td3_pop_exploit: null handle");
    if (!h->pbt) return td3_fail(CN_ERR_ARG, "cn_td3_pop_exploit: cn_td3_pop_pbt_bind first");
    if (!fitness_dev && !h->pbt_logs) return td3_fail(CN_ERR_ARG, "cn_td3_pop_exploit: no fitness_dev and no logs were bound");
    DeviceScope scope(h->device);
    hipStream_t st = (hipStream_t)stream;
    PbtPlanArgs a = h->pbt_args;
    a.fitness = fitness_dev;
    hipLaunchKernelGGL(td3_pbt_plan_kernel, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(td3_pbt_copy_kernel, dim3(h->pbt_chunks, PBT_TENSORS, h->pbt_cfg.n_replace), dim3(256), 0, st, a.plan, h->pbt_tensors);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}
extern "C" const cn_td3_pbt_state* cn_td3_pop_pbt_state_dev(cn_td3_pop_handle h)
{
    return (h && h->pbt) ? h->pbt_args.state : nullptr;
}

// ---- the state blob's view of a handle (crowdnav_state.h; the statement: include/crowdnav.h, cn_td3_state_*) ----------------------
// Member p's segments in the blob's order: the tensors of PbtTensor's table (cn_td3_pop_pbt_bind), then the counter and the loss.
static void td3_member_state(cn_td3_s* m, int p, std::vector<StateSeg>& s)
{
    const cn_td3_mlp* nets[6] = {&m->cfg.actor, &m->cfg.actor_t, &m->cfg.q1, &m->cfg.q1_t, &m->cfg.q2, &m->cfg.q2_t};
    for (int net = 0; net < 6; ++net) {
        const float* w[6] = {nets[net]->w1, nets[net]->b1, nets[net]->w2, nets[net]->b2, nets[net]->w3, nets[net]->b3};
        for (int j = 0; j < 6; ++j)
            s.push_back({(void*)w[j], p, CN_STATE_PARAM, net * 6 + j, (uint32_t)param_count(net < 2 ? m->D : m->D + 2, net < 2 ? 2 : 1, m->H, j)});
    }
    for (int net = 0; net < 3; ++net) for (int j = 0; j < 6; ++j) for (int k = 0; k < 2; ++k)
        s.push_back({m->mom[net][j][k], p, CN_STATE_MOMENT, (net * 6 + j) * 2 + k, (uint32_t)param_count(net == 0 ? m->D : m->D + 2, net == 0 ? 2 : 1, m->H, j)});
    s.push_back({m->adam, p, CN_STATE_ADAM, 0, 4}); s.push_back({m->steps, p, CN_STATE_STEPS, 0, 2}); s.push_back({m->pw, p, CN_STATE_PW, 0, 8});
    s.push_back({m->counter, p, CN_STATE_COUNTER, 0, 2}); s.push_back({m->loss, p, CN_STATE_LOSS, 0, 1});
}
void td3_state_view(cn_td3_handle h, bool full, StateView& v)
{
    v.family = CN_STATE_FAMILY_TD3; v.P = 1; v.obs_dim = h->D; v.hidden = h->H; v.batch = h->B; v.pbt_bound = 0; v.device = h->device;
    v.table = &h->state_tab;
    if (full) td3_member_state(h, 0, v.seg);
}
void td3_pop_state_view(cn_td3_pop_handle h, bool full, StateView& v)
{
    const cn_td3_s* m0 = h->mem[0].get();
    v.family = CN_STATE_FAMILY_TD3; v.P = h->P; v.obs_dim = m0->D; v.hidden = m0->H; v.batch = h->B; v.pbt_bound = h->pbt ? 1 : 0; v.device = h->device;
    v.table = &h->state_tab;
    if (!full) return;
    const int P = h->P, n_gamma = (int)(h->gamma_jobs.size() / (size_t)P);
    for (int p = 0; p < P; ++p) {
        td3_member_state(h->mem[p].get(), p, v.seg);
        v.seg.push_back({nullptr, p, CN_STATE_HYPER, 0, CN_PBT_HYPERS});
        for (int q = 0; q < 2; ++q) {              // where td3_pbt_plan_kernel writes them: both chains' tick tables, both modes' prep tables
            TickArgs* tk = const_cast<TickArgs*>(h->tick[q]) + p;
            PrepArgs* pr = const_cast<PrepArgs*>(h->prep[q]) + p;
            v.scatter.push_back({&tk->lr_actor, p, CN_PBT_LR_ACTOR}); v.scatter.push_back({&tk->lr_critic, p, CN_PBT_LR_CRITIC});
            v.scatter.push_back({&pr->noise_std, p, CN_PBT_NOISE_STD}); v.scatter.push_back({&pr->noise_clip, p, CN_PBT_NOISE_CLIP});
        }
        for (int g = 0; g < n_gamma; ++g)
            v.scatter.push_back({&(const_cast<GemmJob*>(h->jobs) + h->gamma_jobs[(size_t)p * n_gamma + g])->hb_gamma, p, CN_PBT_GAMMA});
    }
    if (h->pbt) {
        v.seg.push_back({h->pbt_args.state, -1, CN_STATE_PBT, 0, (uint32_t)(sizeof(cn_td3_pbt_state) / 4)});
        v.seg.push_back({h->pbt_args.last, -1, CN_STATE_PBT_LAST, 0, (uint32_t)(4 * P)});
    }
}
