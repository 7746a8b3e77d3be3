// crowdnav_ddpg.hip -- DDPG, the reference's baseline learner, as a fused update: cn_ddpg_* (include/crowdnav.h).
// ddpg.py:198-243 of the reference (Agent.learn) on the three GEMM kernels of crowdnav_gemm.hip, with TD3's scaffold (crowdnav_learner.h).
// One critic and its target, no policy delay, no target-policy noise.  The actor loss -mean Q(s, pi(s)) is back-propagated
// BEFORE the critic's step (ddpg.py:226-238), so both gradients are taken at the pre-update weights and the two branches share
// launches.  8 launches:  prep | actor_t L1 (+ actor L1) | L2 (+ L2) | critic_t L1 on (s2, pi_t(s2)), critic L1 on (s, a) and on
// (s, pi(s)) | their L2 (+ q partials of critic_t and critic, dz on the pi(s) branch, tick) | G (critic: dq, dz2 evaluated;
// pi(s) branch: da partials) | G (actor: dl, dz2a evaluated) | H (six jobs: critic and actor W1 / W2 / W3 + Adam + soft updates).
// And cn_ddpg_act: Agent.act(add_noise=True) (ddpg.py:170-196) with OUNoise (:44-64) as ONE launch -- the TD3 actor's tile
// (crowdnav_actor.h: cn_actor_forward's, same matrix work and heads) with the Ornstein-Uhlenbeck term as its output stage's noise.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/crowdnav.h"
#include "crowdnav_actor.h"
#include "crowdnav_learner.h"

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
    launch_prep(pa, st);
    GemmArgs ga;
    memset(&ga, 0, sizeof(ga));
    adam_args(ga, *h, c, 1);                        // both optimizers step on every update
    // 2-3. actor_t's hidden layers on s2 (ddpg.py:219), actor's on s (:216)
    fwd_job(ga.job[0], h->x2, B, Dc, D, c.actor_t.w1, c.actor_t.b1, h->t_h1, H, 1);
    fwd_job(ga.job[1], h->xs, B, Dc, D, c.actor.w1, c.actor.b1, h->a_h1, H, 1);
    launch_gemm(GEMM_F, false, ga, 2, st);
    fwd_job(ga.job[0], h->t_h1, B, H, H, c.actor_t.w2, c.actor_t.b2, h->t_h2, H, 1);
    fwd_job(ga.job[1], h->a_h1, B, H, H, c.actor.w2, c.actor.b2, h->a_h2, H, 1);
    launch_gemm(GEMM_F, false, ga, 2, st);
    // 4. the critics' first layers: critic on (s, a) (:229), critic on (s, pi(s)) (:216, the logits kept for the heads' backward),
    // critic_t on (s2, pi_t(s2)) (:220) -- the policies' last layers and heads evaluated in place of the action columns, no noise
    fwd_job(ga.job[0], h->xs, B, Dc, Dc, c.critic.w1, c.critic.b1, h->c_h1[0], H, 1);
    fwd_job(ga.job[1], h->xs, B, Dc, Dc, c.critic.w1, c.critic.b1, h->c_h1[1], H, 1);
    head_job(ga.job[1], D, H, h->a_h2, c.actor, nullptr, h->logits, c.max_v, c.max_w);
    fwd_job(ga.job[2], h->x2, B, Dc, Dc, c.critic_t.w1, c.critic_t.b1, h->c_h1[2], H, 1);
    head_job(ga.job[2], D, H, h->t_h2, c.actor_t, nullptr, nullptr, c.max_v, c.max_w);
    launch_gemm(GEMM_F, false, ga, 3, st);
    // 5. their second layers; q = h2 . W3 + b3 as per-tile partial sums of critic (slot 0) and critic_t (slot 2); on the pi(s)
    // branch the first link of -mean Q (:217): dz = -(1 / B) W3 [h2 > 0]; the tick
    fwd_job(ga.job[0], h->c_h1[0], B, H, H, c.critic.w2, c.critic.b2, h->c_h2[0], H, 1);
    ga.job[0].qp_w3 = c.critic.w3; ga.job[0].qp_b3 = c.critic.b3; ga.job[0].qp_out = h->qpart; ga.job[0].qp_nt = qnt;
    fwd_job(ga.job[1], h->c_h1[1], B, H, H, c.critic.w2, c.critic.b2, h->c_h2[1], H, 1);
    ga.job[1].dz_w3 = c.critic.w3; ga.job[1].dz_out = h->dz2p; ga.job[1].dz_rows = (float)B;
    fwd_job(ga.job[2], h->c_h1[2], B, H, H, c.critic_t.w2, c.critic_t.b2, h->c_h2[2], H, 1);
    ga.job[2].qp_w3 = c.critic_t.w3; ga.job[2].qp_b3 = c.critic_t.b3; ga.job[2].qp_out = h->qpart + (size_t)2 * B * qnt; ga.job[2].qp_nt = qnt;
    ga.do_tick = 1;
    launch_gemm(GEMM_F, false, ga, 3, st);
    ga.do_tick = 0;
    // 6. both through the PRE-update critic: the TD target y = r + (1 - d) gamma q_t (:221-222, one target), the MSE gradient
    // (:230) and dz1 = (dz2 W2) [h1 > 0]; the pi(s) branch on to the action (the two action columns of W1)
    critic_bwd_job(ga.job[0], *h, c.critic, h->c_h1[0], h->c_h2[0], 0, 1, c.gamma, h->dq, h->dz2c, h->dz1c);
    dgrad_job(ga.job[1], h->dz2p, B, H, c.critic.w2, h->c_h1[1], h->dz1p, H);
    ga.job[1].da_w = c.critic.w1 + D; ga.job[1].da_ld = Dc; ga.job[1].da_out = h->dapart; ga.job[1].da_nt = h->dant();
    launch_gemm(GEMM_G, false, ga, 2, st);
    // 7. the actor: through the heads' derivatives and its second hidden layer
    actor_bwd_job(ga.job[0], *h, c.actor, c.max_v, c.max_w, h->dz2a, h->dz1a);
    launch_gemm(GEMM_G, false, ga, 1, st);
    // 8. weight gradients folded into both Adam steps (:233-238) and the soft updates of both targets (:241-242, from the
    // stepped weights); linear3's gradients are the one- / two-row jobs; loss_out = the critic's MSE
    wgrad_job(ga.job[0], h->dz2c, H, h->c_h1[0], H, H, B, c.critic.w2, c.critic.b2, &h->mom[1][2], h->adam, c.critic_t.w2, c.critic_t.b2);
    wgrad_job(ga.job[1], h->dz1c, H, h->xs, Dc, Dc, B, c.critic.w1, c.critic.b1, &h->mom[1][0], h->adam, c.critic_t.w1, c.critic_t.b1);
    wgrad_job(ga.job[2], h->dq, 1, h->c_h2[0], H, H, B, c.critic.w3, c.critic.b3, &h->mom[1][4], h->adam, c.critic_t.w3, c.critic_t.b3);
    ga.job[2].loss_out = h->loss;
    wgrad_job(ga.job[3], h->dz2a, H, h->a_h1, H, H, B, c.actor.w2, c.actor.b2, &h->mom[0][2], h->adam + 2, c.actor_t.w2, c.actor_t.b2);
    wgrad_job(ga.job[4], h->dz1a, H, h->xs, Dc, D, B, c.actor.w1, c.actor.b1, &h->mom[0][0], h->adam + 2, c.actor_t.w1, c.actor_t.b1);
    wgrad_job(ga.job[5], h->dl, 2, h->a_h2, H, H, B, c.actor.w3, c.actor.b3, &h->mom[0][4], h->adam + 2, c.actor_t.w3, c.actor_t.b3);
    launch_gemm(GEMM_H, false, ga, 6, st);
    CN_HIPCHK(td3_fail, hipGetLastError());
    return CN_OK;
}

// ---- cn_ddpg_act: the actor and its Ornstein-Uhlenbeck noise in one launch ------------------------------------------------------------
// A tile of 16 rows per workgroup, 8 waves: actor_tile (crowdnav_actor.h) as cn_actor_kernel runs it -- same packed weights, same k
// order, same heads, so pi is cn_actor_forward's head value bit for bit -- with OuNoise as the output stage's noise: thread = (row,
// component o), OUNoise.sample and numpy's `action += noise` in float64; the tile clips and stores.  Errors go to the environment's
// channel, cn_last_error, like cn_actor_forward's.
// x + (theta (mu - x) + sigma U) as ddpg.py:59-61 evaluates it: four float64 operations, each rounded on its own (no FMA)
__device__ __forceinline__ double ou_step(double x, double mu, double theta, double sigma, double U)
{
#pragma clang fp contract(off)
    const double drift = theta * (mu - x);
    const double kick = sigma * U;
    const double dx = drift + kick;
    return x + dx;
}
// the device draw (include/crowdnav.h states it): 53 bits keyed by (seed, counter, row, component) and by nothing else
__device__ __forceinline__ double ou_uniform(uint64_t seed, uint64_t counter, uint64_t row, int o)
{
    const uint64_t h = cn_mix64(cn_mix64(seed ^ cn_mix64(counter ^ 0x4F55ull)) ^ (2ull * row + (uint64_t)o));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}
struct OuNoise {
    double* state; const uint8_t* reset; const double* u; double* noise_out;
    double mu, theta, sigma;
    uint64_t seed, counter;
    int add_noise;
    __device__ __forceinline__ float operator()(float pi, int row, int o, bool live) const
    {
        if (!add_noise || !live) return pi;
        const size_t at = 2 * (size_t)row + o;
        const double x0 = (reset && reset[row]) ? mu : state[at];
        const double U = u ? u[at] : ou_uniform(seed, counter, (uint64_t)row, o);
        const double x1 = ou_step(x0, mu, theta, sigma, U);
        state[at] = x1;
        if (noise_out) noise_out[at] = x1;
        return (float)((double)pi + x1);
    }
};
struct DdpgActArgs {
    const float* obs; const float *w1p, *b1, *w2p, *b2, *w3, *b3; float* action;
    OuNoise ou;
    float max_v, max_w;
    int n, D, Dp;
};
extern "C" __global__ void __launch_bounds__(ACT_THREADS) cn_ddpg_act_kernel(const DdpgActArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float act_sm[];
    const int row0 = blockIdx.x * ACT_M;
    actor_tile<ACT_THREADS / 64, false, OuNoise>(a.obs + (size_t)row0 * a.D, min(ACT_M, a.n - row0), row0, a.D, a.Dp, a.w1p, a.b1, a.w2p, a.b2,
                                                 a.w3, a.b3, a.action + 2 * (size_t)row0, nullptr, a.max_v, a.max_w, 0.0f, 0, 0, act_sm, true, -1, &a.ou);
}

extern "C" int cn_ddpg_act(const cn_actor_weights* actor, const cn_ddpg_act_io* io, int device, void* stream)
{
    const std::string f("cn_ddpg_act");
    if (!actor) return fail(CN_ERR_ARG, f + ": actor is null");
    if (!io) return fail(CN_ERR_ARG, f + ": io is null");
    const cn_actor_weights& w = *actor;
    const float* const ps[6] = {w.w1p, w.b1, w.w2p, w.b2, w.w3, w.b3};
    static const char* const pn[6] = {"actor->w1p", "actor->b1", "actor->w2p", "actor->b2", "actor->w3", "actor->b3"};
    for (int i = 0; i < 6; ++i)
        if (!ps[i]) return fail(CN_ERR_ARG, f + ": " + pn[i] + " is null");
    if (!io->obs) return fail(CN_ERR_ARG, f + ": io->obs is null");
    if (!io->action) return fail(CN_ERR_ARG, f + ": io->action is null");
    if (io->add_noise && !io->state) return fail(CN_ERR_ARG, f + ": io->state is null with add_noise set");
    if (io->n < 0) return fail(CN_ERR_ARG, f + ": io->n is negative");
    if (w.hidden != 256) return fail(CN_ERR_CONFIG, f + ": actor->hidden must be 256");
    if (w.obs_dim < 1) return fail(CN_ERR_CONFIG, f + ": actor->obs_dim must be at least 1");
    if (w.obs_dim_padded < w.obs_dim || (w.obs_dim_padded & 31))
        return fail(CN_ERR_CONFIG, f + ": actor->obs_dim_padded must be obs_dim rounded up to a multiple of 32 (the packed layout of cn_actor_pack_weights)");
    const int Dp = w.obs_dim_padded;
    const size_t lds = actor_tile_bytes((size_t)Dp);       // cn_actor_forward's tile
    if (lds > 160 * 1024) return fail(CN_ERR_CONFIG, f + ": actor->obs_dim: observation too wide for one LDS tile");
    if (io->n == 0) return CN_OK;
    int dev = device;
    if (dev < 0) CN_HIPCHK(fail, hipGetDevice(&dev));
    DeviceScope scope(dev);
    if (lds > 64 * 1024) { static bool attr_set[64] = {false}; const int rc = allow_full_lds((const void*)cn_ddpg_act_kernel, dev, attr_set); if (rc != CN_OK) return rc; }
    const DdpgActArgs a{io->obs, w.w1p, w.b1, w.w2p, w.b2, w.w3, w.b3, io->action,
                        OuNoise{io->state, io->reset, io->u, io->noise_out, io->mu, io->theta, io->sigma, io->seed, io->counter, io->add_noise ? 1 : 0},
                        io->max_v, io->max_w, io->n, w.obs_dim, Dp};
    hipLaunchKernelGGL(cn_ddpg_act_kernel, dim3((io->n + 15) / 16), dim3(ACT_THREADS), lds, (hipStream_t)stream, a);
    CN_HIPCHK(fail, hipGetLastError());
    return CN_OK;
}
