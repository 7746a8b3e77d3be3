// crowdnav_ddpg.hip -- DDPG, the reference's baseline learner, as a fused update: cn_ddpg_* (include/crowdnav.h).
// ddpg.py:198-243 of the reference (Agent.learn) on the three GEMM kernels of crowdnav_gemm.hip, with TD3's scaffold (crowdnav_learner.h).
// One critic and its target, no policy delay, no target-policy noise.  The actor loss -mean Q(s, pi(s)) is back-propagated
// BEFORE the critic's step (ddpg.py:226-238), so both gradients are taken at the pre-update weights and the two branches share
// launches.  8 launches:  prep | actor_t L1 (+ actor L1) | L2 (+ L2) | critic_t L1 on (s2, pi_t(s2)), critic L1 on (s, a) and on
// (s, pi(s)) | their L2 (+ q partials of critic_t and critic, dz on the pi(s) branch, tick) | G (critic: dq, dz2 evaluated;
// pi(s) branch: da partials) | G (actor: dl, dz2a evaluated) | H (six jobs: critic and actor W1 / W2 / W3 + Adam + soft updates).
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/crowdnav.h"
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
