// crowdnav_sac.hip -- SAC, the reference's last neural learner, as a fused act and update: cn_sac_* (include/crowdnav.h).  Its four
// kernels, then the host code that launches them and, through crowdnav_learner.h, the GEMM kernels of crowdnav_gemm.hip.
// sac.py of the reference: Agent.learn :231-290, Actor.evaluate :78-93, Agent.act :206-229.
// The three GEMM kernels (crowdnav_gemm.hip) are used as they stand (their code paths, arguments and resources are the parent's);
// what SAC adds is row-wise and lives in kernels of its own.  The update, 10 launches (11 with the soft update as the reference
// wrote it):
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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>

#include "../../include/crowdnav.h"
#include "crowdnav_device.h"
#include "crowdnav_learner.h"
#include "crowdnav_learner_device.h"

namespace {
__device__ __forceinline__ float td3_wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
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
bool sac_actor_ok(const cn_sac_actor& a) { return a.w1 && a.b1 && a.w2 && a.b2 && a.mean_w && a.mean_b && a.log_std_w && a.log_std_b; }
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
    launch_prep(pa, st);
    GemmArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.beta1 = c.beta1; ga.beta2 = c.beta2; ga.eps = c.eps; ga.tau = c.tau;
    // 2-3. every forward pass that does not need the new action, on the pre-update weights (SAC:253-257)
    fwd_job(ga.job[0], h->xs, B, Dc, D, c.actor.w1, c.actor.b1, h->a_h1, H, 1);
    fwd_job(ga.job[1], h->xs, B, Dc, Dc, c.q.w1, c.q.b1, h->q_h1, H, 1);
    fwd_job(ga.job[2], h->xs, B, Dc, D, c.v.w1, c.v.b1, h->v_h1, Hv, 1);
    fwd_job(ga.job[3], h->x2, B, Dc, D, c.v_t.w1, c.v_t.b1, h->t_h1, Hv, 1);
    launch_gemm(GEMM_F, false, ga, 4, st);
    fwd_job(ga.job[0], h->a_h1, B, H, H, c.actor.w2, c.actor.b2, h->a_h2, H, 1);
    fwd_job(ga.job[1], h->q_h1, B, H, H, c.q.w2, c.q.b2, h->q_h2, H, 1);
    ga.job[1].qp_w3 = c.q.w3; ga.job[1].qp_b3 = c.q.b3; ga.job[1].qp_out = h->qpart; ga.job[1].qp_nt = qnt;
    fwd_job(ga.job[2], h->v_h1, B, Hv, Hv, c.v.w2, c.v.b2, h->v_h2, Hv, 1);
    ga.job[2].qp_w3 = c.v.w3; ga.job[2].qp_b3 = c.v.b3; ga.job[2].qp_out = h->qpart + slot; ga.job[2].qp_nt = vnt;
    fwd_job(ga.job[3], h->t_h1, B, Hv, Hv, c.v_t.w2, c.v_t.b2, h->t_h2, Hv, 1);
    ga.job[3].qp_w3 = c.v_t.w3; ga.job[3].qp_b3 = c.v_t.b3; ga.job[3].qp_out = h->qpart + 2 * slot; ga.job[3].qp_nt = vnt;
    launch_gemm(GEMM_F, false, ga, 4, st);
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
    launch_gemm(GEMM_F, false, ga, 1, st);
    fwd_job(ga.job[0], h->n_h1, B, H, H, c.q.w2, c.q.b2, h->n_h2, H, 1);
    ga.job[0].qp_w3 = c.q.w3; ga.job[0].qp_b3 = c.q.b3; ga.job[0].qp_out = h->qpart + 3 * slot; ga.job[0].qp_nt = qnt;
    launch_gemm(GEMM_F, false, ga, 1, st);
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
    launch_gemm(GEMM_G, false, ga, 3, st);
    // 9. Adam of Q, then of V (SAC:275-282); soft_update 1: V_t follows the stepped V in the same epilogue
    const cn_td3_mlp none = {}, &t = c.soft_update == 1 ? c.v_t : none;
    wgrad_job(ga.job[0], h->dz2q, H, h->q_h1, H, H, B, c.q.w2, c.q.b2, &h->mom_q[2], h->adam);
    wgrad_job(ga.job[1], h->dz1q, H, h->xs, Dc, Dc, B, c.q.w1, c.q.b1, &h->mom_q[0], h->adam);
    wgrad_job(ga.job[2], h->dq, 1, h->q_h2, H, H, B, c.q.w3, c.q.b3, &h->mom_q[4], h->adam);
    wgrad_job(ga.job[3], h->dz2v, Hv, h->v_h1, Hv, Hv, B, c.v.w2, c.v.b2, &h->mom_v[2], h->adam + 2, t.w2, t.b2);
    wgrad_job(ga.job[4], h->dz1v, Hv, h->xs, Dc, D, B, c.v.w1, c.v.b1, &h->mom_v[0], h->adam + 2, t.w1, t.b1);
    wgrad_job(ga.job[5], h->dv, 1, h->v_h2, Hv, Hv, B, c.v.w3, c.v.b3, &h->mom_v[4], h->adam + 2, t.w3, t.b3);
    launch_gemm(GEMM_H, false, ga, 6, st);
    // 10. Adam of the actor (SAC:285-287): trunk and the two heads (two-row jobs on the columns of dl [B][4])
    wgrad_job(ga.job[0], h->dz2a, H, h->a_h1, H, H, B, c.actor.w2, c.actor.b2, &h->mom_a[2], h->adam + 4);
    wgrad_job(ga.job[1], h->dz1a, H, h->xs, Dc, D, B, c.actor.w1, c.actor.b1, &h->mom_a[0], h->adam + 4);
    wgrad_job(ga.job[2], h->dl, 2, h->a_h2, H, H, B, c.actor.mean_w, c.actor.mean_b, &h->mom_a[4], h->adam + 4);
    wgrad_job(ga.job[3], h->dl + 2, 2, h->a_h2, H, H, B, c.actor.log_std_w, c.actor.log_std_b, &h->mom_a[6], h->adam + 4);
    ga.job[2].lda = 4; ga.job[3].lda = 4;
    launch_gemm(GEMM_H, false, ga, 4, st);
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
