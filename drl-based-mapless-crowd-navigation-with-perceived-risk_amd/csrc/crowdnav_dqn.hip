// crowdnav_dqn.hip -- DQN, the reference's discrete learner, as a fused act and update: cn_dqn_* (include/crowdnav.h).  Its four
// kernels, then the host code that launches them and, through crowdnav_learner.h, the GEMM kernels of crowdnav_gemm.hip.
// deepq.py of the reference: learnOnMiniBatch, selectAction.
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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/crowdnav.h"
#include "crowdnav_device.h"
#include "crowdnav_learner.h"
#include "crowdnav_learner_device.h"

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
// (the layer both hidden layers run through, dqn_act_layer, is crowdnav_learner_device.h's: sac_act_kernel uses it too)
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
        launch_gemm(GEMM_F, true, ga, nj, st);
        fwd_job(ga.job[0], h->h1, 2 * B, H, H, c.q.w2, c.q.b2, h->h2, H, 1);
        fwd_job(ga.job[1], h->th1, B, H, H, c.q_t.w2, c.q_t.b2, h->th2, H, 1);
        launch_gemm(GEMM_F, true, ga, nj, st);
        fwd_job(ga.job[0], h->h2, 2 * B, H, H, c.q.w3, c.q.b3, q, 3, 0);
        fwd_job(ga.job[1], h->th2, B, H, H, c.q_t.w3, c.q_t.b3, h->tq, 3, 0);
        launch_gemm(GEMM_F, true, ga, nj, st);
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
        launch_gemm(GEMM_G, true, ga, 1, st);
        dgrad_job(ga.job[0], h->dz2, 2 * B, H, c.q.w2, h->h1, h->dz1, H);
        launch_gemm(GEMM_G, true, ga, 1, st);
        wgrad_job(ga.job[0], h->dz2, H, h->h1, H, H, 2 * B, c.q.w2, c.q.b2, &h->acc[2]);
        wgrad_job(ga.job[1], h->dz1, H, h->x, ld, D, 2 * B, c.q.w1, c.q.b1, &h->acc[0]);
        wgrad_job(ga.job[2], h->dq, 3, h->h2, H, H, 2 * B, c.q.w3, c.q.b3, &h->acc[4]);
        launch_gemm(GEMM_H, true, ga, 3, st);
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
