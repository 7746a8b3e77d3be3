// crowdnav_tab.hip -- Q-learning and SARSA, the reference's tabular learners (qlearn.py, sarsa.py), for n rows that share ONE
// table, as one launch of one workgroup (gfx950).  include/crowdnav.h states the semantics; this file keeps them:
//   load     the table into LDS twice: `q0`, the snapshot every bootstrap read of the launch sees, and `q`, the live copy the
//            writes go to.  An absent entry is 0.0 in both, so getQ is a plain read.
//   tiles    the rows are walked in tiles of TAB_T = 512, ascending.  Per tile:
//     phase 1  one row per thread: digitise both observations, look the states up, the bootstrap read(s) from q0, `value`;
//              the row's cell, value and reward go to LDS
//     phase 2  the writes.  Cell c belongs to wavefront c % 8, for the whole launch.  Each wavefront walks the tile in chunks of
//              64 rows, ascending, takes its rows by ballot and applies them one by one, lowest lane first, with every lane of
//              the wavefront computing the same numbers from broadcast LDS reads and lane 0 storing them: the updates of one
//              cell are therefore applied in ascending row order (same wavefront: program order; LDS serves a wavefront's
//              accesses in order), and cells of different wavefronts never meet.  Worst case -- every row on one cell -- is n
//              dependent LDS updates in one wavefront: slow, but neither a race nor a wait on another wavefront.
//   act      after a barrier, one row per thread on the live table.
//   store    the live table back to global memory (only when the launch learned).
// No global atomics, no ordering across workgroups: there is one workgroup.
// Float64 with every operation rounded on its own: __dmul_rn / __dadd_rn / __dsub_rn (and the build's -ffp-contract=off).
//
// Digitising float32 rows.  The env's rows are float32; float32(0.7) < 0.7, so a float32 observation must not be compared with the
// double edges.  The two columns are doubles of the form round(v, 3) narrowed to float32, and the edges are multiples of 0.01.
// Narrowing (round to nearest) is monotone: a <= b implies f32(a) <= f32(b).  Two different multiples of 0.001 of magnitude below
// 16 differ by at least 0.001, more than the float32 spacing there (at most 2^-20 ~ 9.5e-7), so they never narrow to the same
// float32, and with monotonicity a < b implies f32(a) < f32(b).  Hence for an observation x and an edge e, both multiples of 0.001:
// e <= x  <=>  f32(e) <= f32(x), and counting the NARROWED edges <= the float32 observation is np.digitize on the doubles.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <new>
#include <string>
#include <vector>

#include "../../include/crowdnav.h"
#include "crowdnav_device.h"
#include "crowdnav_host.h"

namespace {

thread_local std::string g_tab_err;
int tab_fail(int code, const std::string& msg) { g_tab_err = msg; return code; }

constexpr int TAB_S = CN_TAB_STATES, TAB_A = CN_TAB_ACTIONS, TAB_CELLS = TAB_S * TAB_A;   // 977 x 3 = 2931
constexpr int TAB_ND = 30, TAB_NH = 32;                 // edges: d in 0..30, h in 0..32
constexpr int TAB_PAIRS = (TAB_ND + 1) * (TAB_NH + 1);  // 1023
constexpr int TAB_THREADS = 512, TAB_WAVES = TAB_THREADS / 64, TAB_T = TAB_THREADS;
constexpr uint64_t TAB_K_LEARN = 0x6a09e667f3bcc909ull, TAB_K_ACT = 0xbb67ae8584caa73bull;

// [round(i, 2) for i in np.arange(-3.14, 3.14, 0.19625)] (start_sarsa_training.py:44-45): the decimal literals ARE the doubles
// round() returns
const double RADIAN_BINS[TAB_NH] = {-3.14, -2.94, -2.75, -2.55, -2.36, -2.16, -1.96, -1.77, -1.57, -1.37, -1.18, -0.98, -0.78, -0.59, -0.39, -0.2,
                                    0.0, 0.2, 0.39, 0.59, 0.79, 0.98, 1.18, 1.37, 1.57, 1.77, 1.96, 2.16, 2.36, 2.55, 2.75, 2.94};

struct EpsMemo { double eps0, disc, eps_min, e; long long k; };    // the schedule's loop state, kept between launches

struct TabArgs {
    double* q; uint8_t* present; long long* counts; const uint16_t* state_of; const float* edges; EpsMemo* memo;
    const float *obs_prev, *obs; long long ld; int n, col, learn, act, algo;
    const int32_t* action_prev; const float* reward; const uint8_t* keep;
    double alpha, gamma, eps0, disc, eps_min; const long long* episodes_dev;
    const double *u_learn, *u_act; uint64_t seed, counter;
    int32_t* action; float* twist; int32_t *state, *state_prev; double* q_row;
};

__device__ __forceinline__ double tab_u(const double* u, uint64_t base, int row, int j)
{
    if (u) return u[(size_t)row * 5 + j];
    const uint64_t x = cn_mix64(cn_mix64(base ^ (uint64_t)(uint32_t)row) ^ (uint64_t)j);
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}

// np.digitize(x, edges): the number of edges <= x (edges ascending)
__device__ __forceinline__ int tab_digitize(float x, const float* e, int ne)
{
    int c = 0;
    for (int k = 0; k < ne; ++k) c += (e[k] <= x) ? 1 : 0;
    return c;
}

__device__ __forceinline__ int tab_state(const float* row, int col, const float* edges, const uint16_t* state_of)
{
    const int d = tab_digitize(row[col], edges, TAB_ND), h = tab_digitize(row[col + 1], edges + TAB_ND, TAB_NH);
    return state_of[d * (TAB_NH + 1) + h];
}

__device__ __forceinline__ int tab_pick(double u, int count)     // int(random() * len(seq)), kept inside the sequence
{
    const int k = (int)__dmul_rn(u, (double)count);
    return k < 0 ? 0 : (k >= count ? count - 1 : k);
}

// chooseAction (qlearn.py:47-72, sarsa.py:39-55) on table `t` (absent = 0.0).  qo[3]: the row it ended with.
__device__ __forceinline__ int tab_choose(const double* t, int s, int algo, double eps, const double* u, uint64_t base, int row, double* qo)
{
    double q[3] = {t[3 * s], t[3 * s + 1], t[3 * s + 2]};
    const bool explore = tab_u(u, base, row, 0) < eps;
    int a = -1;
    if (algo == CN_TAB_SARSA) {
        if (explore) a = tab_pick(tab_u(u, base, row, 1), 3);
    } else if (explore) {
        double mx = q[0], mn = q[0];                   // Python's max / min: the first of equal values stays
        if (q[1] > mx) mx = q[1];
        if (q[2] > mx) mx = q[2];
        if (q[1] < mn) mn = q[1];
        if (q[2] < mn) mn = q[2];
        const double amn = fabs(mn), amx = fabs(mx);
        const double mag = amx > amn ? amx : amn;      // max(abs(minQ), abs(maxQ))
        const double half = __dmul_rn(0.5, mag);
        for (int i = 0; i < 3; ++i) q[i] = __dsub_rn(__dadd_rn(q[i], __dmul_rn(tab_u(u, base, row, 1 + i), mag)), half);
    }
    if (a < 0) {
        double mx = q[0];
        if (q[1] > mx) mx = q[1];
        if (q[2] > mx) mx = q[2];
        const int count = (q[0] == mx) + (q[1] == mx) + (q[2] == mx);
        if (count > 1) {
            int k = tab_pick(tab_u(u, base, row, 4), count);
            a = 2;
            for (int i = 0; i < 3; ++i)
                if (q[i] == mx) { if (k == 0) { a = i; break; } --k; }
        } else {
            a = q[0] == mx ? 0 : (q[1] == mx ? 1 : 2);
        }
    }
    qo[0] = q[0]; qo[1] = q[1]; qo[2] = q[2];
    return a;
}

__global__ void __launch_bounds__(TAB_THREADS) tab_learn_act_kernel(TabArgs p)
{
    __shared__ double q0[TAB_CELLS], q[TAB_CELLS];
    __shared__ double t_val[TAB_T];
    __shared__ float t_rew[TAB_T];
    __shared__ float edges[TAB_ND + TAB_NH];
    __shared__ uint16_t state_of[TAB_PAIRS + 1];
    __shared__ short t_cell[TAB_T];
    __shared__ uint8_t present[TAB_CELLS + 5];
    __shared__ long long cnt[TAB_WAVES][2];
    __shared__ double eps_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int c = tid; c < TAB_CELLS; c += TAB_THREADS) {
        const uint8_t pr = p.present[c];
        const double v = pr ? p.q[c] : 0.0;
        q0[c] = v; q[c] = v; present[c] = pr;
    }
    for (int c = tid; c < TAB_PAIRS; c += TAB_THREADS) state_of[c] = p.state_of[c];
    if (tid < TAB_ND + TAB_NH) edges[tid] = p.edges[tid];
    if (tid == 0) {
        // the epsilon of the episode under way: `if epsilon > epsilon_min: epsilon *= discount` once per episode begun, as
        // cn_dqn_act; the loop's state is kept in `memo`, so a launch multiplies only for the episodes finished since the last one
        // (the same products in the same order as from the start)
        double e = p.eps0;
        if (p.episodes_dev && p.disc < 1.0) {
            const long long E = *p.episodes_dev;
            EpsMemo m = *p.memo;
            long long k = 0;
            // (k, e) is a state the loop from k = 0 passes through for this E exactly when k <= E + 1: resume there
            if (m.eps0 == p.eps0 && m.disc == p.disc && m.eps_min == p.eps_min && m.k >= 0 && m.k - 1 <= E) { k = m.k; e = m.e; }
            for (; k <= E && k < (1ll << 22) && e > p.eps_min; ++k) e = __dmul_rn(e, p.disc);
            m.eps0 = p.eps0; m.disc = p.disc; m.eps_min = p.eps_min; m.e = e; m.k = k;
            *p.memo = m;
        }
        eps_s = e;
    }
    long long n_same = 0, n_diff = 0;
    __syncthreads();
    const double eps = eps_s;
    const uint64_t base_learn = cn_mix64(p.seed ^ cn_mix64(p.counter ^ TAB_K_LEARN));
    const uint64_t base_act = cn_mix64(p.seed ^ cn_mix64(p.counter ^ TAB_K_ACT));

    if (p.learn) {
        for (int r0 = 0; r0 < p.n; r0 += TAB_T) {
            {   // phase 1: the bootstrap reads, from the snapshot
                const int i = r0 + tid;
                short cell = -1; double value = 0.0; float rew = 0.f;
                if (i < p.n) {
                    const int s1 = tab_state(p.obs_prev + (size_t)i * p.ld, p.col, edges, state_of);
                    const int s2 = tab_state(p.obs + (size_t)i * p.ld, p.col, edges, state_of);
                    const int a1 = p.action_prev[i];
                    rew = p.reward[i];
                    double boot;
                    if (p.algo == CN_TAB_SARSA) {
                        double qo[3];
                        const int a2 = tab_choose(q0, s2, CN_TAB_SARSA, eps, p.u_learn, base_learn, i, qo);
                        boot = q0[3 * s2 + a2];
                    } else {
                        boot = q0[3 * s2];
                        if (q0[3 * s2 + 1] > boot) boot = q0[3 * s2 + 1];
                        if (q0[3 * s2 + 2] > boot) boot = q0[3 * s2 + 2];
                    }
                    value = __dadd_rn((double)rew, __dmul_rn(p.gamma, boot));
                    if ((!p.keep || p.keep[i]) && a1 >= 0 && a1 < TAB_A) cell = (short)(3 * s1 + a1);
                    if (p.state_prev) p.state_prev[i] = s1;
                }
                t_cell[tid] = cell; t_val[tid] = value; t_rew[tid] = rew;
            }
            __syncthreads();
            // phase 2: the writes of this wavefront's cells, ascending rows
            for (int c0 = 0; c0 < TAB_T && r0 + c0 < p.n; c0 += 64) {
                const int cell = t_cell[c0 + lane];
                const double val = t_val[c0 + lane];
                const float rew = t_rew[c0 + lane];
                unsigned long long mask = __ballot(cell >= 0 && (cell % TAB_WAVES) == wave);
                while (mask) {
                    const int b = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const int cb = __shfl(cell, b, 64);
                    const double vb = __shfl(val, b, 64);
                    const float rb = __shfl(rew, b, 64);
                    const double old = q[cb];
                    double nq;
                    if (!present[cb]) { nq = (double)rb; ++n_same; }                          // learnQ: q[(state, action)] = reward
                    else { nq = __dadd_rn(old, __dmul_rn(p.alpha, __dsub_rn(vb, old))); ++n_diff; }
                    if (lane == 0) { q[cb] = nq; present[cb] = 1; }
                }
            }
            __syncthreads();
        }
        if (lane == 0) { cnt[wave][0] = n_same; cnt[wave][1] = n_diff; }
    }
    __syncthreads();

    if (p.act) {      // on the table after all writes
        for (int i = tid; i < p.n; i += TAB_THREADS) {
            const int s = tab_state(p.obs + (size_t)i * p.ld, p.col, edges, state_of);
            double qo[3];
            const int a = tab_choose(q, s, p.algo, eps, p.u_act, base_act, i, qo);
            p.action[i] = a;
            // environment_stage_1_original.py:412-425: (0.22, 0), (0.22, 2.0), (0.22, -2.0)
            p.twist[2 * i] = 0.22f; p.twist[2 * i + 1] = a == 0 ? 0.f : a == 1 ? 2.0f : -2.0f;
            if (p.q_row) { p.q_row[3 * (size_t)i] = qo[0]; p.q_row[3 * (size_t)i + 1] = qo[1]; p.q_row[3 * (size_t)i + 2] = qo[2]; }
            if (p.state) p.state[i] = s;
        }
    } else if (p.state) {
        for (int i = tid; i < p.n; i += TAB_THREADS) p.state[i] = tab_state(p.obs + (size_t)i * p.ld, p.col, edges, state_of);
    }

    if (p.learn) {
        for (int c = tid; c < TAB_CELLS; c += TAB_THREADS) { p.q[c] = q[c]; p.present[c] = present[c]; }
        if (tid == 0) {
            long long s = 0, d = 0;
            for (int w = 0; w < TAB_WAVES; ++w) { s += cnt[w][0]; d += cnt[w][1]; }
            p.counts[0] += s; p.counts[1] += d;
        }
    }
}

}  // namespace

struct cn_tab_s {
    cn_tab_config cfg;
    int device;
    char* pool = nullptr;          // one allocation: q | counts | memo | edges | state_of | present
    double* q; long long* counts; EpsMemo* memo; float* edges; uint16_t* state_of; uint8_t* present;
    int32_t state_of_host[TAB_PAIRS];
    double dist_host[TAB_ND];
};

extern "C" const char* cn_tab_last_error(void) { return g_tab_err.c_str(); }

extern "C" int cn_tab_create(const cn_tab_config* cfg, int device, cn_tab_handle* out)
{
    if (!cfg || !out) return tab_fail(CN_ERR_ARG, "cn_tab_create: null argument");
    *out = nullptr;
    if (cfg->algo != CN_TAB_QLEARN && cfg->algo != CN_TAB_SARSA) return tab_fail(CN_ERR_CONFIG, "cn_tab_create: algo must be 0 (Q-learning) or 1 (SARSA)");
    if (!(cfg->alpha == cfg->alpha) || !(cfg->gamma == cfg->gamma)) return tab_fail(CN_ERR_CONFIG, "cn_tab_create: alpha / gamma is NaN");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
        return tab_fail(CN_ERR_NO_DEVICE, "cn_tab_create: no HIP device " + std::to_string(device) + " (there is no CPU fallback)");
    cn_tab_s* h = new (std::nothrow) cn_tab_s;
    if (!h) return tab_fail(CN_ERR_SIZE, "cn_tab_create: out of host memory");
    h->cfg = *cfg; h->device = device;
    // the key table: str(d) + str(h) for d ascending, then h ascending, numbered in order of first appearance
    std::vector<std::string> keys;
    uint16_t so[TAB_PAIRS];
    for (int d = 0; d <= TAB_ND; ++d)
        for (int a = 0; a <= TAB_NH; ++a) {
            const std::string k = std::to_string(d) + std::to_string(a);
            size_t j = 0;
            while (j < keys.size() && keys[j] != k) ++j;
            if (j == keys.size()) keys.push_back(k);
            so[d * (TAB_NH + 1) + a] = (uint16_t)j;
            h->state_of_host[d * (TAB_NH + 1) + a] = (int32_t)j;
        }
    if ((int)keys.size() != TAB_S) { delete h; return tab_fail(CN_ERR_CONFIG, "cn_tab_create: the key table does not have 977 states"); }
    float ed[TAB_ND + TAB_NH];
    for (int k = 0; k < TAB_ND; ++k) { h->dist_host[k] = (double)k / 10.0; ed[k] = (float)h->dist_host[k]; }   // round(0.1 k, 2) = the double nearest k / 10
    for (int k = 0; k < TAB_NH; ++k) ed[TAB_ND + k] = (float)RADIAN_BINS[k];
    DeviceScope scope(device);
    const size_t o_q = 0, o_cnt = o_q + sizeof(double) * TAB_CELLS, o_memo = o_cnt + 2 * sizeof(long long), o_ed = o_memo + sizeof(EpsMemo),
                 o_so = o_ed + sizeof(ed), o_pr = o_so + sizeof(so), total = o_pr + TAB_CELLS;
    hipError_t e = hipMalloc((void**)&h->pool, total);
    if (e == hipSuccess) e = hipMemset(h->pool, 0, total);
    if (e == hipSuccess) e = hipMemcpy(h->pool + o_ed, ed, sizeof(ed), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->pool + o_so, so, sizeof(so), hipMemcpyHostToDevice);
    EpsMemo m0; memset(&m0, 0, sizeof(m0)); m0.k = -1;
    if (e == hipSuccess) e = hipMemcpy(h->pool + o_memo, &m0, sizeof(m0), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (h->pool) (void)hipFree(h->pool);
        delete h;
        return tab_fail(CN_ERR_HIP, std::string("cn_tab_create: ") + hipGetErrorString(e));
    }
    h->q = (double*)(h->pool + o_q); h->counts = (long long*)(h->pool + o_cnt); h->memo = (EpsMemo*)(h->pool + o_memo);
    h->edges = (float*)(h->pool + o_ed); h->state_of = (uint16_t*)(h->pool + o_so); h->present = (uint8_t*)(h->pool + o_pr);
    *out = h;
    return CN_OK;
}

extern "C" void cn_tab_destroy(cn_tab_handle h)
{
    if (!h) return;
    DeviceScope scope(h->device);
    (void)hipDeviceSynchronize();
    if (h->pool) (void)hipFree(h->pool);
    delete h;
}

extern "C" int cn_tab_set(cn_tab_handle h, const double* q_host, const uint8_t* present_host, const int64_t* counts_host)
{
    if (!h || !q_host || !present_host) return tab_fail(CN_ERR_ARG, "cn_tab_set: null argument");
    DeviceScope scope(h->device);
    std::vector<double> qv(TAB_CELLS);
    std::vector<uint8_t> pv(TAB_CELLS);
    for (int c = 0; c < TAB_CELLS; ++c) { pv[c] = present_host[c] ? 1 : 0; qv[c] = pv[c] ? q_host[c] : 0.0; }
    long long cn[2] = {counts_host ? (long long)counts_host[0] : 0, counts_host ? (long long)counts_host[1] : 0};
    CN_HIPCHK(tab_fail, hipDeviceSynchronize());
    CN_HIPCHK(tab_fail, hipMemcpy(h->q, qv.data(), sizeof(double) * TAB_CELLS, hipMemcpyHostToDevice));
    CN_HIPCHK(tab_fail, hipMemcpy(h->present, pv.data(), TAB_CELLS, hipMemcpyHostToDevice));
    CN_HIPCHK(tab_fail, hipMemcpy(h->counts, cn, sizeof(cn), hipMemcpyHostToDevice));
    CN_HIPCHK(tab_fail, hipDeviceSynchronize());
    return CN_OK;
}

extern "C" int cn_tab_get(cn_tab_handle h, double* q_host, uint8_t* present_host, int64_t* counts_host)
{
    if (!h || !q_host || !present_host) return tab_fail(CN_ERR_ARG, "cn_tab_get: null argument");
    DeviceScope scope(h->device);
    CN_HIPCHK(tab_fail, hipDeviceSynchronize());
    CN_HIPCHK(tab_fail, hipMemcpy(q_host, h->q, sizeof(double) * TAB_CELLS, hipMemcpyDeviceToHost));
    CN_HIPCHK(tab_fail, hipMemcpy(present_host, h->present, TAB_CELLS, hipMemcpyDeviceToHost));
    if (counts_host) {
        long long cn[2];
        CN_HIPCHK(tab_fail, hipMemcpy(cn, h->counts, sizeof(cn), hipMemcpyDeviceToHost));
        counts_host[0] = cn[0]; counts_host[1] = cn[1];
    }
    return CN_OK;
}

extern "C" int cn_tab_tables(cn_tab_handle h, int32_t* state_of_host, double* distance_bins_host, double* radian_bins_host)
{
    if (!h) return tab_fail(CN_ERR_ARG, "cn_tab_tables: null handle");
    if (state_of_host) memcpy(state_of_host, h->state_of_host, sizeof(h->state_of_host));
    if (distance_bins_host) memcpy(distance_bins_host, h->dist_host, sizeof(h->dist_host));
    if (radian_bins_host) memcpy(radian_bins_host, RADIAN_BINS, sizeof(RADIAN_BINS));
    return CN_OK;
}

extern "C" int cn_tab_learn_act(cn_tab_handle h, const cn_tab_io* io, void* stream)
{
    if (!h || !io || !io->obs) return tab_fail(CN_ERR_ARG, "cn_tab_learn_act: null argument");
    if (!io->learn && !io->act) return tab_fail(CN_ERR_ARG, "cn_tab_learn_act: neither learn nor act");
    if (io->learn && (!io->obs_prev || !io->action_prev || !io->reward)) return tab_fail(CN_ERR_ARG, "cn_tab_learn_act: learn needs obs_prev, action_prev and reward");
    if (io->act && (!io->action || !io->twist)) return tab_fail(CN_ERR_ARG, "cn_tab_learn_act: act needs action and twist");
    if (io->n < 1 || io->col < 0 || io->obs_ld < (int64_t)io->col + 2) return tab_fail(CN_ERR_CONFIG, "cn_tab_learn_act: n < 1, col < 0 or obs_ld < col + 2");
    if (!(io->epsilon_discount >= 0.0 && io->epsilon_discount <= 1.0) || !(io->epsilon_min > 0.0))
        return tab_fail(CN_ERR_CONFIG, "cn_tab_learn_act: epsilon_discount outside [0, 1] or epsilon_min <= 0");
    DeviceScope scope(h->device);
    TabArgs p;
    p.q = h->q; p.present = h->present; p.counts = h->counts; p.state_of = h->state_of; p.edges = h->edges; p.memo = h->memo;
    p.obs_prev = io->obs_prev; p.obs = io->obs; p.ld = io->obs_ld; p.n = io->n; p.col = io->col; p.learn = io->learn != 0; p.act = io->act != 0;
    p.algo = h->cfg.algo; p.action_prev = io->action_prev; p.reward = io->reward; p.keep = io->keep;
    p.alpha = h->cfg.alpha; p.gamma = h->cfg.gamma; p.eps0 = io->epsilon; p.disc = io->epsilon_discount; p.eps_min = io->epsilon_min;
    p.episodes_dev = (const long long*)io->episodes_dev; p.u_learn = io->u_learn; p.u_act = io->u_act; p.seed = h->cfg.seed; p.counter = io->counter;
    p.action = io->action; p.twist = io->twist; p.state = io->state; p.state_prev = io->learn ? io->state_prev : nullptr; p.q_row = io->q_row;
    hipLaunchKernelGGL(tab_learn_act_kernel, dim3(1), dim3(TAB_THREADS), 0, (hipStream_t)stream, p);
    CN_HIPCHK(tab_fail, hipGetLastError());
    return CN_OK;
}
