// crowdnav_record_host.h -- the argument checks of a recorder's members, host only: cn_pop_record_create (crowdnav_pop_record.hip) and
// cn_nstep_record_create (crowdnav_nstep.hip) refuse the same members with the same words, so the checks exist once.  `f` is the
// name of the entry point, which every message starts with; errors go to cn_last_error (crowdnav_host.h).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "crowdnav_host.h"

struct CnRecordNamed { const void* ptr; const char* name; int member; };

// the checks that come before any member's
inline int cn_record_check_call(const std::string& f, const void* members, const void* out, int n_members, int obs_dim)
{
    if (!members) return fail(CN_ERR_ARG, f + ": members is null");
    if (!out) return fail(CN_ERR_ARG, f + ": out is null");
    if (n_members < 1 || n_members > CN_POP_RECORD_MAX) return fail(CN_ERR_ARG, f + ": n_members must be 1 ... 64");
    if (obs_dim < 1) return fail(CN_ERR_CONFIG, f + ": obs_dim must be at least 1");
    return CN_OK;
}

// member p's checks; rows_per_call: the most ring rows one call writes for an environment row (two rows of one call must not share a
// slot).  written: what a launch writes, per member -- no two members may share any of it; m's eleven are appended.
inline int cn_record_check_member(const std::string& f, const cn_pop_record_member& m, int p, int obs_dim, int rows_per_call,
                                  std::vector<CnRecordNamed>& written)
{
    const std::string who = ": member " + std::to_string(p) + ": ";
    if (m.n < 0) return fail(CN_ERR_ARG, f + who + "n is negative");
    if (m.n > 0) {
        if (!m.env && !(m.counters && m.last_return))
            return fail(CN_ERR_ARG, f + who + "neither env nor both counters and last_return are given");
        if (m.env && m.n != m.env->cfg.n_envs)
            return fail(CN_ERR_ARG, f + who + "n is " + std::to_string(m.n) + " but env has n_envs " + std::to_string(m.env->cfg.n_envs));
        const void* const rp[5] = {m.prev, m.obs, m.action, m.reward, m.done};
        static const char* const rn[5] = {"prev", "obs", "action", "reward", "done"};
        for (int i = 0; i < 5; ++i)
            if (!rp[i]) return fail(CN_ERR_ARG, f + who + rn[i] + " is null");
    }
    const cn_replay_ring& r = m.ring;
    if (!r.s || !r.a || !r.r || !r.s2 || !r.d || !r.pos_dev || !r.size_dev || r.capacity < 1 || r.obs_dim < 1)
        return fail(CN_ERR_ARG, f + who + "incomplete ring");
    if (!m.log.rows || !m.log.n_dev || !m.log.tot_dev) return fail(CN_ERR_ARG, f + who + "incomplete log");
    if (m.log.max_rows < 0) return fail(CN_ERR_ARG, f + who + "log.max_rows is negative");
    if (rows_per_call == 1) {
        if ((int64_t)m.n > r.capacity)
            return fail(CN_ERR_ARG, f + who + "n exceeds ring.capacity (two rows of one call would share a slot)");
    } else if ((int64_t)m.n * rows_per_call > r.capacity) {
        return fail(CN_ERR_ARG, f + who + "n * n_step is " + std::to_string((int64_t)m.n * rows_per_call) + " and exceeds ring.capacity " +
                                std::to_string(r.capacity) + " (a call that ends every episode would overrun itself)");
    }
    if (r.obs_dim != obs_dim)
        return fail(CN_ERR_CONFIG, f + who + "ring.obs_dim is " + std::to_string(r.obs_dim) + ", obs_dim " + std::to_string(obs_dim));
    const CnRecordNamed mine[11] = {{r.s, "ring.s", p}, {r.a, "ring.a", p}, {r.r, "ring.r", p}, {r.s2, "ring.s2", p}, {r.d, "ring.d", p},
                                    {r.pos_dev, "ring.pos_dev", p}, {r.size_dev, "ring.size_dev", p}, {m.log.rows, "log.rows", p},
                                    {m.log.n_dev, "log.n_dev", p}, {m.log.tot_dev, "log.tot_dev", p}, {m.prev, "prev", p}};
    for (const CnRecordNamed& x : mine) {
        if (!x.ptr) continue;                          // (prev of a member without rows)
        for (const CnRecordNamed& y : written)
            if (y.ptr == x.ptr)
                return fail(CN_ERR_CONFIG, f + who + x.name + " is also member " + std::to_string(y.member) + "'s " + y.name +
                                           " (they would race inside a launch)");
    }
    written.insert(written.end(), mine, mine + 11);
    return CN_OK;
}
