"""TEST INFRASTRUCTURE.  cn_td3_pop_exploit's statement (include/crowdnav.h) restated in NumPy: fitness from the logs' totals, the
ranking, the source choice and the perturb / clamp of the hyper-parameters.  Python integers masked to 64 bits, numpy float32
multiplication; nothing here touches a device."""
import math

import numpy as np

M64 = (1 << 64) - 1
HYPERS = ("lr_actor", "lr_critic", "gamma", "noise_std", "noise_clip")
NH = len(HYPERS)


def mix64(z):
    """splitmix64's finaliser, as include/crowdnav.h writes it out."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mask_of(names):
    return sum(1 << HYPERS.index(n) for n in names)


def make_config(n_replace, min_episodes=1, explore=HYPERS[:2] + HYPERS[3:4], factor=(0.8, 1.2), lo=None, hi=None, seed=0):
    return dict(n_replace=int(n_replace), min_episodes=int(min_episodes), explore_mask=explore if isinstance(explore, int) else mask_of(explore),
                factor=np.asarray(factor, np.float32), lo=np.asarray(lo if lo is not None else [0.0] * NH, np.float32),
                hi=np.asarray(hi if hi is not None else [1e9] * NH, np.float32), seed=int(seed) & M64)


def make_state(hypers):
    """The state a bind leaves: hypers [P][5]."""
    h = np.asarray(hypers, np.float32).reshape(-1, NH).copy()
    P = h.shape[0]
    return dict(calls=0, applied=0, src=np.arange(P, dtype=np.int32), generation=np.zeros(P, np.int32), fitness=np.zeros(P, np.float32),
                hyper=h, last=np.zeros((P, 2), np.float64))


def fitness_from_totals(tot, last, min_episodes):
    """tot [P][5] float64 (episodes, successes, return sum, ...), last [P][2] -> float32 [P], or None when a member is short of episodes."""
    tot, last = np.asarray(tot, np.float64), np.asarray(last, np.float64)
    de, dr = tot[:, 0] - last[:, 0], tot[:, 2] - last[:, 1]
    if not (de >= float(min_episodes)).all():
        return None
    return (dr / de).astype(np.float32)


def rank(fitness):
    """Member indices, best first: fitness descending (-0.0 == 0.0), NaN last, ties to the lower index."""
    f = [float(x) for x in np.asarray(fitness, np.float32)]
    P = len(f)

    def before(p, q):
        if math.isnan(f[p]) or math.isnan(f[q]):
            tie = math.isnan(f[p]) and math.isnan(f[q])
            return (not math.isnan(f[p]) and math.isnan(f[q])) or (tie and p < q)
        return f[p] > f[q] or (f[p] == f[q] and p < q)
    pos = [sum(before(q, p) for q in range(P)) for p in range(P)]
    order = [0] * P
    for p, r in enumerate(pos):
        order[r] = p
    assert sorted(order) == list(range(P))
    return order


def plan(fitness, n, seed, calls):
    """-> [(dst, src)] for k = 0 .. n-1: bottom[k] (worst first) copies from top[mix64(K ^ (k + 1)) % n]."""
    order = rank(fitness)
    P = len(order)
    K = mix64((seed & M64) ^ mix64(calls))
    return [(order[P - 1 - k], order[mix64(K ^ (k + 1)) % n]) for k in range(n)]


def explore(src_hyper, dst, cfg, calls):
    """The destination's five hyper-parameters (float32) from its source's."""
    K = mix64(cfg["seed"] ^ mix64(calls))
    out = np.array(src_hyper, np.float32)
    for k in range(NH):
        v = out[k]
        if (cfg["explore_mask"] >> k) & 1:
            v = np.float32(v * cfg["factor"][mix64(K ^ mix64(0x100 + 8 * dst + k)) >> 63])
        out[k] = min(max(v, cfg["lo"][k]), cfg["hi"][k])
    return out


def exploit(state, cfg, fitness=None, tot=None):
    """One cn_td3_pop_exploit on `state` in place.  fitness: explicit [P], else from tot [P][5].  -> [(dst, src)], or None = skipped."""
    c = state["calls"]
    state["calls"] = c + 1
    if fitness is None:
        fitness = fitness_from_totals(tot, state["last"], cfg["min_episodes"])
        if fitness is None:
            return None
        state["last"][:, 0], state["last"][:, 1] = np.asarray(tot, np.float64)[:, 0], np.asarray(tot, np.float64)[:, 2]
    fitness = np.asarray(fitness, np.float32)
    pairs = plan(fitness, cfg["n_replace"], cfg["seed"], c)
    before = state["hyper"].copy()
    state["fitness"][:] = fitness
    state["src"][:] = np.arange(len(fitness))
    for dst, src in pairs:
        state["src"][dst] = src
        state["generation"][dst] += 1
        state["hyper"][dst] = explore(before[src], dst, cfg, c)
    state["applied"] += 1
    return pairs
