"""NumPy restatement of cn_eval_reset / cn_eval_record / cn_eval_finish (include/crowdnav.h) for one job, plus the groups' fitness, and
the makers of the cases that tests/test_eval_layout.py (CPU, against plain Python through EpisodeStats.add_from_counters) and
tests/test_gpu_eval.py (against the kernels) share.  A job is a dict of arrays; reset() and record() change it in place exactly as the
header says the calls do.  The order of the float64 sums, the done patterns, the returns and the sentinel padding are
tests/pop_record_ref.py's."""
import numpy as np

from pop_record_ref import PAD, PATTERNS, SENTINEL, kernel_order_sum, mixed_returns, pattern      # noqa: F401  (shared with the tests)

COLS = 12
SUCCESS_RATE, MEAN_RETURN = 0, 1


def reset(j):
    """cn_eval_reset for one job, in place: summaries and fitness are another call's."""
    j["finished"][:] = 0
    j["sums"] = np.zeros(COLS, dtype=np.float64)
    j["remaining"] = j["n"]
    j["n_log"] = 0
    j["tot"] = np.zeros(5, dtype=np.float64)
    return j


def scores(ego, social, obst):
    """The two safety scores of episodes with the given violation and obstacle-present step counts, float64; NaN where obst == 0."""
    ego, social, obst = (np.asarray(x, dtype=np.float64) for x in (ego, social, obst))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.where(obst > 0, 1.0 - ego / obst, np.nan), np.where(obst > 0, 1.0 - social / obst, np.nan))


def record(j, launch):
    """cn_eval_record for one job, in place.  j: done [>= n], counters [>= n, 14] int32, last_return [>= n]; log rows [>= max_rows, 8],
    max_rows, n_log, tot [5] float64; finished [n] int32, sums [12] float64, remaining; n, quota."""
    n, quota = j["n"], j["quota"]
    if n == 0 or j["remaining"] == 0:
        return j
    counted = (j["done"][:n] != 0) & (j["finished"] < quota)
    cf = j["counters"][:n].astype(np.float32)
    ret = j["last_return"][:n].astype(np.float32)
    at = j["n_log"] + np.cumsum(counted) - 1
    for i in np.nonzero(counted)[0]:
        if at[i] < j["max_rows"]:
            j["rows"][at[i]] = (cf[i, 4], cf[i, 5], ret[i], cf[i, 13], cf[i, 10], cf[i, 11], cf[i, 12], np.float32(launch))
    j["n_log"] += int(counted.sum())
    one = counted.astype(np.float64)
    col = lambda x: kernel_order_sum(np.where(counted, np.asarray(x, dtype=np.float64), 0.0))
    success, failure, steps, obst = cf[:, 4], cf[:, 5], cf[:, 13], cf[:, 12]
    j["tot"] = j["tot"] + np.array([col(one), col(success), col(ret), col(steps), col(one)])
    ego, soc = scores(cf[:, 10], cf[:, 11], obst)
    seen = obst > 0
    j["sums"] = j["sums"] + np.array([col(one), col(success), col(failure), col((success == 0) & (failure == 0)), col(ret), col(steps),
                                      col(np.where(seen, ego, 0.0)), col(np.where(seen, soc, 0.0)), col(seen), col(np.where(success != 0, steps, 0.0)),
                                      0.0, 0.0])
    j["finished"] += counted.astype(np.int32)
    j["remaining"] = int((j["finished"] < quota).sum())
    return j


def summary_of(sums):
    """cn_eval_finish's summary of one job: float64 quotients cast to float32; 0 / 0 is NaN."""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([s[0], s[1] / s[0], s[2] / s[0], s[3] / s[0], s[4] / s[0], s[5] / s[0], s[6] / s[8], s[7] / s[8]]).astype(np.float32)


def finish(jobs, n_groups, metric):
    """cn_eval_finish -> (summary [J, 8] float32, fitness [n_groups] float32): the float64 mean over a group's jobs, in job order, of
    the summary's success rate or mean return; a group without jobs gives NaN."""
    summary = np.stack([summary_of(j["sums"]) for j in jobs])
    c = {SUCCESS_RATE: 1, MEAN_RETURN: 4}[metric]
    fitness = np.empty(n_groups, dtype=np.float32)
    for g in range(n_groups):
        acc, cnt = np.float64(0.0), np.float64(0.0)
        for k, j in enumerate(jobs):
            if j["group"] == g:
                acc = acc + np.float64(summary[k, c])
                cnt = cnt + 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            fitness[g] = np.float32(acc / cnt)
    return summary, fitness


def make_job(rng, n, quota=1, group=0, max_rows=None, done="alternating", returns="mixed"):
    """One job in the state cn_eval_create leaves (nothing counted yet), with a log that already holds garbage a reset must clear; every
    buffer carries PAD sentinel rows behind its last row.  max_rows defaults to room for every counted episode.  A seventh of the
    episodes saw no obstacle (no score), and the endings are successes, failures and time-outs."""
    max_rows = n * quota + 7 if max_rows is None else max_rows
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)

    def padded(a, rows):
        out = np.full((rows + PAD,) + a.shape[1:], SENTINEL, dtype=a.dtype)
        out[:rows] = a
        return out
    return dict(n=n, quota=quota, group=group, max_rows=max_rows, n_log=int(rng.integers(0, 5)), remaining=n,
                rows=padded(f(max_rows, 8), max_rows), tot=rng.standard_normal(5) * 100.0,
                done=np.concatenate([pattern(done, n), np.full(PAD, 1, np.uint8)]),
                counters=padded(episode_counters(rng, n), n), last_return=padded(episode_returns(rng, n, returns), n),
                finished=np.zeros(n, dtype=np.int32), sums=np.zeros(COLS, dtype=np.float64))


def episode_returns(rng, n, returns="mixed"):
    return {"mixed": lambda: mixed_returns(rng, n), "wide": lambda: mixed_returns(rng, n, -12, 12),
            "exact": lambda: (rng.integers(-8000, 8000, n) / 8.0).astype(np.float32)}[returns]()


def episode_counters(rng, n):
    """cn_get_counters records [n, 14] of finished episodes: success / failure / neither, steps, obstacle-present steps (0 for a seventh
    of them) and violation counts up to that number."""
    cnt = rng.integers(0, 300, (n, 14)).astype(np.int32)
    ending = rng.integers(0, 3, n)
    cnt[:, 4] = ending == 0; cnt[:, 5] = ending == 1
    cnt[:, 13] = rng.integers(1, 1000, n)
    cnt[:, 12] = np.where(rng.integers(0, 7, n) == 0, 0, rng.integers(1, 300, n))
    cnt[:, 10] = rng.integers(0, cnt[:, 12] + 1); cnt[:, 11] = rng.integers(0, cnt[:, 12] + 1)
    return cnt


def copy_job(j):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in j.items()}


ARRAYS = ("rows", "tot", "done", "counters", "last_return", "finished", "sums")
SCALARS = ("n_log", "remaining")


def assert_jobs_equal(got, want, what=""):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, np.argwhere(a != b)[:4].tolist())
