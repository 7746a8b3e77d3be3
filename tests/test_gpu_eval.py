"""cn_eval_reset / cn_eval_record / cn_eval_finish (include/crowdnav.h) on the GPU.  On explicit arrays every case is compared by bytes,
no tolerance, with the NumPy restatement tests/eval_ref.py (which tests/test_eval_layout.py holds to plain Python on the CPU); with real
environments crowdnav.rollout.DeviceEvaluator is compared with the per-handle loop it replaces, written out in the test.  The only
bytes left open are a NaN's: a summary or a fitness that the statement makes NaN is compared as NaN, not by its payload."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_ref as E
from learner_handle import alias, lib, stream

pytestmark = pytest.mark.gpu

CN_ERR_ARG = -1
DEV_ARRAYS = ("rows", "tot", "done", "counters", "last_return")


def _dev(j):
    """Job j (NumPy, tests/eval_ref.py) on the device: every array with its sentinel rows, the log's counter as int64."""
    t = {k: torch.from_numpy(np.ascontiguousarray(j[k])).cuda() for k in DEV_ARRAYS}
    t["n_log"] = torch.tensor(j["n_log"], dtype=torch.int64, device="cuda")
    return t


def _struct(_abi, t, j):
    """An explicit-array job; one without rows gets NULL row pointers, as the header allows."""
    p = (lambda k: t[k].data_ptr()) if j["n"] else (lambda k: None)
    log = _abi.CnEpisodeLog(rows=t["rows"].data_ptr(), max_rows=j["max_rows"], n_dev=t["n_log"].data_ptr(), tot_dev=t["tot"].data_ptr())
    return _abi.CnEvalJob(env=None, counters=p("counters"), last_return=p("last_return"), done=p("done"), log=log, n=j["n"], quota=j["quota"],
                          group=j["group"], reserved=0)


class Evaluator:
    def __init__(self, structs, n_groups):
        self._abi, self.L = lib()
        self.arr = (self._abi.CnEvalJob * len(structs))(*structs)
        self.h = C.c_void_p()
        rc = self.L.cn_eval_create(self.arr, len(structs), n_groups, 0, C.byref(self.h))
        assert rc == 0, self.L.cn_last_error().decode()
        assert self.L.cn_eval_jobs(self.h) == len(structs)
        self.ptr = self.L.cn_eval_state_dev(self.h)
        assert self.ptr

    def reset(self):
        assert self.L.cn_eval_reset(self.h, stream()) == 0, self.L.cn_last_error().decode()

    def record(self, launch):
        assert self.L.cn_eval_record(self.h, float(launch), stream()) == 0, self.L.cn_last_error().decode()

    def finish(self, metric, fitness=None):
        rc = self.L.cn_eval_finish(self.h, metric, None if fitness is None else C.c_void_p(fitness.data_ptr()), stream())
        assert rc == 0, self.L.cn_last_error().decode()

    def state(self):
        """cn_eval_state as numpy arrays: remaining [64], sums [64, 12], summary [64, 8], fitness [64]."""
        torch.cuda.synchronize()
        st = self._abi.CnEvalState.from_buffer_copy(alias(self.ptr, (C.sizeof(self._abi.CnEvalState),), "|u1").cpu().numpy().tobytes())
        return dict(remaining=np.ctypeslib.as_array(st.remaining).copy(), sums=np.ctypeslib.as_array(st.sums).copy(),
                    summary=np.ctypeslib.as_array(st.summary).copy(), fitness=np.ctypeslib.as_array(st.fitness).copy())

    def close(self):
        torch.cuda.synchronize()
        self.L.cn_eval_destroy(self.h)
        self.h = None


def _same(t, st, k, j, what=""):
    """Device side (tensors t, state st, job index k) against the restatement's job j, by bytes."""
    assert int(t["n_log"]) == j["n_log"], (what, "n_log", int(t["n_log"]), j["n_log"])
    assert int(st["remaining"][k]) == j["remaining"], (what, "remaining", int(st["remaining"][k]), j["remaining"])
    assert st["sums"][k].tobytes() == j["sums"].tobytes(), (what, "sums", st["sums"][k].tolist(), j["sums"].tolist())
    for name in DEV_ARRAYS:
        a, b = t[name].cpu().numpy(), np.asarray(j[name])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:4].tolist())


def _same_nan_aware(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan) and a[~nan].tobytes() == b[~nan].tobytes(), (what, a.tolist(), b.tolist())


def _new_episodes(rng, t, j, returns="mixed"):
    """Fresh episode records of a call, on both sides."""
    n = j["n"]
    j["counters"][:n] = E.episode_counters(rng, n)
    j["last_return"][:n] = E.episode_returns(rng, n, returns)
    t["counters"].copy_(torch.from_numpy(j["counters"])); t["last_return"].copy_(torch.from_numpy(j["last_return"]))


def _set_done(t, j, name):
    n = j["n"]
    j["done"][:n] = E.pattern(name, n)
    t["done"].copy_(torch.from_numpy(j["done"]))


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 2049))
def test_rows_at_the_wave_seam_and_the_tile_every_done_pattern_both_quotas(n):
    """One job, four consecutive calls with done = pattern, pattern, all, pattern and fresh episode records each: `finished` is carried
    from call to call, the quota is crossed mid-run (and, in the third call, for some rows only), and a job that is through is left
    alone.  After every call: the log, the sums and `remaining` against the restatement."""
    _abi, _ = lib()
    rng = np.random.default_rng(n)
    for quota in (1, 2):
        for pat in E.PATTERNS:
            j = E.make_job(rng, n, quota=quota, done=pat)
            t = _dev(j)
            ev = Evaluator([_struct(_abi, t, j)], 1)
            ev.reset(); E.reset(j)
            _same(t, ev.state(), 0, j, (quota, pat, "reset"))
            for call, name in enumerate((pat, pat, "all", pat)):
                _new_episodes(rng, t, j)
                _set_done(t, j, name)
                ev.record(call + 1); E.record(j, call + 1)
                _same(t, ev.state(), 0, j, (quota, pat, call))
            assert j["remaining"] == (0 if quota == 1 or pat == "all" else n - int(E.pattern(pat, n).sum()))
            assert (t["rows"][j["max_rows"]:] == E.SENTINEL).all()
            ev.close()


@pytest.mark.parametrize("case", [
    dict(n=65, max_rows=3, done="all"),                     # three rows fit, 62 are dropped, the count and the sums go on
    dict(n=2049, max_rows=1000, done="alternating"),
    dict(n=17, max_rows=0, done="all"),
], ids=lambda c: "n%d-max%d" % (c["n"], c["max_rows"]))
def test_log_rows_beyond_max_rows_are_dropped_and_counted_and_summed(case):
    _abi, _ = lib()
    rng = np.random.default_rng(case["n"])
    j = E.make_job(rng, quota=2, **case)
    full = E.copy_job(j)
    full["max_rows"] = 2 * case["n"] + 7
    full["rows"] = np.zeros((full["max_rows"] + E.PAD, 8), dtype=np.float32)
    t = _dev(j)
    ev = Evaluator([_struct(_abi, t, j)], 1)
    ev.reset(); E.reset(j); E.reset(full)
    for call in (1, 2):
        ev.record(call); E.record(j, call); E.record(full, call)
    st = ev.state()
    _same(t, st, 0, j)
    counted = 2 * int(E.pattern(case["done"], case["n"]).sum())
    assert int(t["n_log"]) == counted > case["max_rows"]
    assert st["sums"][0].tobytes() == full["sums"].tobytes() and st["sums"][0][0] == counted          # the sums are complete
    assert (t["rows"][case["max_rows"]:] == E.SENTINEL).all()
    ev.close()


@pytest.mark.parametrize("returns", ("mixed", "wide"))
def test_sums_are_added_in_the_log_kernels_order(returns):
    """Returns of 1e-3 ... 1e4 of both signs, and of 1e-12 ... 1e12, where a float64 sum in another order has other bits."""
    _abi, _ = lib()
    rng = np.random.default_rng(3)
    j = E.make_job(rng, 2049, quota=1, done="all", returns=returns)
    t = _dev(j)
    ev = Evaluator([_struct(_abi, t, j)], 1)
    ev.reset(); E.reset(j)
    ev.record(1); E.record(j, 1)
    st = ev.state()
    _same(t, st, 0, j)
    if returns == "wide":
        ret = j["last_return"][:2049].astype(np.float64)
        assert float(np.sum(ret[::-1])) != j["sums"][4]                                # the order is visible in this case
    ev.close()


POP_ROWS, POP_QUOTA, POP_GROUP = (0, 1, 65, 1024, 1500), (1, 2, 1, 3, 2), (0, 0, 2, 2, 0)      # three groups, group 1 without jobs


def _five(seed):
    rng = np.random.default_rng(seed)
    pats = ("all", "all", "last", "alternating", "row1024")
    return rng, [E.make_job(rng, n, quota=q, group=g, done=pats[k]) for k, (n, q, g) in enumerate(zip(POP_ROWS, POP_QUOTA, POP_GROUP))]


def _run_five(js, rng_seed, calls=3, order=None):
    """Jobs js through ONE handle (in `order`) and through the restatement: reset, `calls` record calls with fresh episode records.
    Returns (evaluator, device tensors, state) in js's order."""
    _abi, _ = lib()
    order = list(range(len(js))) if order is None else order
    ts = [_dev(j) for j in js]
    ev = Evaluator([_struct(_abi, ts[k], js[k]) for k in order], 3)
    ev.reset()
    for j in js:
        E.reset(j)
    for call in range(1, calls + 1):
        for k, (t, j) in enumerate(zip(ts, js)):
            _new_episodes(np.random.default_rng(1000 * rng_seed + 10 * call + k), t, j)
        ev.record(call)
        for j in js:
            E.record(j, call)
    return ev, ts, order


def test_five_jobs_three_groups_both_metrics():
    _, js = _five(11)
    ev, ts, _ = _run_five(js, 11)
    st = ev.state()
    for k, (t, j) in enumerate(zip(ts, js)):
        _same(t, st, k, j, "job %d" % k)
        assert (t["rows"][j["max_rows"]:] == E.SENTINEL).all() and (t["counters"][j["n"]:] == int(E.SENTINEL)).all()
        assert (t["last_return"][j["n"]:] == E.SENTINEL).all() and (t["done"][j["n"]:] == 1).all()
    assert int(ts[0]["n_log"]) == 0 and float(ts[0]["tot"].abs().sum()) == 0.0          # the job without rows: reset alone touched its log
    assert (st["summary"] == 0).all() and (st["fitness"] == 0).all()          # not written before a finish
    for metric in (E.SUCCESS_RATE, E.MEAN_RETURN):
        summary, fitness = E.finish(js, 3, metric)
        out = torch.full((3 + E.PAD,), E.SENTINEL, dtype=torch.float32, device="cuda")
        ev.finish(metric, out)
        st = ev.state()
        _same_nan_aware(st["summary"][:5], summary, "summary")
        _same_nan_aware(st["fitness"][:3], fitness, "fitness")
        _same_nan_aware(out[:3].cpu().numpy(), fitness, "fitness_dev")
        assert (out[3:] == E.SENTINEL).all() and (st["fitness"][3:] == 0).all() and (st["summary"][5:] == 0).all()
        # group 1 has no job; group 0 holds the job without rows, whose rates are 0 / 0; group 2 is a number
        assert np.isnan(fitness[1]) and np.isnan(fitness[0]) and not np.isnan(fitness[2])
        assert np.isnan(summary[0, 1:]).all() and summary[0, 0] == 0 and not np.isnan(summary[1:, :6]).any()
    ev.finish(E.SUCCESS_RATE, None)                                        # fitness_dev NULL: the state alone
    _same_nan_aware(ev.state()["fitness"][:3], E.finish(js, 3, E.SUCCESS_RATE)[1])
    for k, (t, j) in enumerate(zip(ts, js)):
        _same(t, ev.state(), k, j, "finish writes nothing else: job %d" % k)
    ev.close()


def test_a_job_gives_the_same_bytes_at_any_position():
    """The 1024-row job at positions 0, 2 and 4 of five, and alone."""
    results = []
    for order in ([3, 0, 1, 2, 4], [0, 1, 3, 2, 4], [0, 1, 2, 4, 3]):
        _, js = _five(12)
        ev, ts, order = _run_five(js, 12, order=order)
        st = ev.state()
        at = order.index(3)
        _same(ts[3], st, at, js[3], "position %d" % at)
        ev.finish(E.MEAN_RETURN)
        results.append((st["sums"][at].tobytes(), ev.state()["summary"][at].tobytes(), ts[3]["rows"].cpu().numpy().tobytes()))
        ev.close()
    assert results[0] == results[1] == results[2]
    _abi, _ = lib()
    _, js = _five(12)
    j = js[3]
    t = _dev(j)
    ev = Evaluator([_struct(_abi, t, j)], 3)
    ev.reset()
    for call in (1, 2, 3):
        _new_episodes(np.random.default_rng(1000 * 12 + 10 * call + 3), t, j)
        ev.record(call)
    ev.finish(E.MEAN_RETURN)
    st = ev.state()
    assert (st["sums"][0].tobytes(), st["summary"][0].tobytes(), t["rows"].cpu().numpy().tobytes()) == results[0]
    ev.close()


def test_a_second_reset_starts_over_and_a_finished_job_is_left_alone():
    _abi, _ = lib()
    rng = np.random.default_rng(13)
    j = E.make_job(rng, 1025, quota=1, done="alternating")
    t = _dev(j)
    ev = Evaluator([_struct(_abi, t, j)], 1)
    first = None
    for run in range(2):
        ev.reset(); E.reset(j)
        _same(t, ev.state(), 0, j, "reset %d" % run)
        _set_done(t, j, "alternating")
        ev.record(1); E.record(j, 1)
        _set_done(t, j, "all")
        ev.record(2); E.record(j, 2)
        st = ev.state()
        _same(t, st, 0, j, "run %d" % run)
        assert j["remaining"] == 0 and j["n_log"] == 1025
        if first is None:
            first = (st["sums"][0].tobytes(), t["rows"].cpu().numpy().tobytes(), t["tot"].cpu().numpy().tobytes())
        else:
            assert first == (st["sums"][0].tobytes(), t["rows"].cpu().numpy().tobytes(), t["tot"].cpu().numpy().tobytes())
    # through: later calls leave everything as it stands, a negative zero in the totals included
    t["tot"][1] = -0.0
    j["tot"][1] = -0.0
    for call in (3, 4):
        _new_episodes(rng, t, j)
        ev.record(call); E.record(j, call)
    _same(t, ev.state(), 0, j, "after the quota")
    assert np.signbit(t["tot"].cpu().numpy()[1])
    ev.close()


def test_captured_in_a_graph_and_replayed():
    """One direct call, then reset + record captured on one stream and replayed twice, against the restatement: the replayed reset
    starts over each time, so the end state is that of reset + one call."""
    _, js = _five(15)
    _abi, _ = lib()
    ts = [_dev(j) for j in js]
    ev = Evaluator([_struct(_abi, t, j) for t, j in zip(ts, js)], 3)
    ev.reset(); ev.record(9)
    torch.cuda.synchronize()
    out = torch.zeros(3, dtype=torch.float32, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev.reset(); ev.record(9); ev.record(10); ev.finish(E.MEAN_RETURN, out)
    g.replay(); g.replay()
    torch.cuda.synchronize()
    for j in js:
        E.reset(j); E.record(j, 9); E.record(j, 10)
    st = ev.state()
    for k, (t, j) in enumerate(zip(ts, js)):
        _same(t, st, k, j, "job %d" % k)
    summary, fitness = E.finish(js, 3, E.MEAN_RETURN)
    _same_nan_aware(st["summary"][:5], summary); _same_nan_aware(out.cpu().numpy(), fitness)
    del g
    ev.close()


def test_the_refusals_that_need_a_live_handle():
    from crowdnav import Config
    from crowdnav.env import VecEnv
    _abi, L = lib()
    j = E.make_job(np.random.default_rng(16), 4)
    t = _dev(j)
    ev = Evaluator([_struct(_abi, t, j)], 1)
    for metric in (-1, 2, 7):
        assert L.cn_eval_finish(ev.h, metric, None, stream()) == CN_ERR_ARG
        msg = L.cn_last_error().decode()
        assert "cn_eval_finish" in msg and "metric" in msg and str(metric) in msg
    ev.close()
    env = VecEnv(Config(n_envs=8, n_peds=20, seed=1, max_steps=9))
    s = _struct(_abi, t, j)
    s.env, s.counters, s.last_return = env.h.value, None, None
    h = C.c_void_p()
    rc = L.cn_eval_create((_abi.CnEvalJob * 1)(s), 1, 1, 0, C.byref(h))
    msg = L.cn_last_error().decode()
    assert rc == CN_ERR_ARG and not h.value and "job 0" in msg and "n_envs 8" in msg and "n is 4" in msg, msg
    env.close()


# ---- real environments: DeviceEvaluator against the per-handle loop ---------------------------------------------------------------------
ENVS, MAX_STEPS, Q = 16, 20, 2


@pytest.fixture(scope="module")
def real():
    """2 actors x 2 worlds, once for the module: the evaluator's run with no read (poll = 0), and the loop it replaces per job on fresh
    handles of the same configurations -- act_mfma(add_noise=False) -> VecEnv.step(auto_reset="next") -> counters() / returns() ->
    EpisodeStats.add_from_counters under the same quota rule -- which also feeds the restatement call by call."""
    from crowdnav import td3, train
    from crowdnav.env import VecEnv
    from crowdnav.rollout import DeviceEvaluator, EpisodeStats
    torch.manual_seed(5)
    specs = [train.scenario_config(s, ENVS, MAX_STEPS, 41) for s in ("crossing_4", "bench")]
    D = specs[0][0].obs_dim
    agents = [td3.Agent(obs_dim=D, device="cuda:0", seed=s, memory_size=16) for s in (1, 2)]
    jobs = [(cfg, init, vel, ag, p) for p, ag in enumerate(agents) for (cfg, init, vel) in specs]
    noise = [ag.noise_state() for ag in agents]
    ev = DeviceEvaluator(jobs, 0)
    launches = ev.run(Q, poll=0)
    fitness = ev.finish("success").cpu()
    out = dict(ev=ev, launches=launches, fitness=fitness, remaining=ev.remaining(), summary=ev.summary(), stats=[ev.stats(k) for k in range(4)],
               noise_kept=[ag.noise_state() for ag in agents] == noise, jobs=jobs,
               logs=[(lg.rows.cpu().numpy().copy(), int(lg.n), lg.tot.cpu().numpy().copy()) for lg in ev.logs],
               sums=ev._eval.state().sums)
    host, restated = [], []
    for cfg, init, vel, ag, group in jobs:
        env = VecEnv(cfg, device=0)
        if init is not None:
            env.set_ped_init(init)
        if vel is not None:
            env.set_ped_preset_vel(vel)
        env.reset()
        obs, st, finished = env.obs, EpisodeStats(), [0] * ENVS
        step_s = (cfg.dt_ms + cfg.scan_latency_ms) / 1000.0
        j = E.reset(E.make_job(np.random.default_rng(0), ENVS, quota=Q, group=group))
        for it in range(1, launches + 1):
            act = ag.act_mfma(obs, add_noise=False)
            obs, _, done = env.step(act, auto_reset="next")
            d = done.cpu().numpy()
            if d.any():
                c, ret = env.counters().cpu(), env.returns()[0].cpu()
                for e in np.nonzero(d)[0].tolist():
                    if finished[e] < Q:
                        st.add_from_counters(c[e], ret[e].item(), step_seconds=step_s)
                        finished[e] += 1
                j["done"][:ENVS], j["counters"][:ENVS], j["last_return"][:ENVS] = d, c.numpy(), ret.numpy()
                E.record(j, it)
        env.close()
        host.append(st); restated.append(j)
    out.update(host=host, restated=restated)
    yield out
    ev.close()


def _rows_equal(a, b):
    same = lambda x, y: x == y or (x != x and y != y)
    return len(a) == len(b) and all(len(r) == len(s) and all(same(x, y) for x, y in zip(r, s)) for r, s in zip(a, b))


def test_real_environments_rows_equal_the_host_loops(real, tmp_path):
    assert real["launches"] == Q * (MAX_STEPS + 1)                         # the bound, derived from the next-step reset convention
    assert real["remaining"].tolist() == [0, 0, 0, 0]                      # ... after which every environment is through
    for k in range(4):
        got, want = real["stats"][k], real["host"][k]
        assert len(got.rows) == ENVS * Q == 32
        assert _rows_equal(got.rows, want.rows), k
        a, b = got.write_csv(str(tmp_path / "device"), "job%d" % k), want.write_csv(str(tmp_path / "host"), "job%d" % k)
        assert open(a).read() == open(b).read()
    assert real["noise_kept"]                                              # the agents' noise streams stand where they stood
    # the two actors differ and so do the worlds: the four jobs are four different evaluations
    assert len({open(str(tmp_path / "device" / ("job%d.csv" % k))).read() for k in range(4)}) == 4


def test_real_environments_log_sums_and_summary_equal_the_restatement(real):
    summary, fitness = E.finish(real["restated"], 2, E.SUCCESS_RATE)
    for k, j in enumerate(real["restated"]):
        rows, n, tot = real["logs"][k]
        assert n == j["n_log"] == 32 and rows[:32].tobytes() == j["rows"][:32].tobytes() and tot.tobytes() == j["tot"].tobytes()
        assert bytes(real["sums"][k]) == j["sums"].tobytes(), k
        assert j["remaining"] == 0
    _same_nan_aware(real["summary"].numpy(), summary)
    _same_nan_aware(real["fitness"].numpy(), fitness)
    assert (real["summary"][:, 0] == 32).all()


def test_real_environments_polling_gives_the_same_rows(real):
    """On fresh handles, as the host loops': an environment that has run before is reset into a world whose clock went on."""
    from crowdnav.rollout import DeviceEvaluator
    ev = DeviceEvaluator(real["jobs"], 0)
    launches = ev.run(Q, poll=16)
    assert launches == real["launches"] or (launches < real["launches"] and launches % 16 == 0)
    assert ev.remaining().tolist() == [0, 0, 0, 0]
    for k in range(4):
        assert _rows_equal(ev.stats(k).rows, real["host"][k].rows), k
    _same_nan_aware(ev.finish("success").cpu().numpy(), real["fitness"].numpy())
    ev.close()
