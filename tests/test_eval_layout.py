"""The device evaluator of include/crowdnav.h (cn_eval_*) without a GPU: cn_eval_job and cn_eval_state against their ctypes mirrors as
gcc lays them out, the seven exports, every refusal that can be reached without a handle (the argument checks come before any device
work; FAKE pointers are compared and never dereferenced; the refusals that need a live handle are in tests/test_gpu_eval.py), the NumPy
restatement of the statement (tests/eval_ref.py) against an independent plain-Python computation through
EpisodeStats.add_from_counters, and crowdnav.train's new switches."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import eval_ref as E
from conftest import GOLDEN, ROOT
from learner_handle import lib

CN_ERR_ARG, CN_ERR_CONFIG = -1, -2
NAMES = ("cn_eval_create", "cn_eval_destroy", "cn_eval_jobs", "cn_eval_reset", "cn_eval_record", "cn_eval_finish", "cn_eval_state_dev")
FAKE = 0x1000        # a non-null "device pointer"
JOB_FIELDS = ["env", "counters", "last_return", "done", "log", "n", "quota", "group", "reserved"]
STATE_FIELDS = ["remaining", "sums", "summary", "fitness"]


def test_structs_match_their_mirrors_field_by_field(tmp_path):
    _abi, _ = lib()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    job, state = _abi.CnEvalJob, _abi.CnEvalState
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("sizeof_job %zu\\n", sizeof(cn_eval_job));', 'printf("sizeof_state %zu\\n", sizeof(cn_eval_state));',
             'printf("max %d\\n", CN_EVAL_MAX);', 'printf("cols %d\\n", CN_EVAL_COLS);', 'printf("abi %d\\n", CN_ABI_VERSION);',
             'printf("metrics %d %d\\n", CN_EVAL_SUCCESS_RATE, CN_EVAL_MEAN_RETURN);',
             'printf("row %zu\\n", sizeof(((cn_eval_state*)0)->sums[0]));', 'printf("srow %zu\\n", sizeof(((cn_eval_state*)0)->summary[0]));']
    for f in job._fields_:
        lines.append('printf("job.%s %%zu\\n", offsetof(cn_eval_job, %s));' % (f[0], f[0]))
    for f in state._fields_:
        lines.append('printf("state.%s %%zu\\n", offsetof(cn_eval_state, %s));' % (f[0], f[0]))
    lines += ["{ int (*f)(const cn_eval_job*, int, int, int, cn_eval_handle*) = cn_eval_create; (void)f; }",
              "{ void (*f)(cn_eval_handle) = cn_eval_destroy; (void)f; }",
              "{ int (*f)(cn_eval_handle) = cn_eval_jobs; (void)f; }",
              "{ int (*f)(cn_eval_handle, void*) = cn_eval_reset; (void)f; }",
              "{ int (*f)(cn_eval_handle, float, void*) = cn_eval_record; (void)f; }",
              "{ int (*f)(cn_eval_handle, int, float*, void*) = cn_eval_finish; (void)f; }",
              "{ const cn_eval_state* (*f)(cn_eval_handle) = cn_eval_state_dev; (void)f; }",
              "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    obj = tmp_path / "layout.o"
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"),
                    "-o", str(obj), str(src)], check=True)
    stubs = tmp_path / "stubs.c"
    stubs.write_text("\n".join("void %s(void) {}" % n for n in NAMES))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(obj), str(stubs)], check=True)
    got = dict(ln.split(None, 1) for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof_job"]) == C.sizeof(job) == 32 + C.sizeof(_abi.CnEpisodeLog) + 16 == 80
    assert int(got["sizeof_state"]) == C.sizeof(state) == 64 * 4 + 64 * 12 * 8 + 64 * 8 * 4 + 64 * 4 == 8704
    for f in job._fields_:
        assert int(got["job." + f[0]]) == getattr(job, f[0]).offset, f[0]
    for f in state._fields_:
        assert int(got["state." + f[0]]) == getattr(state, f[0]).offset, f[0]
    assert [f[0] for f in job._fields_] == JOB_FIELDS and [f[0] for f in state._fields_] == STATE_FIELDS
    assert int(got["row"]) == 12 * 8 and int(got["srow"]) == 8 * 4          # sums [j][12] float64, summary [j][8] float32: job-major
    assert int(got["max"]) == _abi.CN_EVAL_MAX == 64 and int(got["cols"]) == _abi.CN_EVAL_COLS == E.COLS == 12
    assert got["metrics"].split() == ["0", "1"] and (_abi.CN_EVAL_SUCCESS_RATE, _abi.CN_EVAL_MEAN_RETURN) == (0, 1) == (E.SUCCESS_RATE, E.MEAN_RETURN)
    assert _abi.EVAL_METRIC == {"success": 0, "return": 1}
    assert int(got["abi"]) == _abi.EXPECTED_ABI == 7              # additive: the version stays


def test_the_seven_names_are_exported_with_prototypes():
    _abi, L = lib()
    for name in NAMES:
        assert name in _abi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.cn_eval_create.argtypes == [C.POINTER(_abi.CnEvalJob), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    assert L.cn_eval_reset.argtypes == [C.c_void_p, C.c_void_p]
    assert L.cn_eval_record.argtypes == [C.c_void_p, C.c_float, C.c_void_p]
    assert L.cn_eval_finish.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.cn_eval_state_dev.restype is C.c_void_p and L.cn_eval_destroy.restype is None
    assert L.cn_abi_version() == 7


def _log(_abi, base=FAKE, **kw):
    f = dict(rows=base, max_rows=100, n_dev=base + 8, tot_dev=base + 16)
    f.update(kw)
    return _abi.CnEpisodeLog(**f)


def _job(_abi, base, log=None, **kw):
    """A valid explicit-array job whose three written pointers are base + 0, 8, 16 (distinct between bases 0x100 apart)."""
    f = dict(env=None, counters=FAKE, last_return=FAKE, done=FAKE, log=_log(_abi, base, **(log or {})), n=16, quota=1, group=0, reserved=0)
    f.update(kw)
    return _abi.CnEvalJob(**f)


def _create(L, jobs, n_jobs, n_groups, want_rc, *texts, out="fresh"):
    h = C.c_void_p()
    rc = L.cn_eval_create(jobs, n_jobs, n_groups, 0, C.byref(h) if out == "fresh" else out)
    msg = L.cn_last_error().decode()
    assert rc == want_rc, (rc, msg)
    for t in texts:
        assert t in msg, (t, msg)
    assert "cn_eval_create" in msg
    assert not h.value                       # *out stays NULL


def test_create_refusals_name_the_field_and_the_job():
    _abi, L = lib()
    arr = lambda *js: (_abi.CnEvalJob * len(js))(*js)
    A, B, Cc = 0x10000, 0x20000, 0x30000
    good = lambda base=A, **kw: _job(_abi, base, **kw)
    _create(L, None, 1, 1, CN_ERR_ARG, "jobs")
    _create(L, arr(good()), 1, 1, CN_ERR_ARG, "out", out=None)
    big = arr(*[good()] * 65)
    for n in (0, -1, 65, 1 << 20):
        _create(L, big, n, 1, CN_ERR_ARG, "n_jobs", "1 ... 64")
    for g in (0, -1, 65, 1 << 20):
        _create(L, arr(good()), 1, g, CN_ERR_ARG, "n_groups", "1 ... 64")
    for g, G in ((1, 1), (-1, 3), (3, 3), (64, 64)):
        _create(L, arr(good(), good(B, group=g)), 2, G, CN_ERR_ARG, "job 1", "group")
    _create(L, arr(good(), good(B, n=-1)), 2, 1, CN_ERR_ARG, "job 1", "n is negative")
    _create(L, arr(good(n=-(1 << 31))), 1, 1, CN_ERR_ARG, "job 0", "n is negative")
    for q in (0, -1, -(1 << 31)):
        _create(L, arr(good(), good(B), good(Cc, quota=q)), 3, 1, CN_ERR_ARG, "job 2", "quota")
    _create(L, arr(good(), good(B, done=None)), 2, 1, CN_ERR_ARG, "job 1", "done is null")
    # neither an environment nor both explicit arrays
    for kw in (dict(counters=None), dict(last_return=None), dict(counters=None, last_return=None)):
        _create(L, arr(good(), good(B, **kw)), 2, 1, CN_ERR_ARG, "job 1", "env", "counters", "last_return")
    # an incomplete log
    for field in ("rows", "n_dev", "tot_dev"):
        _create(L, arr(good(), good(B, log={field: None})), 2, 1, CN_ERR_ARG, "job 1", "incomplete log")
    _create(L, arr(good(log=dict(max_rows=-1))), 1, 1, CN_ERR_ARG, "job 0", "max_rows")
    # two jobs naming the same written array: each of the three, named on both sides
    for field in ("rows", "n_dev", "tot_dev"):
        shared = getattr(_log(_abi, B), field)
        _create(L, arr(good(), good(B), good(Cc, log={field: shared})), 3, 1, CN_ERR_CONFIG, "job 2", "job 1", "log." + field)
    _create(L, arr(good(), good()), 2, 1, CN_ERR_CONFIG, "job 1", "job 0", "race")
    # the first failing check wins in job order
    _create(L, arr(good(n=-1), good(B, done=None)), 2, 1, CN_ERR_ARG, "job 0")


def test_null_handles_are_refused_everywhere():
    _abi, L = lib()
    assert L.cn_eval_reset(None, None) == CN_ERR_ARG and b"cn_eval_reset: null handle" in L.cn_last_error()
    assert L.cn_eval_record(None, 1.0, None) == CN_ERR_ARG and b"cn_eval_record: null handle" in L.cn_last_error()
    for metric in (0, 1, 2):
        assert L.cn_eval_finish(None, metric, None, None) == CN_ERR_ARG and b"cn_eval_finish: null handle" in L.cn_last_error()
    assert L.cn_eval_jobs(None) == 0 and L.cn_eval_state_dev(None) is None
    L.cn_eval_destroy(None)                                       # a no-op, as free(NULL)


# ---- the restatement against plain Python through EpisodeStats.add_from_counters ------------------------------------------------------
def _python_side(j, dones, quota):
    """evaluate()'s rule written as its loop: per call, per environment in index order, an episode counts while the environment has
    counted fewer than `quota`.  -> (EpisodeStats, the counted (call, env) pairs)."""
    from crowdnav.rollout import EpisodeStats
    st, finished, taken = EpisodeStats(), [0] * j["n"], []
    for c, done in enumerate(dones):
        for e in range(j["n"]):
            if done[e] and finished[e] < quota:
                st.add_from_counters(j["counters"][e], float(j["last_return"][e]))
                finished[e] += 1
                taken.append((c, e))
    return st, taken, finished


@pytest.mark.parametrize("quota", (1, 2, 3))
@pytest.mark.parametrize("n", (5, 70, 1100))
def test_restatement_counts_what_the_host_loop_counts(n, quota):
    """Six consecutive calls with random done flags: which episodes are counted and in what order, each episode's two scores bit for
    bit, the sums of exact returns (multiples of 1/8) bit for bit and the score sums against math.fsum."""
    from crowdnav.train import DeviceEpisodeLog
    from crowdnav.rollout import EpisodeStats
    rng = np.random.default_rng(100 * n + quota)
    j = E.reset(E.make_job(rng, n, quota=quota, returns="exact"))
    dones = [(rng.random(n) < 0.45).astype(np.uint8) for _ in range(6)]
    for c, d in enumerate(dones):
        j["done"][:n] = d
        E.record(j, c + 1)
    st, taken, finished = _python_side(j, dones, quota)
    assert j["n_log"] == len(taken) == len(st.rows) and np.array_equal(j["finished"], finished)
    assert j["remaining"] == sum(1 for f in finished if f < quota)
    rows = j["rows"][:j["n_log"]]
    assert [int(r[7]) - 1 for r in rows] == [c for c, _ in taken]                       # the order: call-major, environment order
    back = EpisodeStats()
    for r in rows.tolist():
        back.add_from_counters(r, r[2], cols=DeviceEpisodeLog.COLS)                     # what DeviceEvaluator.stats does with a log row
    same = lambda a, b: a == b or (a != a and b != b)
    assert all(same(x, y) for ra, rb in zip(back.rows, st.rows) for x, y in zip(ra, rb))
    ego, soc = E.scores(rows[:, 4], rows[:, 5], rows[:, 6])
    for k, (r, a, b) in enumerate(zip(st.rows, ego, soc)):
        assert np.float64(r[5]).tobytes() == a.tobytes() and np.float64(r[6]).tobytes() == b.tobytes(), k      # NaN included
    s = j["sums"]
    assert s[0] == len(st.rows) and s[1] == sum(r[1] for r in st.rows) and s[2] == sum(r[2] for r in st.rows)
    assert s[3] == sum(1 for r in st.rows if not r[1] and not r[2]) and s[3] + s[1] + s[2] == s[0]
    assert s[4] == sum(r[3] for r in st.rows) and s[5] == sum(r[4] for r in st.rows)      # exact in float64 whatever the order
    assert s[8] == sum(1 for r in st.rows if r[5] == r[5]) and s[9] == sum(r[4] for r in st.rows if r[1])
    assert s[10] == 0.0 and s[11] == 0.0
    for col, k in ((6, 5), (7, 6)):
        xs = [r[k] for r in st.rows if r[k] == r[k]]
        assert abs(s[col] - math.fsum(xs)) <= len(st.rows) * 2.0 ** -53 * math.fsum(abs(x) for x in xs), col
    assert np.array_equal(j["tot"], np.array([s[0], s[1], s[4], s[5], s[0]]))          # the log's totals: transitions = counted
    summary, fit = E.finish([j], 1, E.SUCCESS_RATE)
    with np.errstate(invalid="ignore"):
        want = np.array([s[0], s[1] / s[0], s[2] / s[0], s[3] / s[0], s[4] / s[0], s[5] / s[0], s[6] / s[8], s[7] / s[8]]).astype(np.float32)
    assert summary.dtype == np.float32 and np.array_equal(summary[0], want, equal_nan=True)
    assert fit.tolist() == [float(summary[0, 1])] and E.finish([j], 1, E.MEAN_RETURN)[1].tolist() == [float(summary[0, 4])]


def test_a_finished_job_and_an_empty_one_change_nothing():
    rng = np.random.default_rng(5)
    j = E.reset(E.make_job(rng, 9, quota=1, done="all"))
    E.record(j, 1)
    assert j["remaining"] == 0 and j["n_log"] == 9
    before = E.copy_job(j)
    E.record(j, 2)
    E.assert_jobs_equal(j, before)
    empty = E.make_job(rng, 0)
    before = E.copy_job(empty)
    E.assert_jobs_equal(E.record(empty, 1), before)
    assert (j["rows"][j["max_rows"]:] == E.SENTINEL).all()


def test_the_nan_cases():
    """No episode at all, episodes none of which saw an obstacle, and a group without jobs."""
    rng = np.random.default_rng(6)
    none = E.reset(E.make_job(rng, 4, done="none", group=0))
    E.record(none, 1)
    blind = E.reset(E.make_job(rng, 4, done="all", group=2))
    blind["counters"][:, 12] = 0
    E.record(blind, 1)
    summary, fit = E.finish([none, blind], 3, E.SUCCESS_RATE)
    assert summary[0, 0] == 0 and np.isnan(summary[0, 1:]).all()
    assert summary[1, 0] == 4 and not np.isnan(summary[1, :6]).any() and np.isnan(summary[1, 6:]).all()
    assert np.isnan(fit[0]) and np.isnan(fit[1]) and fit[2] == summary[1, 1]
    # two jobs of one group: the float64 mean of the two float32 summaries
    a = E.reset(E.make_job(rng, 7, done="all", group=0)); E.record(a, 1)
    b = E.reset(E.make_job(rng, 3, done="all", group=0)); E.record(b, 1)
    summary, fit = E.finish([a, b], 1, E.MEAN_RETURN)
    assert fit[0] == np.float32((np.float64(summary[0, 4]) + np.float64(summary[1, 4])) / 2.0)


def test_max_rows_drops_rows_but_not_sums():
    rng = np.random.default_rng(7)
    full = E.reset(E.make_job(rng, 30, done="all"))
    short = E.copy_job(full)
    short["max_rows"] = 4
    short["rows"] = full["rows"][:4 + E.PAD].copy()
    short["rows"][4:] = E.SENTINEL
    E.record(full, 3); E.record(short, 3)
    assert short["n_log"] == full["n_log"] == 30 and np.array_equal(short["sums"], full["sums"]) and np.array_equal(short["tot"], full["tot"])
    assert np.array_equal(short["rows"][:4], full["rows"][:4]) and (short["rows"][4:] == E.SENTINEL).all()


# ---- crowdnav.train's switches --------------------------------------------------------------------------------------------------------
NEW_KEYS = {"pbt_fitness": "log", "evaluate_on": "host", "eval_scenarios": ("crossing_8",), "eval_every": 0, "eval_envs": 16, "eval_episodes": 1,
            "eval_metric": "success", "eval_summary": False}         # and eval_max_steps = max_steps, eval_seed = seed


def test_todays_command_lines_parse_as_before():
    """The namespaces recorded from the parser as it was before these switches: equal key by key; the new keys hold their defaults."""
    from crowdnav import train
    rec = json.load(open(os.path.join(GOLDEN, "train_namespaces_before_eval.json")))
    assert len(rec["argvs"]) == len(rec["namespaces"]) >= 7
    for argv, old in zip(rec["argvs"], rec["namespaces"]):
        new = vars(train.parse_args(argv))
        for k, v in old.items():
            assert (list(new[k]) if isinstance(new[k], tuple) else new[k]) == v, (argv, k)
        added = {k: new[k] for k in new if k not in old}
        assert added == dict(NEW_KEYS, eval_max_steps=new["max_steps"], eval_seed=new["seed"]), (argv, added)


POP = ["--algo", "td3", "--learner", "fused", "--population", "2"]
EVAL = ["--evaluate", "--load", "x"]


def test_the_new_switches_parse():
    from crowdnav import train
    a = train.parse_args(POP + ["--eval-every", "500", "--eval-scenarios", "crossing_8,towards_8,random_8", "--eval-envs", "32", "--eval-episodes", "2",
                                "--eval-max-steps", "300", "--eval-seed", "9", "--eval-metric", "return", "--pbt-every", "20", "--pbt-fitness", "eval"])
    assert (a.eval_every, a.eval_scenarios, a.eval_envs, a.eval_episodes, a.eval_max_steps, a.eval_seed, a.eval_metric, a.pbt_fitness) == (
        500, ("crossing_8", "towards_8", "random_8"), 32, 2, 300, 9, "return", "eval")
    assert a.evaluate_on == "host" and not a.eval_summary
    a = train.parse_args(POP + ["--seed", "4", "--max-steps", "77", "--pbt-every", "20", "--pbt-fitness", "eval"])
    assert (a.eval_every, a.eval_scenarios, a.eval_max_steps, a.eval_seed, a.pbt_fitness) == (0, ("crossing_8",), 77, 4, "eval")
    a = train.parse_args(EVAL + ["--evaluate-on", "device", "--scenario", "towards_4"])
    assert a.evaluate_on == "device" and a.eval_scenarios == ("towards_4",) and not a.eval_summary
    a = train.parse_args(EVAL + ["--algo", "ddpg", "--evaluate-on", "device", "--eval-scenarios", "crossing_4,ahead_4"])
    assert a.eval_scenarios == ("crossing_4", "ahead_4") and a.eval_summary
    assert train.parse_args(EVAL + ["--evaluate-on", "host"]).evaluate_on == "host"
    # a hand-built namespace gets the defaults
    import argparse
    b = train.fill_defaults(argparse.Namespace(algo="td3", seed=3))
    assert b.evaluate_on == "host" and b.eval_every == 0 and b.pbt_fitness == "log" and b.seed == 3


@pytest.mark.parametrize("argv,flag,text", [
    (["--eval-every", "5"], "--eval-every", "--population"),
    (["--eval-envs", "5"], "--eval-envs", "--population"),
    (["--eval-episodes", "2"], "--eval-episodes", "--population"),
    (["--eval-max-steps", "20"], "--eval-max-steps", "--population"),
    (["--eval-seed", "1"], "--eval-seed", "--population"),
    (["--eval-metric", "return"], "--eval-metric", "--population"),
    (["--eval-scenarios", "crossing_4"], "--eval-scenarios", "--population"),
    (EVAL + ["--eval-scenarios", "crossing_4"], "--eval-scenarios", "--evaluate-on device"),
    (EVAL + ["--evaluate-on", "device", "--eval-envs", "8"], "--eval-envs", "--population"),
    (["--evaluate-on", "device"], "--evaluate-on", "--evaluate"),
    (["--evaluate-on", "host"], "--evaluate-on", "--evaluate"),
    (EVAL + ["--algo", "dqn", "--evaluate-on", "device"], "--evaluate-on", "td3"),
    (EVAL + ["--evaluate-on", "gpu"], "--evaluate-on", "invalid choice"),
    (POP + ["--pbt-fitness", "eval"], "--pbt-fitness", "--pbt-every"),
    (["--pbt-fitness", "log"], "--pbt-fitness", "--pbt-every"),
    (POP + ["--pbt-every", "5", "--pbt-fitness", "best"], "--pbt-fitness", "invalid choice"),
    (POP + ["--eval-metric", "steps"], "--eval-metric", "invalid choice"),
    (POP + ["--eval-every", "-1"], "--eval-every", ">= 0"),
    (POP + ["--eval-envs", "0"], "--eval-envs", ">= 1"),
    (POP + ["--eval-episodes", "0"], "--eval-episodes", ">= 1"),
    (POP + ["--eval-max-steps", "0"], "--eval-max-steps", ">= 1"),
    (POP + ["--eval-scenarios", ","], "--eval-scenarios", "at least one"),
    (POP + ["--eval-scenarios", "crossing_4,crossing_4"], "--eval-scenarios", "once"),
    (["--algo", "td3", "--learner", "fused", "--population", "33", "--eval-scenarios", "crossing_4,towards_4"], "--eval-scenarios", "at most 64"),
    (POP + ["--evaluate", "--evaluate-on", "device"], "--population", "--evaluate"),                  # stays refused
])
def test_the_new_refusals(argv, flag, text, capsys):
    from crowdnav import train
    with pytest.raises(SystemExit) as ex:
        train.parse_args(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert flag in err and text in err, err
