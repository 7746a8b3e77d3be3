"""crowdnav.train's shared collection loop (train.collect + train.RunLog) on the CPU, with a stub environment and stub learners that
record every call: the order of the calls inside a launch, the keep mask, the update gate and count, when the log-time work and the
checkpoints happen, the time limit, and what lands in progress.txt and the CSV.  And train.fill_defaults on the Namespaces that
tests/test_gpu_configs.py builds by hand.  The same driver (train.run_loop) under a stub population side, train.PopulationSide's
order after a launch over a stub Population, and its two parts, train.Pbt and train.Evaluation, on CPU tensors and files.  (What the
launches compute is the GPU tests' business.)"""
import argparse
import csv
import os

import pytest
import torch

from crowdnav import train as T

PERIOD = (3, 5, 0)        # env 0 finishes on every 3rd launch, env 1 on every 5th, env 2 never
LAUNCHES, LOG_EVERY, CKPT_EVERY, UPDATES, READY_AT = 20, 4, 3, 2, 7


def finished(it):
    """Episodes finished up to and including launch `it`."""
    return sum(it // p for p in PERIOD if p)


class StubEnv:
    N, D = 3, 2
    cfg = argparse.Namespace(dt_ms=150, scan_latency_ms=10)

    def __init__(self, calls):
        self.calls, self.t, self.done = calls, 0, {}

    def reset(self):
        return torch.zeros((self.N, self.D))

    def step(self, act, auto_reset, want_final=False):
        self.t += 1
        self.calls.append(("step", self.t, auto_reset))
        done = torch.tensor([bool(p) and self.t % p == 0 for p in PERIOD])
        self.done[self.t] = done.clone()
        self._cnt = torch.zeros((self.N, 14), dtype=torch.int32)
        self._cnt[:, 4] = done                                   # every episode a success,
        self._cnt[:, 12] = self._cnt[:, 13] = torch.tensor(PERIOD, dtype=torch.int32)   # its length the env's period
        self._ret = torch.tensor(PERIOD, dtype=torch.float32) * 10
        self.final_obs = torch.full((self.N, self.D), -float(self.t))
        return torch.full((self.N, self.D), float(self.t)), torch.ones(self.N), done.to(torch.uint8)

    def counters(self):
        return self._cnt

    def returns(self):
        return (self._ret,)


class RecordingLog(T.DeviceEpisodeLog):
    def __init__(self, calls):
        super().__init__("cpu", 100, fused=False)
        self.calls = calls

    def add(self, done, counters, last_return, launch, transitions):
        self.calls.append(("log", launch))
        super().add(done, counters, last_return, launch, transitions)


class StubLearner:
    """What train.collect and train.RunLog ask of a learner (train.Learner), every call recorded with the launch it came in."""
    consume_after_log, checkpoints, line_updates, line_steps = False, True, True, True
    csv_name, resume, agent = "stub_training", False, "the agent"

    def __init__(self, calls):
        self.calls, self.it, self.keep, self.stored = calls, 0, {}, {}

    def start(self, obs, elog):
        self.calls.append(("start",))

    def act(self, obs, it):
        self.it = it
        self.calls.append(("act", it))
        return torch.zeros((obs.shape[0], 2))

    def consume(self, prev, act, reward, obs, done, keep):
        self.calls.append(("consume", self.it))
        self.keep[self.it], self.stored[self.it] = keep.clone(), (prev.clone(), obs.clone())

    def ready(self):
        self.calls.append(("ready", self.it))
        return self.it >= READY_AT

    def learn(self, n):
        self.calls.append(("learn", self.it, n))

    def after_updates(self):
        self.calls.append(("after_updates", self.it))

    def epsilon_at(self, episodes):
        self.calls.append(("epsilon_at", self.it, episodes))

    def warn(self, run):
        self.calls.append(("warn", self.it))

    def checkpoint(self, outdir, episodes):
        self.calls.append(("checkpoint", self.it, episodes))

    def close(self):
        self.calls.append(("close",))

    def summary(self, run, last, updates, t):
        return " | %d updates" % updates


class TabularStub(StubLearner):
    consume_after_log, line_updates = True, False

    def ready(self):
        self.calls.append(("ready", self.it))
        return False

    def epsilon_at(self, episodes):
        super().epsilon_at(episodes)
        return 0.5


def run_loop(tmp_path, learner_cls, extra=(), **attrs):
    calls = []
    a = T.parse_args(["--launches", str(LAUNCHES), "--log-every", str(LOG_EVERY), "--checkpoint-every", str(CKPT_EVERY), "--updates", str(UPDATES),
                      "--csv", "--out", str(tmp_path / "run")] + list(extra))
    env, learner = StubEnv(calls), learner_cls(calls)
    for k, v in attrs.items():
        setattr(learner, k, v)
    agent, episodes = T.collect(a, env, learner, elog=RecordingLog(calls))
    assert agent == "the agent"
    return a, env, learner, calls, episodes


def expected_calls(tabular=False, checkpoints=True, launches=LAUNCHES):
    want, learning, n, nxt = [("start",)], False, 0, CKPT_EVERY
    for it in range(1, launches + 1):
        want += [("act", it), ("step", it, "next")]
        want += [("log", it), ("consume", it)] if tabular else [("consume", it), ("log", it)]
        if not learning:
            want.append(("ready", it))
            learning = not tabular and it >= READY_AT
        if learning:
            for _ in range(UPDATES):
                n += 1
                want.append(("learn", it, n))
            want.append(("after_updates", it))
        if it % LOG_EVERY == 0 or it == launches:
            want += [("epsilon_at", it, finished(it)), ("warn", it)]
            if checkpoints and finished(it) >= nxt:
                want.append(("checkpoint", it, finished(it)))
                while nxt <= finished(it):
                    nxt += CKPT_EVERY
    want.append(("close",))
    if checkpoints:
        want.append(("checkpoint", launches, finished(launches)))
    return want, n


def test_replay_learner_call_order_keep_updates_log_times_and_files(tmp_path):
    a, env, learner, calls, episodes = run_loop(tmp_path, StubLearner)
    want, n_updates = expected_calls()
    assert calls == want
    assert episodes == finished(LAUNCHES) == 10
    # keep: everything at launch 1, then the complement of the previous launch's done; s is the observation acted on, s' the step's
    assert bool(learner.keep[1].all())
    for it in range(2, LAUNCHES + 1):
        assert torch.equal(learner.keep[it], ~env.done[it - 1]), it
        assert float(learner.stored[it][0][0, 0]) == it - 1 and float(learner.stored[it][1][0, 0]) == it
    # no update before ready() turned true, then --updates per launch, counted 1, 2, 3, ...
    learns = [c for c in calls if c[0] == "learn"]
    assert [c[2] for c in learns] == list(range(1, n_updates + 1)) and n_updates == UPDATES * (LAUNCHES - READY_AT + 1)
    assert min(c[1] for c in learns) == READY_AT and [c[1] for c in calls if c[0] == "ready"] == list(range(1, READY_AT + 1))
    # log-time work at the multiples of --log-every (the last launch is one); checkpoints when the count first reaches 3, 6, 9, and the final one
    assert [c[1] for c in calls if c[0] == "warn"] == [4, 8, 12, 16, 20]
    assert [c[1:] for c in calls if c[0] == "checkpoint"] == [(8, 3), (12, 6), (20, 10), (20, 10)]
    check_progress_and_csv(a.out, n_updates)


def check_progress_and_csv(out, n_updates):
    """A full run's files in `out`.  progress.txt: one line per log interval with the episodes finished so far, then the summary; the
    CSV: one row per finished episode."""
    a = argparse.Namespace(out=out)
    lines = open(os.path.join(a.out, "progress.txt")).read().splitlines()
    assert len(lines) == 6 and all(l.startswith("launch") for l in lines[:5]) and lines[5].startswith("last 10 episodes: success 1.000")
    assert lines[5].endswith(" | %d updates" % n_updates)
    for l, it in zip(lines, (4, 8, 12, 16, 20)):
        f = l.split()
        assert int(f[1]) == it and int(f[f.index("episodes") + 1]) == finished(it) and int(f[f.index("updates") + 1]) == max(0, UPDATES * (it - READY_AT + 1))
        assert "mean steps" in l and "epsilon" not in l
    # (env-steps: the kept rows -- 3 per launch less one per episode that finished before the last launch)
    assert int(lines[4].split()[3]) == 3 * LAUNCHES - finished(LAUNCHES - 1)
    rows = list(csv.reader(open(os.path.join(a.out, "stub_training.csv"))))
    assert rows[0] == T.EpisodeStats.HEADERS and [int(r[0]) for r in rows[1:]] == list(range(1, 11))
    assert [int(r[4]) for r in rows[1:]] == [3, 5, 3, 3, 5, 3, 3, 5, 3, 5]          # in the order the episodes finished (launch, then env)
    assert all(r[1] == "True" and r[2] == "False" and float(r[3]) == 10.0 * int(r[4]) and float(r[5]) == 1.0 and float(r[6]) == 1.0
               and float(r[7]) == pytest.approx(int(r[4]) * 0.16) for r in rows[1:])


def test_same_call_reset_stores_final_obs_and_every_row(tmp_path):
    a, env, learner, calls, episodes = run_loop(tmp_path, StubLearner, extra=["--reset-mode", "same"])
    assert [c[2] for c in calls if c[0] == "step"] == ["same"] * LAUNCHES and episodes == 10
    for it in range(1, LAUNCHES + 1):
        assert bool(learner.keep[it].all()) and float(learner.stored[it][1][0, 0]) == -it


def test_tabular_learner_consumes_after_the_log_add_and_evaluate_saves_nothing(tmp_path):
    a, env, learner, calls, episodes = run_loop(tmp_path / "learn", TabularStub)
    assert calls == expected_calls(tabular=True)[0] and not [c for c in calls if c[0] in ("learn", "after_updates")]
    for it in range(2, LAUNCHES + 1):
        assert torch.equal(learner.keep[it], ~env.done[it - 1]), it
    lines = open(os.path.join(a.out, "progress.txt")).read().splitlines()
    assert "updates" not in lines[0] and "mean steps" in lines[0] and lines[0].split()[-4:-2] == ["epsilon", "0.500"]
    # --evaluate: the same launches, no checkpoint at the cadence or at the end
    a, env, learner, calls, episodes = run_loop(tmp_path / "evaluate", TabularStub, checkpoints=False)
    assert calls == expected_calls(tabular=True, checkpoints=False)[0] and not [c for c in calls if c[0] == "checkpoint"]
    assert len(list(csv.reader(open(os.path.join(a.out, "stub_training.csv"))))) == 11


def test_a_learner_that_is_never_ready_needs_no_learn(tmp_path):
    """train.Tabular has no `learn` attribute at all: the loop must not touch it before ready() says so."""
    class NoLearn(TabularStub):
        learn = property(lambda self: (_ for _ in ()).throw(AttributeError("learn")))
    assert not hasattr(NoLearn([]), "learn")
    a, env, learner, calls, episodes = run_loop(tmp_path, NoLearn)
    assert calls == expected_calls(tabular=True)[0] and episodes == finished(LAUNCHES)


def test_a_time_limit_already_past_stops_at_the_first_log_interval(tmp_path):
    a, env, learner, calls, episodes = run_loop(tmp_path, StubLearner, extra=["--time-limit", "1e-9"])
    assert env.t == LOG_EVERY and calls == expected_calls(launches=LOG_EVERY)[0] and episodes == finished(LOG_EVERY)


def test_fill_defaults_completes_hand_built_namespaces_and_changes_nothing_that_is_set(tmp_path):
    full = T.parse_args(["--algo", "sac", "--envs", "8", "--learner", "fused"])
    before = dict(vars(full))
    assert T.fill_defaults(full) is full and vars(full) == before
    # the two Namespaces of tests/test_gpu_configs.py (test_training_return_rises, test_batched_trainer_runs_on_the_next_step_reset_kernel)
    hand = [argparse.Namespace(scenario="training_as_logged", envs=16, launches=30000, max_steps=1000, updates=16, batch=128,
                               memory=1_000_000, checkpoint_every=10 ** 9, log_every=1000, ped_vmax=None, seed=0, device=0,
                               out=str(tmp_path / "run"), csv=False, load=None, load_episode=0, evaluate=False,
                               episodes_per_env=1, graphs=1, waypoint_reward=0, scan_f32=None, wheel_accel=None,
                               reset_mode="next", max_csv_rows=100000, time_limit=0.0, learner="fused"),
            argparse.Namespace(scenario="bench", envs=64, launches=120, max_steps=25, updates=1, batch=64, memory=20000,
                               checkpoint_every=10 ** 9, log_every=50, ped_vmax=None, seed=3, device=0,
                               out=str(tmp_path / "run"), csv=True, load=None, load_episode=0, evaluate=False,
                               episodes_per_env=1, graphs=1, waypoint_reward=0, scan_f32=None, wheel_accel=None,
                               reset_mode="same", max_csv_rows=100000, time_limit=0.0, learner="torch")]
    defaults = vars(T.parse_args([]))
    for a in hand:
        was = dict(vars(a))
        T.fill_defaults(a)
        assert set(vars(a)) == set(defaults)
        for k, v in vars(a).items():
            assert v == (was[k] if k in was else defaults[k]), k
        assert a.algo == "td3" and a.ou_noise is False and a.replay_sample == "with" and a.population_act == "one-launch" and a.track_capacity is None


# ---- the same driver under a population side ----------------------------------------------------------------------------------------
class StubPopulationSide:
    """What train.run_loop asks of a side, answered by P stub members: each has its own StubEnv, StubLearner and RunLog on a
    RecordingLog, and its own list of calls -- which must be the list the solo run leaves."""
    after_launch = before_log = close = staticmethod(lambda *args: None)

    def __init__(self, a, P=2):
        self.calls = [[] for _ in range(P)]
        self.envs, self.learners = [StubEnv(c) for c in self.calls], [StubLearner(c) for c in self.calls]
        self.obs = [e.reset() for e in self.envs]
        self.resetting = [torch.zeros(e.N, dtype=torch.bool) for e in self.envs]
        self.runs = [T.RunLog(a, os.path.join(a.out, "member%d" % p), RecordingLog(c), 0.16, L)
                     for p, (c, L) in enumerate(zip(self.calls, self.learners))]
        for L, o, r in zip(self.learners, self.obs, self.runs):
            L.start(o, r.elog)

    def launch(self, it):
        for p, (e, L, r) in enumerate(zip(self.envs, self.learners, self.runs)):
            act = L.act(self.obs[p], it)
            prev = self.obs[p]
            self.obs[p], reward, done = e.step(act, auto_reset="next")
            keep = ~self.resetting[p]
            L.consume(prev, act, reward, self.obs[p], done, keep)
            self.resetting[p] = done.bool()
            r.elog.add(done, e.counters(), e.returns()[0], it, keep)

    def ready(self):
        return all([L.ready() for L in self.learners])               # (every member is asked)

    def learn(self, n):
        for L in self.learners:
            L.learn(n)

    def after_updates(self):
        for L in self.learners:
            L.after_updates()


def population_args(tmp_path, extra=()):
    return T.parse_args(["--launches", str(LAUNCHES), "--log-every", str(LOG_EVERY), "--checkpoint-every", str(CKPT_EVERY), "--updates", str(UPDATES),
                         "--csv", "--out", str(tmp_path / "run")] + list(extra))


def test_the_driver_holds_a_population_side_to_the_solo_statement(tmp_path):
    a = population_args(tmp_path)
    side = StubPopulationSide(a)
    assert T.run_loop(a, side) is side
    want, n_updates = expected_calls()
    for p in range(2):
        assert side.calls[p] == want, p
        assert side.runs[p].episodes == finished(LAUNCHES)
        check_progress_and_csv(os.path.join(a.out, "member%d" % p), n_updates)
    # --time-limit: checked at log time, so a limit already past stops the run at the first log interval
    a = population_args(tmp_path / "limit", extra=["--time-limit", "1e-9"])
    side = StubPopulationSide(a)
    T.run_loop(a, side)
    for p in range(2):
        assert side.envs[p].t == LOG_EVERY and side.calls[p] == expected_calls(launches=LOG_EVERY)[0], p


# ---- train.PopulationSide over a stub Population: what follows a launch, and in which order -------------------------------------------
class StubPopulation:
    """td3.Population's surface as train.PopulationSide, train.Pbt and train.Evaluation use it; every call is recorded."""

    def __init__(self, calls, ready_at=10 ** 9, applied_at=(), summary=None):
        self.calls, self.ready_at, self.applied_at, self.table = calls, ready_at, applied_at, summary
        self.it = self.pbt_calls = self.applied = 0
        self.tot_seen, self.bound_tot = [], None

    def bind_act(self, obs, out):
        self.calls.append(("bind_act",))

    def bind_record(self, envs, prev, obs, act, reward, done, elogs):
        self.calls.append(("bind_record",))

    def bind_pbt(self, n_replace, elogs=None, **kw):
        self.calls.append(("bind_pbt", n_replace))
        self.bound_tot = [e.tot for e in elogs]

    def bind_eval(self, specs, quota, metric, step):
        self.calls.append(("bind_eval", len(specs), quota, metric, step))

    def act(self, add_noise):
        self.calls.append(("act",))

    def record(self, it):
        self.it = it
        self.calls.append(("record", it))

    def resetting(self, p):
        return torch.zeros(2, dtype=torch.uint8)

    def ready(self):
        self.calls.append(("ready", self.it))
        return self.it >= self.ready_at

    def learn(self, n):
        self.calls.append(("learn", self.it, n))

    def sync_actors(self):
        self.calls.append(("sync_actors",))

    def evaluate(self):
        self.calls.append(("evaluate", self.it))
        return "the fitness"

    def evaluator(self):
        pop = self
        return argparse.Namespace(summary=lambda: pop.table, jobs=list(range(len(pop.table))), close=lambda: pop.calls.append(("evaluator_close",)))

    def exploit(self, fitness):
        self.calls.append(("exploit", self.it, fitness))
        self.tot_seen.append(torch.stack(self.bound_tot).clone())     # what cn_td3_pop_exploit would rank on

    def pbt_state(self):
        self.calls.append(("pbt_state", self.it))
        self.pbt_calls += 1
        self.applied += self.pbt_calls in self.applied_at
        members = [dict(src=1 - p, generation=self.applied, fitness=0.5 + p, lr_actor=3e-4, lr_critic=1e-3 * (p + 1), gamma=0.99,
                        noise_std=0.2, noise_clip=0.5) for p in range(2)]
        return dict(calls=self.pbt_calls, applied=self.applied, members=members)

    save_state = load_state = None


class StubMemberEnvs:
    """env.MemberEnvs for P = 2 members of 2 environments, on the CPU."""
    N, D, device = 4, 3, "cpu"
    cfg = argparse.Namespace(dt_ms=150, scan_latency_ms=10)

    def __init__(self, calls):
        self.calls, self.envs = calls, [argparse.Namespace(N=2), argparse.Namespace(N=2)]
        self.reward, self.done = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)

    def bind_step_all(self, act, auto_reset):
        self.calls.append(("bind_step_all", auto_reset))
        return lambda: self.calls.append(("step",))

    def reset(self, group=False):
        return torch.zeros((self.N, self.D))

    def rows(self, p):
        return slice(2 * p, 2 * p + 2)

    def fork(self):
        self.calls.append(("fork",))

    def join(self):
        self.calls.append(("join",))


class StubAgent:
    memory, learn = argparse.Namespace(sync_len=lambda: 0), None      # (Member: its close(); Learner binds learn, the population learns)

    def __init__(self, calls, p):
        self.calls, self.p = calls, p

    def act_mfma(self, obs, out, add_noise):
        self.calls.append(("act_mfma", self.p))

    def sync_fused_weights(self):
        self.calls.append(("sync", self.p))

    def save(self, outdir, episodes):
        pass

    def noise_state(self):
        return 0, 0


POP_SWITCHES = ["--algo", "td3", "--learner", "fused", "--population", "2", "--population-act", "per-member", "--pbt-every", "4", "--eval-every", "8",
                "--launches", "8", "--log-every", "4", "--updates", "2"]


def population_side(tmp_path, monkeypatch, ready_at):
    calls = []
    a = T.parse_args(POP_SWITCHES + ["--out", str(tmp_path)])
    a.state_every = 8            # (parse_args refuses a state beside an evaluation: set past it, the state write below is a recording stub)
    members = [argparse.Namespace(**dict(vars(a), seed=p, out=str(tmp_path / ("member%d" % p)), resume=None)) for p in range(2)]
    pop = StubPopulation(calls, ready_at=ready_at, applied_at=(1,), summary=torch.zeros((2, 8)))
    flush, flush_add = T.DeviceEpisodeLog.flush, T.Pbt.before_log
    monkeypatch.setattr(T.DeviceEpisodeLog, "flush", lambda self: calls.append(("flush",)) or flush(self))
    monkeypatch.setattr(T.Pbt, "before_log", lambda self: calls.append(("flush_add",)) or flush_add(self))
    monkeypatch.setattr(T, "write_state", lambda a, it, save, runs, counts, handles, tensors, scalars, files:
                        calls.append(("state", it, sorted(tensors), dict(counts, **scalars), [os.path.relpath(f, a.out) for f in files])))
    side = T.PopulationSide(a, members, StubMemberEnvs(calls), [StubAgent(calls, p) for p in range(2)], pop)
    setup = list(calls)
    del calls[:]
    T.run_loop(a, side)
    return setup, calls


def test_after_a_launch_updates_repack_evaluation_exploit_flush_log_state_in_that_order(tmp_path, monkeypatch):
    setup, calls = population_side(tmp_path, monkeypatch, ready_at=5)
    sync = [("sync", 0), ("sync", 1)]
    # the switches are resolved before the loop: one step binding, the actors packed per member, one recorder, PBT and the evaluation bound
    assert setup == [("bind_step_all", "next")] + sync + [("bind_record",), ("bind_pbt", 1), ("bind_eval", 1, 1, "success", "multi")]
    launch = lambda it: [("act_mfma", 0), ("act_mfma", 1), ("fork",), ("step",), ("join",), ("record", it)]
    want = []
    for it in range(1, 9):
        want += launch(it)
        if it <= 5:
            want.append(("ready", it))
        if it >= 5:
            want += [("learn", it, 2 * (it - 5) + 1), ("learn", it, 2 * (it - 5) + 2)] + sync
        if it == 8:
            want += [("evaluate", 8), ("exploit", 8, None)] + sync + [("pbt_state", 8)]
        if it % 4 == 0:
            want += [("flush_add",), ("flush",), ("flush",)]
        if it == 8:
            want.append(("state", 8, ["act", "done", "obs", "pbt_flushed", "pbt_tot", "prev", "record_resetting0", "record_resetting1", "resetting", "reward"],
                         dict(it=8, updates_done=8, learning=True, pbt_applied=1), ["pbt_log.csv"]))
    want += [("evaluator_close",)]
    assert calls == want
    # launch 4 was a --pbt-every launch before ready() turned true: no exploit, no read of the PBT state, nothing in the file but the header
    rows = list(csv.reader(open(tmp_path / "pbt_log.csv")))
    assert rows[0] == list(T.PBT_CSV_COLUMNS) and [r[0] for r in rows[1:]] == ["8", "8"]
    assert [r[:2] for r in csv.reader(open(tmp_path / "eval_log.csv"))][1:] == [["8", "0"], ["8", "1"]]


def test_the_evaluation_is_not_tied_to_learning_and_pbt_is(tmp_path, monkeypatch):
    setup, calls = population_side(tmp_path, monkeypatch, ready_at=10 ** 9)
    assert [c for c in calls if c[0] in ("evaluate", "exploit", "pbt_state", "learn")] == [("evaluate", 8)]
    assert [c[1] for c in calls if c[0] == "ready"] == list(range(1, 9))
    assert len(open(tmp_path / "pbt_log.csv").read().splitlines()) == 1 and len(open(tmp_path / "eval_log.csv").read().splitlines()) == 3


# ---- the two parts ------------------------------------------------------------------------------------------------------------------
def test_pbt_ranks_on_flushed_plus_running_totals_and_logs_applied_exploits_only(tmp_path):
    a = T.parse_args(POP_SWITCHES + ["--out", str(tmp_path)])
    calls = []
    pop = StubPopulation(calls, applied_at=(1, 3))
    elogs = [T.DeviceEpisodeLog("cpu", 10, fused=False) for _ in range(2)]
    pbt = T.Pbt(a, pop, elogs, lambda: calls.append(("sync_unbound",)))
    assert calls == [("bind_pbt", 1)] and open(pbt.path).read() == ",".join(T.PBT_CSV_COLUMNS) + "\n"
    plant = lambda k: [e.tot.copy_(torch.arange(5, dtype=torch.float64) * k + 100 * p + k) for p, e in enumerate(elogs)]
    running = lambda: torch.stack([e.tot for e in elogs]).clone()
    plant(1)
    A = running()
    pbt.exploit(4, None)                     # before any flush: the running totals alone
    assert calls[1:] == [("exploit", 0, None), ("sync_unbound",), ("pbt_state", 0)]
    pbt.before_log()                         # the first flush: RunLog.log() reads the totals and restarts them
    for e in elogs:
        e.flush()
    plant(2)
    B = running()
    pbt.exploit(8, "fitness")
    pbt.before_log()                         # the second flush
    for e in elogs:
        e.flush()
    pbt.exploit(10, None)                    # right after a flush: nothing running
    plant(3)
    C = running()
    pbt.exploit(12, None)
    assert [t.tolist() for t in pop.tot_seen] == [A.tolist(), (A + B).tolist(), (A + B).tolist(), (A + B + C).tolist()]
    assert float(C[1, 4]) == 3 * 4 + 100 + 3 and calls[4] == ("exploit", 0, "fitness")
    # rows only when `applied` grew (the first and the third call), PBT_CSV_COLUMNS in order
    rows = list(csv.reader(open(pbt.path)))
    assert rows[0] == list(T.PBT_CSV_COLUMNS) and len(rows) == 5 and pbt.applied == 2
    for r, (it, call, p, gen) in zip(rows[1:], [(4, 0, 0, 1), (4, 0, 1, 1), (10, 2, 0, 2), (10, 2, 1, 2)]):
        assert r == ["%d" % it, "%d" % call, "%d" % p, "%d" % (1 - p), "%d" % gen, "%.9g" % (0.5 + p), "0.0003", "%.9g" % (1e-3 * (p + 1)),
                     "0.99", "0.2", "0.5"]
    # a resumed run opens the part on the same directory: it appends, and there is no second header
    again = T.Pbt(a, StubPopulation([], applied_at=(1,)), elogs, lambda: None)
    again.exploit(16, None)
    rows = list(csv.reader(open(pbt.path)))
    assert len(rows) == 7 and [r[0] for r in rows].count("launch") == 1 and [r[0] for r in rows[5:]] == ["16", "16"]


def test_evaluation_writes_a_row_per_member_and_world_and_the_header_once(tmp_path, capsys):
    worlds = ("crossing_8", "towards_8", "random_8")
    a = T.parse_args(POP_SWITCHES + ["--eval-scenarios", ",".join(worlds), "--eval-episodes", "3", "--eval-metric", "return", "--out", str(tmp_path)])
    table = torch.arange(2 * 3 * 8, dtype=torch.float64).reshape(6, 8) / 7
    calls = []
    pop = StubPopulation(calls, summary=table)
    ev = T.Evaluation(a, pop, "group")
    assert calls == [("bind_eval", 3, 3, "return", "group")]
    assert ev.run(8) == "the fitness" and ev.run(16) == "the fitness" and ev.runs == 2
    path = tmp_path / "eval_log.csv"
    rows = list(csv.reader(open(path)))
    assert rows[0] == list(T.EVAL_CSV_COLUMNS) == ["launch", "member", "world"] + list(T.EVAL_SUMMARY_COLUMNS) and len(rows) == 1 + 2 * 6
    for k, r in enumerate(rows[1:]):
        j = k % 6
        assert r == ["%d" % (8, 16)[k // 6], "%d" % (j // 3), worlds[j % 3]] + ["%.9g" % v for v in table[j].tolist()]
    ev.close(0.0)
    assert calls[-1] == ("evaluator_close",) and "evaluation: 2 runs of 6 jobs" in capsys.readouterr().out
    T.Evaluation(a, pop, "group").run(24)                              # reopened on the same directory: appended under the one header
    rows = list(csv.reader(open(path)))
    assert len(rows) == 1 + 3 * 6 and [r[0] for r in rows].count("launch") == 1 and rows[-1][:3] == ["24", "1", "random_8"]
