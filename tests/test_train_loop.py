"""crowdnav.train's shared collection loop (train.collect + train.RunLog) on the CPU, with a stub environment and stub learners that
record every call: the order of the calls inside a launch, the keep mask, the update gate and count, when the log-time work and the
checkpoints happen, the time limit, and what lands in progress.txt and the CSV.  And train.fill_defaults on the Namespaces that
tests/test_gpu_configs.py builds by hand.  (What the launches compute is the GPU tests' business.)"""
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
    # progress.txt: one line per log interval with the episodes finished so far, then the summary; the CSV: one row per finished episode
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
