"""crowdnav.train --population with its two --population-record values: one cn_pop_record (two launches) for all members' replay writes
and episode logs per training launch, against one cn_replay_write, cn_get_counters, cn_get_returns and cn_episode_log_add per member.
The two runs end with equal networks -- all six, every member --, equal noise states, equal CSV rows and episode counts, by
torch.equal and row for row: there is no tolerance.  (That either equals the solo runs is tests/test_gpu_train_population.py's
statement, which runs the default, one-call.)"""
import csv

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, P = 23, 3
SWITCHES = ["--algo", "td3", "--learner", "fused", "--scenario", "training_as_logged", "--waypoint-reward", "0", "--envs", "4", "--updates", "2",
            "--launches", "40", "--max-steps", "9", "--memory", "64", "--batch", "8", "--log-every", "10", "--csv",
            "--population", str(P), "--seed", str(SEED)]
NETS = ("actor", "actor_t", "q1", "q1_t", "q2", "q2_t")


def _rows(path):
    return list(csv.reader(open(path)))


def test_the_two_population_record_paths_give_the_same_run(tmp_path, monkeypatch):
    from crowdnav import td3, train
    calls = {"record": 0, "add_masked": 0, "log_add": 0}
    for name, key, cls in (("record", "record", td3.Population), ("add_masked", "add_masked", td3.DeviceReplay),
                           ("add", "log_add", train.DeviceEpisodeLog)):
        orig = getattr(cls, name)

        def counted(self, *a, _orig=orig, _key=key, **kw):
            calls[_key] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(cls, name, counted)
    runs = {}
    for mode in ("one-call", "per-member"):
        before = dict(calls)
        a = train.parse_args(SWITCHES + ["--population-record", mode, "--out", str(tmp_path / mode)])
        agents, episodes = train.train_population(a)
        torch.cuda.synchronize()
        runs[mode] = (agents, episodes, {k: calls[k] - before[k] for k in calls})
    one, per = runs["one-call"], runs["per-member"]
    # each path ran its own calls: 40 record calls and no per-member write, against 40 x P writes and log adds and no record call
    assert one[2] == {"record": 40, "add_masked": 0, "log_add": 0}
    assert per[2] == {"record": 0, "add_masked": 40 * P, "log_add": 40 * P}
    assert one[1] == per[1] and len(one[0]) == len(per[0]) == P and all(e > 0 for e in one[1])
    for p in range(P):
        x, y = one[0][p], per[0][p]
        assert len(x.memory) > 8 and len(x.memory) == len(y.memory)                    # updates started within the run
        for k in ("s", "s2", "a", "r", "d", "pos_dev", "size_dev"):
            assert torch.equal(getattr(x.memory, k), getattr(y.memory, k)), (p, k)
        for net in NETS:
            for u, v in zip(getattr(x, net).parameters(), getattr(y, net).parameters()):
                assert torch.equal(u, v), (p, net, float((u - v).abs().max()))
        assert not torch.equal(next(x.actor.parameters()), next(x.actor_t.parameters()))      # ... and moved the actor
        assert x.noise_state() == y.noise_state() and x.noise_state()[1] == 40
        got, want = _rows(tmp_path / "one-call" / ("member%d" % p) / "td3_training.csv"), _rows(tmp_path / "per-member" / ("member%d" % p) / "td3_training.csv")
        assert len(want) > 1 and got == want, (p, len(got), len(want))
        assert one[1][p] == len(want) - 1
    for u, v in zip(one[0][0].actor.parameters(), one[0][1].actor.parameters()):
        assert not torch.equal(u, v)                # the members are different runs
