"""crowdnav.train --population with its two --population-act values: one launch for all members' actors and one for their re-pack
(cn_actor_pop_forward / cn_actor_pop_pack) against one cn_actor_forward and one four-launch re-pack per member.  The two runs end
with equal networks -- all six, every member -- and equal CSV rows, by torch.equal and row for row: there is no tolerance.  (That
either equals the solo runs is tests/test_gpu_train_population.py's statement, which runs the default, one-launch.)"""
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


def test_the_two_population_act_paths_give_the_same_run(tmp_path, monkeypatch):
    from crowdnav import td3, train
    calls = {"act": 0, "sync": 0, "mfma": 0}
    for name, key, cls in (("act", "act", td3.Population), ("sync_actors", "sync", td3.Population), ("act_mfma", "mfma", td3.Agent)):
        orig = getattr(cls, name)

        def counted(self, *a, _orig=orig, _key=key, **kw):
            calls[_key] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(cls, name, counted)
    runs = {}
    for mode in ("one-launch", "per-member"):
        before = dict(calls)
        a = train.parse_args(SWITCHES + ["--population-act", mode, "--out", str(tmp_path / mode)])
        agents, episodes = train.train_population(a)
        torch.cuda.synchronize()
        runs[mode] = (agents, episodes, {k: calls[k] - before[k] for k in calls})
    one, per = runs["one-launch"], runs["per-member"]
    # each path ran its own calls: 40 population launches and no act_mfma, against 40 x P act_mfma and no population launch
    assert one[2]["act"] == 40 and one[2]["mfma"] == 0 and one[2]["sync"] > 0
    assert per[2]["act"] == 0 and per[2]["sync"] == 0 and per[2]["mfma"] == 40 * P
    assert one[1] == per[1] and len(one[0]) == len(per[0]) == P
    for p in range(P):
        x, y = one[0][p], per[0][p]
        assert len(x.memory) > 8                    # updates started within the run
        for net in NETS:
            for u, v in zip(getattr(x, net).parameters(), getattr(y, net).parameters()):
                assert torch.equal(u, v), (p, net, float((u - v).abs().max()))
        assert not torch.equal(next(x.actor.parameters()), next(x.actor_t.parameters()))      # ... and moved the actor
        assert x.noise_state() == y.noise_state() and x.noise_state()[1] == 40
        got, want = _rows(tmp_path / "one-launch" / ("member%d" % p) / "td3_training.csv"), _rows(tmp_path / "per-member" / ("member%d" % p) / "td3_training.csv")
        assert len(want) > 1 and got == want, (p, len(got), len(want))
    for u, v in zip(one[0][0].actor.parameters(), one[0][1].actor.parameters()):
        assert not torch.equal(u, v)                # the members are different runs
