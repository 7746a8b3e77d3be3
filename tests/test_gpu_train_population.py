"""crowdnav.train --population against the solo runs it is built from: member p of `--population 2 --seed s` ends with the networks and
the CSV rows of `--seed s + p`, by torch.equal and row for row.  If this fails, the fault is in how train_population builds a member
(a shared generator, a stream ordering, a shared noise counter), not in a tolerance: there is none."""
import csv
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 11
SWITCHES = ["--algo", "td3", "--learner", "fused", "--scenario", "training_as_logged", "--waypoint-reward", "0", "--envs", "4", "--updates", "2",
            "--launches", "40", "--max-steps", "9", "--memory", "64", "--batch", "8", "--log-every", "10", "--csv"]
NETS = ("actor", "actor_t", "q1", "q1_t", "q2", "q2_t")


def _rows(path):
    return list(csv.reader(open(path)))


def test_member_p_is_the_solo_run_of_seed_plus_p(tmp_path):
    from crowdnav import train
    a = train.parse_args(SWITCHES + ["--population", "2", "--seed", str(SEED), "--out", str(tmp_path / "pop")])
    agents, episodes = train.train_population(a)
    torch.cuda.synchronize()
    assert len(agents) == 2
    for p in range(2):
        out = tmp_path / ("solo%d" % p)
        solo, solo_eps = train.train(train.parse_args(SWITCHES + ["--seed", str(SEED + p), "--out", str(out)]))
        torch.cuda.synchronize()
        assert len(solo.memory) > 8                 # updates started within the run
        for net in NETS:
            for x, y in zip(getattr(agents[p], net).parameters(), getattr(solo, net).parameters()):
                assert torch.equal(x, y), (p, net, float((x - y).abs().max()))
        assert not torch.equal(next(solo.actor.parameters()), next(solo.actor_t.parameters()))      # ... and moved the actor
        mdir = tmp_path / "pop" / ("member%d" % p)
        got, want = _rows(mdir / "td3_training.csv"), _rows(out / "td3_training.csv")
        assert len(want) > 1 and got == want, (p, len(got), len(want))
        assert episodes[p] == solo_eps == len(want) - 1
        assert sorted(f for f in os.listdir(mdir) if not f.startswith("progress")) == sorted(f for f in os.listdir(out) if not f.startswith("progress"))
        assert len(open(mdir / "progress.txt").read().splitlines()) == len(open(out / "progress.txt").read().splitlines())
    for x, y in zip(agents[0].actor.parameters(), agents[1].actor.parameters()):
        assert not torch.equal(x, y)                # two seeds, two runs
