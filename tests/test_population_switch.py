"""crowdnav.train's --population switch: what parse_args accepts and every combination it refuses (no GPU: only the command line)."""
import pytest

BASE = ["--algo", "td3", "--learner", "fused"]


def _parse(argv):
    from crowdnav import train
    return train.parse_args(argv)


def test_population_is_off_by_default_and_accepted_with_fused_td3():
    assert _parse([]).population == 0 and _parse(BASE).population == 0
    for p in (1, 2, 64):
        a = _parse(BASE + ["--population", str(p), "--envs", "4", "--updates", "2", "--seed", "5"])
        assert a.population == p and a.algo == "td3" and a.learner == "fused" and a.seed == 5 and a.out == "runs/td3"
    a = _parse(["--learner", "fused", "--population", "3", "--replay-sample", "without", "--csv"])      # td3 is the default algorithm
    assert a.population == 3 and a.replay_sample == "without" and a.csv


@pytest.mark.parametrize("argv,text", [
    (["--population", "2"], "--learner fused"),                                              # the default learner is torch
    (["--population", "2", "--learner", "torch"], "--learner fused"),
    (["--population", "2", "--learner", "fused", "--algo", "ddpg"], "--algo td3"),
    (["--population", "2", "--learner", "fused", "--algo", "dqn"], "--algo td3"),
    (["--population", "2", "--learner", "fused", "--algo", "sac"], "--algo td3"),
    (["--population", "2", "--learner", "fused", "--algo", "qlearn"], "--algo td3"),
    (["--population", "2", "--learner", "fused", "--algo", "sarsa"], "--algo td3"),
    (BASE + ["--population", "2", "--evaluate"], "--evaluate"),
    (BASE + ["--population", "2", "--load", "runs/td3"], "--load"),
    (BASE + ["--population", "65"], "1 ... 64"),
    (BASE + ["--population", "-1"], "1 ... 64"),
    (BASE + ["--population", "2", "--reset-mode", "same"], "--reset-mode next"),
])
def test_population_refusals(argv, text, capsys):
    with pytest.raises(SystemExit) as ex:
        _parse(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "--population" in err and text in err, err


def test_main_routes_a_population_to_train_population(monkeypatch):
    from crowdnav import train
    seen = []
    monkeypatch.setattr(train, "train_population", lambda a: seen.append(a.population) or "pop")
    monkeypatch.setattr(train, "train", lambda a: "solo")
    assert train.main(BASE + ["--population", "4"]) == "pop" and seen == [4]
    assert train.main(BASE) == "solo"
