"""crowdnav.train's --state-every / --state-keep / --resume switches: off by default, the accepted forms, every refusal, the `latest`
pointer (no GPU: only the command line and the state directory's names)."""
import os

import pytest

BASE = ["--algo", "td3", "--learner", "fused"]
POP = BASE + ["--population", "4"]


def _parse(argv):
    from crowdnav import train
    return train.parse_args(argv)


def _run_with_state(tmp_path, name="launch60"):
    run = tmp_path / "run"
    (run / "state" / name).mkdir(parents=True)
    (run / "state" / "latest").write_text(name + "\n")
    return str(run)


def test_state_is_off_by_default():
    for argv in ([], BASE, POP):
        a = _parse(argv)
        assert a.state_every == 0 and a.state_keep == 1 and a.resume is None


def test_accepted_forms(tmp_path):
    a = _parse(BASE + ["--state-every", "1000"])
    assert a.state_every == 1000 and a.state_keep == 1 and a.out == "runs/td3"
    a = _parse(POP + ["--state-every", "500", "--state-keep", "3", "--pbt-every", "100"])
    assert (a.state_every, a.state_keep, a.pbt_every) == (500, 3, 100)
    run = _run_with_state(tmp_path)
    from crowdnav import train
    assert train.resolve_resume(run) == os.path.join(run, "state", "launch60")
    a = _parse(BASE + ["--resume", run])
    assert a.resume == run and a.out == run                           # continues into the run's own directory
    a = _parse(POP + ["--resume", run, "--state-every", "10", "--out", str(tmp_path / "elsewhere")])
    assert a.out == str(tmp_path / "elsewhere") and a.state_every == 10


@pytest.mark.parametrize("extra,text", [
    (["--learner", "torch"], "--learner fused"),
    (["--algo", "ddpg", "--learner", "fused"], "--algo td3"),
    (["--algo", "sac", "--learner", "fused"], "--algo td3"),
    (["--algo", "dqn", "--learner", "fused"], "--algo td3"),
    (["--algo", "qlearn", "--learner", "fused"], "--algo td3"),
    (["--algo", "sarsa", "--learner", "fused"], "--algo td3"),
    (BASE + ["--reset-mode", "same"], "--reset-mode next"),
    (POP + ["--eval-every", "10"], "evaluation"),
    (POP + ["--pbt-every", "10", "--pbt-fitness", "eval"], "evaluation"),
    (BASE + ["--evaluate", "--load", "x"], "--evaluate"),
])
@pytest.mark.parametrize("switch", ["--state-every", "--resume"])
def test_refusals(tmp_path, capsys, switch, extra, text):
    value = "100" if switch == "--state-every" else _run_with_state(tmp_path)
    with pytest.raises(SystemExit):
        _parse(extra + [switch, value])
    err = capsys.readouterr().err
    assert text in err and switch in err, err


def test_the_default_learner_is_refused(tmp_path, capsys):
    for argv in (["--state-every", "100"], ["--resume", _run_with_state(tmp_path)]):
        with pytest.raises(SystemExit):
            _parse(argv)                                              # --learner torch is the default
        assert "--learner fused" in capsys.readouterr().err


@pytest.mark.parametrize("argv,text", [
    (BASE + ["--state-every", "-1"], ">= 0"),
    (BASE + ["--state-every", "10", "--state-keep", "0"], ">= 1"),
    (BASE + ["--state-keep", "2"], "--state-every"),
])
def test_bad_values(capsys, argv, text):
    with pytest.raises(SystemExit):
        _parse(argv)
    assert text in capsys.readouterr().err


def test_resume_and_load_exclude_each_other(tmp_path, capsys):
    with pytest.raises(SystemExit):
        _parse(BASE + ["--resume", _run_with_state(tmp_path), "--load", "x"])
    assert "--load does not apply" in capsys.readouterr().err


def test_population_with_load_points_to_resume(capsys):
    with pytest.raises(SystemExit):
        _parse(POP + ["--load", "x"])
    err = capsys.readouterr().err
    assert "--population starts its members fresh" in err and "--resume" in err


def test_resume_needs_the_latest_pointer(tmp_path, capsys):
    from crowdnav import train
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(SystemExit):
        _parse(BASE + ["--resume", str(empty)])
    err = capsys.readouterr().err
    assert "--resume" in err and "latest" in err and "does not exist" in err
    with pytest.raises(FileNotFoundError):
        train.resolve_resume(str(empty))
    half = tmp_path / "half"                                          # a state directory that was never completed has no pointer
    (half / "state" / "launch10.tmp123").mkdir(parents=True)
    with pytest.raises(SystemExit):
        _parse(POP + ["--resume", str(half)])
    assert "latest" in capsys.readouterr().err
    gone = tmp_path / "gone"                                          # a pointer to a directory that is not there
    (gone / "state").mkdir(parents=True)
    (gone / "state" / "latest").write_text("launch5\n")
    with pytest.raises(SystemExit):
        _parse(BASE + ["--resume", str(gone)])
    assert "launch5" in capsys.readouterr().err
