"""crowdnav.train --population-replay own|shared: its default, its refusal without --population, and that it is held beside vars() of
the parsed namespace, so that the namespaces recorded from earlier parsers stay what they were.  No GPU."""
import json
import os

import pytest

from test_eval_layout import GOLDEN

POP = ["--algo", "td3", "--learner", "fused", "--population", "2"]


def test_the_default_is_own_and_shared_parses():
    from crowdnav import train
    assert train.parse_args(POP).population_replay == "own"
    assert train.parse_args(POP + ["--population-replay", "own"]).population_replay == "own"
    assert train.parse_args(POP + ["--population-replay", "shared"]).population_replay == "shared"
    assert train.parse_args([]).population_replay == "own"           # a solo run: nothing to choose, nothing refused


def test_it_needs_a_population_and_a_known_value(capsys):
    from crowdnav import train
    for argv in (["--population-replay", "shared"], ["--population-replay", "own"], ["--algo", "ddpg", "--population-replay", "shared"]):
        with pytest.raises(SystemExit):
            train.parse_args(argv)
        assert "--population-replay" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(POP + ["--population-replay", "pooled"])
    assert "invalid choice" in capsys.readouterr().err


def test_it_is_held_beside_the_namespace():
    """vars() of a parsed command line has no key for it, with or without the switch; a copy of vars() (what a population's members
    are built from) simply lacks it; a hand-built namespace filled with the defaults trains with "own"."""
    import argparse
    from crowdnav import train
    for argv in (POP, POP + ["--population-replay", "shared"]):
        a = train.parse_args(argv)
        assert "population_replay" not in vars(a)
        assert not hasattr(argparse.Namespace(**vars(a)), "population_replay")
    assert vars(train.parse_args(POP)) == vars(train.parse_args(POP + ["--population-replay", "shared"]))
    hand = train.fill_defaults(argparse.Namespace(algo="td3"))
    assert getattr(hand, "population_replay", None) is None


def test_recorded_namespaces_are_unchanged():
    """The namespaces recorded before the evaluation switches, key by key, and no key beyond the ones that pull request added."""
    from crowdnav import train
    from test_eval_layout import NEW_KEYS
    rec = json.load(open(os.path.join(GOLDEN, "train_namespaces_before_eval.json")))
    for argv, old in zip(rec["argvs"], rec["namespaces"]):
        new = vars(train.parse_args(argv))
        assert set(new) - set(old) == set(NEW_KEYS) | {"eval_max_steps", "eval_seed"}, argv
        for k, v in old.items():
            assert (list(new[k]) if isinstance(new[k], tuple) else new[k]) == v, (argv, k)
