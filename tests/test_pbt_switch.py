"""crowdnav.train's --pbt-* switches (population-based training): off by default, the accepted forms, every refusal, and n_replace from
the fraction (no GPU: only the command line and the keyed spread)."""
import math

import pytest

BASE = ["--algo", "td3", "--learner", "fused"]
POP = BASE + ["--population", "8"]


def _parse(argv):
    from crowdnav import train
    return train.parse_args(argv)


def test_pbt_is_off_by_default():
    for argv in ([], BASE, POP):
        a = _parse(argv)
        assert a.pbt_every == 0 and a.pbt_spread == 0 and a.pbt_n_replace == 0
        assert a.pbt_fraction == 0.25 and a.pbt_factor == (0.8, 1.2) and a.pbt_explore == ("lr_actor", "lr_critic", "noise_std")
        assert a.pbt_min_episodes == 10


def test_accepted_forms():
    a = _parse(POP + ["--pbt-every", "200"])
    assert a.pbt_every == 200 and a.pbt_n_replace == 2 and a.population == 8
    a = _parse(POP + ["--pbt-every", "50", "--pbt-fraction", "0.5", "--pbt-factor", "0.5", "2", "--pbt-explore", "gamma,noise_clip",
                      "--pbt-min-episodes", "1", "--pbt-spread", "3"])
    assert (a.pbt_every, a.pbt_n_replace, a.pbt_factor, a.pbt_explore, a.pbt_min_episodes, a.pbt_spread) == (50, 4, (0.5, 2.0), ("gamma", "noise_clip"), 1, 3.0)
    a = _parse(POP + ["--pbt-spread", "2"])                    # a sweep without exploit
    assert a.pbt_every == 0 and a.pbt_spread == 2.0 and a.pbt_n_replace == 0
    a = _parse(POP + ["--pbt-every", "0"])                     # off, said out loud
    assert a.pbt_every == 0 and a.pbt_n_replace == 0
    a = _parse(BASE + ["--population", "1", "--pbt-spread", "2"])
    assert a.population == 1 and a.pbt_spread == 2.0
    assert _parse(POP + ["--pbt-every", "10", "--pbt-explore", ""]).pbt_explore == ()          # exploit only


@pytest.mark.parametrize("P,fraction,n", [(2, 0.25, 1), (2, 0.5, 1), (5, 0.25, 1), (5, 0.4, 2), (5, 0.5, 2), (64, 0.25, 16), (64, 0.5, 32),
                                          (64, 0.0, 1), (3, 0.25, 1)])
def test_n_replace_from_the_fraction(P, fraction, n):
    a = _parse(BASE + ["--population", str(P), "--pbt-every", "10", "--pbt-fraction", str(fraction)])
    assert a.pbt_n_replace == n == max(1, math.floor(P * fraction)) and n <= P // 2


@pytest.mark.parametrize("argv,text", [
    (["--pbt-every", "10"], "--population"),                                                 # every switch, without a population
    (BASE + ["--pbt-every", "0"], "--population"),
    (BASE + ["--pbt-fraction", "0.25"], "--population"),
    (BASE + ["--pbt-factor", "0.8", "1.2"], "--population"),
    (BASE + ["--pbt-explore", "gamma"], "--population"),
    (BASE + ["--pbt-min-episodes", "5"], "--population"),
    (BASE + ["--pbt-spread", "3"], "--population"),
    (BASE + ["--population", "1", "--pbt-every", "10"], "--population >= 2"),
    (BASE + ["--population", "5", "--pbt-every", "10", "--pbt-fraction", "0.6"], "at most half"),
    (BASE + ["--population", "2", "--pbt-every", "10", "--pbt-fraction", "1"], "at most half"),
    (BASE + ["--population", "64", "--pbt-every", "10", "--pbt-fraction", "0.52"], "at most half"),
    (POP + ["--pbt-every", "10", "--pbt-explore", "lr_actor,beta1"], "beta1"),
    (POP + ["--pbt-every", "-1"], ">= 0"),
    (POP + ["--pbt-every", "10", "--pbt-factor", "0", "1.2"], "> 0"),
    (POP + ["--pbt-every", "10", "--pbt-factor", "0.8", "inf"], "finite"),
    (POP + ["--pbt-every", "10", "--pbt-min-episodes", "0"], ">= 1"),
    (POP + ["--pbt-spread", "-2"], ">= 0"),
    (POP + ["--pbt-every", "10", "--pbt-fraction", "1.5"], "0 ... 1"),
])
def test_pbt_refusals(argv, text, capsys):
    with pytest.raises(SystemExit) as ex:
        _parse(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "--pbt-" in err and text in err, err


def test_what_a_population_refuses_stays_refused_with_pbt(capsys):
    for argv, text in ((["--population", "4", "--pbt-every", "10"], "--learner fused"),
                       (BASE + ["--population", "4", "--pbt-every", "10", "--load", "runs/td3"], "--load"),
                       (["--learner", "fused", "--algo", "ddpg", "--population", "4", "--pbt-every", "10"], "--algo td3")):
        with pytest.raises(SystemExit):
            _parse(argv)
        assert text in capsys.readouterr().err


def test_spread_is_keyed_log_uniform():
    from crowdnav import train
    f = [train.pbt_spread_factors(7, p, 3.0) for p in range(64)]
    assert f == [train.pbt_spread_factors(7, p, 3.0) for p in range(64)] and len(f[0]) == 3
    flat = [x for row in f for x in row]
    assert all(1 / 3.0 <= x <= 3.0 for x in flat) and len(set(flat)) == len(flat)
    assert min(flat) < 0.5 and max(flat) > 2.0 and 64 < sum(x < 1 for x in flat) < 128       # both halves of the log range
    assert train.pbt_spread_factors(8, 0, 3.0) != f[0]
    assert train.pbt_spread_factors(7, 5, 1.0) == [1.0, 1.0, 1.0]
    assert train.PBT_CSV_COLUMNS == ("launch", "call", "member", "src", "generation", "fitness", "lr_actor", "lr_critic", "gamma", "noise_std", "noise_clip")
