"""crowdnav.train's --n-step without a GPU: the default, the accepted forms, every refusal (each names the switch), and that the
switch stays beside vars() like the other late switches."""
import pytest

TD3 = ["--algo", "td3", "--learner", "fused"]
SMALL = ["--envs", "4", "--memory", "64"]


def test_default_is_one_step():
    from crowdnav import train
    for argv in ([], TD3, TD3 + ["--population", "2"], ["--algo", "ddpg"], ["--algo", "qlearn"]):
        a = train.parse_args(argv)
        assert a.n_step == 1 and "n_step" not in vars(a)
    assert train.parse_args(TD3 + ["--n-step", "1"]).n_step == 1
    for algo in ("ddpg", "sac", "dqn"):                        # the default given by name changes nothing for anybody
        assert train.parse_args(["--algo", algo, "--n-step", "1"]).n_step == 1


@pytest.mark.parametrize("argv", [
    ["--algo", "td3", "--n-step", "3"],                                                           # solo, the PyTorch update
    TD3 + ["--n-step", "3"],                                                                      # solo, the fused update
    TD3 + ["--n-step", "16"] + SMALL,                                                             # the widest window, a ring of exactly n W rows
    TD3 + ["--n-step", "3", "--reset-mode", "next"],
    TD3 + ["--n-step", "3", "--population", "2"],
    TD3 + ["--n-step", "5", "--population", "2", "--population-record", "one-call", "--population-replay", "shared"],
    TD3 + ["--n-step", "3", "--population", "4", "--pbt-every", "20"],                            # the default explore set has no gamma
    TD3 + ["--n-step", "3", "--population", "4", "--pbt-every", "20", "--pbt-explore", "lr_actor,noise_clip"],
    TD3 + ["--n-step", "3", "--state-every", "10"],
], ids=lambda v: " ".join(v[2:]))
def test_accepted_forms(argv):
    from crowdnav import train
    a = train.parse_args(argv)
    assert a.n_step == int(argv[argv.index("--n-step") + 1]) and "n_step" not in vars(a)


@pytest.mark.parametrize("argv,text", [
    (["--algo", "ddpg", "--n-step", "3"], "--algo td3"),
    (["--algo", "sac", "--n-step", "3"], "--algo td3"),
    (["--algo", "dqn", "--n-step", "3"], "--algo td3"),
    (["--algo", "qlearn", "--n-step", "3"], "--algo td3"),
    (TD3 + ["--n-step", "3", "--reset-mode", "same"], "--reset-mode next"),
    (TD3 + ["--n-step", "3", "--population", "2", "--population-record", "per-member"], "--population-record one-call"),
    (TD3 + ["--n-step", "3", "--population", "4", "--pbt-every", "20", "--pbt-explore", "lr_actor,gamma"], "gamma in --pbt-explore"),
    (TD3 + ["--n-step", "3", "--population", "4", "--pbt-every", "20", "--pbt-explore", "gamma"], "gamma in --pbt-explore"),
    (TD3 + ["--n-step", "0"], "1 ... 16"),
    (TD3 + ["--n-step", "-2"], "1 ... 16"),
    (TD3 + ["--n-step", "17"], "1 ... 16"),
    (TD3 + ["--n-step", "3", "--envs", "32", "--memory", "64"], "--memory"),
    (TD3 + ["--n-step", "three"], "invalid int value"),
], ids=lambda v: " ".join(v[2:]) if isinstance(v, list) else None)
def test_refusals_name_the_switch(argv, text, capsys):
    from crowdnav import train
    with pytest.raises(SystemExit) as ex:
        train.parse_args(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "--n-step" in err and text in err, err


def test_members_and_hand_built_namespaces():
    """A Namespace built by hand has no n_step and means 1; fill_defaults leaves one that was set."""
    import argparse
    from crowdnav import train
    a = train.fill_defaults(argparse.Namespace(algo="td3"))
    assert getattr(a, "n_step", 1) == 1
    a = train.fill_defaults(argparse.Namespace(algo="td3", n_step=3))
    assert a.n_step == 3


def test_agent_keeps_gamma_and_bootstraps_with_the_recorders_power():
    import numpy as np
    from crowdnav import td3
    from learner_handle import lib
    _, L = lib()
    one = td3.Agent(obs_dim=5, device="cpu", memory_size=8)
    assert one.n_step == 1 and one.bootstrap_gamma is one.gamma                  # today's expression, the same object
    three = td3.Agent(obs_dim=5, device="cpu", memory_size=8, n_step=3, gamma=0.99)
    assert three.gamma == 0.99 and three.n_step == 3
    assert np.float32(three.bootstrap_gamma) == np.float32(L.cn_nstep_discount(0.99, 3)) != np.float32(0.99)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="n_step"):
            td3.Agent(obs_dim=5, device="cpu", memory_size=8, n_step=bad)
