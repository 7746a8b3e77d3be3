"""CPU checks of the replay-sample switch: the command line, the names' mapping, and the refusals of the new exports that come before
any device work."""
import ctypes as C

import pytest


def test_replay_sample_names():
    from crowdnav import _abi
    assert _abi.replay_sample_mode("with") == _abi.CN_SAMPLE_WITH_REPLACEMENT == 0
    assert _abi.replay_sample_mode("without") == _abi.CN_SAMPLE_DISTINCT == 1
    for bad in ("distinct", "", None, 1):
        with pytest.raises(ValueError):
            _abi.replay_sample_mode(bad)


def test_train_command_line():
    from crowdnav import train
    for algo in ("td3", "ddpg", "dqn", "sac"):
        assert train.parse_args(["--algo", algo]).replay_sample == "with"
        assert train.parse_args(["--algo", algo, "--learner", "fused", "--replay-sample", "without"]).replay_sample == "without"
    assert train.parse_args(["--algo", "td3", "--graphs", "0", "--replay-sample", "without"]).replay_sample == "without"
    assert train.parse_args(["--algo", "ddpg", "--replay-sample", "without"]).replay_sample == "without"
    for argv in (["--algo", "qlearn", "--replay-sample", "with"], ["--algo", "sarsa", "--replay-sample", "without"],
                 ["--algo", "td3", "--replay-sample", "without"],              # the captured PyTorch update draws with replacement
                 ["--algo", "td3", "--replay-sample", "sometimes"]):
        with pytest.raises(SystemExit):
            train.parse_args(argv)


def test_agents_refuse_other_names_before_touching_a_device():
    from crowdnav import ddpg, dqn, sac, td3
    for mod in (td3, ddpg, dqn, sac):
        with pytest.raises(ValueError):
            mod.Agent(device="cpu", replay_sample="both")


def test_exports_refuse_bad_arguments_without_a_device():
    import crowdnav
    L = crowdnav.lib()
    for fam in ("td3", "ddpg", "dqn", "sac"):
        f = getattr(L, "cn_%s_set_replay_sample" % fam)
        assert f(None, 1) == -1 and b"null handle" in L.cn_td3_last_error()
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)
    for args, text in (((1, 0, 4, None, 1, p), b"null"), ((1, 0, 4, p, 1, None), b"null"), ((1, 0, 0, p, 1, p), b"B < 1"),
                       ((1, 0, 4, p, 2, p), b"mode"), ((1, 0, 4, p, -1, p), b"mode")):
        assert L.cn_replay_sample_indices(*args, 0, None) == -1 and text in L.cn_td3_last_error(), args
