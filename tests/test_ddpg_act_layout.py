"""cn_ddpg_act (include/crowdnav.h; csrc/crowdnav_ddpg.hip) without a GPU: cn_ddpg_act_io against its ctypes mirror as gcc lays it
out, the export, every refusal (the argument checks come before any device work, so they answer on a machine that has no GPU), and
crowdnav.train's --ou-act switch."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from learner_handle import lib

CN_ERR_ARG, CN_ERR_CONFIG = -1, -2
FAKE = 0x1000        # a non-null "device pointer": the checks compare with NULL and never dereference
FIELDS = ["obs", "state", "reset", "u", "action", "noise_out", "mu", "theta", "sigma", "seed", "counter", "max_v", "max_w", "n", "add_noise"]


def test_io_struct_matches_its_mirror_field_by_field(tmp_path):
    _abi, _ = lib()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _abi.CnDdpgActIO
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(cn_ddpg_act_io));', 'printf("abi %d\\n", CN_ABI_VERSION);',
             'printf("config %zu\\n", sizeof(cn_ddpg_config));']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(cn_ddpg_act_io, %s));' % (f[0], f[0]))
    lines += ["{ int (*f)(const cn_actor_weights*, const cn_ddpg_act_io*, int, void*) = cn_ddpg_act; (void)f; }", "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    obj = tmp_path / "layout.o"
    subprocess.run(["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"),
                    "-o", str(obj), str(src)], check=True)
    stubs = tmp_path / "stubs.c"             # the function's address is only taken: resolve it with a stub of the same name
    stubs.write_text("void cn_ddpg_act(void) {}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(obj), str(stubs)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls) == 104
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]
    assert [f[0] for f in cls._fields_] == FIELDS
    assert int(got["abi"]) == _abi.EXPECTED_ABI == 7              # additive: the version stays
    assert int(got["config"]) == C.sizeof(_abi.CnDdpgConfig)      # and so does cn_ddpg_config


def test_the_name_is_exported_with_its_prototype():
    _abi, L = lib()
    assert "cn_ddpg_act" in _abi.EXPORTS and hasattr(C.CDLL(_abi.LIB_PATH), "cn_ddpg_act")
    assert L.cn_ddpg_act.argtypes[0] is C.POINTER(_abi.CnActorWeights) and L.cn_ddpg_act.argtypes[1] is C.POINTER(_abi.CnDdpgActIO)


def _weights(_abi, **kw):
    f = dict(w1p=FAKE, b1=FAKE, w2p=FAKE, b2=FAKE, w3=FAKE, b3=FAKE, obs_dim=363, obs_dim_padded=384, hidden=256, reserved=0)
    f.update(kw)
    return _abi.CnActorWeights(**f)


def _io(_abi, **kw):
    f = dict(obs=FAKE, state=FAKE, reset=FAKE, u=FAKE, action=FAKE, noise_out=FAKE, mu=0.0, theta=0.15, sigma=0.2, seed=1, counter=1,
             max_v=0.22, max_w=2.0, n=16, add_noise=1)
    f.update(kw)
    return _abi.CnDdpgActIO(**f)


def _refused(L, w, io, want_rc, *texts):
    rc = L.cn_ddpg_act(None if w is None else C.byref(w), None if io is None else C.byref(io), 0, None)
    msg = L.cn_last_error().decode()
    assert rc == want_rc, (rc, msg)
    assert "cn_ddpg_act" in msg
    for t in texts:
        assert t in msg, (t, msg)


def test_refusals_come_before_any_device_work_and_name_the_field():
    _abi, L = lib()
    w, io = _weights(_abi), _io(_abi)
    _refused(L, None, io, CN_ERR_ARG, "actor")
    _refused(L, w, None, CN_ERR_ARG, "io")
    for field in ("w1p", "b1", "w2p", "b2", "w3", "b3"):
        _refused(L, _weights(_abi, **{field: None}), io, CN_ERR_ARG, "actor->" + field)
    _refused(L, w, _io(_abi, obs=None), CN_ERR_ARG, "obs")
    _refused(L, w, _io(_abi, action=None), CN_ERR_ARG, "action")
    _refused(L, w, _io(_abi, state=None), CN_ERR_ARG, "state", "add_noise")
    for n in (-1, -(1 << 31)):
        _refused(L, w, _io(_abi, n=n), CN_ERR_ARG, "n is negative")
    for hidden in (0, 128, 255, 257, 512):
        _refused(L, _weights(_abi, hidden=hidden), io, CN_ERR_CONFIG, "hidden", "256")
    for D in (0, -1, -363):
        _refused(L, _weights(_abi, obs_dim=D, obs_dim_padded=32), io, CN_ERR_CONFIG, "obs_dim")
    for D, Dp in ((363, 352), (363, 383), (33, 32)):
        _refused(L, _weights(_abi, obs_dim=D, obs_dim_padded=Dp), io, CN_ERR_CONFIG, "obs_dim_padded", "multiple of 32")
    for D in (2273, 2304, 4000):          # Dp 2304 is the first tile above 160 KiB, as cn_actor_forward refuses
        _refused(L, _weights(_abi, obs_dim=D, obs_dim_padded=(D + 31) // 32 * 32), io, CN_ERR_CONFIG, "obs_dim", "too wide")
    # the argument checks win over the configuration's, and every check over n == 0
    _refused(L, _weights(_abi, hidden=128), _io(_abi, obs=None), CN_ERR_ARG, "obs")
    _refused(L, _weights(_abi, hidden=128), _io(_abi, n=0), CN_ERR_CONFIG, "hidden")


def test_zero_rows_and_the_deterministic_policys_null_state_are_accepted():
    """n == 0 launches nothing and returns 0 (no device is touched); add_noise = 0 does not need a state (with n = 0 here: the
    acceptance is what can be seen without a GPU)."""
    _abi, L = lib()
    w = _weights(_abi)
    assert L.cn_ddpg_act(C.byref(w), C.byref(_io(_abi, n=0)), 0, None) == 0
    assert L.cn_ddpg_act(C.byref(w), C.byref(_io(_abi, n=0, add_noise=0, state=None, reset=None, u=None, noise_out=None)), 0, None) == 0
    # the widest tile that fits: Dp 2272
    assert L.cn_ddpg_act(C.byref(_weights(_abi, obs_dim=2272, obs_dim_padded=2272)), C.byref(_io(_abi, n=0)), 0, None) == 0


def test_ou_act_flag():
    from crowdnav import train
    assert train.parse_args([]).ou_act == "torch"
    assert train.parse_args(["--algo", "ddpg", "--ou-noise"]).ou_act == "torch"
    a = train.parse_args(["--algo", "ddpg", "--ou-noise", "--ou-act", "fused"])
    assert a.ou_act == "fused" and a.ou_noise and a.algo == "ddpg"
    assert train.parse_args(["--algo", "ddpg", "--ou-noise", "--ou-act", "torch"]).ou_act == "torch"


@pytest.mark.parametrize("argv", [["--algo", "ddpg", "--ou-act", "fused"], ["--algo", "ddpg", "--ou-act", "torch"], ["--ou-act", "fused"]])
def test_ou_act_is_refused_without_ou_noise(argv, capsys):
    from crowdnav import train
    with pytest.raises(SystemExit):
        train.parse_args(argv)
    msg = capsys.readouterr().err
    assert "--ou-act" in msg and "--ou-noise" in msg


def test_fill_defaults_picks_the_flag_up():
    import argparse
    from crowdnav import train
    a = train.fill_defaults(argparse.Namespace(algo="ddpg", ou_noise=True))
    assert a.ou_act == "torch" and a.ou_noise is True
    assert train.fill_defaults(argparse.Namespace(algo="ddpg", ou_noise=True, ou_act="fused")).ou_act == "fused"
