"""CPU checks of the wide tracker table (cn_config.track_capacity 128 ... 1024): the status bits the Python side knows agree with
the CN_ST_* enum of include/crowdnav.h, and the golden that pins the wide table past 64 tracks does go past 64 tracks."""
import os
import re

import numpy as np

from conftest import GOLDEN, ROOT


def _header_status_bits():
    src = open(os.path.join(ROOT, "include", "crowdnav.h")).read()
    m = re.search(r"enum\s*\{([^}]*CN_ST_TRACK_OVERFLOW[^}]*)\}", src)
    assert m, "CN_ST_* enum not found"
    return {k: int(v) for k, v in re.findall(r"CN_ST_(\w+)\s*=\s*(\d+)", m.group(1))}


def test_status_bits_match_the_header():
    from crowdnav import _abi
    from crowdnav.env import VecEnv
    hdr = _header_status_bits()
    assert hdr["TRACK_WIDE"] == 16
    assert {k.upper(): v for k, v in _abi.STATUS_BITS.items()} == hdr
    assert VecEnv.STATUS_BITS == _abi.STATUS_BITS
    # the keys status_counts() reported before the wide table, with the same bits
    for k, v in {"track_overflow": 1, "ttc_zero": 2, "dt_zero": 4, "conf_overflow": 8}.items():
        assert VecEnv.STATUS_BITS[k] == v


def test_track_capacities_match_the_header():
    from crowdnav import _abi
    src = open(os.path.join(ROOT, "include", "crowdnav.h")).read()
    assert int(re.search(r"#define CN_MAX_TRACKS_WIDE (\d+)", src).group(1)) == _abi.CN_MAX_TRACKS_WIDE == max(_abi.TRACK_CAPACITIES)


def test_wide_golden_goes_past_64_tracks():
    z = np.load(os.path.join(GOLDEN, "seq_wide_tracks.npz"))
    nt = z["n_tracks"]
    assert nt.max() > 64 and nt.max() < 256
    C = len(nt)
    for k in ("obs", "ranges", "reward", "done", "counters", "collision_prob", "ego_score", "wp", "bb", "status"):
        assert len(z[k]) == C, k
    assert z["track_pose"].shape == (C, nt.max(), 2) and z["track_vel"].shape == (C, nt.max(), 2)
    # padding beyond each call's live tracks is zero
    for i in range(C):
        assert not z["track_dist"][i, nt[i]:].any()
