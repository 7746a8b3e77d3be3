"""crowdnav._abi's snapshot helpers against the blob include/crowdnav.h describes, on blobs made up on the host (no library, no GPU):
    cn_snapshot_header | sd [N][sd_count] f64 | si [N][si_count] i32 | ped_p [N][P][2] f64 | ped_v [N][P][2] f64
    | trk [N][track_capacity][tf_count] f64 | ped_init [N][P][2] f64 | ped_preset [N][P][2] f64 | ped_aux [N][P][3] f64
The offsets below are worked out from that comment, not from SNAPSHOT_SECTIONS."""
import ctypes as C

import numpy as np
import pytest

from crowdnav import _abi

N, CAP = 3, 32
HDR = C.sizeof(_abi.CnSnapshotHeader)


def layout(P):
    """[(name, dtype, shape, byte offset)] and the blob's size."""
    secs = [("sd", np.float64, (N, _abi.CN_SD_COUNT)), ("si", np.int32, (N, _abi.CN_SI_COUNT)), ("ped_p", np.float64, (N, P, 2)),
            ("ped_v", np.float64, (N, P, 2)), ("trk", np.float64, (N, CAP, _abi.CN_TF_COUNT)), ("ped_init", np.float64, (N, P, 2)),
            ("ped_preset", np.float64, (N, P, 2)), ("ped_aux", np.float64, (N, P, 3))]
    out, off = [], HDR
    for name, dt, shape in secs:
        out.append((name, dt, shape, off))
        off += int(np.prod(shape)) * np.dtype(dt).itemsize
    return out, off


def blob(P, seed=0):
    _, total = layout(P)
    hd = _abi.CnSnapshotHeader(magic=_abi.CN_SNAPSHOT_MAGIC, abi_version=_abi.EXPECTED_ABI, header_bytes=HDR, sd_count=_abi.CN_SD_COUNT,
                               si_count=_abi.CN_SI_COUNT, tf_count=_abi.CN_TF_COUNT, track_capacity=CAP, total_bytes=total)
    hd.config.n_envs, hd.config.n_peds = N, P
    b = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
    b[:HDR] = np.frombuffer(bytes(hd), dtype=np.uint8)
    return b


def test_the_section_list_is_the_headers_order():
    assert [s[0] for s in _abi.SNAPSHOT_SECTIONS] == ["sd", "si", "ped_p", "ped_v", "trk", "ped_init", "ped_preset", "ped_aux"]


@pytest.mark.parametrize("P", [2, 0])
def test_split_returns_views_at_the_documented_offsets_and_join_inverts_it(P):
    b = blob(P)
    hd, arrs = _abi.split_snapshot(b)
    want, total = layout(P)
    assert (hd.total_bytes, b.size) == (total, total) and list(arrs) == [w[0] for w in want]
    base = b.__array_interface__["data"][0]
    for name, dt, shape, off in want:
        a = arrs[name]
        assert a.shape == shape and a.dtype == dt, name
        assert np.shares_memory(a, b) and a.__array_interface__["data"][0] - base == off or a.size == 0, name
        assert a.tobytes() == b[off:off + a.nbytes].tobytes(), name
    back = _abi.join_snapshot(hd, arrs)
    assert back.dtype == np.uint8 and back.tobytes() == b.tobytes()
    # the arrays are authoritative when they are joined again (tools/bisect_divergence.py edits them)
    edited = dict(arrs, sd=np.full(arrs["sd"].shape, 1.5))
    assert np.array_equal(_abi.split_snapshot(_abi.join_snapshot(hd, edited))[1]["sd"], edited["sd"])


@pytest.mark.parametrize("P", [2, 0])
def test_split_refuses_what_is_not_a_whole_snapshot(P):
    b = blob(P)
    for bad in (b[:-1], b[:b.size // 2], b[:HDR], b[:HDR - 1]):           # truncated, down to less than a header
        with pytest.raises(_abi.CrowdNavError):
            _abi.split_snapshot(bad)
    bad = b.copy(); bad[0] ^= 0xFF                                          # the magic
    with pytest.raises(_abi.CrowdNavError):
        _abi.split_snapshot(bad)
    bad = b.copy(); bad[12] ^= 0x10                                         # header_bytes (after magic u64, abi_version i32)
    with pytest.raises(_abi.CrowdNavError):
        _abi.split_snapshot(bad)
