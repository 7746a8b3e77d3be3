"""cn_sac_act (sac_act_kernel in csrc/crowdnav_sac.hip) held to the float64 statement of tests/sac_f64.py (act_pass: run()'s own
head, clamp, sample and squash statements) around every tile edge of the kernel: the 16-unit tile and the 32-unit padding of
hidden, the four head lanes, the ragged block of 16 inputs, eight blocks in flight, the 16-row workgroup, the LDS limit and a grid
of more than 4096 workgroups.  Raw calls through crowdnav._abi.CnSacActIO.  Every bound is td3_f64.propagated_bounds' (float32
unit roundoff through the signed Jacobians, times LAMBDA); the clamp, the deterministic path, the padding, the optional outputs,
the rows past n and the on-device draw are compared bit for bit or against the documented hash.  No comparison leaves a row out:
sac_f64.act_case gives every row margins.  `-s` prints the worst |got - float64| / bound of every output."""
import ctypes as C

import numpy as np
import pytest
import torch

import sac_f64 as S
import td3_f64 as R
from learner_handle import lib, stream
from sac_f64 import SCALE_ERR

pytestmark = pytest.mark.gpu

DEV = "cuda"
CN_ERR_CONFIG = -2
SENTINEL = -12345.678          # what every output buffer holds before a call; 16 spare rows of it follow the n rows
SPARE = 16
OUTS = ("mean", "log_std", "z")
c = S.CFG


def _dev(pa):
    return {k: v.detach().float().to(DEV).contiguous() for k, v in pa.items()}


def _act(pd, obs, D, H, n, eps=None, det=False, seed=1, counter=0, outs=OUTS, expect=0, **over):
    """One cn_sac_act on device tensors -> {twist, mean, log_std, z} (the first n rows of each buffer asked for).  The SPARE rows
    behind them must keep every bit; with expect != 0 the call must be refused with that code and ALL rows keep every bit."""
    _abi, L = lib()
    buf = {k: torch.full((n + SPARE, 2), SENTINEL, device=DEV) for k in ("twist",) + tuple(outs)}
    ptr = lambda k: buf[k].data_ptr() if k in buf else None
    kw = dict(obs=obs.data_ptr(), obs_ld=obs.stride(0), n=n, obs_dim=D, hidden=H, deterministic=int(det),
              actor=_abi.CnSacActor(*[pd[k].data_ptr() for k in S.ACTOR_NAMES]), max_v=c["max_v"], max_w=c["max_w"],
              log_std_min=c["ls_min"], log_std_max=c["ls_max"], eps=eps.data_ptr() if eps is not None else None, seed=seed, counter=counter,
              twist=ptr("twist"), mean=ptr("mean"), log_std=ptr("log_std"), z=ptr("z"))
    kw.update(over)
    rc = L.cn_sac_act(C.byref(_abi.CnSacActIO(**kw)), 0, stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.cn_td3_last_error())
    keep = 0 if expect else n
    for k, b in buf.items():
        assert bool((b[keep:] == SENTINEL).all()), ("rows past n were written" if not expect else "a refused call wrote", k, H, D, n)
    return {k: b[:n] for k, b in buf.items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _ratios(got, want, bound):
    return {k: R.worst_ratio(got[k].cpu(), want[k], bound[k]) for k in S.ACT_KEYS}


def _check(H, D, n, worst):
    """Everything the float64 test asserts for one (hidden, D, n); the worst ratios are folded into `worst`."""
    pa, obs, eps = S.act_case(H, D, D, n)
    pd, e_d = _dev(pa), eps.to(DEV).contiguous()
    x = {ld: S.act_case(H, D, ld, n)[1].to(DEV).contiguous() for ld in (D, D + 3)}
    assert bool(torch.isnan(x[D + 3][:, D:]).all())
    ref = DEV if n > 4096 else "cpu"                    # the float64 passes: a few dozen rows are quicker on the host
    p64, x64, e64 = {k: v.double().to(ref) for k, v in pa.items()}, obs.double().to(ref), eps.double().to(ref)
    below, inside, above = S.act_classes(pa, obs)
    if S.act_promises_classes(H, n):
        assert bool(below.any()) and bool(inside.any()) and bool(above.any())
    for det in (False, True):
        tag = (H, D, n, "deterministic" if det else "sampled")
        got = _act(pd, x[D], D, H, n, eps=e_d, det=det)
        assert _same(got, _act(pd, x[D + 3], D, H, n, eps=e_d, det=det)), ("padding columns were read", tag)
        assert torch.equal(got["twist"], _act(pd, x[D], D, H, n, eps=e_d, det=det, outs=())["twist"]), ("mean = log_std = z = NULL", tag)
        if det:
            assert torch.equal(got["z"], got["mean"]), tag
            assert _same(got, _act(pd, x[D], D, H, n, eps=None, det=True)), ("eps changed a deterministic call", tag)
        want, bound = S.act_reference(p64, x64, e64, det)
        ratios = _ratios(got, {k: v.cpu() for k, v in want.items()}, {k: v.cpu() for k, v in bound.items()})
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(ratios.values()) <= 1.0, (tag, ratios)
        ls = got["log_std"].cpu()
        assert bool((ls[below] == c["ls_min"]).all()) and bool((ls[above] == c["ls_max"]).all()), tag
        assert bool(((ls[inside] > c["ls_min"]) & (ls[inside] < c["ls_max"])).all()), tag
        tw = got["twist"].cpu()
        assert all(bool(torch.isfinite(v).all()) for v in got.values()), tag
        assert bool((tw[:, 0] >= 0).all()) and bool((tw[:, 0] <= c["max_v"]).all()) and bool((tw[:, 1].abs() <= c["max_w"]).all()), tag
    return 2 * n


@pytest.mark.parametrize("H", S.ACT_HIDDEN)
def test_act_outputs_within_the_float64_bound_at_every_tile_edge(H):
    """Every (hidden, D, n) of ACT_HIDDEN x ACT_D x ACT_N, sampled with supplied eps and deterministic, EVERY row: mean, log_std,
    z and twist within act_reference's propagated bound; log_std exactly -20.0 or 2.0 on every element float64 clamps and
    strictly between on every other; 0 <= v <= max_v, |w| <= max_w, all finite.  ld = D and ld = D + 3 with NaN in the padding
    give the same bits; so does mean = log_std = z = NULL for the twist; every buffer's 16 spare rows keep their sentinel;
    deterministic: z is mean bit for bit and a supplied eps changes nothing.

    Not tested, because it cannot be: the clip.  sigmoid(t) lies in (0, 1) and |tanh(t)| <= 1, so max_v sigmoid and max_w tanh
    never leave [0, max_v] x [-max_w, max_w] and the clip changes no value; only the range is asserted."""
    worst, rows = {}, 0
    for D in S.ACT_D:
        for n in S.ACT_N:
            rows += _check(H, D, n, worst)
    print("sac act hidden %d: worst |got - float64| / bound %s over %d rows (sampled + deterministic) x 2 strides" % (
        H, " ".join("%s %.3g" % kv for kv in worst.items()), rows))


def test_act_on_a_grid_beyond_4096_workgroups_with_a_ragged_last_one():
    """n = 65541 at hidden 32, D 17: 4097 workgroups, the last with five rows (the i0 + li clamp of the obs row): the same
    assertions on every row."""
    worst = {}
    H, D, n = S.ACT_LARGE
    _check(H, D, n, worst)
    print("sac act hidden %d D %d n %d: worst |got - float64| / bound %s" % (H, D, n, " ".join("%s %.3g" % kv for kv in worst.items())))


def test_saturated_tanh_stays_finite_and_gives_the_squash_of_one():
    """Past sac_f64.tame_eps' |eps| std <= Z_STEP_MAX: (a) a mean head whose output has both signs and a median |mean| of 50, (b) eps = +-5 on the
    elements clamped at log_std 2 (std = e^2: |z - mean| = 36.9), in either column.  Everything stays finite and within act_reference's
    bound, and where float64 has |tanh z| = 1 to 2^-53 the twist is (max_v sigmoid(+-1), max_w tanh(+-1)) within that bound."""
    H, D, n = 33, 45, 40
    pa, obs, eps = S.act_case(H, D, D, n)
    hot = {k: v.clone() for k, v in pa.items()}
    raw = S.trunk({k: v.double() for k, v in pa.items()}, obs.double())[1]          # (spread over the rows by plant_clamp_head)
    mid = raw.median(0).values
    k50 = 50.0 / (raw - mid).abs().median(0).values                                 # mean := k50 (raw - mid): both signs, median 50
    hot["mean_w"], hot["mean_b"] = (pa["ls_w"].double() * k50[:, None]).float(), ((pa["ls_b"].double() - mid) * k50).float()
    flip = {k: (v[[1, 0]].contiguous() if k in ("ls_w", "ls_b") else v) for k, v in pa.items()}       # the upper edge in the other column
    x_d = obs.to(DEV).contiguous()
    seen = set()
    for tag, p_, det, five in (("mean 50", hot, False, False), ("mean 50, deterministic", hot, True, False), ("eps 5", pa, False, True),
                               ("eps 5, log_std outputs exchanged", flip, False, True)):
        above = S.act_classes(p_, obs)[2]
        e_ = eps
        if five:                                                   # both signs among the elements clamped at 2
            e_ = torch.full((n, 2), 5.0)
            for j in (0, 1):
                e_[above[:, j].nonzero().reshape(-1)[::2], j] = -5.0
        got = _act(_dev(p_), x_d, D, H, n, eps=e_.to(DEV).contiguous(), det=det)
        want, bound = S.act_reference({k: v.double() for k, v in p_.items()}, obs.double(), e_.double(), det)
        assert all(bool(torch.isfinite(v).all()) for v in got.values()), tag
        ratios = _ratios(got, want, bound)
        t = torch.tanh(want["z"])
        sat = t.abs() == 1.0                                       # float64's tanh is 1 to 2^-53: |z| > 19.06
        sign = t.sign()
        if five:
            assert bool(above.any()) and bool(sat[above].all()), tag
            seen |= {(j, s_) for j in (0, 1) for s_ in (-1.0, 1.0) if bool((above[:, j] & (sign[:, j] == s_)).any())}
        else:
            assert all(bool((sat[:, j] & (sign[:, j] == s_)).any()) for j in (0, 1) for s_ in (-1.0, 1.0)), (tag, "a saturation class is missing")
        one = torch.stack([c["max_v"] * torch.sigmoid(sign[:, 0]), c["max_w"] * torch.tanh(sign[:, 1])], 1)
        r_one = R.worst_ratio(got["twist"].cpu()[sat], one[sat], bound["twist"][sat])
        print("sac act saturation, %s: %d of %d elements saturated; worst / bound %s; against the squash of +-1 %.3g" % (
            tag, int(sat.sum()), 2 * n, " ".join("%s %.3g" % kv for kv in ratios.items()), r_one))
        assert max(ratios.values()) <= 1.0 and r_one <= 1.0, (tag, ratios, r_one)
    assert len(seen) == 4, ("clamped at 2 with eps = +-5: a (column, sign) class is missing", seen)


@pytest.mark.parametrize("shape", S.ACT_DISCRIMINATE, ids=lambda s: "x".join(map(str, s)))
def test_wrong_act_variants_scalings_and_a_rotated_block_are_rejected(shape):
    """The acceptance rule of the float64 test (worst ratio <= 1 against act_reference) accepts the kernel and rejects: every
    ACT_VARIANTS restatement (against ITS reference and bounds); each of mean, log_std (its unclamped elements), z, twist[:, 0]
    and twist[:, 1] scaled by 1 + SCALE_ERR; the rows of the first 16-row block rotated by one."""
    H, D, n = shape
    pa, obs, eps = S.act_case(H, D, D, n)
    p64, x64, e64 = {k: v.double() for k, v in pa.items()}, obs.double(), eps.double()
    got = {k: v.cpu() for k, v in _act(_dev(pa), obs.to(DEV).contiguous(), D, H, n, eps=eps.to(DEV).contiguous()).items()}
    want, Bd = S.act_reference(p64, x64, e64, False)
    assert max(_ratios(got, want, Bd).values()) <= 1.0
    for var in S.ACT_VARIANTS:
        wrong, wb = S.act_reference(p64, x64, e64, False, variant=var)
        worst = max(_ratios(got, wrong, wb).values())
        print(shape, var, "%.3g" % worst)
        assert worst > 1.0, (var, "accepted", worst)
    inside = S.act_classes(pa, obs)[1]
    scaled = {"mean": (got["mean"], want["mean"], Bd["mean"]), "z": (got["z"], want["z"], Bd["z"]),
              "log_std": (got["log_std"][inside], want["log_std"][inside], Bd["log_std"][inside]),
              "twist[:, 0]": (got["twist"][:, 0], want["twist"][:, 0], Bd["twist"][:, 0]),
              "twist[:, 1]": (got["twist"][:, 1], want["twist"][:, 1], Bd["twist"][:, 1])}
    for k, (g_, w_, b_) in scaled.items():
        r = R.worst_ratio(g_, w_ * (1 + SCALE_ERR), b_)
        print(shape, k, "x (1 + %g): %.3g" % (SCALE_ERR, r))
        assert r > 1.0, (k, "scaled by 1 + 1e-3 was accepted", r)
    rot = lambda v: torch.cat([v[:16].roll(1, 0), v[16:]], 0)
    r = max(_ratios(got, {k: rot(v) for k, v in want.items()}, {k: rot(v) for k, v in Bd.items()}).values())
    print(shape, "first block rotated by one row: %.3g" % r)
    assert r > 1.0, ("a rotated block was accepted", r)


DRAW_N = 4099


@pytest.mark.parametrize("seed", [7, 0xD1B54A32D192ED03], ids=["seed7", "seed_high_bit"])
def test_the_draw_is_the_documented_hash_of_seed_counter_and_row(seed):
    """Both heads zeroed (weights and biases): mean = 0, std = expf(0) = 1 and z = eps 1 + 0 = eps exactly.  With eps = NULL EVERY
    row's z of a 4099-row call equals sac_f64.box_muller_draw(seed, counter, row) at rtol 2e-5, atol 2e-6 (the tolerance
    test_replay_path_samples_only_live_rows_and_its_eps_is_the_documented_draw holds this hash to), for counters 0, 1, 2^32 and
    2^63 + 5; no two rows of a call are bit-equal, calls c and c + 1 differ on every row, the same (seed, counter) repeats."""
    H, D, n = 32, 17, DRAW_N
    g = torch.Generator().manual_seed(11)
    pa = S.new_params(D, H, 1, g)["actor"]
    for k in ("mean_w", "mean_b", "ls_w", "ls_b"):
        pa[k].zero_()
    pd, x = _dev(pa), (torch.randn((n, D), generator=g) * 0.5).to(DEV).contiguous()
    rows = np.arange(n)
    zs = {}
    for counter in (0, 1, 1 << 32, (1 << 63) + 5):
        got = _act(pd, x, D, H, n, eps=None, seed=seed, counter=counter)
        assert bool((got["mean"] == 0).all()) and bool((got["log_std"] == 0).all())
        z = got["z"].cpu().numpy()
        zs[counter] = z
        np.testing.assert_allclose(z, S.box_muller_draw(seed, counter, rows), rtol=2e-5, atol=2e-6)
        assert len(np.unique(np.ascontiguousarray(z).view(np.int64))) == n, (counter, "two rows drew the same pair")
        assert torch.equal(_act(pd, x, D, H, n, eps=None, seed=seed, counter=counter)["z"], got["z"]), counter
    assert bool((zs[0] != zs[1]).any(1).all()), "calls c and c + 1 share a row's draw"


def test_the_agents_call_counter_keys_its_draws():
    """Agent.act_fused called k + 1 times: its last call has the bits of a fresh agent after set_noise_state(seed, k) and one
    call, and noise_state() is (seed, k + 1) afterwards."""
    from crowdnav.sac import Agent
    k, n = 3, 37
    obs = (torch.rand((n, 45), generator=torch.Generator().manual_seed(1)) * 3.5).to(DEV)
    a, b = (Agent(obs_dim=45, hidden=33, device="cuda:0", seed=5, memory_size=16) for _ in range(2))
    seed = a.noise_state()[0]
    assert a.noise_state() == (seed, 0) == b.noise_state()
    outs = []
    for _ in range(k + 1):
        z = torch.empty((n, 2), device=DEV)
        outs.append((a.act_fused(obs, z=z).clone(), z))
    b.set_noise_state(seed, k)
    zb = torch.empty((n, 2), device=DEV)
    tb = b.act_fused(obs, z=zb)
    torch.cuda.synchronize()
    assert torch.equal(outs[k][0], tb) and torch.equal(outs[k][1], zb)
    assert all(not torch.equal(outs[j][1], zb) for j in range(k))
    assert a.noise_state() == (seed, k + 1) == b.noise_state()


def test_act_refuses_hidden_481_and_a_reversed_clamp_with_nothing_enqueued():
    _, L = lib()
    g = torch.Generator().manual_seed(3)
    for H, over, text in ((481, {}, b"hidden <= 480"), (32, dict(log_std_min=3.0), b"log_std_min > log_std_max")):
        pd = _dev(S.new_params(16, H, 1, g)["actor"])
        x = torch.zeros((4, 16), device=DEV)
        _act(pd, x, 16, H, 4, eps=None, expect=CN_ERR_CONFIG, **over)                # every row of every output keeps its sentinel
        assert text in L.cn_td3_last_error(), L.cn_td3_last_error()
