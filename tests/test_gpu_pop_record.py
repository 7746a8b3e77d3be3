"""cn_pop_record (include/crowdnav.h) on the GPU against what it replaces: every case is compared with torch.equal -- no tolerance,
the float64 totals by their bits -- against per-member cn_replay_write + cn_episode_log_add (and, with real environments,
cn_get_counters + cn_get_returns) run on second copies of the same inputs.  The cases and the sentinel-padded buffers come from
tests/pop_record_ref.py, whose NumPy restatement tests/test_pop_record_layout.py holds to the PyTorch formulations on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import pop_record_ref as R
from learner_handle import lib, stream

pytestmark = pytest.mark.gpu

CN_ERR_ARG = -1


def _dev(m):
    """Member m (NumPy, tests/pop_record_ref.py) on the device: every array with its sentinel rows, the three counters as int64."""
    t = {k: torch.from_numpy(np.ascontiguousarray(m[k])).cuda() for k in R.ARRAYS}
    for k in R.SCALARS:
        t[k] = torch.tensor(m[k], dtype=torch.int64, device="cuda")
    return t


def _ring(_abi, t, m):
    return _abi.CnReplayRing(s=t["s"].data_ptr(), a=t["a"].data_ptr(), r=t["r"].data_ptr(), s2=t["s2"].data_ptr(), d=t["d"].data_ptr(),
                             capacity=m["cap"], pos_dev=t["pos"].data_ptr(), size_dev=t["size"].data_ptr(), obs_dim=m["D"], reserved=0)


def _log(_abi, t, m):
    return _abi.CnEpisodeLog(rows=t["rows"].data_ptr(), max_rows=m["max_rows"], n_dev=t["n_log"].data_ptr(), tot_dev=t["tot"].data_ptr())


def _struct(_abi, t, m):
    """An explicit-array member; one without rows gets NULL row pointers, as the header allows."""
    p = (lambda k: t[k].data_ptr()) if m["n"] else (lambda k: None)
    return _abi.CnPopRecordMember(env=None, counters=p("counters"), last_return=p("last_return"), prev=p("prev"), obs=p("obs"),
                                  action=p("action"), reward=p("reward"), done=p("done"), ring=_ring(_abi, t, m), log=_log(_abi, t, m),
                                  n=m["n"], reserved=0)


class Recorder:
    def __init__(self, structs, obs_dim):
        self._abi, self.L = lib()
        self.arr = (self._abi.CnPopRecordMember * len(structs))(*structs)
        self.h = C.c_void_p()
        rc = self.L.cn_pop_record_create(self.arr, len(structs), obs_dim, 0, C.byref(self.h))
        assert rc == 0, self.L.cn_last_error().decode()
        assert self.L.cn_pop_record_members(self.h) == len(structs)

    def flags(self, p):
        n = int(self.arr[p].n)
        ptr = self.L.cn_pop_record_resetting(self.h, p)
        assert ptr
        if n == 0:
            return torch.zeros(0, dtype=torch.uint8, device="cuda")

        class _Arr:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(_Arr(), device="cuda")

    def record(self, launch):
        rc = self.L.cn_pop_record(self.h, float(launch), stream())
        assert rc == 0, self.L.cn_last_error().decode()

    def close(self):
        torch.cuda.synchronize()
        self.L.cn_pop_record_destroy(self.h)
        self.h = None


def _reference(t, m, launch):
    """What the call replaces, for one member, in place on t: cn_replay_write and cn_episode_log_add with keep = !resetting, then
    resetting <- done and prev <- obs."""
    _abi, L = lib()
    n = m["n"]
    if n == 0:
        return
    keep = (t["resetting"][:n] == 0).to(torch.uint8).contiguous()
    slot = torch.zeros(n, dtype=torch.int32, device="cuda")
    ring, log = _ring(_abi, t, m), _log(_abi, t, m)
    vp = lambda x: C.c_void_p(x.data_ptr())
    rc = L.cn_replay_write(C.byref(ring), vp(t["prev"]), vp(t["action"]), vp(t["reward"]), vp(t["obs"]), vp(t["done"]), vp(keep), n, vp(slot),
                           0, stream())
    assert rc == 0, L.cn_td3_last_error().decode()
    rc = L.cn_episode_log_add(C.byref(log), vp(t["done"]), vp(t["counters"]), 14, vp(t["last_return"]), vp(keep), float(launch), n, 0, stream())
    assert rc == 0, L.cn_td3_last_error().decode()
    t["resetting"][:n] = t["done"][:n] != 0
    t["prev"][:n] = t["obs"][:n]


def _equal(got, want, what=""):
    for k in R.ARRAYS + R.SCALARS:
        a, b = got[k], want[k]
        if k == "tot":
            a, b = a.view(torch.int64), b.view(torch.int64)          # bit for bit
        assert torch.equal(a, b), (what, k, (a != b).nonzero()[:4].tolist())


def _run(ms, launches=(7,), mutate=None):
    """Members ms through ONE handle for the given launches, against the per-member kernels on second copies.  The handle's flags are
    written by the caller before the first call and read back after the last.  mutate(t, m, call): new inputs between calls, applied
    to both sides.  Returns (got, want) per member."""
    _abi, _ = lib()
    got, want = [_dev(m) for m in ms], [_dev(m) for m in ms]
    rec = Recorder([_struct(_abi, t, m) for t, m in zip(got, ms)], ms[0]["D"])
    for p, (t, m) in enumerate(zip(got, ms)):
        f = rec.flags(p)
        assert f.shape == (m["n"],) and not f.any()                  # zero at create
        f.copy_(t["resetting"][:m["n"]])
    for c, launch in enumerate(launches):
        rec.record(launch)
        for t, m in zip(want, ms):
            _reference(t, m, launch)
        if mutate is not None and c + 1 < len(launches):
            for side in (got, want):
                for t, m in zip(side, ms):
                    mutate(t, m, c)
    for p, (t, m) in enumerate(zip(got, ms)):
        t["resetting"][:m["n"]] = rec.flags(p)
    torch.cuda.synchronize()
    rec.close()
    for p, (g, w) in enumerate(zip(got, want)):
        _equal(g, w, "member %d" % p)
    return got, want


def _changed(t, m):
    """The call did something: the flags are the done pattern, prev is obs, and sentinels stand."""
    n = m["n"]
    assert torch.equal(t["resetting"][:n], (t["done"][:n] != 0).to(torch.uint8)) and torch.equal(t["prev"][:n], t["obs"][:n])
    assert (t["resetting"][n:] == 9).all() and (t["prev"][n:] == R.SENTINEL).all() and (t["rows"][m["max_rows"]:] == R.SENTINEL).all()
    for k in ("s", "s2", "a", "r", "d"):
        assert (t[k][m["cap"]:] == R.SENTINEL).all(), k


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 2049))
def test_rows_at_the_wave_seam_and_the_tile_every_keep_and_done_pattern(n):
    """One member; the 25 pairs of patterns (all, none, alternating, only the last row, only row 1024) for keep and done.  The ring
    starts two slots before its end, so every write that keeps more than two rows wraps; the log starts with room."""
    rng = np.random.default_rng(n)
    for resetting in R.PATTERNS:
        for done in R.PATTERNS:
            m = R.make_member(rng, n, 3, cap=n + 5, pos=n + 3, size=n // 2, done=done, resetting=resetting)
            want_np = R.record(R.copy_member(m), 7)
            (got,), _ = _run([m])
            _changed(got, m)
            # ... and both equal the restatement
            for k in R.SCALARS:
                assert int(got[k]) == want_np[k], (resetting, done, k)
            for k in R.ARRAYS:
                assert got[k].cpu().numpy().tobytes() == want_np[k].tobytes(), (resetting, done, k)


@pytest.mark.parametrize("D", (1, 255, 256, 257, 398))
def test_observation_widths_around_the_copy_stride(D):
    m = R.make_member(np.random.default_rng(D), 65, D, done="alternating", resetting="last")
    (got,), _ = _run([m])
    _changed(got, m)
    assert int(got["size"]) == 64


@pytest.mark.parametrize("case", [
    dict(n=65, cap=70, pos=68, size=10),                    # the write wraps
    dict(n=65, cap=65, pos=63, size=60),                    # capacity == n: every slot is written once, size saturates
    dict(n=1025, cap=1030, pos=1028, size=1029),            # ... across the tile's carry
    dict(n=17, cap=64, pos=0, size=64),                     # a full ring stays full
], ids=lambda c: "n%d-cap%d" % (c["n"], c["cap"]))
def test_ring_wrap_and_saturation(case):
    m = R.make_member(np.random.default_rng(case["cap"]), D=5, done="alternating", resetting="none", **case)
    (got,), _ = _run([m])
    _changed(got, m)
    assert int(got["pos"]) == (case["pos"] + case["n"]) % case["cap"] and int(got["size"]) == case["cap"]


@pytest.mark.parametrize("case", [
    dict(n=65, max_rows=40, n_log=37, done="all"),          # three rows fit, 62 are dropped, the count goes on
    dict(n=2049, max_rows=2000, n_log=1997, done="alternating"),
    dict(n=17, max_rows=0, n_log=0, done="all"),
    dict(n=17, max_rows=0, n_log=5, done="last"),
], ids=lambda c: "n%d-max%d" % (c["n"], c["max_rows"]))
def test_log_rows_beyond_max_rows_are_dropped_and_counted(case):
    m = R.make_member(np.random.default_rng(case["n"]), D=2, resetting="alternating", **case)
    before = m["rows"].copy()
    (got,), _ = _run([m])
    _changed(got, m)
    finished = int(R.pattern(case["done"], case["n"]).sum())
    assert int(got["n_log"]) == case["n_log"] + finished
    assert np.array_equal(got["rows"].cpu().numpy()[:case["n_log"]], before[:case["n_log"]])      # earlier rows stand


@pytest.mark.parametrize("returns", ("mixed", "wide"))
def test_totals_are_summed_in_the_log_kernels_order(returns):
    """Returns of 1e-3 ... 1e4 of both signs, and of 1e-12 ... 1e12, where a float64 sum in another order has other bits: the totals
    equal cn_episode_log_add's by their bits (in _run) and the restatement's order (thread partials, butterfly, wave totals)."""
    m = R.make_member(np.random.default_rng(3), 2049, 1, done="all", resetting="alternating", returns=returns)
    want_np = R.record(R.copy_member(m), 7)
    (got,), _ = _run([m])
    assert got["tot"].cpu().numpy().tobytes() == want_np["tot"].tobytes()
    if returns == "wide":
        ret = m["last_return"][:2049].astype(np.float64)
        assert m["tot"][2] + float(np.sum(ret[::-1])) != want_np["tot"][2]          # the order is visible in this case


POP_ROWS = (1, 65, 0, 1025, 17)


def _population(seed, D=6):
    rng = np.random.default_rng(seed)
    pats = ("all", "alternating", "none", "row1024", "last")
    return [R.make_member(rng, n, D, pos=2, size=1, done=pats[p], resetting=pats[(p + 2) % 5]) for p, n in enumerate(POP_ROWS)]


def test_five_members_of_different_sizes_one_of_them_empty():
    ms = _population(11)
    got, _ = _run(ms)
    for t, m in zip(got, ms):
        _changed(t, m)
    empty, before = got[2], _dev(ms[2])
    _equal(empty, before, "the member without rows")                  # nothing of it is touched


def test_a_member_gives_the_same_result_at_any_position():
    """The 1025-row member at positions 0, 2 and 4 of five (the others keep their order around it)."""
    ms = _population(12)
    star, others = ms[3], [ms[0], ms[1], ms[2], ms[4]]
    results = []
    for at in (0, 2, 4):
        order = others[:at] + [star] + others[at:]
        got, _ = _run([R.copy_member(m) for m in order])
        results.append(got[at])
    _equal(results[0], results[1], "position 0 / 2")
    _equal(results[0], results[2], "position 0 / 4")
    alone, _ = _run([R.copy_member(star)])                            # ... and in a population of one
    _equal(results[0], alone[0], "position 0 / alone")


def test_three_consecutive_calls_carry_done_and_obs():
    """resetting carries done from call to call and prev follows obs: between the calls only obs, action, reward, done and the
    episode records change, as in a collection loop."""
    ms = _population(13)
    gen = torch.Generator(device="cuda").manual_seed(5)
    draws = {}

    def mutate(t, m, c):
        n = m["n"]
        if n == 0:
            return
        key = (c, n)
        if key not in draws:                                          # the same new inputs for both sides
            draws[key] = (torch.randn((n, m["D"]), generator=gen, device="cuda"), torch.randn((n, 2), generator=gen, device="cuda"),
                          torch.randn(n, generator=gen, device="cuda"), (torch.rand(n, generator=gen, device="cuda") < 0.4).to(torch.uint8),
                          torch.randn(n, generator=gen, device="cuda") * 100)
        o, a, r, d, ret = draws[key]
        t["obs"][:n] = o; t["action"][:n] = a; t["reward"][:n] = r; t["done"][:n] = d; t["last_return"][:n] = ret

    got, want = _run(ms, launches=(1, 2, 3), mutate=mutate)
    for t, m in zip(got, ms):
        _changed(t, m)
    big = got[3]
    assert 0 < int(big["size"]) < 3 * 1025 and int(big["n_log"]) > 1                  # rows were both kept and left out
    assert set(big["rows"][:int(big["n_log"]), 7].tolist()) == {1.0, 2.0, 3.0}        # the launch index travels by value


def test_flags_written_by_the_caller_are_honoured():
    """The same member with the flags left at zero and with flags set through cn_pop_record_resetting: the set rows are not written."""
    m0 = R.make_member(np.random.default_rng(14), 65, 4, done="none", resetting="none")
    m1 = R.copy_member(m0)
    m1["resetting"][:65] = R.pattern("alternating", 65)
    (g0,), _ = _run([m0])
    (g1,), _ = _run([m1])
    assert int(g0["size"]) == 65 and int(g1["size"]) == 33
    assert np.array_equal(g1["s"][:33].cpu().numpy(), m1["prev"][:65][0::2])          # rows 0, 2, ... in row order
    assert round(float(g0["tot"][4]) - m0["tot"][4]) == 65 and round(float(g1["tot"][4]) - m1["tot"][4]) == 33


def test_captured_in_a_graph_and_replayed():
    """One direct call, then the call captured on one stream (a single linear branch: two kernel nodes) and replayed twice, against three
    direct calls with the same launch on second copies."""
    _abi, _ = lib()
    ms = _population(15)
    got, want = [_dev(m) for m in ms], [_dev(m) for m in ms]
    rec = Recorder([_struct(_abi, t, m) for t, m in zip(got, ms)], ms[0]["D"])
    for p, (t, m) in enumerate(zip(got, ms)):
        rec.flags(p).copy_(t["resetting"][:m["n"]])
    rec.record(9)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rec.record(9)
    g.replay(); g.replay()
    torch.cuda.synchronize()
    for _ in range(3):
        for t, m in zip(want, ms):
            _reference(t, m, 9)
    for p, (t, m) in enumerate(zip(got, ms)):
        t["resetting"][:m["n"]] = rec.flags(p)
    torch.cuda.synchronize()
    del g
    rec.close()
    for p, (a, b) in enumerate(zip(got, want)):
        _equal(a, b, "member %d" % p)
    assert int(got[3]["n_log"]) == 3                                   # row 1024 finished in each of the three calls


def test_the_two_refusals_that_need_a_live_handle():
    from crowdnav import Config
    from crowdnav.env import VecEnv
    _abi, L = lib()
    m = R.make_member(np.random.default_rng(16), 4, 398)
    t = _dev(m)
    rec = Recorder([_struct(_abi, t, m)], 398)
    for p in (-1, 1, 64):
        assert L.cn_pop_record_resetting(rec.h, p) is None
        msg = L.cn_last_error().decode()
        assert "cn_pop_record_resetting" in msg and "member %d" % p in msg and "out of range" in msg
    rec.close()
    env = VecEnv(Config(n_envs=8, n_peds=20, seed=1, max_steps=9))
    assert env.D == 398
    s = _struct(_abi, t, m)
    s.env, s.counters, s.last_return = env.h.value, None, None
    h = C.c_void_p()
    rc = L.cn_pop_record_create((_abi.CnPopRecordMember * 1)(s), 1, 398, 0, C.byref(h))
    msg = L.cn_last_error().decode()
    assert rc == CN_ERR_ARG and not h.value and "member 0" in msg and "n_envs 8" in msg and "n is 4" in msg, msg
    env.close()


# ---- real environments ---------------------------------------------------------------------------------------------------------------
SWITCHES = ["--algo", "td3", "--learner", "fused", "--scenario", "training_as_logged", "--waypoint-reward", "0", "--envs", "4",
            "--max-steps", "9", "--memory", "64", "--batch", "8", "--population", "3", "--seed", "31"]


def _side(out):
    """P = 3 members of 4 environments as train_population builds them (train.build_members): environments, agents, the one-launch
    actor, episode logs."""
    from crowdnav import train
    a = train.parse_args(SWITCHES + ["--out", str(out)])
    train.fill_defaults(a)
    P = a.population
    _, envs, agents, pop = train.build_members(a)
    obs = envs.reset()
    rows = [envs.rows(p) for p in range(P)]
    act = torch.zeros((envs.N, 2), dtype=torch.float32, device=obs.device)
    pop.bind_act([obs[r] for r in rows], [act[r] for r in rows])
    elogs = [train.DeviceEpisodeLog(obs.device, 1000) for _ in range(P)]
    return dict(envs=envs, agents=agents, pop=pop, obs=obs, act=act, rows=rows, elogs=elogs, prev=torch.empty_like(obs),
                step_all=envs.bind_step_all(act, auto_reset="next"))


def test_real_environments_forty_launches_against_the_per_member_path(tmp_path):
    """Twin handles of the same seeds: act, step, then one side records with Population.record and the other with the per-member
    sequence train_population ran before (prev.copy_, P x (add_masked, counters, returns, log add), ~resetting, done.bool()).  Rings,
    logs and the flushed rows are equal; episodes ended and reset launches were left out, so both branches ran."""
    one, per = _side(tmp_path / "one"), _side(tmp_path / "per")
    P = 3
    one["prev"].copy_(one["obs"])
    one["pop"].bind_record(one["envs"].envs, *[[x[r] for r in one["rows"]] for x in
                                               (one["prev"], one["obs"], one["act"], one["envs"].reward, one["envs"].done)], one["elogs"])
    resetting = torch.zeros(per["envs"].N, dtype=torch.bool, device="cuda")
    for it in range(1, 41):
        for sd in (one, per):
            sd["pop"].act(add_noise=True)
            if sd is per:
                sd["prev"].copy_(sd["obs"])
            sd["envs"].fork(); sd["step_all"]()
            if sd is per:
                cnt = [e.counters() for e in sd["envs"].envs]
                ret = [e.returns()[0] for e in sd["envs"].envs]
            sd["envs"].join()
        one["pop"].record(it)
        keep = ~resetting
        for p, (ag, r) in enumerate(zip(per["agents"], per["rows"])):
            ag.memory.add_masked(per["prev"][r], per["act"][r], per["envs"].reward[r], per["obs"][r], per["envs"].done[r], keep[r])
            per["elogs"][p].add(per["envs"].done[r], cnt[p], ret[p], it, keep[r])
        resetting = per["envs"].done.bool()
    torch.cuda.synchronize()
    assert torch.equal(one["obs"], per["obs"]) and torch.equal(one["prev"], one["obs"])
    for p in range(P):
        x, y = one["agents"][p].memory, per["agents"][p].memory
        for k in ("s", "s2", "a", "r", "d", "pos_dev", "size_dev"):
            assert torch.equal(getattr(x, k), getattr(y, k)), (p, k)
        assert x._ub == y._ub and len(x) == len(y) and x.ready(8)
        assert torch.equal(one["pop"].resetting(p).bool(), resetting[one["rows"][p]])
        lx, ly = one["elogs"][p], per["elogs"][p]
        assert torch.equal(lx.rows, ly.rows) and torch.equal(lx.n, ly.n) and torch.equal(lx.tot.view(torch.int64), ly.tot.view(torch.int64))
        (rx, tx), (ry, ty) = lx.flush(), ly.flush()
        assert torch.equal(rx, ry) and tx == ty and len(rx) >= 4          # 40 launches of episodes at most 9 steps long
        assert tx[4] < 160 and int(x.size_dev) == min(64, int(tx[4]))      # reset launches are not transitions
    for sd in (one, per):
        sd["envs"].close()
