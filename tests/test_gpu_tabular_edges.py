"""cn_tab_learn_act (csrc/crowdnav_tab.hip) held to its statement (include/crowdnav.h) where tests/test_gpu_tabular.py does not go: rows
on either side of the 512-row tile seam, cells that all belong to one wavefront, action_prev outside 0..2, all 1023 (d, h) pairs with
cn_tab_tables, the env's float64 rows, the epsilon memo under changing schedules and a replayed graph, and every argument check.
The expectation is tests/tabular_ref.py (`Ref`, `epsilon`: plain Python that does not call crowdnav.tabular); the cases and the wrong
variants each of them separates are checked on the CPU in tests/test_tabular_ref_helpers.py.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import tabular_ref as R
from tabular_ref import Ref, obs_at, states_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CN_ERR_ARG, CN_ERR_CONFIG, CN_ERR_NO_DEVICE = -1, -2, -3


def _agent(sarsa, **kw):
    from crowdnav import tabular
    ag = (tabular.Sarsa if sarsa else tabular.QLearn)(alpha=R.ALPHA, gamma=R.GAMMA, device=DEV, **kw)
    ag.enable_fused()
    return ag


def _dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _check_table(ag, ref):
    q, p, counts = ag.table()
    rq, rp = ref.arrays()
    assert np.array_equal(p, rp)
    assert np.array_equal(q, rq)
    assert counts == (ref.same, ref.diff)


def _launch_both(ag, ref, o1, a1, r, o2, keep=None, eps=0.3, rng=None, learn=True, act=True):
    """One launch on the device and through `ref`: states, actions, rows, twists, table and counts are equal."""
    from crowdnav.dqn import TWISTS
    n = len(o2)
    ul, ua = rng.random((n, 5)), rng.random((n, 5))
    r32 = np.asarray(r, dtype=np.float32) if learn else None
    out = ag.learn_act(_dev(o1, torch.float32) if learn else None, _dev(a1, torch.int32) if learn else None, _dev(r32, torch.float32) if learn else None,
                       _dev(o2, torch.float32), keep=_dev(keep, torch.uint8) if keep is not None else None, u_learn=ul, u_act=ua,
                       learn=learn, act=act, epsilon=eps, want=True)
    s1, s2 = (states_of(o1) if learn else None), states_of(o2)
    acts, rows = ref.launch(s1, a1, r32.astype(np.float64) if learn else None, s2, keep, ul, ua, eps, learn, act)
    torch.cuda.synchronize()
    assert out["state"].cpu().tolist() == s2
    if learn:
        assert out["state_prev"].cpu().tolist() == s1
    if act:
        assert out["action"].cpu().tolist() == acts
        assert np.array_equal(out["q_row"].cpu().numpy(), np.array(rows))
        assert np.array_equal(out["twist"].cpu().numpy(), np.array(TWISTS, dtype=np.float32)[acts])
    _check_table(ag, ref)
    return out


# ---- the tile seam -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sarsa", [False, True])
@pytest.mark.parametrize("n", [511, 512, 513, 1025])
@pytest.mark.parametrize("name", R.SEAM_CASES)
def test_rows_on_both_sides_of_the_tile_seam(name, n, sarsa):
    """late_first: a cell absent until row 512 gets ONE first write there and blends after it (a kernel that judged absence per tile
    would set it again in tile 2).  seam_cell: rows 509..514 of one cell, in row order across the seam.  seam_chain: row 512 bootstraps
    from the cell row 511 wrote and must read the pre-launch value.  seam_keep: unkept rows 511, 512 and n - 1 leave their cell
    absent.  At n = 511 and 512 the same structures stand on the chunk seam 447 | 448."""
    rng = np.random.default_rng(1000 * n + len(name) + sarsa)
    eps = 0.0 if name == "seam_chain" else 0.3
    ag, ref = _agent(sarsa), Ref(sarsa)
    for launch in (0, 1):                                   # from the empty (seam_chain: seeded) table, then on what that left
        c = R.seam_case(name, n, rng, launch)
        assert c["seam"] == (512 if n > 512 else 448)
        if launch == 0 and c["seeded"]:
            ref.q = R.seed_entries(np.random.default_rng(5), states_of(c["o1"]), 1.0)
            ag.set_table(*ref.arrays())
        _launch_both(ag, ref, c["o1"], c["a1"], c["r"], c["o2"], c["keep"], eps=eps, rng=rng)
        if name in ("late_first", "seam_cell"):
            assert ref.same_of[c["cell"]] == 1 and ref.diff_of.get(c["cell"], 0) == len(c["rows"]) - 1
        if name == "seam_keep":
            assert c["cell"] not in ref.q and not ag.table()[1][c["cell"]]


# ---- one wavefront's cells -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sarsa", [False, True])
@pytest.mark.parametrize("n", [64, 130])
@pytest.mark.parametrize("kind", ["r0", "r7", "mixed"])
def test_cells_of_one_wavefront_and_of_all_eight(kind, n, sarsa):
    """Cell c is applied by wavefront c % 8.  r0 / r7: every row of the launch is a different cell of wavefront 0 / 7, so one
    wavefront's ballot holds whole chunks and seven hold nothing.  mixed: 64 cells, eight per wavefront, interleaved."""
    rng = np.random.default_rng(10 * n + len(kind))
    o1, a1, r, o2, cells = R.wavefront_case(kind, n, rng)
    ag, ref = _agent(sarsa), Ref(sarsa)
    _launch_both(ag, ref, o1, a1, r, o2, rng=rng)
    assert ref.same == (min(n, 64) if kind == "mixed" else n)
    _launch_both(ag, ref, o2, a1, r[::-1].copy(), o1, rng=rng)


# ---- action_prev outside 0..2 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sarsa", [False, True])
def test_rows_whose_action_is_no_action_are_neither_written_nor_counted(sarsa):
    n, rng = 130, np.random.default_rng(31)
    o1, a1, r, o2 = R.action_range_case(n, rng)
    ag, ref = _agent(sarsa), Ref(sarsa)
    valid = int(((a1 >= 0) & (a1 <= 2)).sum())
    _launch_both(ag, ref, o1, a1, r, o2, rng=rng)             # state_prev of every row, the act phase, table and counts
    assert ref.same + ref.diff == valid < n
    _launch_both(ag, ref, o2, a1, r[::-1].copy(), o1, rng=rng)
    assert sum(ag.table()[2]) == 2 * valid


# ---- all 1023 pairs, cn_tab_tables ---------------------------------------------------------------------------------------------
def test_every_pair_of_bins_and_the_handles_own_tables():
    from crowdnav import _abi
    pairs, obs = R.all_pairs()
    want = [R._state_table()[p] for p in pairs]
    ag = _agent(False)
    out = ag.learn_act(None, None, None, _dev(obs, torch.float32), learn=False, act=True, epsilon=0.0, want=True)
    assert out["state"].cpu().tolist() == want
    so, dist, rad = np.full((31, 33), -1, dtype=np.int32), np.zeros(30), np.zeros(32)
    assert _abi.lib().cn_tab_tables(ag._h, so.ctypes.data, dist.ctypes.data, rad.ctypes.data) == 0
    assert so.reshape(-1).tolist() == want
    assert dist.tolist() == [round(i, 2) for i in np.arange(0, 3, 0.1)]
    assert rad.tolist() == [round(i, 2) for i in np.arange(-3.14, 3.14, 0.19625)]
    only = np.zeros(32)
    assert _abi.lib().cn_tab_tables(ag._h, None, None, only.ctypes.data) == 0 and np.array_equal(only, rad)     # any may be NULL
    state = dict(zip(pairs, out["state"].cpu().tolist()))
    al = R.aliased_keys()
    assert len(al) == 46
    for key, (p0, p1) in al.items():
        assert state[p0] == state[p1] == so[p0] == so[p1], key
    assert len(set(state.values())) == 977
    # the same rows read in place from the last two of 363 columns, through a view that does not start at its buffer
    buf = torch.full((1024, 363), 7.0, dtype=torch.float32, device=DEV)
    wide = buf[1:]
    wide[:, 361:] = _dev(obs, torch.float32)
    assert wide.stride(0) == 363 and wide.shape[1] - 2 == 361 and wide.data_ptr() != buf.data_ptr()
    out = ag.learn_act(None, None, None, wide, learn=False, act=True, epsilon=0.0, want=True)
    assert out["state"].cpu().tolist() == want


# ---- the env's rows against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("py2_round", [0, 1])
def test_env_rows_are_thousandths_below_16_and_digitise_as_their_doubles(py2_round):
    """The premise of the float32 digitising argument on real rows: the env's last two float64 columns are round(v, 3) of magnitude
    below 16 and the float32 row is their narrowing; the device state of the float32 row is np.digitize on the float64 row."""
    from crowdnav import Config
    from crowdnav.env import VecEnv
    env = VecEnv(Config(n_envs=16, n_peds=6, obs_layout=1, max_steps=12, seed=3 + py2_round, py2_round=py2_round))
    env.enable_f64_obs()
    ag = _agent(False)
    rng = np.random.default_rng(8 + py2_round)
    obs = env.reset()
    ds, hs = set(), set()
    for step in range(41):
        torch.cuda.synchronize()
        x = env.obs_f64[:, -2:].cpu().numpy()
        assert x.dtype == np.float64 and np.all(np.abs(x) < 16)
        assert all(float(v) == round(float(v), 3) for v in x.reshape(-1))
        assert np.array_equal(obs[:, -2:].cpu().numpy(), x.astype(np.float32))
        want = states_of(x)
        out = ag.learn_act(None, None, None, obs, learn=False, act=True, epsilon=0.0, want=True)
        assert out["state"].cpu().tolist() == want, step
        out64 = ag.learn_act(None, None, None, env.obs_f64, learn=False, act=True, epsilon=0.0, want=True)
        assert out64["state"].cpu().tolist() == want, step
        ds |= {int(np.digitize([v], R.DIST)[0]) for v in x[:, 0]}; hs |= {int(np.digitize([v], R.RAD)[0]) for v in x[:, 1]}
        if step == 40:
            break
        twist = np.stack([rng.uniform(0, 0.22, 16), rng.uniform(-2, 2, 16)], 1).astype(np.float32)
        obs, _, _ = env.step(torch.from_numpy(twist).to(DEV), auto_reset="next")
    assert len(ds) > 1 and len(hs) > 1
    env.close()


# ---- the epsilon memo ----------------------------------------------------------------------------------------------------------
def _probe(ag, sarsa, want, E, o):
    """Draws one ulp below `want`, `want` itself and one ulp above: a row explores (action 0) exactly when its draw is below."""
    u = np.zeros((3, 5))
    u[:, 0] = [max(np.nextafter(want, -1.0), 0.0), want, np.nextafter(want, 2.0)]
    u[:, 1:4] = [0.0, 0.0, 0.99] if sarsa else [0.99, 0.0, 0.0]      # exploring picks action 0 (as tests/test_gpu_tabular.py's schedule test)
    out = ag.learn_act(None, None, None, o, u_act=u, learn=False, act=True, episodes_dev=E)
    return out["action"].cpu().tolist(), [0 if x < want else 2 for x in u[:, 0]]


@pytest.mark.parametrize("sarsa", [False, True])
def test_epsilon_memo_under_changing_schedules(sarsa):
    ag = _agent(sarsa)
    ag.set_table(np.array([[1.0, 2.0, 3.0]] * 977), np.ones((977, 3), dtype=bool))     # greedy: action 2, no tie
    o = _dev([obs_at(9, 9)] * 3, torch.float32)
    E = torch.zeros((), dtype=torch.int64, device=DEV)
    A, B = (0.9, 0.9986, 0.05), (0.5, 0.99, 0.1)
    steps = [(A, 700), (B, 5), (A, 700), (B, 3000), (A, 0), (A, 3000),          # the memo is reset when the schedule changes
             ((0.9, 1.0, 0.05), 1000), ((0.9, 0.0, 0.05), 0), ((0.9, 0.0, 0.05), 9), (A, -1), (B, -1), (A, 2), (A, 1), (A, 3)]
    for sched, e in steps:
        ag.epsilon0, ag.epsilon_discount, ag.epsilon_min = sched
        want = R.epsilon(e, *sched)
        E.fill_(e)
        got, expect = _probe(ag, sarsa, want, E, o)
        assert got == expect, (sched, e, want)
        if want > 0.0:
            assert expect == [0, 2, 2]
    assert R.epsilon(1000, 0.9, 1.0, 0.05) == 0.9 == R.epsilon(-1, *A) and R.epsilon(0, 0.9, 0.0, 0.05) == 0.0 == R.epsilon(9, 0.9, 0.0, 0.05)


@pytest.mark.parametrize("sarsa", [False, True])
def test_captured_act_launch_reads_episodes_dev_at_every_replay(sarsa):
    n = 130
    table = (np.array([[1.0, 2.0, 3.0]] * 977), np.ones((977, 3), dtype=bool))
    g, plain = _agent(sarsa), _agent(sarsa)
    g.set_table(*table); plain.set_table(*table)
    o = _dev([obs_at(9, 9)] * n, torch.float32)
    u = np.zeros((n, 5))
    u[:, 0] = (np.arange(n) + 0.5) / n                       # draws spread over (0, 1): the exploring rows are those below epsilon
    u[:, 1:4] = [0.0, 0.0, 0.99] if sarsa else [0.99, 0.0, 0.0]
    ud = _dev(u, torch.float64)
    E = torch.zeros((), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            out = g.learn_act(None, None, None, o, u_act=ud, learn=False, act=True, episodes_dev=E)
    torch.cuda.current_stream().wait_stream(st)
    seen = set()
    for e in (0, 5, 2, 700):
        E.fill_(e)
        graph.replay()
        want = plain.learn_act(None, None, None, o, u_act=ud, learn=False, act=True, episodes_dev=E)
        torch.cuda.synchronize()
        eps = R.epsilon(e, 0.9, 0.9986, 0.05)
        assert out["action"].cpu().tolist() == [0 if x < eps else 2 for x in u[:, 0]], e
        assert torch.equal(out["action"], want["action"]) and torch.equal(out["twist"], want["twist"])
        seen.add(int((out["action"] == 0).sum()))
    assert len(seen) >= 3                                      # the replays did not all act under one epsilon


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _err():
    from crowdnav import _abi
    return _abi.lib().cn_tab_last_error().decode()


class _Launch:
    """A valid cn_tab_io for n = 70 rows and the tensors behind it; io(**changes) is that struct with fields replaced."""

    def __init__(self, n=70):
        rng = np.random.default_rng(17)
        pairs = [R.A_PAIRS[j] for j in rng.integers(0, len(R.A_PAIRS), n + 1)]
        o = _dev(np.array([obs_at(*p) for p in pairs]), torch.float32)
        self.n = n
        self.o1, self.o2 = o[:-1].contiguous(), o[1:].contiguous()
        self.a1, self.r = _dev(rng.integers(0, 3, n), torch.int32), _dev(np.round(rng.normal(0, 10, n), 2), torch.float32)
        self.ul, self.ua = _dev(rng.random((n, 5)), torch.float64), _dev(rng.random((n, 5)), torch.float64)
        self.action = torch.full((n,), -77, dtype=torch.int32, device=DEV)
        self.twist = torch.full((n, 2), -77.0, dtype=torch.float32, device=DEV)

    def io(self, **changes):
        from crowdnav import _abi
        f = dict(obs_prev=self.o1.data_ptr(), obs=self.o2.data_ptr(), obs_ld=2, n=self.n, col=0, learn=1, act=1, action_prev=self.a1.data_ptr(),
                 reward=self.r.data_ptr(), done=None, keep=None, epsilon=0.3, epsilon_discount=0.9986, epsilon_min=0.05, episodes_dev=None,
                 u_learn=self.ul.data_ptr(), u_act=self.ua.data_ptr(), counter=0, action=self.action.data_ptr(), twist=self.twist.data_ptr(),
                 state=None, state_prev=None, q_row=None)
        f.update(changes)
        return _abi.CnTabIO(**f)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.action == -77).all()) and bool((self.twist == -77.0).all())


def _raw_get(L, h):
    q, p, c = np.full((977, 3), -5.0), np.full((977, 3), 9, dtype=np.uint8), np.full(2, -1, dtype=np.int64)
    assert L.cn_tab_get(h, q.ctypes.data, p.ctypes.data, c.ctypes.data) == 0
    return q, p, c


def test_create_rejects_bad_arguments_and_leaves_out_null():
    from crowdnav import _abi
    L = _abi.lib()
    good = dict(algo=0, reserved=0, alpha=0.2, gamma=0.9, seed=1)
    ndev = torch.cuda.device_count()
    cases = [(None, 0, True, CN_ERR_ARG, "null argument"),
             (good, 0, False, CN_ERR_ARG, "null argument"),
             (dict(good, algo=2), 0, True, CN_ERR_CONFIG, "algo must be 0 (Q-learning) or 1 (SARSA)"),
             (dict(good, algo=-1), 0, True, CN_ERR_CONFIG, "algo must be 0"),
             (dict(good, alpha=float("nan")), 0, True, CN_ERR_CONFIG, "alpha / gamma is NaN"),
             (dict(good, gamma=float("nan")), 0, True, CN_ERR_CONFIG, "alpha / gamma is NaN"),
             (good, -1, True, CN_ERR_NO_DEVICE, "no HIP device -1"),
             (good, ndev, True, CN_ERR_NO_DEVICE, "no HIP device %d" % ndev)]
    for cfg, device, with_out, code, words in cases:
        h = C.c_void_p(0xDEAD)
        rc = L.cn_tab_create(C.byref(_abi.CnTabConfig(**cfg)) if cfg else None, device, C.byref(h) if with_out else None)
        assert rc == code and "cn_tab_create" in _err() and words in _err(), (cfg, device, rc, _err())
        if with_out and cfg:
            assert h.value is None, (cfg, device)                  # *out stays NULL


def test_set_get_tables_reject_null_and_set_stores_absent_as_zero():
    from crowdnav import _abi
    L = _abi.lib()
    ag = _agent(False)
    q, p = np.zeros((977, 3)), np.zeros((977, 3), dtype=np.uint8)
    for fn, args, words in ((L.cn_tab_set, (None, q.ctypes.data, p.ctypes.data, None), "cn_tab_set: null argument"),
                            (L.cn_tab_set, (ag._h, None, p.ctypes.data, None), "cn_tab_set: null argument"),
                            (L.cn_tab_set, (ag._h, q.ctypes.data, None, None), "cn_tab_set: null argument"),
                            (L.cn_tab_get, (None, q.ctypes.data, p.ctypes.data, None), "cn_tab_get: null argument"),
                            (L.cn_tab_get, (ag._h, None, p.ctypes.data, None), "cn_tab_get: null argument"),
                            (L.cn_tab_get, (ag._h, q.ctypes.data, None, None), "cn_tab_get: null argument"),
                            (L.cn_tab_tables, (None, None, None, None), "cn_tab_tables: null handle")):
        assert fn(*args) == CN_ERR_ARG and words in _err(), words
    # a q value under present == 0 reads back 0.0; any nonzero present byte reads back 1; counts NULL zeroes them
    q[:] = 3.25; q[5, 1] = -0.0
    p[5, 1] = 1; p[6, 2] = 200
    assert L.cn_tab_set(ag._h, q.ctypes.data, p.ctypes.data, np.array([4, 9], dtype=np.int64).ctypes.data) == 0
    gq, gp, gc = _raw_get(L, ag._h)
    want = np.zeros((977, 3)); want[6, 2] = 3.25
    assert gq.tobytes() == np.where(np.arange(977 * 3).reshape(977, 3) == 16, -0.0, want).tobytes()
    assert gp.sum() == 2 and gp[5, 1] == 1 and gp[6, 2] == 1 and gc.tolist() == [4, 9]
    assert L.cn_tab_set(ag._h, q.ctypes.data, p.ctypes.data, None) == 0
    assert _raw_get(L, ag._h)[2].tolist() == [0, 0]


@pytest.mark.parametrize("sarsa", [False, True])
def test_learn_act_rejects_bad_arguments_with_nothing_enqueued(sarsa):
    """Every argument check of cn_tab_learn_act, on a handle that holds a seeded table: the code and the words of each refusal; the
    outputs keep their sentinels; afterwards the table and counts are the same bytes, and one valid launch gives what it gives on a
    handle that was never refused."""
    from crowdnav import _abi
    L = _abi.lib()
    x = _Launch()
    nan = float("nan")
    seeds = R.seed_entries(np.random.default_rng(2), [R.STATE[p] for p in R.A_PAIRS])
    ref = Ref(sarsa); ref.q = dict(seeds)
    refused, fresh = _agent(sarsa), _agent(sarsa)
    for ag in (refused, fresh):
        ag.set_table(*ref.arrays(), counts=(3, 8))
    before = _raw_get(L, refused._h)
    null_words, cfg_words = "cn_tab_learn_act: null argument", "cn_tab_learn_act: n < 1, col < 0 or obs_ld < col + 2"
    eps_words = "cn_tab_learn_act: epsilon_discount outside [0, 1] or epsilon_min <= 0"
    cases = [(dict(obs=None), CN_ERR_ARG, null_words),
             (dict(learn=0, act=0), CN_ERR_ARG, "cn_tab_learn_act: neither learn nor act"),
             (dict(obs_prev=None), CN_ERR_ARG, "cn_tab_learn_act: learn needs obs_prev, action_prev and reward"),
             (dict(action_prev=None), CN_ERR_ARG, "learn needs obs_prev, action_prev and reward"),
             (dict(reward=None), CN_ERR_ARG, "learn needs obs_prev, action_prev and reward"),
             (dict(action=None), CN_ERR_ARG, "cn_tab_learn_act: act needs action and twist"),
             (dict(twist=None), CN_ERR_ARG, "act needs action and twist"),
             (dict(n=0), CN_ERR_CONFIG, cfg_words), (dict(n=-3), CN_ERR_CONFIG, cfg_words),
             (dict(col=-1), CN_ERR_CONFIG, cfg_words),
             (dict(col=0, obs_ld=1), CN_ERR_CONFIG, cfg_words),             # obs_ld = col + 1
             (dict(col=361, obs_ld=362), CN_ERR_CONFIG, cfg_words),
             (dict(epsilon_discount=-0.1), CN_ERR_CONFIG, eps_words), (dict(epsilon_discount=1.1), CN_ERR_CONFIG, eps_words),
             (dict(epsilon_discount=nan), CN_ERR_CONFIG, eps_words),
             (dict(epsilon_min=0.0), CN_ERR_CONFIG, eps_words), (dict(epsilon_min=nan), CN_ERR_CONFIG, eps_words)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.cn_tab_learn_act(None, C.byref(x.io()), st) == CN_ERR_ARG and null_words in _err()
    assert L.cn_tab_learn_act(refused._h, None, st) == CN_ERR_ARG and null_words in _err()
    for changes, code, words in cases:
        rc = L.cn_tab_learn_act(refused._h, C.byref(x.io(**changes)), st)
        assert rc == code and words in _err(), (changes, rc, _err())
    assert x.untouched()
    after = _raw_get(L, refused._h)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and after[2].tolist() == [3, 8]
    ref.same, ref.diff = 3, 8
    o1, o2 = x.o1.cpu().numpy().astype(np.float64).round(3), x.o2.cpu().numpy().astype(np.float64).round(3)
    acts, _ = ref.launch(states_of(o1), x.a1.cpu().numpy(), x.r.cpu().numpy().astype(np.float64), states_of(o2), None,
                         x.ul.cpu().numpy(), x.ua.cpu().numpy(), 0.3)
    got = []
    for ag in (refused, fresh):
        assert L.cn_tab_learn_act(ag._h, C.byref(x.io()), st) == 0
        torch.cuda.synchronize()
        got.append((x.action.cpu().tolist(),) + tuple(a.tobytes() for a in _raw_get(L, ag._h)))
        assert x.action.cpu().tolist() == acts
        _check_table(ag, ref)
    assert got[0] == got[1]
