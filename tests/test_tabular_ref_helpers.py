"""tests/tabular_ref.py on the CPU: `Ref` replays the reference's recorded sequences at n = 1, equals crowdnav.tabular's NumPy path on
every case tests/test_gpu_tabular_edges.py launches, and every order case tells the statement from each wrong variant it is there
to catch -- a case that separates nothing would let that wrong kernel pass.  Every comparison is equality."""
import os

import numpy as np
import pytest

import tabular_ref as R
from conftest import GOLDEN

SEAM_N = (511, 512, 513, 1025)


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "tabular.npz"))


def _numpy_agent(sarsa, ref=None):
    from crowdnav import tabular
    ag = (tabular.Sarsa if sarsa else tabular.QLearn)(alpha=R.ALPHA, gamma=R.GAMMA)
    if ref is not None:
        ag.set_table(*ref.arrays())
    return ag


def _both(ag, ref, o1, a1, r, o2, keep, ul, ua, eps, learn=True):
    """One launch through `Ref` and through crowdnav.tabular's NumPy path on the float32 rows; actions, rows, states, table and
    counts must be equal."""
    r32 = np.asarray(r, dtype=np.float32) if learn else None
    s1, s2 = (R.states_of(o1) if learn else None), R.states_of(o2)
    acts, rows = ref.launch(s1, a1, r32.astype(np.float64) if learn else None, s2, keep, ul, ua, eps, learn, True)
    out = ag.learn_act(o1.astype(np.float32) if learn else None, np.asarray(a1, dtype=np.int32) if learn else None, r32, o2.astype(np.float32),
                       keep=keep, u_learn=ul, u_act=ua, learn=learn, epsilon=eps, want=True)
    assert out["state"].tolist() == s2 and out["action"].tolist() == acts
    assert np.array_equal(out["q_row"].numpy(), np.array(rows))
    if learn:
        assert out["state_prev"].tolist() == s1
    q, p, counts = ag.table()
    rq, rp = ref.arrays()
    assert np.array_equal(p, rp) and np.array_equal(q, rq) and counts == (ref.same, ref.diff)


def _run_seam_case(name, n, sarsa, refs, ag=None):
    """The two launches of a seam case through every Ref of `refs` (and the NumPy agent, against refs[0])."""
    rng = np.random.default_rng(1000 * n + len(name) + sarsa)
    eps = 0.0 if name == "seam_chain" else 0.3
    cases = []
    for launch in (0, 1):
        c = R.seam_case(name, n, rng, launch)
        if launch == 0 and c["seeded"]:
            seeds = R.seed_entries(np.random.default_rng(5), R.states_of(c["o1"]), 1.0)
            for ref in refs:
                ref.q = dict(seeds)
            if ag is not None:
                ag.set_table(*refs[0].arrays())
        ul, ua = rng.random((n, 5)), rng.random((n, 5))
        r64 = np.asarray(c["r"], np.float32).astype(np.float64)
        for ref in refs[1:]:
            ref.launch(R.states_of(c["o1"]), c["a1"], r64, R.states_of(c["o2"]), c["keep"], ul, ua, eps)
        if ag is not None:
            _both(ag, refs[0], c["o1"], c["a1"], c["r"], c["o2"], c["keep"], ul, ua, eps)
        else:
            refs[0].launch(R.states_of(c["o1"]), c["a1"], r64, R.states_of(c["o2"]), c["keep"], ul, ua, eps)
        cases.append(c)
    return cases


# ---- n = 1: the reference's own sequences ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["ql", "sa"])
def test_ref_at_n1_reproduces_the_reference_sequence(G, prefix):
    eps, alpha, gamma = (float(v) for v in G["hyper"])
    ref = R.Ref(prefix == "sa", alpha=alpha, gamma=gamma)
    s = R.states_of(G[prefix + "_obs"])
    T = len(s) - 1
    ua, ul, rew = G[prefix + "_u_act"], G[prefix + "_u_learn"], G[prefix + "_reward"]
    a, _ = ref.launch(None, None, None, s[0:1], None, None, ua[0:1], eps, learn=False)
    for t in range(1, T + 1):
        assert a[0] == int(G[prefix + "_action"][t - 1]), t
        prev = a
        a, _ = ref.launch(s[t - 1:t], prev, [float(np.float32(rew[t - 1]))], s[t:t + 1], None, ul[t - 1:t], ua[t:t + 1] if t < T else None, eps,
                          act=t < T)
        assert ref.q[(s[t - 1], prev[0])] == G[prefix + "_touched"][t - 1], t
    index = {}
    for d in range(31):
        for h in range(33):
            index.setdefault(str(d) + str(h), R.STATE[(d, h)])
    final = {(index[k.decode()], int(x)): float(v) for k, x, v in zip(G[prefix + "_q_keys"], G[prefix + "_q_actions"], G[prefix + "_q_values"])}
    assert ref.q == final and (ref.same, ref.diff) == tuple(int(c) for c in G[prefix + "_counts"])


def test_key_table_of_the_restatement():
    assert len(R.STATE) == 1023 and sorted(set(R.STATE.values())) == list(range(977))
    al = R.aliased_keys()
    assert len(al) == 46 and all(len(v) == 2 and R.STATE[v[0]] == R.STATE[v[1]] for v in al.values()) and al["110"] == [(1, 10), (11, 0)]
    pairs, obs = R.all_pairs()
    assert len(pairs) == 1023 and R.states_of(obs) == [R.STATE[p] for p in pairs]
    assert len({tuple(o) for o in obs}) == 1023


# ---- the seam cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sarsa", [False, True])
@pytest.mark.parametrize("n", SEAM_N)
@pytest.mark.parametrize("name", R.SEAM_CASES)
def test_seam_case_equals_the_numpy_path_and_separates_its_wrong_variants(name, n, sarsa):
    wrong = [R.wrong_variant(v, n, sarsa) for v in R.SEPARATES[name]]
    ref = R.Ref(sarsa)
    cases = _run_seam_case(name, n, sarsa, [ref] + wrong, _numpy_agent(sarsa))
    for v, w in zip(R.SEPARATES[name], wrong):
        assert ref.q != w.q or (ref.same, ref.diff) != (w.same, w.diff), (name, n, v)
    seam = 512 if n > 512 else 448
    assert all(c["seam"] == seam for c in cases)
    for launch, c in enumerate(cases):
        if name == "late_first":           # one first write on B, at row `seam`; the rest of its rows blend
            assert c["rows"][0] == seam and ref.same_of[c["cell"]] == 1 and ref.diff_of.get(c["cell"], 0) == len(c["rows"]) - 1
            assert list(c["keep"][seam - 2:seam]) == [0, 0]
        if name == "seam_cell":
            assert ref.same_of[c["cell"]] == 1 and ref.diff_of.get(c["cell"], 0) == len(c["rows"]) - 1
            assert min(c["rows"]) == seam - 3 and max(c["rows"]) == min(seam + 2, n - 1)
        if name == "seam_keep":
            assert c["cell"] not in ref.q and {seam - 1, seam, n - 1} == set(c["rows"])
            assert all(c["keep"][i] == 0 for i in c["rows"]) and int(c["keep"].sum()) == n - len(c["rows"])
    if n == 1025 and name == "late_first":
        assert cases[0]["rows"] == [512, 513, 600, 1024]
    if n == 1025 and name == "seam_chain":
        assert cases[0]["rows"] == list(range(499, 531))


@pytest.mark.parametrize("sarsa", [False, True])
def test_seam_chain_separates_the_tile_snapshot_at_row_512_alone(sarsa):
    """With the snapshot retaken at row 512, the only read that changes is row 512's, of the cell row 511 wrote: the first launch of
    the two tables differs in the cell row 512 writes and nowhere else."""
    n = 1025
    rng = np.random.default_rng(1000 * n + len("seam_chain") + sarsa)
    c = R.seam_case("seam_chain", n, rng, 0)
    ref, wrong = R.Ref(sarsa), R.Ref(sarsa, tile_snapshot=512)
    ref.q = R.seed_entries(np.random.default_rng(5), R.states_of(c["o1"]), 1.0); wrong.q = dict(ref.q)
    ul, ua = rng.random((n, 5)), rng.random((n, 5))
    for x in (ref, wrong):
        x.launch(R.states_of(c["o1"]), c["a1"], c["r"], R.states_of(c["o2"]), None, ul, ua, 0.0)
    s1 = R.states_of(c["o1"])
    assert {k for k in ref.q if ref.q[k] != wrong.q[k]} == {(s1[512], 1)} and c["cell"] == (s1[511], 1)


# ---- one wavefront's cells, the action range ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sarsa", [False, True])
@pytest.mark.parametrize("n", [64, 130])
@pytest.mark.parametrize("kind", ["r0", "r7", "mixed"])
def test_wavefront_case_equals_the_numpy_path(kind, n, sarsa):
    rng = np.random.default_rng(10 * n + len(kind))
    o1, a1, r, o2, cells = R.wavefront_case(kind, n, rng)
    if kind == "mixed":
        assert sorted(c % 8 for c in cells[:64]) == sorted(list(range(8)) * 8) and all(cells[i] == cells[i % 64] for i in range(n))
    else:
        assert {c % 8 for c in cells} == {int(kind[1])} and len(set(cells)) == n
    ag, ref = _numpy_agent(sarsa), R.Ref(sarsa)
    _both(ag, ref, o1, a1, r, o2, None, rng.random((n, 5)), rng.random((n, 5)), 0.3)
    assert (ref.same, ref.diff) == (min(n, 64) if kind == "mixed" else n, n - 64 if kind == "mixed" and n > 64 else 0)
    _both(ag, ref, o2, a1, r[::-1].copy(), o1, None, rng.random((n, 5)), rng.random((n, 5)), 0.3)


@pytest.mark.parametrize("sarsa", [False, True])
def test_action_range_case_equals_the_numpy_path_and_skips_what_is_no_action(sarsa):
    n, rng = 130, np.random.default_rng(31)
    o1, a1, r, o2 = R.action_range_case(n, rng)
    ag, ref = _numpy_agent(sarsa), R.Ref(sarsa)
    _both(ag, ref, o1, a1, r, o2, None, rng.random((n, 5)), rng.random((n, 5)), 0.3)
    valid = int(((a1 >= 0) & (a1 <= 2)).sum())
    assert 0 < valid < n and ref.same + ref.diff == valid and all(0 <= a <= 2 for _, a in ref.q)
    _both(ag, ref, o2, a1, r[::-1].copy(), o1, None, rng.random((n, 5)), rng.random((n, 5)), 0.3)
    assert ref.same + ref.diff == 2 * valid


# ---- epsilon -----------------------------------------------------------------------------------------------------------------
def test_epsilon_is_the_reference_loop():
    from crowdnav.dqn import epsilon_after
    for eps0, disc, floor in ((0.9, 0.9986, 0.05), (0.5, 0.99, 0.1)):
        e, seq = eps0, []
        for k in range(3001):                      # start_sarsa_training.py:51-52, once per episode begun
            if e > floor:
                e *= disc
            seq.append(e)
        for E in (0, 2, 3, 5, 700, 3000):
            assert R.epsilon(E, eps0, disc, floor) == seq[E] == epsilon_after(E + 1, eps0, disc, floor)
        assert R.epsilon(-1, eps0, disc, floor) == eps0
    assert R.epsilon(1000, 0.9, 1.0, 0.05) == 0.9
    assert R.epsilon(0, 0.9, 0.0, 0.05) == 0.0 == R.epsilon(9, 0.9, 0.0, 0.05)
    assert R.epsilon(3000, 0.9, 0.9986, 0.05) <= 0.05 < R.epsilon(700, 0.9, 0.9986, 0.05)
    assert R.epsilon(3000, 0.5, 0.99, 0.1) <= 0.1 < R.epsilon(5, 0.5, 0.99, 0.1)
