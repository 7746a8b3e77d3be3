"""The shared restatement of cn_tab_learn_act (csrc/crowdnav_tab.hip) for tests/test_gpu_tabular.py, tests/test_gpu_tabular_edges.py
and tests/test_tabular_ref_helpers.py: a Python loop on a dict, written from the rules in include/crowdnav.h, that does not call
crowdnav.tabular.  `Ref` with no switch set is the statement; every switch is a WRONG variant, there so that a test can show that
a case tells the statement from it.  The case builders below place rows on the seams of the kernel's walk -- tiles of 512 rows, in
chunks of 64, cell c applied by wavefront c % 8 -- and assert what they built."""
import numpy as np

ALPHA, GAMMA = 0.2, 0.9
M64 = 0xFFFFFFFFFFFFFFFF
TILE, CHUNK, WAVES = 512, 64, 8
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

DIST = [round(i, 2) for i in np.arange(0, 3, 0.1)]
RAD = [round(i, 2) for i in np.arange(-3.14, 3.14, 0.19625)]


def _state_table():
    seen, tab = {}, {}
    for d in range(31):
        for h in range(33):
            tab[(d, h)] = seen.setdefault(str(d) + str(h), len(seen))
    return tab


STATE = _state_table()


def states_of(obs64):
    """State indices of double observations [n, 2]: np.digitize on the doubles, the string key, its number."""
    return [STATE[(int(np.digitize([x], DIST)[0]), int(np.digitize([y], RAD)[0]))] for x, y in obs64]


def obs_at(d, h):
    """A multiple of 0.001 inside bin (d, h)."""
    x = round(0.1 * d - 0.05, 3)
    y = -3.2 if h == 0 else 3.0 if h == 32 else round((RAD[h - 1] + RAD[h]) / 2, 3)
    assert int(np.digitize([x], DIST)[0]) == d and int(np.digitize([y], RAD)[0]) == h
    return (x, y)


def epsilon(E, eps0, disc, eps_min):
    """The exploration rate of a launch that reads E finished episodes: `if e > eps_min: e *= disc` once per episode begun, E + 1
    times (float64, at most 2^22 times); disc >= 1 is no schedule."""
    e = float(eps0)
    if disc >= 1.0:
        return e
    for k in range(min(int(E) + 1, 1 << 22)):
        if e > eps_min:
            e *= disc
    return e


class Ref:
    """The statement.  Wrong variants: live_reads (a bootstrap read sees the writes of earlier rows), tile_snapshot = T (the
    snapshot the bootstrap reads see is retaken every T rows), tile_present = T (absence is judged against the table as the T-row
    tile began), descending (rows applied highest first), first_write_value (an absent cell becomes `value`, not `reward`)."""

    def __init__(self, sarsa, alpha=ALPHA, gamma=GAMMA, live_reads=False, tile_snapshot=0, tile_present=0, descending=False,
                 first_write_value=False):
        self.sarsa, self.alpha, self.gamma, self.live = sarsa, alpha, gamma, live_reads
        self.tile_snapshot, self.tile_present, self.descending, self.first_write_value = tile_snapshot, tile_present, descending, first_write_value
        self.q, self.same, self.diff = {}, 0, 0
        self.same_of, self.diff_of = {}, {}                        # the two counts per cell

    def choose(self, q, s, u, eps):
        row = [q.get((s, a), 0.0) for a in range(3)]
        u = [float(x) for x in u]
        if self.sarsa:
            if u[0] < eps:
                return int(u[1] * 3), row
        elif u[0] < eps:
            mag = max(abs(min(row)), abs(max(row)))
            row = [row[i] + u[1 + i] * mag - .5 * mag for i in range(3)]
        mx = max(row)
        if row.count(mx) > 1:
            best = [i for i in range(3) if row[i] == mx]
            return best[int(u[4] * len(best))], row
        return row.index(mx), row

    def _value(self, old, i, r, s2, u_learn, eps):
        if self.sarsa:
            a2, _ = self.choose(old, s2[i], u_learn[i], eps)
            boot = old.get((s2[i], a2), 0.0)
        else:
            boot = max(old.get((s2[i], a), 0.0) for a in range(3))
        return float(r[i]) + self.gamma * boot

    def launch(self, s1, a1, r, s2, keep=None, u_learn=None, u_act=None, eps=0.0, learn=True, act=True):
        n = len(s2)
        if learn:
            old = self.q if self.live else dict(self.q)           # 1. bootstrap reads: the table as the launch began
            order = range(n)
            value = None
            if self.descending:                                    # WRONG: the rows of a cell highest first
                value = [self._value(old, i, r, s2, u_learn, eps) for i in range(n)]
                order = range(n - 1, -1, -1)
            began = None
            for i in order:                                        # 2. writes, ascending rows
                if self.tile_snapshot and i % self.tile_snapshot == 0 and not self.live:
                    old = dict(self.q)                             # WRONG: the snapshot retaken per tile
                if self.tile_present and (began is None or i % self.tile_present == 0):
                    began = set(self.q)                            # WRONG: absence as the tile began
                v = value[i] if value is not None else self._value(old, i, r, s2, u_learn, eps)    # (live_reads interleaves: WRONG)
                if keep is not None and not keep[i]:
                    continue
                if not 0 <= int(a1[i]) <= 2:                       # no such action: neither written nor counted
                    continue
                k = (s1[i], int(a1[i]))
                if k not in (self.q if began is None else began):
                    self.q[k] = v if self.first_write_value else float(r[i]); self.same += 1
                    self.same_of[k] = self.same_of.get(k, 0) + 1
                else:
                    old_q = self.q.get(k, 0.0)
                    self.q[k] = old_q + self.alpha * (v - old_q); self.diff += 1
                    self.diff_of[k] = self.diff_of.get(k, 0) + 1
        out = [self.choose(self.q, s2[i], u_act[i], eps) for i in range(n)] if act else []       # 3. act: after all writes
        return [o[0] for o in out], [o[1] for o in out]

    def arrays(self):
        q, p = np.zeros((977, 3)), np.zeros((977, 3), dtype=bool)
        for (s, a), v in self.q.items():
            q[s, a] = v; p[s, a] = True
        return q, p


# ---- the documented device draw ------------------------------------------------------------------------------------------------
def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _draws(seed, counter, n, const):
    base = _mix(seed ^ _mix(counter ^ const))
    return np.array([[(_mix(_mix(base ^ i) ^ j) >> 11) * 2.0 ** -53 for j in range(5)] for i in range(n)])


# ---- case builders -------------------------------------------------------------------------------------------------------------
A_PAIRS = [(2, 12), (3, 13), (4, 14), (5, 15), (6, 16)]                  # the cells the filler rows fall on
QUIET_PAIRS = [(8, 25), (9, 26), (8, 27)]                                # states no row of a case writes
SPECIAL_PAIRS = [(25, 20), (26, 21)]                                     # the cell under test of launch 0 / launch 1
CHAIN_PAIRS = [(10 + (j % 13), 5 + (j % 7)) for j in range(40)]          # 40 different states
SEAM_CASES = ("late_first", "seam_cell", "seam_chain", "seam_keep")
# the wrong variants each case must tell from the statement; T is the case's seam period (512, or 64 where the launch has one tile)
SEPARATES = {"late_first": ("tile_present",), "seam_cell": ("descending", "first_write_value"), "seam_chain": ("live_reads", "tile_snapshot"),
             "seam_keep": ()}


def seam_of(n):
    """The seam a case of n rows is built on: the tile seam 511 | 512 when the launch has rows past one tile, else the chunk seam
    447 | 448 inside its only tile."""
    return TILE if n > TILE else TILE - CHUNK


def wrong_variant(name, n, sarsa):
    """The wrong Ref of that name, with the period of the seam an n-row case is built on."""
    period = TILE if n > TILE else CHUNK
    kw = {"tile_present": dict(tile_present=period), "tile_snapshot": dict(tile_snapshot=period), "descending": dict(descending=True),
          "first_write_value": dict(first_write_value=True), "live_reads": dict(live_reads=True)}[name]
    return Ref(sarsa, **kw)


def _state(pair):
    return STATE[pair]


def seam_case(name, n, rng, launch=0):
    """-> dict(o1, a1, r, o2, keep, seam, cell, rows, seeded): the rows of launch `launch` (0: from the empty -- seam_chain: seeded
    -- table, 1: on what launch 0 left; the cell under test differs between the two, so it is absent both times).  `cell` is the
    (state, action) under test and `rows` the rows placed on it."""
    seam = seam_of(n)
    assert (seam == 512) == (n > 512) and seam < n, (n, seam)     # which seam this is, and that a row stands on either side of it
    pools = [_state(p) for p in A_PAIRS + QUIET_PAIRS + SPECIAL_PAIRS + CHAIN_PAIRS]
    assert len(set(pools)) == len(pools)                                   # no two pairs of the pools share a key
    fill = rng.integers(0, len(A_PAIRS), n)
    o1 = [obs_at(*A_PAIRS[j]) for j in fill]
    o2 = [obs_at(*A_PAIRS[j]) for j in rng.integers(0, len(A_PAIRS), n)]
    a1 = rng.integers(0, 3, n)
    r = np.round(rng.normal(0, 10, n), 2)
    keep = None
    special = SPECIAL_PAIRS[launch]
    cell = (_state(special), 1)
    last = n - 1
    if name == "late_first":        # B is absent; rows seam - 2, seam - 1 point at it unkept; its first kept row is `seam`
        rows = sorted({i for i in (seam, seam + 1, seam + 88, last) if seam <= i < n})
        keep = np.ones(n, dtype=np.uint8)
        for i in (seam - 2, seam - 1):
            o1[i] = obs_at(*special); a1[i] = 1; keep[i] = 0
        for i in rows:
            o1[i] = obs_at(*special); a1[i] = 1
        assert rows[0] == seam
    elif name == "seam_cell":       # one cell written by rows seam - 3 .. seam + 2 and by no others
        rows = [i for i in range(seam - 3, seam + 3) if i < n]
        for i in rows:
            o1[i] = obs_at(*special); a1[i] = 1
        assert [i for i in rows if i < seam] == [seam - 3, seam - 2, seam - 1] and rows[-1] >= seam
    elif name == "seam_chain":      # row i's s2 is row i - 1's s1 for i in seam - 12 .. seam + 18; nobody else writes or reads those
        lo, hi = seam - 12, min(seam + 18, last)
        for i in range(lo - 1, hi + 1):
            o1[i] = obs_at(*CHAIN_PAIRS[i - lo + 1]); a1[i] = 1
            r[i] = 600.0 + (i % 7)                                         # far above every seed: the written cell becomes its row's maximum
        for i in range(lo, hi + 1):
            o2[i] = o1[i - 1]
        for i in list(range(0, lo)) + list(range(hi + 1, n)):
            o2[i] = obs_at(*QUIET_PAIRS[i % len(QUIET_PAIRS)])
        o2[lo - 1] = obs_at(*QUIET_PAIRS[0])
        rows = list(range(lo - 1, hi + 1))
        if seam < n:
            assert o2[seam] == o1[seam - 1] and lo <= seam - 1 and seam <= hi         # row `seam` bootstraps from what row seam - 1 wrote
        cell = (states_of([o1[seam - 1]])[0], 1)
        assert len(set(states_of([o1[i] for i in rows]))) == len(rows)
    elif name == "seam_keep":       # keep = 0 on rows seam - 1, seam and n - 1, all on a cell nobody else writes: it stays absent
        rows = sorted({i for i in (seam - 1, seam, last) if i < n})
        keep = np.ones(n, dtype=np.uint8)
        for i in rows:
            o1[i] = obs_at(*special); a1[i] = 1; keep[i] = 0
        assert seam - 1 in rows and last in rows
    else:
        raise KeyError(name)
    s1 = states_of(o1)
    if name != "seam_chain":         # the cell under test is written (or pointed at) by `rows` and the unkept rows only
        on_cell = [i for i in range(n) if (s1[i], int(a1[i])) == cell]
        extra = [seam - 2, seam - 1] if name == "late_first" else []
        assert on_cell == sorted(set(rows) | set(extra)), (on_cell, rows)
    return dict(o1=np.array(o1), a1=a1, r=r, o2=np.array(o2), keep=keep, seam=seam, cell=cell, rows=rows, seeded=name == "seam_chain")


def seed_entries(rng, states, fraction=0.6):
    """Pre-launch entries {(s, a): value} for about `fraction` of the cells of `states` (seam_chain takes all of them: a blend,
    unlike a first write, depends on the bootstrap read)."""
    q = {}
    for s in sorted(set(states)):
        for a in range(3):
            if rng.random() < fraction:
                q[(s, a)] = float(np.round(rng.normal(0, 5), 3))
    return q


def _cells_by_residue():
    """{cell % 8: [(pair, action), ...]} over one pair per state, in (d, h) order."""
    out, seen = {k: [] for k in range(WAVES)}, set()
    for d in range(1, 31):
        for h in range(1, 32):
            s = STATE[(d, h)]
            if s in seen:
                continue
            seen.add(s)
            for a in range(3):
                out[(3 * s + a) % WAVES].append(((d, h), a))
    return out


def wavefront_case(kind, n, rng):
    """-> (o1, a1, r, o2, cells).  kind "r0" / "r7": n rows on n distinct cells that all belong to one wavefront (cell % 8 == 0 / 7);
    "mixed": rows i on cell i % 64 of 64 distinct cells, eight of each residue, interleaved."""
    by = _cells_by_residue()
    if kind in ("r0", "r7"):
        res = int(kind[1])
        picks = by[res][:n]
        assert len(picks) == n
    elif kind == "mixed":
        base = [by[k % WAVES][k // WAVES] for k in range(64)]
        picks = [base[i % 64] for i in range(n)]
        assert sorted(((3 * STATE[p] + a) % WAVES) for p, a in base) == sorted(list(range(WAVES)) * 8)
    else:
        raise KeyError(kind)
    cells = [3 * STATE[p] + a for p, a in picks]
    if kind != "mixed":
        assert len(set(cells)) == n and all(c % WAVES == res for c in cells)
    else:
        assert len(set(cells)) == min(n, 64)
    o1 = np.array([obs_at(*p) for p, _ in picks])
    a1 = np.array([a for _, a in picks])
    assert [3 * s + int(a) for s, a in zip(states_of(o1), a1)] == cells
    return o1, a1, np.round(rng.normal(0, 10, n), 2), o1[::-1].copy(), cells


def action_range_case(n, rng):
    """n rows over a few cells with action_prev drawn from {-1, 3, INT32_MIN, INT32_MAX, 0, 1, 2}: every value at least once."""
    values = np.array([-1, 3, INT32_MIN, INT32_MAX, 0, 1, 2], dtype=np.int64)
    a1 = np.concatenate([values, values[rng.integers(0, len(values), n - len(values))]])
    pairs = [A_PAIRS[j] for j in rng.integers(0, len(A_PAIRS), n + 1)]
    o = np.array([obs_at(*p) for p in pairs])
    assert set(a1.tolist()) == set(values.tolist()) and len(a1) == n
    return o[:-1], a1, np.round(rng.normal(0, 10, n), 2), o[1:]


def all_pairs():
    """The 1023 (d, h) pairs in table order and their observations."""
    pairs = [(d, h) for d in range(31) for h in range(33)]
    return pairs, np.array([obs_at(*p) for p in pairs])


def aliased_keys():
    """{key: [pair, pair]} for the string keys that two pairs share."""
    by = {}
    for d in range(31):
        for h in range(33):
            by.setdefault(str(d) + str(h), []).append((d, h))
    return {k: v for k, v in by.items() if len(v) > 1}
