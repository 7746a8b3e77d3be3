"""tests/kernel_matrix.py without a GPU: the cells cover the 68 kernels of the table exactly once, each cell's forcing selects its
kernel whatever the CU count (the selection written out as data, and csrc/crowdnav_variants.h's own cn_select_kernel compiled with
g++), the oracle alone ends episodes in every environment of every world without outgrowing its tables, and the comparers reject a
1-ulp / one-byte / one-swap / one-field change of an oracle run held against itself."""
import ctypes as C
import shutil

import numpy as np
import pytest

import kernel_matrix as M
import kernel_table_ref as T
import test_kernel_table as KT

N_CUS = (64, 104, 256, 304)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_cells_name_every_kernel_of_the_table_exactly_once():
    names = [c.kernel for c in M.CELLS]
    assert len(names) == len(set(names)) == 68 and set(names) == set(T.UNIT)
    col = {"step": 1, "same": 2, "external": 3, "sequence": 4, "policy": 5}
    for c in M.CELLS:
        assert c.form in M.FORMS and c.world in T.WORLDS and c.world in M.CONFIGS, c
        assert set(c.forcing.env) <= {"CN_X2", "CN_WPB"} and c.forcing.arbitration in ("oldest_first", "fair"), c
        row = T.WORLDS[c.world]
        if c.form == "step" and c.world in T.PLAIN_TRACKER:
            assert c.kernel == row[1] or c.kernel in T.HEADLINE_ONLY, c
        else:
            assert row[col[c.form]] == c.kernel, c              # the world's row launches this kernel for this form
        if c.form != "step":
            assert c.forcing == M.PLAIN, c
    # every (world, form) whose kernel is in the table has the cell of that kernel; external only where the row has a name
    by_name = {c.kernel: c for c in M.CELLS}
    for w, row in T.WORLDS.items():
        for form, k in zip(M.FORMS, (row[1], row[2], row[3], row[4], row[5])):
            if k is None:
                assert form == "external" and w.startswith("gt")
                continue
            assert by_name[k].form == form, (w, form)
    assert sum(1 for c in M.CELLS if c.form == "external") == 4 == len({r[3] for r in T.WORLDS.values() if r[3]})
    assert [sum(1 for c in M.CELLS if c.form == f) for f in M.FORMS] == [21, 13, 4, 15, 15]


def test_a_shared_kernel_has_one_cell_under_the_world_that_owns_it():
    for col in (2, 3):
        users = {}
        for w, row in T.WORLDS.items():
            if row[col]:
                users.setdefault(row[col], []).append(w)
        shared = {k: ws for k, ws in users.items() if len(ws) > 1}
        assert set(shared) == {k for k in M.OWNER if k in users}, col
        for k, ws in shared.items():
            cell, = [c for c in M.CELLS if c.kernel == k]
            assert cell.world == M.OWNER[k] and cell.world in ws, k
    assert M.OWNER == {"cn_env_kernel_same": "generic", "cn_env_kernel_ext": "generic"}


def test_external_cells_point_at_a_test_that_asserts_their_kernel():
    """tests/test_gpu_external.py::test_pre_get_state_reward_one_by_one_equal_the_whole_flow asserts KERNEL[name] for every name of
    PHASE_GOLDENS before it replays the golden: the cell's golden is one of them, maps to the cell's kernel, has the cell's layout
    and is the smallest of its layout there"""
    import test_gpu_external as X
    from test_external_worlds_helpers import PHASE_GOLDENS, load_golden
    import inspect
    src = inspect.getsource(X.test_pre_get_state_reward_one_by_one_equal_the_whole_flow)
    assert 'assert whole.kernel_name("external") == KERNEL[name]' in src and "_assert_golden(whole, z, reward, name, i)" in src
    calls = {g: len(load_golden(g)[0]["now"]) for g in PHASE_GOLDENS}
    for c in M.CELLS:
        if c.form != "external":
            assert c.held_by is None
            continue
        g = M.EXTERNAL_GOLDEN[c.kernel]
        assert c.held_by == M.EXTERNAL_TEST % g and g in PHASE_GOLDENS and X.KERNEL[g] == c.kernel, c
        assert calls[g] == min(n for h, n in calls.items() if X.KERNEL[h] == c.kernel), (c.kernel, calls)
    assert set(X.KERNEL.values()) == {c.kernel for c in M.CELLS if c.form == "external"}


# ---- selection -----------------------------------------------------------------------------------------------------------------------
def _step_queries():
    """(cell, launch facts) for every step cell: n_cus x overlapped (both for the cells that are not fair: an overlapped launch is
    never fair by the auto rule, and these forcings never ask for auto), 22 environments alone"""
    out = []
    for c in M.CELLS:
        if c.form != "step":
            continue
        arb, x2, wpb = M.launch_facts(c.forcing)
        for ncu in N_CUS:
            for ov in ((0,) if c.forcing.arbitration == "fair" else (0, 1)):
                out.append((c, (arb, ov, ncu, M.N_ENVS, 0, x2, wpb)))
    return out


def test_every_step_cells_forcing_selects_its_kernel_by_the_table_as_data():
    qs = _step_queries()
    assert len(qs) == 4 * (2 * 17 + 4)
    for c, L in qs:
        assert T.want_step(c.world, *L) == c.kernel, (c, L)
    # the forcings are what makes it so: without them the 360-ray world's cells all land on the two-wave kernel at 22 environments
    assert {T.want_step("s360", a, 0, ncu, M.N_ENVS, 0, -1, 4) for a in (1, 2) for ncu in N_CUS} == {"cn_env_kernel_s360_x2"}
    assert M.launch_facts(M.Forcing({}, "fair")) == (T.ARB_FAIR, -1, 4)
    assert M.launch_facts(M.Forcing({"CN_X2": "0", "CN_WPB": "0"}, "oldest_first")) == (T.ARB_OLDEST_FIRST, 0, 0)
    assert M.launch_facts(M.Forcing({"CN_X2": "1", "CN_WPB": "3"}, "oldest_first")) == (T.ARB_OLDEST_FIRST, 1, 0)


def test_every_cells_forcing_selects_its_kernel_through_cn_select_kernel(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    qs = _step_queries()
    facts = {}
    for c, L in qs:
        facts.setdefault(c.world, set()).add(L)
    lines = []
    for w in T.WORLDS:
        lines += KT.query_lines(w, lambda form: sorted(facts[w]) if form == "step" else [KT.QUIET])
    sel = KT.walk(tmp_path, lines)
    for c, L in qs:
        assert sel[(c.world, "step", L)] == c.kernel, (c, L)
    for c in M.CELLS:
        if c.form != "step":
            assert sel[(c.world, c.form, KT.QUIET)] == c.kernel, c


# ---- premise -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_runs(oracle_mod):
    """{(world, mode): (oracle after reset + 40 steps, [the dict of every step])}: every world, both reset conventions"""
    from crowdnav import Config
    acts = M.actions()
    out = {}
    for w in T.WORLDS:
        for mode in ("next", "same"):
            cfg = Config(**M.config_kw(w))
            orc = oracle_mod.Oracle(cfg.as_dict())
            steps = [dict(obs=orc.reset())]
            steps += [M.oracle_step(orc, a, mode) for a in acts]
            out[(w, mode)] = (cfg, orc, steps)
    return out


def test_the_oracle_alone_ends_episodes_everywhere_and_stays_the_reference(oracle_runs):
    assert (M.N_ENVS, M.STEPS, M.COMMON) == (22, 40, dict(n_envs=22, max_steps=9, seed=61, ped_cycle_ms=1400))
    assert M.N_ENVS % 4 == 2 and M.N_ENVS % 16 == 6 and M.N_ENVS % 8 == 6 and M.LAUNCHES * M.T_LAUNCH == M.STEPS
    for (w, mode), (cfg, orc, steps) in oracle_runs.items():
        episodes, status = M.oracle_episodes_and_status(orc)
        assert episodes.min() >= 2, (w, mode, episodes)
        assert not (status & (M.ST_TRACK_OVERFLOW | M.ST_CONF_OVERFLOW)).any(), (w, mode, status)
        assert sum(int(s["done"].sum()) for s in steps[1:]) >= 2 * M.N_ENVS, (w, mode)
        assert orc.D == cfg.obs_dim
    held = M.sequence_actions()
    assert held.shape == (5, 8, 22, 2) and (held[M.HELD_LAUNCH] == held[M.HELD_LAUNCH, 0]).all() and (held[1, 1] != held[1, 0]).any()
    assert np.array_equal(held[0], M.actions()[:8]) and held.dtype == np.float32


# ---- the comparers discriminate --------------------------------------------------------------------------------------------------------
def _got(step):
    """what a kernel that equals the oracle leaves: host arrays of the dtypes VecEnv's buffers have"""
    return dict(done=step["done"].copy(), topk_idx=step["topk_idx"].copy(), reward=step["reward"].astype(np.float32),
                obs=step["obs"].astype(np.float32), obs_f64=step["obs"].copy(), final_obs=step["final"].astype(np.float32))


def _oracle_snapshot(cfg, orc, cap=64):
    """a cn_snapshot blob holding the oracle's own state records, as VecEnv.snapshot() lays one out"""
    from crowdnav import _abi
    states = [orc.get_state(e, trk_cap=cap) for e in range(orc.N)]
    arrs = {k: np.stack([s[k] for s in states]) for k in ("sd", "si", "ped_p", "ped_v", "trk", "ped_aux")}
    arrs["ped_init"] = arrs["ped_preset"] = np.zeros((orc.N, orc.P, 2))
    hd = _abi.CnSnapshotHeader(magic=_abi.CN_SNAPSHOT_MAGIC, abi_version=_abi.EXPECTED_ABI, header_bytes=C.sizeof(_abi.CnSnapshotHeader),
                               sd_count=_abi.CN_SD_COUNT, si_count=_abi.CN_SI_COUNT, tf_count=_abi.CN_TF_COUNT, track_capacity=cap,
                               config=cfg.to_c())
    hd.total_bytes = hd.header_bytes + sum(np.ascontiguousarray(arrs[k], dtype=dt).nbytes for k, dt, _ in _abi.SNAPSHOT_SECTIONS)
    return _abi.join_snapshot(hd, arrs), arrs


@pytest.mark.parametrize("world", ["s360", "gt", "rw"])
def test_comparers_pass_an_unperturbed_copy_and_reject_each_small_change(oracle_runs, world):
    from crowdnav import _abi
    for mode, form in (("next", "step"), ("same", "same")):
        cfg, orc, steps = oracle_runs[(world, mode)]
        assert M.first_reset_difference(dict(obs=steps[0]["obs"].astype(np.float32), obs_f64=steps[0]["obs"].copy()), steps[0]["obs"], form) is None
        for s in steps[1:]:
            assert M.first_output_difference(_got(s), s, form) is None
        s = steps[17]
        # a 1-ulp change in one float64 observation element (one that float32 does not see)
        g = _got(s)
        g["obs_f64"][13, 5] = np.nextafter(g["obs_f64"][13, 5], np.inf)
        assert g["obs_f64"][13, 5].astype(np.float32) == g["obs"][13, 5]
        assert M.first_output_difference(g, s, form).startswith("obs_f64[13, 5]")
        # ... and one ulp of float32 in the float32 observation, the reward and the final observation
        for name in ("obs", "final_obs", "reward"):
            g = _got(s)
            i = (21, 3) if g[name].ndim == 2 else (21,)
            g[name][i] = np.nextafter(g[name][i], np.float32(np.inf))
            d = M.first_output_difference(g, s, form)
            assert (d is None) if (name == "final_obs" and form == "step") else d.startswith(name + "["), (name, form, d)
        # one flipped done byte
        g = _got(s)
        g["done"][21] ^= 1
        assert M.first_output_difference(g, s, form).startswith("done[21]")
        # one swapped pair of top-K indices (layouts 1 and 2 have no risk rows: every index is -1 and a swap changes nothing)
        if cfg.obs_layout == 0:
            e, s2 = next((e, q) for q in steps[1:] for e in range(M.N_ENVS) if q["topk_idx"][e, 0] != q["topk_idx"][e, 1])
            g = _got(s2)
            g["topk_idx"][e, [0, 1]] = g["topk_idx"][e, [1, 0]]
            assert M.first_output_difference(g, s2, form).startswith("topk_idx[%d, 0]" % e)
        else:
            assert all((q["topk_idx"] == -1).all() for q in steps[1:])
        # a form that writes an output needs it: no silent skip
        g = _got(s)
        del g["obs_f64"]
        with pytest.raises(KeyError):
            M.first_output_difference(g, s, form)
        assert M.first_output_difference(g, s, "sequence") is None
        # the state record: the oracle's own passes, one changed sd field of one environment does not
        blob, arrs = _oracle_snapshot(cfg, orc)
        assert M.first_state_record_difference(blob, orc, cfg.risk_mode) is None
        for env, field in ((0, "RX"), (21, "EP_RETURN"), (9, "CLOCK")):
            a2 = {k: v.copy() for k, v in arrs.items()}
            a2["sd"][env, _abi.SD[field]] = np.nextafter(a2["sd"][env, _abi.SD[field]], np.inf)
            hd, _ = _abi.split_snapshot(blob)
            d = M.first_state_record_difference(_abi.join_snapshot(hd, a2), orc, cfg.risk_mode)
            assert d is not None and d.startswith("state of env %d, sd.%s" % (env, field)), d
        a2 = {k: v.copy() for k, v in arrs.items()}
        a2["ped_p"][21, 3, 1] = np.nextafter(a2["ped_p"][21, 3, 1], np.inf)
        assert "ped_p[3].y" in M.first_state_record_difference(_abi.join_snapshot(_abi.split_snapshot(blob)[0], a2), orc, cfg.risk_mode)
        # end of run
        counters = np.concatenate([orc.counters(), np.full((M.N_ENVS, 8), 7, dtype=np.int32)], 1)
        ret = orc.returns().astype(np.float32)
        assert M.first_final_difference(counters, ret, orc) is None
        c2 = counters.copy(); c2[21, 5] += 1
        assert M.first_final_difference(c2, ret, orc).startswith("counters[21, 5]")
        r2 = ret.copy(); r2[0] = np.nextafter(r2[0], np.float32(np.inf))
        assert M.first_final_difference(counters, r2, orc).startswith("last_return[0]")
        assert M.first_final_difference(counters, ret.astype(np.float64), orc).startswith("last_return: got float64")
