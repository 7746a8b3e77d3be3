"""Planted state records on the device (`-m gpu`): one case per step cell, per same-call-reset cell and for the s360 sequence cell of
tests/kernel_matrix.py.  A case creates the cell's handle (its forcing; the kernel's name is asserted first) with one environment per
record of tests/planted_states.py, resets, plants the records through join_snapshot + restore -- the oracle holds the same arrays
through set_state -- and runs four steps of the plan's actions (0 for the records at rest).  After every step the outputs and the whole
state record of every environment equal the oracle's.  The sequence cell's four steps are one launch: its outputs are compared step by
step, but its state records and the overflow bit can only be read after the launch, and are compared there.
Equality, no tolerance.  The only environments not held to equality are those whose record names the track overflow: there both
sides outgrow the slots in the named step; their number is what tests/test_planted_states.py fixed, so none is added silently.  What the
records are and that the oracle alone does what they name: tests/test_planted_states.py, on the CPU; the oracle's run of a world and
reset convention is made once and shared by the cells of that world.

One further test: cn_restore refuses a snapshot with one field out of range, for each field of csrc/crowdnav_snapshot_check.h's list,
naming environment and field; the handle is untouched (byte-equal snapshots) and steps on equal to a twin that was never offered one."""
import numpy as np
import pytest

import kernel_matrix as M
import planted_states as PS
from test_gpu_kernel_matrix import OUT, _create, _host

pytestmark = pytest.mark.gpu

T_SEQ = 4
CELLS = [c for c in M.CELLS if c.form in ("step", "same")] + [c for c in M.CELLS if c.form == "sequence" and c.world == "s360"]


def _planted_handle(cell, monkeypatch, p):
    """the cell's handle with the plan's records planted, and the blob that planted them"""
    import torch
    from crowdnav import Config, _abi
    N = len(p.records)
    cfg, env = _create(cell, monkeypatch, Config(**dict(M.config_kw(cell.world), n_envs=N)))
    assert env.kernel_name(cell.form) == cell.kernel
    env.reset()
    torch.cuda.synchronize()
    hd, fresh = _abi.split_snapshot(env.snapshot())
    assert hd.track_capacity == p.world.slots and fresh["sd"].shape[0] == N
    blob = _abi.join_snapshot(hd, PS.snapshot_arrays(p, fresh))
    env.restore(blob)
    assert np.array_equal(env.snapshot(), blob)                       # what the kernels start from is what was planted, byte for byte
    return cfg, env, blob, fresh


def _rows(d, keep):
    return {k: v[keep] for k, v in d.items()}


def _status(snapshot):
    from crowdnav import _abi
    return _abi.split_snapshot(snapshot)[1]["si"][:, PS.SI["STATUS"]]


@pytest.mark.parametrize("cell", CELLS, ids=[c.kernel for c in CELLS])
def test_planted_records_step_as_the_oracle_does(oracle_mod, monkeypatch, cell):
    import torch
    p = PS.plan(cell.world, oracle_mod)
    W, N = p.world, len(p.records)
    mode = "same" if cell.form == "same" else "next"
    before, steps, (counters, returns) = PS.run_oracle(p, oracle_mod, mode)
    cfg, env, blob, fresh = _planted_handle(cell, monkeypatch, p)
    assert np.array_equal(fresh["ped_init"], oracle_mod.Oracle(W.config(N)).get_ped_init())      # both sides reset to the same crowd
    over = {e: p.records[e].expect[mode][1] for e in PS.overflow_records(p)}
    assert len(over) == PS.N_OVERFLOW[cell.world] and all(p.records[e].expect[mode][0] == "overflow" for e in over)
    keep = np.array([e not in over for e in range(N)])
    assert int(keep.sum()) + len(over) == N == fresh["sd"].shape[0]                               # every planted environment is compared or named
    status0 = before["si"][:, PS.SI["STATUS"]]

    assert all(at == 0 for at in over.values())                       # the overflow falls in the first step, after the planted status

    def both_overflowed(snapshot):
        """the first step's snapshot: the device raised CN_ST_TRACK_OVERFLOW, which it had not, and the oracle's list outgrew the slots"""
        now = _status(snapshot)
        for e in over:
            assert now[e] & PS.ST_TRACK_OVERFLOW and not status0[e] & PS.ST_TRACK_OVERFLOW, "env %d (%s): no CN_ST_TRACK_OVERFLOW" % (e, p.records[e].name)
            assert PS.oracle_overflowed(steps[0][1]["si"][e:e + 1], W)[0] and not PS.oracle_overflowed(before["si"][e:e + 1], W)[0]

    if cell.form == "sequence":
        acts = torch.from_numpy(p.actions).cuda().contiguous()
        traj = dict(obs=torch.zeros((T_SEQ, N, env.D), device="cuda"), reward=torch.zeros((T_SEQ, N), device="cuda"),
                    done=torch.zeros((T_SEQ, N), dtype=torch.uint8, device="cuda"), topk_idx=torch.zeros((T_SEQ, N, env.K), dtype=torch.int32, device="cuda"))
        assert PS.STEPS == T_SEQ
        env.step_sequence(acts, traj=traj)
        torch.cuda.synchronize()
        for t in range(T_SEQ):
            d = M.first_output_difference(_rows(_host(traj, OUT, t), keep), _rows(steps[t][0], keep), cell.form)
            assert d is None, "step %d: %s (rows are the environments not named as overflowing)" % (t, d)
        snap = env.snapshot()
        both_overflowed(snap)                                          # (one launch: the sticky bit is there afterwards)
        d = PS.first_state_record_difference(snap, steps[-1][1], cfg.risk_mode, skip=over)
        assert d is None, "after the launch: %s" % d
    else:
        env.enable_f64_obs()
        for t, a in enumerate(p.actions):
            env.step(torch.from_numpy(a).cuda(), auto_reset=mode, want_final=True)
            torch.cuda.synchronize()
            d = M.first_output_difference(_rows(_host(env, OUT + ("obs_f64", "final_obs")), keep), _rows(steps[t][0], keep), cell.form)
            assert d is None, "step %d: %s (rows are the environments not named as overflowing)" % (t, d)
            snap = env.snapshot()
            if t == 0:
                both_overflowed(snap)
            d = PS.first_state_record_difference(snap, steps[t][1], cfg.risk_mode, skip=over)
            assert d is None, "after step %d: %s (%s)" % (t, d, p.records[int(d.split()[3].rstrip(","))].name)
    got_counters, got_last = env.counters().cpu().numpy(), env.returns()[0].cpu().numpy()
    torch.cuda.synchronize()
    d = (M._first("counters", got_counters[keep, :6], counters[keep]) or M._first("last_return", got_last[keep], returns.astype(np.float32)[keep]))
    assert d is None, d
    env.close()


@pytest.mark.parametrize("world", ["s360", "gt", "wide"])          # (wide: the tracker rows are 256 slots apart in the blob)
def test_restore_refuses_each_field_out_of_range_and_leaves_the_handle_untouched(oracle_mod, monkeypatch, world):
    import torch
    import crowdnav
    from crowdnav import _abi
    cell = next(c for c in M.CELLS if c.world == world and c.form == "step")
    p = PS.plan(world, oracle_mod)
    cfg, env, blob, fresh = _planted_handle(cell, monkeypatch, p)
    _, twin, twin_blob, _ = _planted_handle(cell, monkeypatch, p)
    assert np.array_equal(blob, twin_blob)
    hd, _ = _abi.split_snapshot(blob)
    vio = PS.violations(p.world, p.arrays)
    names = {name.split("=")[0] for name, _, _ in vio}
    assert {"si.NTRACKS", "si.DQ_LEN", "si.DONE", "si.PENDING_RESET", "si.EP_STEP", "si.NCONF", "si.NENTRIES", "si.CROWD_HI", "sd.RX", "sd.RY", "sd.RYAW",
            "trk[0].DQLEN", "trk[0].PX", "trk[0].T"} <= names and any(n.startswith("ped_p") for n in names) and any(n.startswith("ped_v") for n in names)
    for name, text, edit in vio:
        arrs = {k: v.copy() for k, v in PS.snapshot_arrays(p, fresh).items()}
        edit(arrs)
        with pytest.raises(crowdnav.CrowdNavError) as ex:
            env.restore(_abi.join_snapshot(hd, arrs))
        assert "libcrowdnav error -2" in str(ex.value) and text in str(ex.value), (name, str(ex.value))      # CN_ERR_CONFIG, environment and field
        assert np.array_equal(env.snapshot(), blob), name                                                      # nothing was written
    # ... and the handle steps on from its untouched state, as the twin that was never offered a bad blob
    for t, a in enumerate(p.actions[:2]):
        for h in (env, twin):
            h.step(torch.from_numpy(a).cuda(), auto_reset="next", want_final=True)
        torch.cuda.synchronize()
        for k in OUT + ("final_obs",):
            assert torch.equal(getattr(env, k), getattr(twin, k)), (t, k)
        assert np.array_equal(env.snapshot(), twin.snapshot()), t
    env.close(); twin.close()
