"""crowdnav.env's io-struct builders without the library and without a GPU: step_io, sequence_io, policy_io and multi_io driven with
CPU tensors and a stand-in for a handle (N = 3, D = 7, K = 2).  Every field of every struct is compared with what this file works out
from the members' meaning in include/crowdnav.h: a pointer is the tensor's data_ptr(), a stride the ELEMENTS between two slots (0 =
one slot that every step overwrites), auto_reset the code of cn_step_io."""
import ctypes as C
import types

import pytest
import torch

from crowdnav import _abi
from crowdnav import env as E

N, D, K = 3, 7, 2
F32, U8, I32 = torch.float32, torch.uint8, torch.int32


def handle(obs_f64=False, h=0x1000, stream=0x2000):
    e = types.SimpleNamespace(N=N, D=D, K=K, device=torch.device("cpu"), h=C.c_void_p(h), _stream=lambda: C.c_void_p(stream),
                              obs=torch.zeros((N, D)), final_obs=torch.zeros((N, D)), reward=torch.zeros(N),
                              obs_f64=torch.zeros((N, D), dtype=torch.float64) if obs_f64 else None,
                              done=torch.zeros(N, dtype=U8), topk_idx=torch.full((N, K), -1, dtype=I32))
    return e


def fields(io):
    return {name: getattr(io, name) for name, _ in io._fields_}


def own_buffers(e):
    return dict(obs=e.obs.data_ptr(), reward=e.reward.data_ptr(), done=e.done.data_ptr(), topk_idx=e.topk_idx.data_ptr())


def trajectory(T, topk=True, action=False):
    t = dict(obs=torch.zeros((T, N, D)), reward=torch.zeros((T, N)), done=torch.zeros((T, N), dtype=U8))
    if topk:
        t["topk_idx"] = torch.zeros((T, N, K), dtype=I32)
    if action:
        t["action"] = torch.zeros((T, N, 2))
    return t


def slot_fields(e, traj):
    """obs / reward / done / topk_idx and their strides: the handle's own buffers in place, else slot 0 of the trajectory's."""
    if traj is None:
        return dict(own_buffers(e), obs_stride=0, reward_stride=0, done_stride=0, topk_stride=0)
    tk = traj.get("topk_idx")
    return dict(obs=traj["obs"].data_ptr(), reward=traj["reward"].data_ptr(), done=traj["done"].data_ptr(),
                topk_idx=tk.data_ptr() if tk is not None else None, obs_stride=N * D, reward_stride=N, done_stride=N,
                topk_stride=N * K if tk is not None else 0)


# ---- cn_step_io ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_counter", [False, True])
@pytest.mark.parametrize("want_final", [False, True])
@pytest.mark.parametrize("obs_f64", [False, True])
def test_step_io_points_at_the_action_and_the_handles_buffers(with_counter, want_final, obs_f64):
    e = handle(obs_f64)
    a = torch.zeros((N, 2))
    sc = torch.ones(N, dtype=I32) if with_counter else None
    want = dict(own_buffers(e), action=a.data_ptr(), step_counter=sc.data_ptr() if with_counter else None,
                final_obs=e.final_obs.data_ptr() if want_final else None, obs_f64=e.obs_f64.data_ptr() if obs_f64 else None,
                auto_reset=2, reserved=0)
    assert fields(E.step_io(e, a, sc, "next", want_final)) == want


@pytest.mark.parametrize("given, code", [(False, 0), (None, 0), (True, 1), ("same", 1), ("next", 2), (2, 2)])
def test_auto_reset_codes(given, code):
    assert E.step_io(handle(), torch.zeros((N, 2)), auto_reset=given).auto_reset == code


# ---- cn_sequence_io -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("traj", [None, "topk", "no topk"])
def test_sequence_io_in_place_and_into_a_trajectory(T, traj):
    e = handle()
    a = torch.zeros((T, N, 2))
    tr = None if traj is None else trajectory(T, topk=traj == "topk")
    want = dict(slot_fields(e, tr), action=a.data_ptr(), action_stride=2 * N, n_steps=T, reserved=0)
    assert fields(E.sequence_io(e, a, tr)) == want


def test_sequence_io_holds_an_expanded_action_for_every_step():
    e = handle()
    a = torch.zeros((N, 2)).expand(3, N, 2)
    assert a.stride(0) == 0
    for tr in (None, trajectory(3)):
        want = dict(slot_fields(e, tr), action=a.data_ptr(), action_stride=0, n_steps=3, reserved=0)
        assert fields(E.sequence_io(e, a, tr)) == want


# ---- cn_policy_io -------------------------------------------------------------------------------------------------------------
def agent():
    return types.SimpleNamespace(_fw_struct=object(), _fw=object(), max_v=0.22, max_w=2.0, explore_sigma=0.1, _noise_seed=77, _fused_calls=5)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("traj", [None, "topk", "no topk"])
def test_policy_io_in_place_and_into_a_trajectory(T, traj):
    e, ag = handle(), agent()
    tr = None if traj is None else trajectory(T, topk=traj == "topk", action=True)
    io, keep = E.policy_io(e, ag, T, tr)
    f32 = lambda x: C.c_float(x).value
    want = dict(slot_fields(e, tr), obs0=e.obs.data_ptr(), n_steps=T, reserved=0, max_v=f32(0.22), max_w=f32(2.0), sigma=f32(0.1),
                reserved_f=0.0, seed=77, counter=0)           # counter: the caller's, per launch
    if tr is None:
        want.update(action=e._pol_action.data_ptr(), action_stride=0)
        assert tuple(e._pol_action.shape) == (N, 2) and e._pol_action.dtype == F32
    else:
        want.update(action=tr["action"].data_ptr(), action_stride=2 * N)
    assert fields(io) == want
    assert len(keep) == 4 and all(x is y for x, y in zip(keep, (e.obs, tr, ag._fw_struct, ag._fw)))


def test_policy_io_noise_switch_seed_and_first_observation():
    e, ag = handle(), agent()
    o0 = torch.zeros((N, D))
    io, keep = E.policy_io(e, ag, 2, None, add_noise=False, noise_seed=9, obs0=o0)
    assert (io.obs0, io.sigma, io.seed) == (o0.data_ptr(), 0.0, 9) and keep[0] is o0
    first = e._pol_action
    assert E.policy_io(e, ag, 2)[0].action == first.data_ptr() and e._pol_action is first      # allocated once per handle


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refused(build, traj):
    with pytest.raises(AssertionError):
        build(traj)


@pytest.mark.parametrize("form", ["sequence", "policy"])
def test_trajectory_refusals(form):
    e, T = handle(), 3
    build = (lambda tr: E.sequence_io(e, torch.zeros((T, N, 2)), tr)) if form == "sequence" else (lambda tr: E.policy_io(e, agent(), T, tr))
    good = lambda: trajectory(T, action=form == "policy")
    build(good())
    refused(build, dict(good(), obs=torch.zeros((T, N, D), dtype=torch.float64)))             # wrong dtype
    refused(build, dict(good(), obs=torch.zeros((T, N, D + 1))))                                # wrong shape, array by array
    refused(build, dict(good(), reward=torch.zeros((T, N + 1))))
    refused(build, dict(good(), done=torch.zeros((T + 1, N), dtype=U8)))
    refused(build, dict(good(), topk_idx=torch.zeros((T, N, K + 1), dtype=I32)))
    refused(build, dict(good(), obs=torch.zeros((T, D, N)).transpose(1, 2)))                    # right shape, not contiguous


def test_action_refusals():
    e = handle()
    with pytest.raises(AssertionError):
        E.sequence_io(e, torch.zeros((3, N + 1, 2)))                    # wrong row count
    with pytest.raises(AssertionError):
        E.sequence_io(e, torch.zeros((3, N, 2), dtype=torch.float64))
    with pytest.raises(AssertionError):
        E.sequence_io(e, torch.zeros((3, 2, N)).transpose(1, 2))
    with pytest.raises(AssertionError):
        E.policy_io(e, agent(), 3, dict(trajectory(3), action=torch.zeros((3, N + 1, 2))))


# ---- cn_step_multi ------------------------------------------------------------------------------------------------------------
def multi_fields(args):
    n, hs, ios, sts = args
    return n, [hs[j] for j in range(n)], [fields(ios[j]) for j in range(n)], [sts[j] for j in range(n)]


def test_multi_io_is_step_major_and_each_entry_reads_its_groups_rows():
    G, steps = 2, 3
    envs = [handle(h=0x1000 * (g + 1), stream=0x100 * (g + 1)) for g in range(G)]
    actions = [torch.zeros((G * N, 2)) for _ in range(steps)]
    args, keep = E.multi_io(envs, actions, auto_reset="same")
    n, hs, ios, sts = multi_fields(args)
    assert n == G * steps
    for i in range(steps):
        for g, e in enumerate(envs):
            j = i * G + g
            assert hs[j] == e.h.value and sts[j] == e._stream().value
            assert ios[j] == dict(own_buffers(e), action=actions[i].data_ptr() + 4 * 2 * N * g, step_counter=None, final_obs=None,
                                  obs_f64=None, auto_reset=1, reserved=0)
    assert keep[0] is actions and len(keep) == 1 + n


@pytest.mark.parametrize("want_final", [False, True])
def test_bind_step_all_is_the_one_action_case(want_final):
    calls = []
    L = types.SimpleNamespace(cn_step_multi=lambda *a: calls.append(a) or 0)
    grp = object.__new__(E.VecEnvGroups)
    grp.envs = [handle(h=0x1000 * (g + 1), stream=0x100 * (g + 1)) for g in range(2)]
    for e in grp.envs:
        e.L = L
    a = torch.zeros((2 * N, 2))
    call = grp.bind_step_all(a, auto_reset="same", want_final=want_final)
    assert calls == []                       # binding enqueues nothing
    call(); call()
    assert len(calls) == 2 and all(x is y for x, y in zip(calls[0], calls[1]))      # the same pre-built arguments every time
    want, _ = E.multi_io(grp.envs, [a], "same", want_final)
    assert multi_fields(calls[0]) == multi_fields(want)
    assert [f["final_obs"] for f in multi_fields(want)[2]] == [e.final_obs.data_ptr() if want_final else None for e in grp.envs]
    if not want_final:
        grp.bind_step_sequence([a], auto_reset="same")()
        assert multi_fields(calls[2]) == multi_fields(want)
