"""crowdnav.env's launch forms against each other and the snapshot against an independent reader, on the GPU (`-m gpu`): three
environments whose episodes time out at step 2, four steps, so done flags, the reset launch and final_obs all occur."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS = 3, 4


def _actions():
    import torch
    g = torch.Generator(device="cpu").manual_seed(11)
    return torch.stack([torch.rand((STEPS, N), generator=g) * 0.22, torch.rand((STEPS, N), generator=g) * 4 - 2], 2).cuda().contiguous()


def test_bound_sequence_equals_eager_with_an_expanded_action_and_indices():
    """bind_step_sequence takes what step_sequence takes -- one [N, 2] action expanded over the steps, a trajectory with topk_idx --
    and its callable fills the trajectory as step_sequence does."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    cfg = Config(n_envs=N, max_steps=2)
    action = _actions()[0].expand(STEPS, N, 2)
    assert action.stride(0) == 0
    trajs = []
    for bound in (True, False):
        env = VecEnv(cfg)
        env.reset()
        traj = dict(obs=torch.zeros((STEPS, N, env.D), device="cuda"), reward=torch.zeros((STEPS, N), device="cuda"),
                    done=torch.zeros((STEPS, N), dtype=torch.uint8, device="cuda"),
                    topk_idx=torch.full((STEPS, N, env.K), -7, dtype=torch.int32, device="cuda"))
        if bound:
            env.bind_step_sequence(action, traj)()
        else:
            env.step_sequence(action, traj)
        torch.cuda.synchronize()
        trajs.append(traj)
        env.close()
    for k in ("obs", "reward", "done", "topk_idx"):
        assert torch.equal(trajs[0][k], trajs[1][k]), k
    assert bool(trajs[0]["done"][1].all()) and not bool(trajs[0]["done"][2].any())      # the time-out, then the reset launch
    assert bool((trajs[0]["topk_idx"] != -7).any())                                     # the indices were written into the trajectory


def test_group_binders_equal_per_group_eager_steps():
    """Three groups of one environment: bind_step_all's callable (same-call reset, final_obs) called four times, bind_step_sequence's
    over the same four actions, and four rounds of per-group eager step leave the same outputs."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnvGroups
    cfg = Config(n_envs=N, max_steps=2)
    acts = _actions()
    streams = [torch.cuda.Stream() for _ in range(N)]
    one, seq, eager = (VecEnvGroups(cfg, groups=N, streams=streams) for _ in range(3))
    for grp in (one, seq, eager):
        grp.reset()
    abuf = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
    call = one.bind_step_all(abuf, auto_reset="same", want_final=True)
    finished = 0
    for t in range(STEPS):
        abuf.copy_(acts[t])
        one.fork(); call(); one.join()
        eager.fork()
        for g in range(N):
            eager.step_group(g, acts[t, eager.rows(g)], auto_reset="same", want_final=True)
        eager.join()
        torch.cuda.synchronize()
        for k in ("obs", "reward", "done", "topk_idx", "final_obs"):
            assert torch.equal(getattr(one, k), getattr(eager, k)), (t, k)
        finished += int(eager.done.sum().item())
    assert finished == 2 * N                                                             # every environment timed out twice
    assert not torch.equal(eager.final_obs, eager.obs)                                   # terminal observation next to the new episode's first
    seq.fork(); seq.bind_step_sequence([acts[t] for t in range(STEPS)], auto_reset="same")(); seq.join()
    torch.cuda.synchronize()
    for k in ("obs", "reward", "done", "topk_idx"):
        assert torch.equal(getattr(seq, k), getattr(eager, k)), k
    for grp in (one, seq, eager):
        grp.close()


def test_snapshot_sections_equal_the_debug_view():
    """split_snapshot(env.snapshot()) against readers that do not go through the section list: cn_debug_env per environment,
    cn_get_ped_init, cn_snapshot_size."""
    import torch
    from crowdnav import Config, _abi
    from crowdnav.env import VecEnv
    env = VecEnv(Config(n_envs=N, n_peds=5, max_steps=2))
    env.reset()
    for a in _actions():
        env.step(a, auto_reset="next")
    torch.cuda.synchronize()
    blob = env.snapshot()
    hd, arrs = _abi.split_snapshot(blob)
    assert env.L.cn_snapshot_size(env.h) == blob.size == hd.total_bytes
    for e in range(N):
        dbg = env.debug_env(e)
        for k in ("sd", "si", "ped_p", "ped_v"):
            assert np.array_equal(arrs[k][e], dbg[k]), (e, k)
    assert np.array_equal(arrs["ped_init"], env.get_ped_init())
    assert arrs["ped_p"].shape == (N, 5, 2) and np.abs(arrs["ped_p"]).max() > 0          # live pedestrians, not zeros against zeros
    env.close()
