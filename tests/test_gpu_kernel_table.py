"""Every row of the kernel table (csrc/crowdnav_variants.h) on a live handle (`-m gpu`): one world per row of
tests/kernel_table_ref.py with three environments -- fewer than one workgroup of every launch geometry, and no multiple of 4, 8 or
16 -- names the table's kernel for every call, and every call launches: the function the table holds under a name is the
launchable kernel of that name.  (What each kernel computes is pinned, kernel by kernel and by name, by tests/test_gpu_kernel_matrix.py:
one case per kernel of the table against the CPU oracle.  tests/test_gpu_parity.py and tests/test_gpu_configs.py hold the larger and
the full-size runs, whose kernel depends on the launch.)"""
import pytest

import kernel_table_ref as T
from test_gpu_configs import ONE_LAUNCH_WORLDS

pytestmark = pytest.mark.gpu

CONFIGS = {w: kw for w, (kw, _, _) in ONE_LAUNCH_WORLDS.items()}
CONFIGS.update(gt=dict(risk_mode=1), wide=dict(track_capacity=256), generic=dict(n_peds=12, n_rays=300, k_obstacles=6), s360=dict())
assert sorted(CONFIGS) == sorted(T.WORLDS)


@pytest.mark.parametrize("world", sorted(T.WORLDS))
def test_a_handle_of_every_world_names_and_launches_the_tables_kernels(world):
    import torch
    import crowdnav
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.td3 import Agent
    N, T_ = 3, 2
    cfg = Config(n_envs=N, max_steps=9, seed=61, **CONFIGS[world])
    env = VecEnv(cfg)
    _, step, same, ext, seq, pol = T.WORLDS[world]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for what, overlapped in (("step", 0), ("multi", 1)):
        assert env.kernel_name(what) == T.want_step(world, T.ARB_AUTO, overlapped, ncu, N, 0, -1, 4), what
    assert env.kernel_name("step") == ("cn_env_kernel_s360_x2" if world == "s360" else step)
    assert env.kernel_name("same") == same and env.kernel_name("sequence") == seq and env.kernel_name("policy") == pol
    if ext is None:
        assert world.startswith("gt")
        with pytest.raises(crowdnav.CrowdNavError):
            env.kernel_name("external")
    else:
        assert env.kernel_name("external") == ext
    # every call returns without an error (VecEnv raises CrowdNavError on one) and leaves finite observations
    g = torch.Generator(device="cpu").manual_seed(3)
    acts = torch.stack([torch.rand((T_, N), generator=g) * 0.22, torch.rand((T_, N), generator=g) * 4 - 2], 2).cuda().contiguous()
    seen = [env.reset().clone()]
    seen.append(env.step(acts[0].contiguous(), auto_reset="next")[0].clone())
    seen.append(env.step(acts[1].contiguous(), auto_reset="same")[0].clone())
    traj = dict(obs=torch.zeros((T_, N, env.D), device="cuda"), reward=torch.zeros((T_, N), device="cuda"),
                done=torch.zeros((T_, N), dtype=torch.uint8, device="cuda"))
    env.step_sequence(acts, traj=traj)
    seen.append(traj["obs"].clone())
    agent = Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=6, memory_size=16)
    agent.sync_fused_weights()
    ptraj = dict(action=torch.zeros((T_, N, 2), device="cuda"), obs=torch.zeros((T_, N, env.D), device="cuda"),
                 reward=torch.zeros((T_, N), device="cuda"), done=torch.zeros((T_, N), dtype=torch.uint8, device="cuda"))
    env.rollout_policy(agent, T_, traj=ptraj)
    torch.cuda.synchronize()
    seen += [ptraj["obs"], ptraj["action"]]
    for i, o in enumerate(seen):
        assert bool(torch.isfinite(o).all()), (world, i)
    assert float(seen[0].abs().sum()) > 0 and float(ptraj["obs"].abs().sum()) > 0      # ... that the launches wrote
