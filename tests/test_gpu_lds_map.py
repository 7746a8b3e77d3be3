"""The corners of the LDS map (csrc/crowdnav_lds.h) on the GPU, each held to the CPU oracle bit for bit the way
tests/test_gpu_parity.py holds its rollouts: 2 environments, 40 steps, episodes of 15 steps so every world goes through resets.

  overlay_binds   33 rays x 48 pedestrians, 64-slot table: the near-pedestrian list is overlaid on region B, and its 49 entries of 32
                  bytes (1 568) are what sizes B -- gradients and confirmed objects need 1 216.  lidar_max 4.1 m exceeds the room's
                  diagonal + the pedestrian radius + the lidar's offset (3.960 + 0.0505 + 0.032), so all 48 pedestrians are within
                  reach of every robot position and the list is full at every step: entries 38 ... 48 lie past the 1 216 bytes.
  realworld_pad   41 rays x 12 pedestrians, real-world layout: everything in front of the layout's own lists ends 8 bytes short of
                  a multiple of 16, so the lists start after a pad (tests/test_lds_map.py has the numbers).
  wide_table      33 rays x 48 pedestrians with track_capacity 128: the table is in HBM and region A holds the end points only
                  (320 bytes instead of the 64-slot table's 6 144, which also gives the near list a region of its own).  Same
                  lidar_max: this near list is full at every step too.

The oracle alone runs all three without raising a status bit (CN_ST_TRACK_OVERFLOW, CN_ST_CONF_OVERFLOW: checked below at every
step), so the pedestrian counts are the ones asked for, none had to shrink."""
import numpy as np
import pytest

STEPS = 40
WORLDS = {
    "overlay_binds": dict(n_rays=33, n_peds=48, lidar_max=4.1, seed=71),
    "realworld_pad": dict(n_rays=41, n_peds=12, obs_layout=2, dt_ms=50, seed=72),
    "wide_table": dict(n_rays=33, n_peds=48, lidar_max=4.1, track_capacity=128, seed=73),
}
KERNEL = {"overlay_binds": "cn_env_kernel", "realworld_pad": "cn_env_kernel_rw", "wide_table": "cn_env_kernel_wide"}
ST_OVERFLOW = 1 | 8


def config_of(world):
    from crowdnav import Config
    return Config(n_envs=2, max_steps=15, **WORLDS[world])


@pytest.mark.gpu
@pytest.mark.parametrize("world", sorted(WORLDS))
def test_world_equals_the_oracle_bit_for_bit(oracle_mod, world, monkeypatch):
    from crowdnav import lib
    from crowdnav.env import VecEnv
    from test_gpu_parity import _compare_rollout
    monkeypatch.delenv("CN_NO_SHAPE_KERNELS", raising=False)
    cfg = config_of(world)
    R, P, K, mc = cfg.n_rays, cfg.n_peds, cfg.k_obstacles, (cfg.n_rays - 1) // 4 + 2
    tc = cfg.track_capacity or (32 if P <= 40 else 64)
    if world == "overlay_binds":
        assert lib().cn_near_separate(R, P, K, mc, tc) == 0 and lib().cn_lds_bytes(R, P, K, mc, tc) == 9408
    if world != "realworld_pad":
        assert cfg.lidar_max > 2 * 2 ** 0.5 * cfg.room_half + cfg.ped_radius + abs(cfg.lidar_offset_x)
    probe = VecEnv(cfg)
    assert probe.kernel_name("step") == KERNEL[world]
    probe.close()
    n_done, exact = _compare_rollout(oracle_mod, steps=STEPS, n_envs=2, max_steps=15, **WORLDS[world])
    assert n_done >= 2 and exact == 1.0


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_the_oracle_alone_raises_no_overflow_bit(oracle_mod, world):
    """no GPU: the premise of the comparison above: no environment leaves the range in which the oracle is the reference"""
    cfg = config_of(world)
    orc = oracle_mod.Oracle(cfg.as_dict())
    orc.reset()
    rng = np.random.default_rng(cfg.seed)
    for t in range(STEPS):
        act = np.stack([rng.uniform(0, 0.22, 2), rng.uniform(-2, 2, 2)], 1)
        orc.step(act.astype(np.float32).astype(np.float64), auto_reset=True)
        assert not any(orc.get_state(e)["si"][9] & ST_OVERFLOW for e in range(2)), t
