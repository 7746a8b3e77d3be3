#!/usr/bin/env python
"""Host-side cost of one call of each launch form of crowdnav.env (enqueue only, no synchronise inside the timed loop)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav import Config
from crowdnav.env import VecEnv, VecEnvGroups
from crowdnav.td3 import Agent


def timed(label, f, n=300):   # n stays within the HIP queue depth so the host never blocks on the GPU
    for _ in range(50): f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): f()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    print("%-32s %.2f us per call" % (label, (t1 - t0) / n * 1e6))


env = VecEnv(Config(n_envs=64)); env.reset()
a = torch.zeros((64, 2), device="cuda"); a[:, 0] = 0.1
timed("VecEnv.step host enqueue time:", lambda: env.step(a, auto_reset="next"))
timed("VecEnv.bind_step callable:", env.bind_step(a, auto_reset="next"))
a1 = a.unsqueeze(0).contiguous()
timed("VecEnv.step_sequence (T = 1):", lambda: env.step_sequence(a1))
agent = Agent(obs_dim=env.cfg.obs_dim, device="cuda:0", seed=1, memory_size=16)
timed("VecEnv.rollout_policy (T = 1):", lambda: env.rollout_policy(agent, 1))
grp = VecEnvGroups(Config(n_envs=64), groups=2); grp.reset()
timed("VecEnvGroups.bind_step_all, G=2:", grp.bind_step_all(a, auto_reset="next"))
