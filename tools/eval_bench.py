#!/usr/bin/env python
"""What one evaluation launch costs: crowdnav.rollout.DeviceEvaluator (J jobs: one cn_actor_pop_forward, one cn_step_multi, one
cn_eval_record per launch, `remaining` read every 16 launches) against the host loop rollout.evaluate (one job at a time: the PyTorch
actor, cn_step, one host read per launch), run once per job in sequence at the same environments per job.  Medians (min - max) of
--samples samples of --launches evaluation launches on the host clock, enqueue included, one box and one build; per launch of ALL J
jobs.  Then the record launch alone against what it replaces per job: cn_get_counters + cn_get_returns + cn_episode_log_add.
The quota is set out of reach, so neither side stops early and both run the same number of launches.
--step group: the jobs' environments step in ONE launch (cn_step_group_step) instead of cn_step_multi; --step both: two evaluators,
one of each, their samples alternating, and only the device figures (no host loop, no record-alone legs)."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav import train
from crowdnav.env import VecEnv
from crowdnav.rollout import DeviceEvaluator, evaluate
from crowdnav.td3 import Agent

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--jobs", default="1,4,16,32")
ap.add_argument("--envs", default="16,64")
ap.add_argument("--samples", type=int, default=7)
ap.add_argument("--launches", type=int, default=400)
ap.add_argument("--scenario", default="crossing_8")
ap.add_argument("--max-steps", type=int, default=50)
ap.add_argument("--step", default="multi", choices=["multi", "group", "both"])
args = ap.parse_args()
K, QUOTA = args.launches, 1000


def spread(xs):
    return "%.1f us (%.1f - %.1f)" % (statistics.median(xs), min(xs), max(xs))


def clock(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e6


for n in [int(x) for x in args.envs.split(",")]:
    for J in [int(x) for x in args.jobs.split(",")]:
        agents = [Agent(obs_dim=398, device="cuda:0", seed=p, memory_size=16) for p in range(min(J, 4))]
        specs = [train.scenario_config(args.scenario, n, args.max_steps, 100 + j) for j in range(J)]
        jobs = [(cfg, init, vel, agents[j % len(agents)], j) for j, (cfg, init, vel) in enumerate(specs)]
        if args.step == "both":
            evs = {st: DeviceEvaluator(jobs, 0, step=st) for st in ("multi", "group")}
            us = {st: [] for st in evs}
            for e in evs.values():
                e.run(QUOTA, poll=16, max_launches=50)                               # warm-up
            for _ in range(args.samples):
                for st, e in evs.items():
                    us[st].append(clock(lambda: e.run(QUOTA, poll=16, max_launches=K)))
            print("J %2d x %3d envs: device, cn_step_multi %s  device, cn_step_group_step %s  ratio %.3f  (%d samples of %d launches, alternated, per launch of all jobs)"
                  % (J, n, spread(us["multi"]), spread(us["group"]), statistics.median(us["group"]) / statistics.median(us["multi"]), args.samples, K), flush=True)
            for e in evs.values():
                e.close()
            del evs
            continue
        ev = DeviceEvaluator(jobs, 0, step=args.step)
        ev.run(QUOTA, poll=16, max_launches=50)                                      # warm-up
        dev = [clock(lambda: ev.run(QUOTA, poll=16, max_launches=K)) for _ in range(args.samples)]
        # the record launch alone, on the state the last run left
        rec = [clock(lambda: [ev._eval.record(it) for it in range(K)]) for _ in range(args.samples)]
        logs = [train.DeviceEpisodeLog("cuda:0", n * QUOTA) for _ in range(J)]

        def per_job_record():
            for it in range(K):
                for e, r, lg in zip(ev.envs.envs, ev.rows, logs):
                    d = ev.envs.done[r]
                    lg.add(d, e.counters(), e.returns()[0], it, d)
        torch.cuda.synchronize()
        per = [clock(per_job_record) for _ in range(args.samples)]
        ev.close()
        del ev
        envs = []
        for cfg, init, vel in specs:
            e = VecEnv(cfg, device=0)
            if init is not None:
                e.set_ped_init(init)
            if vel is not None:
                e.set_ped_preset_vel(vel)
            envs.append(e)
        evaluate(envs[0], agents[0], episodes_per_env=QUOTA, max_launches=50)       # warm-up
        host = [clock(lambda: [evaluate(e, agents[j % len(agents)], episodes_per_env=QUOTA, max_launches=K) for j, e in enumerate(envs)])
                for _ in range(args.samples)]
        for e in envs:
            e.close()
        print("J %2d x %3d envs: device %s  host loop %s  ratio %.2f | record alone: one launch %s  per-job calls %s  (%d samples of %d launches, per launch of all jobs)"
              % (J, n, spread(dev), spread(host), statistics.median(host) / statistics.median(dev), spread(rec), spread(per), args.samples, K), flush=True)
