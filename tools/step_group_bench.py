#!/usr/bin/env python
"""The environment step of J handles, one build, one process: for J = 1, 2, 4, 8, 16, 32, 64 jobs of --envs environments each
  (a) fork(); cn_step_multi; join() -- one step kernel per handle on the handle's stream between two rounds of J stream waits
      (MemberEnvs.bind_step_all, what a population and an evaluation do by default);
  (b) ONE cn_step_group_step on the current stream (MemberEnvs.bind_step_group).
Two sets of handles of the same configurations and seeds, reset once; both step from the same fixed actions, so both walk the same
episodes (next-step reset).  Each figure is the median, min and max of --samples samples of --calls calls, the two sides ALTERNATING
sample by sample: a host clock around the enqueues and one device synchronise, so it is the rate a loop sees (enqueue cost included),
not a kernel time.  --worlds training,crossing_8 (the population's default world and the evaluation's); --envs 16,64; --jobs selects the
job counts."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav.env import MemberEnvs
from crowdnav.train import scenario_config

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--envs", default="16,64", help="environments per job")
ap.add_argument("--jobs", default="1,2,4,8,16,32,64")
ap.add_argument("--worlds", default="training,crossing_8")
ap.add_argument("--samples", type=int, default=7)
ap.add_argument("--calls", type=int, default=400)
args = ap.parse_args()


def timed(fn, K):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(K): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e3


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def line(name, m):
    return "%-38s median %.4f ms per call (min %.4f, max %.4f, %d samples of %d)" % ((name,) + m + (args.samples, args.calls))


def side(world, J, N):
    """J handles of `world` with seeds 0 ... J - 1, reset, and their action buffer."""
    specs = [scenario_config(world, N, 1000, j) for j in range(J)]
    envs = MemberEnvs([sp[0] for sp in specs], 0)
    for e, (_, init, vel) in zip(envs.envs, specs):
        if init is not None: e.set_ped_init(init)
        if vel is not None: e.set_ped_preset_vel(vel)
    envs.reset()
    g = torch.Generator(device="cpu").manual_seed(7)
    act = torch.stack([torch.rand(J * N, generator=g) * 0.22, torch.rand(J * N, generator=g) * 4 - 2], 1).cuda().contiguous()
    return envs, act


for world in args.worlds.split(","):
    for N in [int(x) for x in args.envs.split(",")]:
        for J in [int(x) for x in args.jobs.split(",")]:
            (ea, acta), (eb, actb) = side(world, J, N), side(world, J, N)
            step_all, step_group = ea.bind_step_all(acta, auto_reset="next"), eb.bind_step_group(actb, auto_reset="next")

            def multi():
                ea.fork(); step_all(); ea.join()
            for _ in range(50): multi(); step_group()
            ms = {"multi": [], "group": []}
            for _ in range(args.samples):
                ms["multi"].append(timed(multi, args.calls))
                ms["group"].append(timed(step_group, args.calls))
            torch.cuda.synchronize()
            assert torch.equal(ea.obs, eb.obs) and torch.equal(ea.done, eb.done)          # the same run on both sides
            m, g = stats(ms["multi"]), stats(ms["group"])
            head = "%s, %d envs, J %2d (%s / %s):" % (world, N, J, ea.envs[0].kernel_name("multi"), eb.step_group_kernel(actb))
            print(head, line("(a) fork, cn_step_multi, join", m), flush=True)
            print(head, line("(b) one cn_step_group_step", g), flush=True)
            print("%s group %.4f ms against %.4f ms: ratio %.3f; spreads %.4f and %.4f ms" % (head, g[0], m[0], g[0] / m[0], g[2] - g[1], m[2] - m[1]), flush=True)
            ea.close(); eb.close()
            del step_all, step_group, ea, eb
