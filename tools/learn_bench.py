#!/usr/bin/env python
"""TD3 updates per second: the eager torch path, Agent.enable_graphs (one hipGraph launch per update) and cn_td3_update
(Agent.enable_fused_update: 7 + 5 hand-written launches, csrc/crowdnav_td3.hip; also captured into hipGraphs here).
--replay-sample {with,without}: how the updates draw their mini-batch (cn_*_set_replay_sample; `without` times the fused and the
eager update only: the captured PyTorch update draws with replacement).  --samples N (with CN_LEARN_MODES=fused): the median, min and
max of N samples of 400 updates instead of one mean.  --algo dqn: cn_dqn_update at (361 of 363, 300, batch) in the same way (fused only).
--population P: P solo cn_td3_update handles updated one after another on one stream against ONE cn_td3_pop_update of P members
(crowdnav.td3.Population) on the same build -- the medians of 7 samples of 400 updates, their spread and the ratio; the solo line
(one handle) is the figure to hold against the parent commit.  --replay-source {own,shared,both} (with --population): whose rings
the population's updates sample (cn_td3_pop_set_replay_source); both = one population, its 7 samples of 400 updates taken in turn
with the own and the shared source (the switch is a host flag), and the difference of the medians: the prep launch is all that differs."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav.td3 import Agent

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--replay-sample", default="with", choices=["with", "without"])
ap.add_argument("--algo", default="td3", choices=["td3", "dqn"])
ap.add_argument("--samples", type=int, default=0)
ap.add_argument("--population", type=int, default=0)
ap.add_argument("--replay-source", default="own", choices=["own", "shared", "both"])
args = ap.parse_args()
RS = args.replay_sample


def fill(ag, n=100000):
    ag.memory.add(torch.randn((n, 398), device="cuda"), torch.rand((n, 2), device="cuda"), torch.randn(n, device="cuda"),
                  torch.randn((n, 398), device="cuda"), torch.rand(n, device="cuda") < 0.05)


def timed(fn, K=400, warm=50):
    for i in range(warm): fn(i)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(K): fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e3


def report(B, name, fn):
    if args.samples > 0:
        ms = [timed(fn, warm=50 if j == 0 else 0) for j in range(args.samples)]
        print("batch %5d: %s, replay sample %s: median %.4f ms per update (min %.4f, max %.4f, %d samples of 400)" % (
            B, name, RS, statistics.median(ms), min(ms), max(ms), len(ms)), flush=True)
    else:
        print("batch %5d: %s %.3f ms per update (replay sample %s)" % (B, name, timed(fn), RS), flush=True)


def samples_of(fn, n=7):
    ms = [timed(fn, warm=50 if j == 0 else 0) for j in range(n)]
    return statistics.median(ms), min(ms), max(ms)


def population_bench(B, P):
    from crowdnav.td3 import Population
    line = lambda name, m: "%s median %.4f ms per update (min %.4f, max %.4f, 7 samples of 400)" % ((name,) + m)

    def agents():
        out = [Agent(obs_dim=398, device="cuda", seed=p, batch_size=B, memory_size=20000, replay_sample=RS) for p in range(P)]
        for a in out: fill(a, 10000)
        return out
    solo = agents()
    for a in solo: a.enable_fused_update()
    one = samples_of(solo[0].learn)
    print("batch %5d: %s" % (B, line("solo (one handle)", one)), flush=True)
    seq = samples_of(lambda i: [a.learn(i) for a in solo])
    print("batch %5d: %s" % (B, line("%d solo handles in sequence" % P, seq)), flush=True)
    del solo
    pop = Population(agents(), replay_source="own" if args.replay_source == "both" else args.replay_source)
    if args.replay_source == "both":
        ms = {"own": [], "shared": []}
        for j in range(7):
            for source in ("own", "shared"):
                pop.set_replay_source(source)
                ms[source].append(timed(pop.learn, warm=50 if j == 0 else 10))
        own, shared = [(statistics.median(v), min(v), max(v)) for v in (ms["own"], ms["shared"])]
        print("batch %5d: %s" % (B, line("population of %d, replay source own   " % P, own)), flush=True)
        print("batch %5d: %s" % (B, line("population of %d, replay source shared" % P, shared)), flush=True)
        print("batch %5d: population %d: shared - own = %+.4f ms per update (%+.2f %%), alternated sample by sample" % (
            B, P, shared[0] - own[0], 100.0 * (shared[0] - own[0]) / own[0]), flush=True)
        pop.set_replay_source("own")
    tog = samples_of(pop.learn)
    print("batch %5d: %s" % (B, line("population of %d%s" % (P, ", replay source shared" if args.replay_source == "shared" else ""), tog)), flush=True)
    print("batch %5d: population %d: %.4f ms against %.4f ms in sequence: ratio %.3f (%.4f ms per member and update)" % (
        B, P, tog[0], seq[0], tog[0] / seq[0], tog[0] / P), flush=True)


ONLY_FUSED = os.environ.get("CN_LEARN_MODES", "") == "fused"      # (tools/learn_profile.sh: the fused chain alone under rocprofv3)
for B in [int(x) for x in os.environ.get("CN_BATCHES", "128,1024" if args.algo == "td3" else "64").split(",")]:
    row = []
    if args.population > 0:
        population_bench(B, args.population)
        continue
    if args.algo == "dqn":
        from crowdnav import dqn
        ag = dqn.Agent(obs_dim=361, obs_ld=363, device="cuda", seed=0, batch_size=B, memory_size=200000, replay_sample=RS)
        n = 100000
        ag.memory.add(torch.randn((n, 363), device="cuda"), torch.randint(0, 3, (n, 2), device="cuda").float(), torch.randn(n, device="cuda"),
                      torch.randn((n, 363), device="cuda"), torch.rand(n, device="cuda") < 0.05)
        ag.enable_fused_update()
        report(B, "dqn fused", ag.learn)
        continue
    if ONLY_FUSED:
        ag = Agent(obs_dim=398, device="cuda", seed=0, batch_size=B, memory_size=200000, replay_sample=RS)
        fill(ag); ag.enable_fused_update()
        report(B, "fused", ag.learn)
        continue
    if RS == "without":
        for mode in ("eager", "fused"):
            ag = Agent(obs_dim=398, device="cuda", seed=0, batch_size=B, memory_size=200000, replay_sample=RS)
            fill(ag)
            if mode == "fused": ag.enable_fused_update()
            report(B, mode, ag.learn)
        continue
    for mode in ("eager", "graphs", "fused"):
        ag = Agent(obs_dim=398, device="cuda", seed=0, batch_size=B, memory_size=200000)
        fill(ag)
        if mode == "graphs": ag.enable_graphs()
        if mode == "fused": ag.enable_fused_update()
        row.append(timed(ag.learn))
    # the fused update replayed as hipGraphs (the chain is enqueue-only, so it captures like any other kernel sequence)
    ag = Agent(obs_dim=398, device="cuda", seed=0, batch_size=B, memory_size=200000)
    fill(ag); ag.enable_fused_update()
    for i in range(4): ag.learn(i)
    torch.cuda.synchronize()
    gs = {}
    side = torch.cuda.Stream()
    for do_actor in (0, 1):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ag.learn(do_actor)            # step 0: actor too; step 1: critics only
        gs[do_actor] = g
    row.append(timed(lambda i: gs[i & 1].replay()))
    print("batch %5d: eager %.3f ms per update, graphed %.3f ms, fused %.3f ms (%.0f updates/s), fused + hipGraph %.3f ms (%.0f updates/s)" % (
        B, row[0], row[1], row[2], 1e3 / row[2], row[3], 1e3 / row[3]), flush=True)
