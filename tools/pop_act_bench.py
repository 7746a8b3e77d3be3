#!/usr/bin/env python
"""The act side of a TD3 population on one stream, one build: for P = 1, 2, 4, 8 members of --envs rows each (398 inputs)
  (a) P agent.act_mfma calls in sequence (one cn_actor_forward each) against ONE Population.act (cn_actor_pop_forward);
  (b) P agent.sync_fused_weights calls (two transposing copies + two cn_actor_pack_weights each) against ONE Population.sync_actors
      (cn_actor_pop_pack);
  (c) one agent's act_mfma alone: the figure to hold against the parent commit (same kernel, same instruction stream).
Each figure is the median, min and max of 7 samples of 400 calls: a host clock around 400 enqueues and one device synchronise, so it
is the rate a training loop sees (enqueue cost included), not a kernel time.  --envs 64 is the default; the tables in DESIGN.md
section 9 also give 16 and 1024.  --members 1,2,4,8 selects the member counts, --solo-only prints (c) alone."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav.td3 import Agent, Population

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--envs", type=int, default=64, help="rows per member")
ap.add_argument("--members", default="1,2,4,8")
ap.add_argument("--solo-only", action="store_true")
ap.add_argument("--samples", type=int, default=7)
ap.add_argument("--calls", type=int, default=400)
args = ap.parse_args()
D, N = 398, args.envs


def timed(fn, K, warm):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(K): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / K * 1e3


def samples_of(fn):
    ms = [timed(fn, args.calls, 50 if j == 0 else 0) for j in range(args.samples)]
    return statistics.median(ms), min(ms), max(ms)


def line(name, m):
    return "%-34s median %.4f ms per call (min %.4f, max %.4f, %d samples of %d)" % ((name,) + m + (args.samples, args.calls))


def agents(P):
    return [Agent(obs_dim=D, device="cuda", seed=p, batch_size=8, memory_size=16) for p in range(P)]


solo = agents(1)[0]
obs1, out1 = torch.randn((N, D), device="cuda"), torch.zeros((N, 2), device="cuda")
solo.sync_fused_weights()
print("envs %5d: %s" % (N, line("(c) solo act_mfma", samples_of(lambda: solo.act_mfma(obs1, out=out1)))), flush=True)
if not args.solo_only:
    for P in [int(x) for x in args.members.split(",")]:
        ags = agents(P)
        obs = torch.randn((P * N, D), device="cuda")
        act = torch.zeros((P * N, 2), device="cuda")
        rows = [slice(p * N, (p + 1) * N) for p in range(P)]
        for a in ags: a.sync_fused_weights()
        pop = Population(ags).bind_act([obs[r] for r in rows], [act[r] for r in rows])

        def seq_act():
            for a, r in zip(ags, rows): a.act_mfma(obs[r], out=act[r])

        def seq_sync():
            for a in ags: a.sync_fused_weights()
        a_seq, a_one = samples_of(seq_act), samples_of(pop.act)
        b_seq, b_one = samples_of(seq_sync), samples_of(pop.sync_actors)
        print("envs %5d: P %d: %s" % (N, P, line("(a) %d act_mfma in sequence" % P, a_seq)), flush=True)
        print("envs %5d: P %d: %s" % (N, P, line("(a) one Population.act", a_one)), flush=True)
        print("envs %5d: P %d: %s" % (N, P, line("(b) %d sync_fused_weights" % P, b_seq)), flush=True)
        print("envs %5d: P %d: %s" % (N, P, line("(b) one Population.sync_actors", b_one)), flush=True)
        print("envs %5d: P %d: act %.4f ms against %.4f ms in sequence: ratio %.3f; re-pack %.4f ms against %.4f ms: ratio %.3f" % (
            N, P, a_one[0], a_seq[0], a_one[0] / a_seq[0], b_one[0], b_seq[0], b_one[0] / b_seq[0]), flush=True)
        del pop, ags
