#!/usr/bin/env python
"""The record side of a TD3 population on one stream, one build: for P = 1, 2, 4, 8 members of --envs rows each (398 inputs)
  (a) the per-member sequence of a training launch: prev.copy_(obs), P x (DeviceReplay.add_masked, VecEnv.counters, VecEnv.returns,
      DeviceEpisodeLog.add), ~resetting, done.bool();
  (b) ONE Population.record (cn_pop_record: two launches).
The members' environments are real handles, reset once and not stepped (both sides read their state records); done is a fixed pattern
with one row in ten set, so rows are kept, left out and logged as in a run.  Each figure is the median, min and max of 7 samples of 400
calls: a host clock around 400 enqueues and one device synchronise, so it is the rate a training loop sees (enqueue cost included), not
a kernel time.  --envs 64 is the default; the table in DESIGN.md section 9 also gives 16 and 1024.  --members 1,2,4,8 selects the
member counts.
--n-step W[,W ...] measures the n-step recorder instead: per P and W, (b) against (c) ONE Population.record of a population bound with
n_step = W (cn_nstep_record: two launches; W = 1 binds cn_pop_record itself), the two alternated sample by sample in one process.  With
the fixed done pattern nine rows in ten emit one full-window row per call and the tenth alternates between ending its episode and its
reset launch, so the recorder runs in its steady state after W calls (the 50 warm-up calls cover them)."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav import Config
from crowdnav.td3 import Agent, Population
from crowdnav.train import DeviceEpisodeLog, MemberEnvs

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--envs", type=int, default=64, help="rows per member")
ap.add_argument("--members", default="1,2,4,8")
ap.add_argument("--samples", type=int, default=7)
ap.add_argument("--calls", type=int, default=400)
ap.add_argument("--n-step", default="", help="windows, e.g. 1,3,5: cn_nstep_record against cn_pop_record instead of (a) against (b)")
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


def side(P, n_step=1):
    """P members: environments, agents with rings of 4096 rows, logs, and the buffers of a training launch."""
    envs = MemberEnvs([Config(n_envs=N, n_peds=20, seed=p, max_steps=50) for p in range(P)], 0)
    obs = envs.reset()
    assert envs.D == D
    ags = [Agent(obs_dim=D, device="cuda", seed=p, batch_size=8, memory_size=max(4096, N * n_step), n_step=n_step) for p in range(P)]
    rows = [envs.rows(p) for p in range(P)]
    act = torch.rand((P * N, 2), device="cuda")
    envs.reward.normal_(); envs.done.copy_((torch.arange(P * N, device="cuda") % 10 == 3).to(torch.uint8))
    elogs = [DeviceEpisodeLog("cuda", 1 << 20) for _ in range(P)]
    return dict(envs=envs, obs=obs, ags=ags, rows=rows, act=act, elogs=elogs, prev=obs.clone())


def bound(P, W):
    """-> (side, a call that records once) for a population of P bound with n_step = W"""
    s = side(P, W)
    pop = Population(s["ags"])
    pop.bind_record(s["envs"].envs, *[[x[r] for r in s["rows"]] for x in (s["prev"], s["obs"], s["act"], s["envs"].reward, s["envs"].done)],
                    s["elogs"], n_step=W)
    it = [0]

    def call():
        it[0] += 1
        pop.record(it[0])
    s["pop"] = pop
    return s, call


for P, W in [(int(x), int(w)) for x in args.members.split(",") for w in args.n_step.split(",") if w]:
    (b, one_call), (c, nstep_call) = bound(P, 1), bound(P, W)
    pairs = [(timed(one_call, args.calls, 50 if j == 0 else 0), timed(nstep_call, args.calls, 50 if j == 0 else 0)) for j in range(args.samples)]
    one, nst = [(statistics.median(x), min(x), max(x)) for x in zip(*pairs)]
    print("envs %5d: P %d: %s" % (N, P, line("(b) cn_pop_record", one)), flush=True)
    print("envs %5d: P %d: %s" % (N, P, line("(c) cn_nstep_record, W = %d" % W, nst)), flush=True)
    print("envs %5d: P %d: W %d: n-step %.4f ms against %.4f ms: ratio %.3f; spreads %.4f and %.4f ms" % (
        N, P, W, nst[0], one[0], nst[0] / one[0], nst[2] - nst[1], one[2] - one[1]), flush=True)
    for s in (b, c):
        s["envs"].close()
    del b, c, one_call, nstep_call

for P in [int(x) for x in args.members.split(",") if not args.n_step]:
    a, b = side(P), side(P)
    state = {"resetting": torch.zeros(P * N, dtype=torch.bool, device="cuda"), "it": 0}

    def per_member(s=a, st=state):
        st["it"] += 1
        s["prev"].copy_(s["obs"])
        cnt = [e.counters() for e in s["envs"].envs]
        ret = [e.returns()[0] for e in s["envs"].envs]
        s["envs"].join()
        keep = ~st["resetting"]
        reward, done = s["envs"].reward, s["envs"].done
        for p, (ag, r) in enumerate(zip(s["ags"], s["rows"])):
            ag.memory.add_masked(s["prev"][r], s["act"][r], reward[r], s["obs"][r], done[r], keep[r])
            s["elogs"][p].add(done[r], cnt[p], ret[p], st["it"], keep[r])
        st["resetting"] = done.bool()

    pop = Population(b["ags"])
    pop.bind_record(b["envs"].envs, *[[x[r] for r in b["rows"]] for x in (b["prev"], b["obs"], b["act"], b["envs"].reward, b["envs"].done)],
                    b["elogs"])
    it = [0]

    def one_call():
        it[0] += 1
        pop.record(it[0])
    seq, one = samples_of(per_member), samples_of(one_call)
    print("envs %5d: P %d: %s" % (N, P, line("(a) per-member sequence", seq)), flush=True)
    print("envs %5d: P %d: %s" % (N, P, line("(b) one Population.record", one)), flush=True)
    print("envs %5d: P %d: record %.4f ms against %.4f ms per member: ratio %.3f; spreads %.4f and %.4f ms" % (
        N, P, one[0], seq[0], one[0] / seq[0], one[2] - one[1], seq[2] - seq[1]), flush=True)
    for s in (a, b):
        s["envs"].close()
    del pop, a, b
