#!/usr/bin/env python
"""Population-based training's exploit step on one stream, one build: for P = 2, 4, 8 TD3 members of 398 inputs and hidden 256
  (a) ONE cn_td3_pop_exploit (two launches) with the largest n_replace, P / 2, through Population's handle; an explicit fitness makes
      every call apply;
  (b) a PyTorch restatement of the same exploit: per replaced member copy_ over the 36 parameter tensors and five hyper-parameter
      writes on the Python side.  It cannot reach Adam's state, which lives in the handle, so it does less than (a);
  (c) cn_td3_pop_update before a bind and after one (and after the exploits of (a)): the update must not have moved.
Each figure is the median, min and max of 7 samples of 400 calls: a host clock around 400 enqueues and one device synchronise, so it
is the rate a training loop sees (enqueue cost included), not a kernel time.  --members 2,4,8 selects the member counts."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav.td3 import Agent, Population

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--members", default="2,4,8")
ap.add_argument("--samples", type=int, default=7)
ap.add_argument("--calls", type=int, default=400)
args = ap.parse_args()
D, H, B = 398, 256, 128
NETS = ("actor", "actor_t", "q1", "q1_t", "q2", "q2_t")


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
    return "%-38s median %.4f ms per call (min %.4f, max %.4f, %d samples of %d)" % ((name,) + m + (args.samples, args.calls))


def agents(P):
    out = []
    for p in range(P):
        a = Agent(obs_dim=D, hidden=H, batch_size=B, memory_size=4096, device="cuda", seed=p)
        g = torch.Generator().manual_seed(p)
        n = 1024
        a.memory.add(torch.randn((n, D), generator=g).cuda(), torch.rand((n, 2), generator=g).cuda(), torch.randn(n, generator=g).cuda(),
                     torch.randn((n, D), generator=g).cuda(), (torch.rand(n, generator=g) < 0.1).cuda())
        out.append(a)
    return out


for P in [int(x) for x in args.members.split(",")]:
    n = P // 2
    pop = Population(agents(P))
    step = [0]

    def update():
        step[0] += 1
        pop.learn(step[0])
    before = samples_of(update)
    pop.bind_pbt(n, explore=("lr_actor", "lr_critic", "gamma", "noise_std", "noise_clip"), factor=(0.99, 1.01), seed=1)
    fitness = torch.randn(P, device="cuda")

    def exploit():
        pop.exploit(fitness)
    fused = samples_of(exploit)
    after = samples_of(update)
    st = pop.pbt_state()
    assert st["applied"] == st["calls"] == args.samples * args.calls + 50, st["calls"]
    ags = agents(P)
    params = [[t for net in NETS for t in getattr(a, net).parameters()] for a in ags]

    @torch.no_grad()
    def restated():
        for k in range(n):                                   # the n worst (here: the last n) copy from the n best
            dst, src = P - 1 - k, k % n
            for x, y in zip(params[dst], params[src]):
                x.copy_(y)
            d, s = ags[dst], ags[src]
            d.opt_a.param_groups[0]["lr"] = s.opt_a.param_groups[0]["lr"] * 1.01
            d.opt_q1.param_groups[0]["lr"] = d.opt_q2.param_groups[0]["lr"] = s.opt_q1.param_groups[0]["lr"] * 1.01
            d.gamma, d.noise_std, d.noise_clip = min(s.gamma * 1.01, 0.999), s.noise_std * 1.01, s.noise_clip * 1.01
    torch_side = samples_of(restated)
    print("P %d, n_replace %d: %s" % (P, n, line("(a) cn_td3_pop_exploit", fused)), flush=True)
    print("P %d, n_replace %d: %s" % (P, n, line("(b) PyTorch copy_ x 36 + hyper writes", torch_side)), flush=True)
    print("P %d, n_replace %d: exploit %.4f ms against %.4f ms: ratio %.3f (the restatement leaves Adam's state behind)" % (
        P, n, fused[0], torch_side[0], fused[0] / torch_side[0]), flush=True)
    print("P %d: %s" % (P, line("(c) cn_td3_pop_update before the bind", before)), flush=True)
    print("P %d: %s" % (P, line("(c) cn_td3_pop_update after", after)), flush=True)
    del pop, ags, params
