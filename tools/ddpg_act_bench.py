#!/usr/bin/env python
"""DDPG's act with the reference's Ornstein-Uhlenbeck noise on one stream, one build, at 16, 64 and 1 024 rows of 363 inputs:
  (a) Agent.act_ou_fused(obs, reset=mask): ONE cn_ddpg_act launch (actor, OU update, noise.reset(), float64 add, clip);
  (b) Agent.act(obs, add_noise=True) + Agent.reset_noise(mask): three eager linears and about a dozen elementwise launches;
  (c) Agent.act_mfma(obs): cn_actor_forward, the same matrix work without the noise.
Each figure is the median, min and max of 7 samples of 400 calls: a host clock around 400 enqueues and one device synchronise, so it
is the rate a training loop sees (enqueue cost included), not a kernel time.  --rows 16,64,1024 selects the row counts."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav.ddpg import Agent

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--rows", default="16,64,1024")
ap.add_argument("--samples", type=int, default=7)
ap.add_argument("--calls", type=int, default=400)
args = ap.parse_args()
D = 363


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
    return "%-40s median %.4f ms per call (min %.4f, max %.4f, %d samples of %d)" % ((name,) + m + (args.samples, args.calls))


for n in [int(x) for x in args.rows.split(",")]:
    ag = Agent(obs_dim=D, n_envs=n, device="cuda", seed=0, memory_size=16)
    ag.sync_fused_weights()
    obs, out = torch.randn((n, D), device="cuda"), torch.zeros((n, 2), device="cuda")
    mask = (torch.arange(n, device="cuda") % 25 == 0).to(torch.uint8)       # an episode in 25 ends per step

    def torch_path():
        ag.act(obs, add_noise=True)
        ag.reset_noise(mask)
    a = samples_of(lambda: ag.act_ou_fused(obs, reset=mask, out=out))
    b = samples_of(torch_path)
    c = samples_of(lambda: ag.act_mfma(obs, out=out))
    print("rows %5d: %s" % (n, line("(a) act_ou_fused(reset=mask)", a)), flush=True)
    print("rows %5d: %s" % (n, line("(b) act(add_noise=True) + reset_noise", b)), flush=True)
    print("rows %5d: %s" % (n, line("(c) act_mfma", c)), flush=True)
    print("rows %5d: (a) / (b) %.3f, (a) / (c) %.3f" % (n, a[0] / b[0], a[0] / c[0]), flush=True)
