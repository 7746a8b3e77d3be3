#!/usr/bin/env python
"""The learner state blob on one stream, one build: for P = 1, 2, 4, 8 TD3 members of 398 inputs and hidden 256
  (a) ONE cn_td3_pop_state_save (one launch) plus the asynchronous copy of the blob to pinned memory, through Population's handle:
      what train.py --state-every pays for the learner;
  (b) a PyTorch restatement: .cpu() of the 36 P parameter tensors.  It cannot reach Adam's moments, the step counters or the update
      counter, which live in the handle, so it moves a third of the bytes and does less than (a);
  (c) the save's launch alone (no copy to the host), and cn_td3_pop_state_load's (its small synchronous header read included);
  (d) cn_td3_pop_update before the first save and after the saves and loads: the update must not have moved.
Each figure is the median, min and max of 7 samples of 400 calls: a host clock around 400 enqueues and one device synchronise, so it
is the rate a training loop sees (enqueue cost included), not a kernel time.  --members 1,2,4,8 selects the member counts."""
import argparse, ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "drl-based-mapless-crowd-navigation-with-perceived-risk_amd"))
import torch
from crowdnav.td3 import Agent, Population

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--members", default="1,2,4,8")
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
    ms = [timed(fn, args.calls, 20 if j == 0 else 0) for j in range(args.samples)]
    return statistics.median(ms), min(ms), max(ms)


def line(name, m):
    return "%-44s median %.4f ms per call (min %.4f, max %.4f, %d samples of %d)" % ((name,) + m + (args.samples, args.calls))


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
    ags = agents(P)
    pop = Population(ags)
    fused = pop._fused
    step = [0]

    def update():
        step[0] += 1
        pop.learn(step[0])
    before = samples_of(update)
    nbytes = fused.state_size()

    def save_and_copy():
        fused.save_state(wait=False)
    saved = samples_of(save_and_copy)
    dev, host = fused._state_buffers()
    L, h = fused._L, fused.h

    def save_only():
        assert L.cn_td3_pop_state_save(h, C.c_void_p(dev.data_ptr()), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0

    def load_only():
        assert L.cn_td3_pop_state_load(h, C.c_void_p(dev.data_ptr()), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    launch = samples_of(save_only)
    loaded = samples_of(load_only)
    after = samples_of(update)
    params = [t for a in ags for net in NETS for t in getattr(a, net).parameters()]
    pbytes = sum(t.numel() * 4 for t in params)

    def restated():
        return [t.detach().cpu() for t in params]
    torch_side = samples_of(restated)
    print("P %d: blob %.2f MB (%d bytes), the parameters alone %.2f MB" % (P, nbytes / 1e6, nbytes, pbytes / 1e6), flush=True)
    print("P %d: %s" % (P, line("(a) cn_td3_pop_state_save + copy to pinned", saved)), flush=True)
    print("P %d: %s" % (P, line("(b) PyTorch .cpu() x %d parameter tensors" % len(params), torch_side)), flush=True)
    print("P %d: save + copy %.4f ms for %.2f MB against %.4f ms for %.2f MB: %.2f and %.2f GB/s" % (
        P, saved[0], nbytes / 1e6, torch_side[0], pbytes / 1e6, nbytes / saved[0] / 1e6, pbytes / torch_side[0] / 1e6), flush=True)
    print("P %d: %s" % (P, line("(c) cn_td3_pop_state_save alone", launch)), flush=True)
    print("P %d: %s" % (P, line("(c) cn_td3_pop_state_load", loaded)), flush=True)
    print("P %d: %s" % (P, line("(d) cn_td3_pop_update before the first save", before)), flush=True)
    print("P %d: %s" % (P, line("(d) cn_td3_pop_update after", after)), flush=True)
    del pop, ags, params, fused, dev, host
