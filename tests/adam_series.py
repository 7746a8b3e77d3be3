"""TEST INFRASTRUCTURE.  What the learners' "Adam across four updates" checks share, stated once: the optimiser's turn and the
per-tensor step with their learner-independent wrong variants, and the driver run() that walks a learner -- a device handle, or
a float32 emulation on the CPU -- beside the float64 series.  What is a learner's own (its case, gradients, margins, re-planting,
soft updates and further variants) stays in ddpg_f64.py / sac_f64.py and reaches run() as a record of callables and tables.
test_gpu_td3_f64's four-update test uses tensor_step alone: with policy delay its optimisers do not share a step count."""
import math
from types import SimpleNamespace

import numpy as np
import torch

import td3_f64 as R
from td3_f64 import dead_slices            # noqa: F401 (the series' records use it from here)

UPDATES = 4


def pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(max(x, 2.0 ** -60)))


def series_ratios(got, pred, bound):
    """{(net, name): worst |got - pred| / bound}"""
    return {(n, k): R.worst_ratio(got[n][k], pred[n][k], bound[n][k]) for n in pred for k in pred[n]}


def net_worst(ratios, net, alias=None):
    """The worst ratio over a network's tensors; alias: {name: (net, its tensors' names)} for a part of a network."""
    if alias and net in alias:
        n, names = alias[net]
        return max(ratios[(n, k)] for k in names)
    return max(v for (n, _), v in ratios.items() if n == net)


def new_state(hp, nets):
    """What a series carries from update to update: the shared step count, one td3_f64.Adam64 per optimiser of `nets` (each its
    own lr and moments) and the running element-wise maximum of the gradient bounds."""
    return dict(t=0, opt={n: R.Adam64(hp["lr_" + n], hp["beta1"], hp["beta2"], hp["eps"]) for n in nets}, gerr={})


def optimiser_turn(o, t, net, hp, lr_nets, variant=None):
    """Sets the Adam64 `o` of `net` up for step `t` of the series.  The learner-independent wrong variants: one_lr (the lr of
    lr_nets[0] for every optimiser), betas_exchanged, moments_not_carried, frozen_bias_correction.  -> the t to pass to step()."""
    o.t = t
    o.lr = hp["lr_" + (lr_nets[0] if variant == "one_lr" else net)]
    o.b1, o.b2 = (hp["beta2"], hp["beta1"]) if variant == "betas_exchanged" else (hp["beta1"], hp["beta2"])
    if variant == "moments_not_carried":
        o.m.clear(); o.v.clear()
    return 1 if variant == "frozen_bias_correction" else None


def tensor_step(o, gerr, net, k, w0, g, gbound, eps, t=None):
    """One tensor's step: gerr[(net, k)] becomes the running maximum of the gradient bounds so far, Adam64 steps w0 by g
    -> (w1, td3_f64.adam_step_bound of it)."""
    ge = gerr[(net, k)] = torch.maximum(gerr.get((net, k), torch.zeros_like(gbound)), gbound)
    w1, ratio = o.step(k, w0, g, t=t)
    return w1, R.adam_step_bound(w1, ratio, o.lr, eps, ge)


def emulated_adam(P, mom, t, hp, net_names, grad):
    """td3_f64.adam_f32_emulation over every (net, name) of net_names, in place on the float32 CPU tensors P with the moments
    carried in `mom`; grad(net, name): the float64 gradient, rounded to float32 here."""
    for net, names in net_names:
        for k in names:
            m0, v0 = mom.get((net, k), (None, None))
            w1, m, v = R.adam_f32_emulation(P[net][k].numpy(), grad(net, k).float().numpy(), hp["lr_" + net], hp["eps"], hp["beta1"], hp["beta2"],
                                            m0, v0, t)
            mom[(net, k)] = (m, v)
            P[net][k] = torch.from_numpy(w1)


def soft_f32(t, w, tau):
    """t (1 - tau) + w tau in float32, as the kernels' soft update rounds it."""
    f = np.float32
    return torch.from_numpy((t.numpy() * (f(1) - f(tau)) + w.numpy() * f(tau)).astype(f))


def series(**kw):
    """A learner's record for run():
      tag, shape         the case's label in messages; what make_learner gets
      case()             -> the initial float32 parameters P
      reference(P)       the float64 gradients (and whatever else step needs) at the float32 parameters P
      hp(ref)            the hyper-parameters, from the first update's reference
      lr_nets, local     the networks with an optimiser: in the order of the lr line, the first one's lr being one_lr's; in the
                         order of the new handle's line
      state(hp), step(state, P64, ref, hp, variant) -> (pred, bound)
      replant(P)         before every update after the first, in place on P
      margins_ok(P), top(ref)   no ambiguous mask at P; the largest gradient element
      inputs()           update()'s arguments
      frozen(P), frozen_msg     the tensors of P that must keep every bit, and what to say if one does not
      before(u, ref), after(u, post)   further assertions per update (or None)
      variants, rules    the wrong variants and {variant: (the first update at which it can differ, the nets it concerns)}
      report, alias      the nets whose worst ratio is reported; net_worst's alias map"""
    return SimpleNamespace(**kw)


def run(s, make_learner, log=print):
    """UPDATES updates of `make_learner(P, shape, hp)` -- read() -> its float32 tensors (copies), write(P), update(*inputs),
    close() -- beside the float64 series of the record `s` (series()), margins re-planted on the learner's weights before every
    update after the first; then a NEW learner on the stepped parameters for one more update (fresh state at create).  Asserts,
    per update: no ambiguous mask; eps >= every gradient element; every tensor within the series' bound; every wrong variant
    rejected on each network it concerns from the update at which it can differ; the frozen tensors bit for bit.
    -> dict(worst={net: ratio}, rejected={variant: smallest rejecting ratio}, hp)."""
    tag, worst_of = s.tag, lambda ratios, n: net_worst(ratios, n, s.alias)
    P = s.case()
    ref = s.reference(P)
    hp = s.hp(ref)
    assert len({hp["lr_" + n] for n in s.lr_nets}) == len(s.lr_nets)
    log("%s: lr %s, eps %g" % (tag, " ".join("%s %g" % (n, hp["lr_" + n]) for n in s.lr_nets), hp["eps"]))
    right, wrong = s.state(hp), {v: s.state(hp) for v in s.variants}
    worst, rejected = {}, {}
    zeros0 = None
    be = make_learner(P, s.shape, hp)
    try:
        for u in range(UPDATES + 1):
            if u == UPDATES:                                   # fresh state at create: a new learner on the stepped parameters
                stepped = be.read()
                be.close()
                be = make_learner(stepped, s.shape, hp)
            cur = be.read()
            if u:
                s.replant(cur)
                be.write(cur)
                ref = s.reference(cur)
            P64 = R.to64(cur)
            assert s.margins_ok(cur), (tag, u, "margins")
            top = s.top(ref)
            assert top <= hp["eps"], (tag, u, "eps %g below the largest gradient element %g" % (hp["eps"], top))
            if s.before:
                s.before(u, ref)
            zeros0 = [x.clone() for x in s.frozen(cur)] if zeros0 is None else zeros0
            be.update(*s.inputs())
            post = be.read()
            got = R.to64(post)
            assert all(torch.equal(a_, b_) for a_, b_ in zip(s.frozen(post), zeros0)), (tag, u, s.frozen_msg)
            if u == UPDATES:
                fresh = series_ratios(got, *s.step(s.state(hp), P64, ref, hp, None))
                carried = series_ratios(got, *s.step(right, P64, ref, hp, None))
                log("%s: new handle: fresh Adam %.3g, the carried one %s" % (tag, max(fresh.values()), {n: "%.3g" % worst_of(carried, n) for n in s.local}))
                assert max(fresh.values()) <= 1.0, (tag, "fresh state at create", fresh)
                for n in s.local:
                    assert worst_of(carried, n) > 1.0, (tag, "carried state accepted after create", n)
                    rejected["carried_after_create"] = min(rejected.get("carried_after_create", math.inf), worst_of(carried, n))
                break
            ratios = series_ratios(got, *s.step(right, P64, ref, hp, None))
            for n in s.report:
                worst[n] = max(worst.get(n, 0.0), worst_of(ratios, n))
            log("%s: update %d worst/bound %s" % (tag, u, {n: "%.3g" % worst_of(ratios, n) for n in s.report}))
            assert max(ratios.values()) <= 1.0, (tag, u, {k: v for k, v in ratios.items() if v > 1.0})
            for var in s.variants:
                rv = series_ratios(got, *s.step(wrong[var], P64, ref, hp, var))
                first, nets = s.rules[var]
                if u < first:
                    continue
                per = {n: worst_of(rv, n) for n in nets}
                log("%s: update %d %s %s" % (tag, u, var, {n: "%.3g" % v for n, v in per.items()}))
                for n, v in per.items():
                    assert v > 1.0, (tag, u, var, n, v)
                    rejected[var] = min(rejected.get(var, math.inf), v)
            if s.after:
                s.after(u, post)
    finally:
        be.close()
    return dict(worst=worst, rejected=rejected, hp=hp)
