"""A float64 statement of one TD3 update (crowdnav.td3.Agent._update, td3.py:225-285 of the reference) and the tools the
tests of the fused update (csrc/crowdnav_td3.hip; its kernels: csrc/crowdnav_gemm.hip) use to compare float32 kernel output with it:

- the reference: forward passes, the TD target, the critics' MSE gradients, the actor's -mean Q1(s, pi(s)) gradient, Adam and
  the soft update, in float64 with torch autograd (no kernel code, no libcrowdnav);
- error bounds derived from the arithmetic: every quantity gets a MAGNITUDE -- the same expression evaluated on absolute values
  (|W|, |x|, |b|, the ReLU masks of the real network, subtraction turned into addition) -- and a float32 evaluation of it in any
  summation order is within N u M of the exact value, u = 2^-24, N = the number of roundings on the longest dependency chain
  (the sum of the reduction lengths from the batch to that quantity, chain_length()) -- the ReLU masks use this strict form;
  gradients are compared at a rounding-error estimate propagated through the signed Jacobians (see LAMBDA);
- the "invertible Adam" configuration (beta1 = beta2 = 0): the kernel's step becomes w' = w - lr g / (|g| + eps), which is
  inverted per element to recover the gradient the kernel used;
- ReLU margins: biases shifted so that no pre-activation lies within its rounding bound of zero (every mask is the same in
  float32 and float64, whatever the order), and planted dead units (zero row, zero bias: exactly 0 in any order).

Device-agnostic: the CPU tests run it on small shapes, the GPU tests on the device in float64."""
import math

import torch

U = 2.0 ** -24                     # unit roundoff of float32 (round to nearest)
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
NETS = ("actor", "actor_t", "q1", "q1_t", "q2", "q2_t")
LOCAL = ("actor", "q1", "q2")
# Gradient tolerance: a rounding-error estimate propagated through the network's SIGNED Jacobians (propagated_bounds below).
# Local model (Higham & Mary's probabilistic rounding analysis): a float32 product C = A B of reduction length K, in any order,
# leaves err = sum_k delta_k s_k + sum_i delta'_i a_i b_i with |delta| <= u, independent and mean zero, s_k the partial sums.
# Its standard deviation is <= u / sqrt(3) (sqrt(sum s_k^2) + sqrt(sum (a_i b_i)^2)) <= u (sqrt(K) + 1) (|A||B|) elementwise
# (every |s_k| <= sum |a_i b_i|); an elementwise operation leaves <= u |result| (4 u for expf / tanhf).  Every product and
# elementwise result of a float64 restatement of the kernel's forward and backward passes gets a Gaussian perturbation of that
# standard deviation, the masks held at the unperturbed run's; the change of each gradient element over SAMPLES such runs
# estimates the standard deviation s of its float32 error with the cancellations of the real network (the old bound summed
# |.| through every layer, 30x to 1e5x too wide).  Tolerance = LAMBDA x the sample RMS: with 32 samples the RMS is >= 0.4 s
# except with probability P(chi2_32 < 5.12) < 1e-7, so LAMBDA = 16 is >= 6.4 s, and s itself is an upper estimate
# (|s_k| <= sum |a b| is the worst partial sum).
SAMPLES = 32
LAMBDA = 16.0


def chain_length(obs_dim, hidden, batch):
    """Roundings on the longest chain of one update: the target actor (D + 2H to the logits), the target critic (Dc + 2H),
    the data gradient through a critic (H), the actor-loss chain back through Q1 and the actor (3H), a weight gradient's sum
    over the batch (B), and 64 spare for the heads, the TD target, the partial-sum tiles and the cross-wavefront sums."""
    return 2 * (obs_dim + 2) + 6 * hidden + batch + 64


# ---- networks --------------------------------------------------------------------------------------------------------------
def new_params(obs_dim, hidden, gen, dtype=torch.float64, device="cpu"):
    """nn.Linear's default initialisation (uniform +-1/sqrt(fan_in)) for the six networks, as float32 values."""
    def lin(i, o):
        k = 1.0 / math.sqrt(i)
        w = (torch.rand((o, i), generator=gen, dtype=torch.float64) * 2 - 1) * k
        b = (torch.rand((o,), generator=gen, dtype=torch.float64) * 2 - 1) * k
        return [w.float().to(dtype).to(device), b.float().to(dtype).to(device)]
    P = {}
    for n in NETS:
        i0 = obs_dim if n.startswith("actor") else obs_dim + 2
        o3 = 2 if n.startswith("actor") else 1
        P[n] = dict(zip(NAMES, lin(i0, hidden) + lin(hidden, hidden) + lin(hidden, o3)))
    return P


def to64(P):
    return {n: {k: v.detach().to(torch.float64) for k, v in p.items()} for n, p in P.items()}


def _mlp(p, x, xm=None):
    """Forward pass of one 3-layer MLP; with magnitudes xm of the input: the magnitudes of every pre-activation too."""
    z1 = x @ p["w1"].T + p["b1"]
    h1 = torch.relu(z1)
    z2 = h1 @ p["w2"].T + p["b2"]
    h2 = torch.relu(z2)
    out = h2 @ p["w3"].T + p["b3"]
    f = dict(z1=z1, h1=h1, z2=z2, h2=h2, out=out)
    if xm is not None:
        m1 = xm @ p["w1"].abs().T + p["b1"].abs()
        mh1 = m1 * (z1 > 0)
        m2 = mh1 @ p["w2"].abs().T + p["b2"].abs()
        mh2 = m2 * (z2 > 0)
        f.update(m_z1=m1, m_h1=mh1, m_z2=m2, m_h2=mh2, m_out=mh2 @ p["w3"].abs().T + p["b3"].abs())
    return f


def head_derivs(logits, max_v, max_w):
    s = torch.sigmoid(logits[:, 0])
    t = torch.tanh(logits[:, 1])
    return torch.stack([max_v * s * (1 - s), max_w * (1 - t * t)], 1)


def actor_fwd(p, s, cfg, with_mag=True):
    """Actor.forward (td3.py:101-105): (sigmoid(l0) max_v, tanh(l1) max_w).  m_act folds the logits' error through the heads:
    err(act) <= |head'| err(logit) + 4 u |act| <= N u (|head'| M(logit) + |act|)."""
    f = _mlp(p, s, s.abs() if with_mag else None)
    lg = f["out"]
    f["logits"] = lg
    f["act"] = torch.stack([torch.sigmoid(lg[:, 0]) * cfg["max_v"], torch.tanh(lg[:, 1]) * cfg["max_w"]], 1)
    f["hd"] = head_derivs(lg, cfg["max_v"], cfg["max_w"])
    if with_mag:
        f["m_act"] = f["act"].abs() + f["hd"] * f["m_out"]
    return f


def target_noise(noise, cfg):
    """TD3:241-242: clamp(noise std, +-clip).  noise_std is a power of two in these tests, so the float32 product is exact."""
    return (noise * cfg["noise_std"]).clamp(-cfg["noise_clip"], cfg["noise_clip"])


def td_target(P, batch, cfg, y_from="min"):
    """y = r + (1 - d) gamma min(Q1_t, Q2_t)(s2, actor_t(s2) + clipped noise) and its magnitude.  y_from="q1t": the wrong
    variant that takes Q1_t alone."""
    s, a, r, s2, d, nz = batch
    ft = actor_fwd(P["actor_t"], s2, cfg)
    noise = target_noise(nz, cfg)
    a2 = ft["act"] + noise
    x2 = torch.cat([s2, a2], 1)
    xm2 = torch.cat([s2.abs(), ft["m_act"] + noise.abs()], 1)
    f1, f2 = _mlp(P["q1_t"], x2, xm2), _mlp(P["q2_t"], x2, xm2)
    q1t, q2t = f1["out"][:, 0], f2["out"][:, 0]
    y = r + (1 - d) * cfg["gamma"] * (torch.minimum(q1t, q2t) if y_from == "min" else q1t)
    m_y = r.abs() + (1 - d) * cfg["gamma"] * torch.maximum(f1["m_out"][:, 0], f2["m_out"][:, 0])
    return dict(y=y, m_y=m_y, q1t=q1t, q2t=q2t, a2=a2, m_a2=xm2[:, -2:], ft=ft)


def _grad_of(fn, p):
    """autograd gradient of fn(params) with respect to the six tensors of p."""
    ps = {k: p[k].detach().clone().requires_grad_(True) for k in NAMES}
    out = fn(ps)
    g = torch.autograd.grad(out, [ps[k] for k in NAMES])
    return dict(zip(NAMES, [x.detach() for x in g])), out.detach()


def _abs_grad(p, xm, masks, seed):
    """Magnitudes of the weight gradients of sum(seed * out): the gradient of the same network on |W|, |b|, input magnitudes
    xm with the real network's ReLU masks held fixed (every product of the backward pass then sums non-negative terms)."""
    m1, m2 = masks[0].double(), masks[1].double()
    xm, seed = xm.double(), seed.double()

    def fn(ps):
        h1 = (xm @ ps["w1"].T + ps["b1"]) * m1
        h2 = (h1 @ ps["w2"].T + ps["b2"]) * m2
        return ((h2 @ ps["w3"].T + ps["b3"]) * seed).sum()
    g, _ = _grad_of(fn, {k: v.double().abs() for k, v in p.items()})
    return g


def critic_grads(P, batch, cfg, y_from="min"):
    """The two critic steps' gradients (TD3:249-260) at P: {q1, q2: {g: {name: g}, bound: {name: LAMBDA x propagated RMS}}},
    the loss l1 and the TD target's pieces (t) for the tests' coverage checks.  g by autograd; the bound by propagated_bounds
    (whose own exact pass, a hand-written backward, must agree with autograd: test_td3_f64_helpers)."""
    s, a, r, s2, d, nz = batch
    with torch.no_grad():
        t = td_target(P, batch, cfg, y_from)
    x = torch.cat([s, a], 1)
    out = dict(t=t)
    _, bnd = propagated_bounds(lambda ps: {(n, k): v for n, g in ps.critics(P, batch, cfg, y_from).items() for k, v in g.items()})
    for net in ("q1", "q2"):
        g, loss = _grad_of(lambda ps: ((_mlp(ps, x)["out"][:, 0] - t["y"]) ** 2).mean(), P[net])
        out[net] = dict(g=g, bound={k: bnd[(net, k)] for k in NAMES}, loss=loss, q=_mlp(P[net], x)["out"][:, 0])
    out["l1"] = out["q1"]["loss"]
    return out


def actor_grads(P, s, cfg, q1=None, N_mask=None):
    """The actor step's gradient (TD3:268-269), d(-mean Q1(s, pi(s)))/d actor, through the critic q1 (default P["q1"]; the
    multi-step test passes the critic the kernel stepped in the same update), with its per-tensor bounds.  A unit of q1 whose
    pre-activation lies within its rounding bound of zero (possible only for a critic whose biases were not placed by
    establish_margins) may take either mask in float32: its whole contribution to da is added to the bound (flip_rows counts
    the rows where that happens)."""
    q1 = P["q1"] if q1 is None else q1
    B = s.shape[0]
    g, _ = _grad_of(lambda ps: -_mlp(q1, torch.cat([s, actor_fwd(ps, s, cfg, False)["act"]], 1))["out"].mean(), P["actor"])
    fa = actor_fwd(P["actor"], s, cfg)
    xq = torch.cat([s, fa["act"]], 1)
    xqm = torch.cat([s.abs(), fa["m_act"]], 1)
    fq = _mlp(q1, xq, xqm)
    qa = {k: v.double().abs() for k, v in q1.items()}
    xqm = xqm.double()

    def m_da(m1, m2):       # magnitude of da = d(mean Q1)/d action through |W| with the masks m1, m2
        xm = xqm.clone().requires_grad_(True)
        qabs = (((xm @ qa["w1"].T + qa["b1"]) * m1) @ qa["w2"].T + qa["b2"]) * m2 @ qa["w3"].T
        return torch.autograd.grad(qabs.sum() / B, xm)[0][:, -2:].detach()
    on1, on2 = (fq["z1"] > 0).double(), (fq["z2"] > 0).double()
    Nm = chain_length(s.shape[1], q1["w2"].shape[0], B) if N_mask is None else N_mask
    amb1 = (fq["z1"].abs() < Nm * U * fq["m_z1"]).double()
    amb2 = (fq["z2"].abs() < Nm * U * fq["m_z2"]).double()
    flip = m_da(torch.maximum(on1, amb1), torch.maximum(on2, amb2)) - m_da(on1 * (1 - amb1), on2 * (1 - amb2))
    _, bnd = propagated_bounds(lambda ps: ps.actor(P, s, cfg, q1))
    mg = _abs_grad(P["actor"], s.abs(), ((fa["z1"] > 0).double(), (fa["z2"] > 0).double()), fa["hd"] * flip)
    mg = {k: bnd[k] + mg[k] for k in NAMES}
    flip_rows = int(((amb1.sum(1) + amb2.sum(1)) > 0).sum())
    return dict(g=g, bound=mg, logits=fa["logits"], flip_rows=flip_rows)


# ---- rounding errors through the signed Jacobians ---------------------------------------------------------------------------
class _Pass:
    """One float64 evaluation of the kernel's arithmetic, optionally with every rounding replaced by a Gaussian perturbation of
    the local model's standard deviation (gen = None: exact; the ReLU masks are recorded then and reused)."""

    def __init__(self, gen=None, masks=None):
        self.gen, self.masks = gen, {} if masks is None else masks

    def _noise(self, x, sd):
        if self.gen is None:
            return x
        return x + sd * torch.randn(x.shape, generator=self.gen, dtype=x.dtype, device=x.device)

    def mm(self, A, B):                          # A [m][K] @ B [K][n]
        return self._noise(A @ B, U * (math.sqrt(A.shape[-1]) + 1) * (A.abs() @ B.abs()))

    def ew(self, x, ulps=1.0):
        return self._noise(x, ulps * U * x.abs())

    def mask(self, key, z):
        if self.gen is None:
            self.masks[key] = (z > 0).to(z.dtype)
        return self.masks[key]

    def mlp(self, p, x, key):
        ones = torch.ones((x.shape[0], 1), dtype=x.dtype, device=x.device)
        lin = lambda h, w, b: self.mm(torch.cat([h, ones], 1), torch.cat([w, b[:, None]], 1).T)   # (the bias: one more term)
        z1 = lin(x, p["w1"], p["b1"]); h1 = z1 * self.mask(key + ".1", z1)
        z2 = lin(h1, p["w2"], p["b2"]); h2 = z2 * self.mask(key + ".2", z2)
        return dict(z1=z1, z2=z2, h1=h1, h2=h2, out=lin(h2, p["w3"], p["b3"]), m1=self.masks[key + ".1"], m2=self.masks[key + ".2"])

    def heads(self, lg, cfg):
        """actions and head derivatives.  The derivatives are max_v s (1 - s) and max_w (1 - t^2): near saturation 1 - s and
        1 - t^2 cancel, and the float32 roundings of s (<= 4 u s: expf, the division) and t (<= 4 u |t|: tanhf) land on them
        as absolute errors -- max_v s 4 u s and max_w 2 t 4 u |t| (+ u t^2 of the square), up to ~1e3 u relative at |logit| 8."""
        s, th = torch.sigmoid(lg[:, 0]), torch.tanh(lg[:, 1])
        act = torch.stack([s * cfg["max_v"], th * cfg["max_w"]], 1)
        hd = head_derivs(lg, cfg["max_v"], cfg["max_w"])
        sd_hd = U * torch.stack([4 * hd[:, 0].abs() + 4 * cfg["max_v"] * s * s, 4 * hd[:, 1].abs() + 9 * cfg["max_w"] * th * th], 1)
        return self.ew(act, 4.0), self._noise(hd, sd_hd)

    def wgrad(self, dz, x, f=None):               # dW = dz^T x, db = sum over rows of dz
        ones = torch.ones((x.shape[0], 1), dtype=x.dtype, device=x.device)
        return self.mm(dz.T, x), self.mm(dz.T, ones)[:, 0]

    def backward(self, p, x, f, dout):
        """weight gradients of a 3-layer MLP given d(loss)/d(out) = dout [B][out]."""
        g = {}
        g["w3"], g["b3"] = self.wgrad(dout, f["h2"])
        dz2 = self.mm(dout, p["w3"]) * f["m2"]
        g["w2"], g["b2"] = self.wgrad(dz2, f["h1"])
        dz1 = self.mm(dz2, p["w2"]) * f["m1"]
        g["w1"], g["b1"] = self.wgrad(dz1, x)
        return g, dz1

    def critics(self, P, batch, cfg, y_from="min"):
        s, a, r, s2, d, nz = batch
        B = s.shape[0]
        ft = self.mlp(P["actor_t"], s2, "actor_t")
        act, _ = self.heads(ft["out"], cfg)
        x2 = torch.cat([s2, self.ew(act + target_noise(nz, cfg))], 1)
        q1t, q2t = self.mlp(P["q1_t"], x2, "q1_t")["out"][:, 0], self.mlp(P["q2_t"], x2, "q2_t")["out"][:, 0]
        y = self.ew(r + self.ew((1 - d) * cfg["gamma"] * (torch.minimum(q1t, q2t) if y_from == "min" else q1t), 2.0))
        x = torch.cat([s, a], 1)
        out = {}
        for net in ("q1", "q2"):
            f = self.mlp(P[net], x, net)
            dq = self.ew(2.0 * self.ew(f["out"][:, 0] - y) / B, 2.0)
            out[net], _ = self.backward(P[net], x, f, dq[:, None])
        return out

    def actor(self, P, s, cfg, q1):
        B, D = s.shape
        fa = self.mlp(P["actor"], s, "actor")
        act, hd = self.heads(fa["out"], cfg)
        xq = torch.cat([s, act], 1)
        fq = self.mlp(q1, xq, "q1pi")
        dz2 = self.ew(-q1["w3"] / B).expand(B, -1) * fq["m2"]
        dz1 = self.mm(dz2, q1["w2"]) * fq["m1"]
        da = self.mm(dz1, q1["w1"][:, D:])
        g, _ = self.backward(P["actor"], s, fa, self.ew(da * hd))
        return g


def propagated_bounds(run, samples=SAMPLES, seed=0, device=None):
    """run(_Pass) -> {name: tensor}.  Returns (exact values, LAMBDA x RMS over `samples` perturbed runs of their change)."""
    exact_pass = _Pass()
    exact = run(exact_pass)
    dev = next(iter(exact.values())).device
    gen = torch.Generator(device=dev).manual_seed(seed)
    acc = {k: torch.zeros_like(v) for k, v in exact.items()}
    for _ in range(samples):
        pert = run(_Pass(gen, exact_pass.masks))
        for k in acc:
            acc[k] += (pert[k] - exact[k]) ** 2
    return exact, {k: LAMBDA * (v / samples).sqrt() for k, v in acc.items()}


# ---- Adam ----------------------------------------------------------------------------------------------------------------
def invert_step(w, w_new, lr, eps):
    """The kernel's step with beta1 = beta2 = 0 is w' = w - lr g / (|g| + eps) (adam0 = lr, adam1 = 1): with u = (w - w') / lr,
    g = eps u / (1 - |u|).  Exact in float64 given the two float32 values."""
    u = (w.double() - w_new.double()) / lr
    return eps * u / (1 - u.abs())


def inversion_bound(g, w, w_new, lr, eps):
    """What float32 rounding of w' = fl(w - fl(lr g / fl(fl(sqrt(fl(g g))) + eps))) leaves in the recovered g: <= 4 relative
    roundings of the step (|u| <= 1/2 doubles them through 1 / (1 - |u|)) and the final subtraction's half-ulp of |w'|, which is
    absolute: u (|w| + |w'|) eps / lr, quadrupled by the inversion's conditioning at |u| <= 1/2."""
    return 10 * U * g.abs() + 4 * U * (w.double().abs() + w_new.double().abs()) * eps / lr


def adam_f32_emulation(w, g, lr, eps, beta1=0.0, beta2=0.0, m0=None, v0=None, t=1):
    """numpy float32 emulation of the kernel's Adam formula (td3_wgrad_kernel): m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g g,
    w' = w - adam0 m / (sqrt(v) / adam1 + eps) with adam0 = lr / (1 - b1^t), adam1 = sqrt(1 - b2^t)."""
    import numpy as np
    f = np.float32
    w, g = w.astype(f), g.astype(f)
    m0 = np.zeros_like(w) if m0 is None else m0.astype(f)
    v0 = np.zeros_like(w) if v0 is None else v0.astype(f)
    m = f(beta1) * m0 + f(1 - beta1) * g
    v = f(beta2) * v0 + f(1 - beta2) * g * g
    adam0 = f(lr) / f(1.0 - float(beta1) ** t)
    adam1 = np.sqrt(f(1.0 - float(beta2) ** t))
    return (w - adam0 * m / (np.sqrt(v) / adam1 + f(eps))).astype(f), m, v


class Adam64:
    """float64 Adam (bias-corrected) with the kernel's formula, one per optimizer: step counts and moments carried here."""

    def __init__(self, lr, beta1, beta2, eps):
        self.lr, self.b1, self.b2, self.eps, self.t, self.m, self.v = lr, beta1, beta2, eps, 0, {}, {}

    def step(self, key, w, g, t=None):
        """w' for this tensor; t overrides the bias-correction step (the wrong-variant checks)."""
        m = self.b1 * self.m.get(key, torch.zeros_like(g)) + (1 - self.b1) * g
        v = self.b2 * self.v.get(key, torch.zeros_like(g)) + (1 - self.b2) * g * g
        tt = self.t if t is None else t
        mh, vh = m / (1 - self.b1 ** tt), v / (1 - self.b2 ** tt)
        self.m[key], self.v[key] = m, v
        return w - self.lr * mh / (vh.sqrt() + self.eps), mh / (vh.sqrt() + self.eps)


def adam_step_bound(w_new, ratio, lr, eps, gerr):
    """Error of the kernel's w' against Adam64's, given per-element bounds gerr >= the largest error of any gradient that
    entered the moments: m-hat and sqrt(v-hat) are weighted means (of g, and in the l2 sense of |g|), so each moves by <= gerr;
    with eps >= max |g| the step lr m / (sqrt v + eps) moves by <= 2 lr gerr / eps; plus float32 rounding of the formula:
    <= 8 u of the step and one half-ulp of w' (doubled for the float32 moments' own rounding)."""
    return 2 * lr * gerr / eps + 8 * U * lr * ratio.abs() + 2 * U * w_new.abs()


def soft_update(t, w, tau):
    return t * (1 - tau) + w * tau


def soft_bound(t, w, tau):
    """float32 target (1 - tau) + local tau with tau a power of two (local tau and 1 - tau exact): two roundings."""
    return 2 * U * (t.abs() + (w * tau).abs()) + 1e-45


# ---- comparison --------------------------------------------------------------------------------------------------------------
def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 counts as 0)."""
    diff = (got.double() - want.double()).abs()
    r = torch.where(bound > 0, diff / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(diff > 0, torch.full_like(diff, math.inf), torch.zeros_like(diff)))
    return float(r.max()) if r.numel() else 0.0


def compare_grads(got, want, bound, extra=None):
    """{name: worst |got - want| / (bound + extra)} for the six tensors of a network."""
    return {k: worst_ratio(got[k], want[k], bound[k] + (extra[k] if extra is not None else 0.0)) for k in NAMES}


def recover(P0, P1, net, lr, eps):
    """(the gradients invert_step reads from net's step P0 -> P1, their inversion bounds), per tensor."""
    g = {k: invert_step(P0[net][k], P1[net][k], lr, eps) for k in NAMES}
    return g, {k: inversion_bound(g[k], P0[net][k], P1[net][k], lr, eps) for k in NAMES}


def accept(ratios):
    return max(ratios.values()) <= 1.0


def same(P0, P1, net):
    return all(torch.equal(P0[net][k], P1[net][k]) for k in NAMES)


def rejects_gross(g, ref, extra, net):
    """at every shape: a zero gradient (a network that is never stepped) and one twice too large are rejected"""
    if any(bool((v != 0).any()) for v in ref["g"].values()):
        assert not accept(compare_grads(g, {k: torch.zeros_like(v) for k, v in ref["g"].items()}, ref["bound"], extra)), net
        assert not accept(compare_grads(g, {k: 2 * v for k, v in ref["g"].items()}, ref["bound"], extra)), net


def zero_tile(g, i0=0, j0=0, size=16):
    g = g.clone()
    if g.dim() == 2:
        g[i0:i0 + size, j0:j0 + size] = 0
    else:
        g[i0:i0 + size] = 0
    return g


# ---- ReLU margins -------------------------------------------------------------------------------------------------------------
def plant_dead_units(P, hidden, nets=LOCAL):
    """Unit 1 of the first and unit hidden - 2 of the second hidden layer of each local network (`nets`) get a zero weight row and
    a zero bias: their pre-activation is exactly 0 in any summation order, so nothing flows through them (hidden >= 4).  Returns
    {net: (unit of layer 1, unit of layer 2)}."""
    if hidden < 4:
        return {}
    dead = {}
    for n in nets:
        u1, u2 = 1, hidden - 2
        P[n]["w1"][u1].zero_(); P[n]["b1"][u1] = 0
        P[n]["w2"][u2].zero_(); P[n]["b2"][u2] = 0
        dead[n] = (u1, u2)
    return dead


def dead_slices(p, dead):
    """The slices of a network's six tensors that its dead pair of units owns (in and out): each must keep every bit."""
    u1, u2 = dead
    return [p["w1"][u1], p["b1"][u1], p["w2"][:, u1], p["w2"][u2], p["b2"][u2], p["w3"][:, u2]]


def check_dead(P0, P1, net, dead):
    if net not in dead:
        return
    for a, b in zip(dead_slices(P0[net], dead[net]), dead_slices(P1[net], dead[net])):
        assert torch.equal(a, b), net


def _is_dead(w, b):
    return (w == 0).all(1) & (b == 0)


def _choose_bias(p, e_rel, nu):
    """Per unit (column) of the bias-free products p [rows][units] and their bounds e_rel = N u |x||W|: a threshold t such that
    |p - t| >= e_rel + (N u + 2 u) |t| for every row -- the new bias -t (rounded to float32: the 2 u) leaves no pre-activation
    within its bound N u (|x||W| + |b|).  Candidates: the midpoints of the 64 widest row-free gaps, and one point below and one
    above all rows.  Among the valid ones the one closest to the median row (the most mixed mask) wins.
    Returns (t, mixed: the chosen threshold splits the rows, feasible: some candidate is valid)."""
    rows, units = p.shape
    ps, order = p.sort(0)
    es = torch.gather(e_rel, 0, order)
    k = nu + 2 * U
    pad = 2 * (e_rel.max(0).values + k * ps.abs().max(0).values) + 1e-300
    ends = torch.stack([ps[0] - pad, ps[-1] + pad], 0)
    cand, below = [ends], [torch.zeros_like(ps[:1]), torch.full_like(ps[:1], rows)]
    below = torch.cat(below, 0)
    if rows > 1:
        width = (ps[1:] - ps[:-1]) - es[1:] - es[:-1]
        kk = min(64, rows - 1)
        gi = width.topk(kk, 0).indices                                                 # [kk][units]
        mid = 0.5 * (torch.gather(ps, 0, gi) + torch.gather(ps, 0, gi + 1))
        cand.append(mid)
        below = torch.cat([below, (gi + 1).to(ps.dtype)], 0)
    cand = torch.cat(cand, 0)                                                          # [c][units]
    ok = torch.empty(cand.shape, dtype=torch.bool, device=p.device)
    step = max(1, int(2 ** 24 // max(1, rows * units)))
    for c0 in range(0, cand.shape[0], step):
        c = cand[c0:c0 + step]
        ok[c0:c0 + step] = ((p[None] - c[:, None]).abs() >= e_rel[None] + k * c[:, None].abs()).all(1)
    score = (below - rows / 2).abs() + torch.where(ok, 0.0, math.inf)
    best = score.argmin(0)
    t = torch.gather(cand, 0, best[None])[0]
    nb = torch.gather(below, 0, best[None])[0]
    mixed = ok.gather(0, best[None])[0] & (nb > 0) & (nb < rows)
    return t, mixed, ok.any(0)


def _layer_margins(w, b, xs, xms, N):
    """Shift the biases of one layer (w [units][in], b [units], float32, in place) evaluated on the row sets xs (magnitudes xms)."""
    x = torch.cat(xs, 0)
    xm = torch.cat(xms, 0)
    prod = x @ w.double().T
    e_rel = N * U * (xm @ w.double().abs().T)
    dead = _is_dead(w, b)
    t, mixed, feas = _choose_bias(prod, e_rel, N * U)
    b.copy_(torch.where(dead, torch.zeros_like(t), -t).to(b.dtype))
    return dict(mixed=int((mixed & ~dead).sum()), units=int((~dead).sum()), infeasible=int((~feas & ~dead).sum()))


def establish_margins(P, batch, cfg, N, logit_scale=8.0, rescale=True):
    """Scale both policies' last layers so that the logits reach +-logit_scale (the heads near saturation), then shift every
    hidden unit's bias, layer by layer and network by network in the order the rows depend on each other (actor on s, actor_t on
    s2, Q1 on (s, a) and (s, pi(s)), Q2 on (s, a), the targets on (s2, a2)), so that no pre-activation of any row the kernel
    evaluates lies within its rounding bound of zero.  Dead units stay dead.  Modifies P's float32 tensors in place; returns a
    per-layer report.  Afterwards Q2_t's output bias is moved so that min(Q1_t, Q2_t) picks each side in about half the rows.
    rescale=False (re-establishing the margins between updates): only the hidden biases move."""
    s, a, r, s2, d, nz = [x.double() for x in batch]
    rep = {}

    def net_margins(name, xs, xms):
        p = P[name]
        rep[name + ".1"] = _layer_margins(p["w1"], p["b1"], xs, xms, N)
        p64 = {k: v.double() for k, v in p.items()}
        h = [_mlp(p64, x, xm) for x, xm in zip(xs, xms)]
        rep[name + ".2"] = _layer_margins(p["w2"], p["b2"], [f["h1"] for f in h], [f["m_h1"] for f in h], N)

    for name, x in (("actor", s), ("actor_t", s2)):
        net_margins(name, [x], [x.abs()])
        p64 = {k: v.double() for k, v in P[name].items()}
        lg = _mlp(p64, x)["out"]
        if rescale:
            P[name]["w3"].mul_(logit_scale / max(float((lg - p64["b3"]).abs().max()), 1e-30))
    P64 = to64(P)
    fa = actor_fwd(P64["actor"], s, cfg)
    ft = actor_fwd(P64["actor_t"], s2, cfg)
    noise = target_noise(nz, cfg)
    xsa, xsam = torch.cat([s, a], 1), torch.cat([s, a], 1).abs()
    xpi, xpim = torch.cat([s, fa["act"]], 1), torch.cat([s.abs(), fa["m_act"]], 1)
    x2, x2m = torch.cat([s2, ft["act"] + noise], 1), torch.cat([s2.abs(), ft["m_act"] + noise.abs()], 1)
    net_margins("q1", [xsa, xpi], [xsam, xpim])
    net_margins("q2", [xsa], [xsam])
    net_margins("q1_t", [x2], [x2m])
    net_margins("q2_t", [x2], [x2m])
    P64 = to64(P)
    t = td_target(P64, batch_double(batch), cfg)
    if rescale:
        P["q2_t"]["b3"].sub_(float((t["q2t"] - t["q1t"]).median()))
    return rep


def batch_double(batch):
    return tuple(x.double() for x in batch)


def margin_report(P, batch, cfg, N):
    """min over every non-dead unit and every row the kernel evaluates it on of |pre-activation| / bound (>= 1: no mask is
    ambiguous), and the number of dead units seen.  The pre-activations' bounds include the input columns' own errors."""
    s, a, r, s2, d, nz = batch_double(batch)
    P64 = to64(P)
    fa = actor_fwd(P64["actor"], s, cfg)
    ft = actor_fwd(P64["actor_t"], s2, cfg)
    noise = target_noise(nz, cfg)
    rows = dict(actor=[(s, s.abs())], actor_t=[(s2, s2.abs())],
                q1=[(torch.cat([s, a], 1), torch.cat([s, a], 1).abs()), (torch.cat([s, fa["act"]], 1), torch.cat([s.abs(), fa["m_act"]], 1))],
                q2=[(torch.cat([s, a], 1), torch.cat([s, a], 1).abs())])
    rows["q1_t"] = rows["q2_t"] = [(torch.cat([s2, ft["act"] + noise], 1), torch.cat([s2.abs(), ft["m_act"] + noise.abs()], 1))]
    worst, ndead, per = math.inf, 0, {}
    for n, sets in rows.items():
        p = P64[n]
        for si, (x, xm) in enumerate(sets):
            f = _mlp(p, x, xm)
            for z, m, w, b in ((f["z1"], f["m_z1"], p["w1"], p["b1"]), (f["z2"], f["m_z2"], p["w2"], p["b2"])):
                dead = _is_dead(w, b)
                ndead += int(dead.sum())
                r_ = (z.abs() / (N * U * m))[:, ~dead]
                if r_.numel():
                    worst = min(worst, float(r_.min()))
                    per[(n, si)] = min(per.get((n, si), math.inf), float(r_.min()))
    return worst, ndead, per
