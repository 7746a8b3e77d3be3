"""SAC, the reference's fourth neural learner (turtlebot3_rl_sim/src/sac.py, start_sac_training.py), in PyTorch-ROCm with the
update also available as libcrowdnav's cn_sac_update and action selection as cn_sac_act (csrc/crowdnav_sac.hip).

start_sac_training.py cannot run (it passes batch_size, memory_size, discount_factor into slots named batch_size, discount_factor,
buffer_size, and network_inputs = 54); sac.py itself can.  Every value is taken AT ITS NAME -- batch 64, memory 1e6, gamma 0.99 --
and the input width from the environment.  What is kept from sac.py as committed:
- actor Linear(D, H) - ReLU - Linear(H, H) - ReLU - {mean_linear, log_std_linear}(H, 2), both heads U(-3e-3, 3e-3), log_std clamped
  to [-20, 2] (SAC:43-76); z = Normal(mean, std).sample() -- not rsample, so z carries no gradient; t = tanh z; the action is
  squashed a second time, (sigmoid(t0) max_v, tanh(t1) max_w) (SAC:84-91): v in about [0.27, 0.73] max_v, w in +-0.76 max_w;
- act() samples (its docstring says deterministic) and clips (SAC:206-229); deterministic=True (z = mean) is opt-in;
- value_net="as_written": ValueNetwork(state_size, action_size, hidden_size) against (state_dim, hidden_dim, init_w) (SAC:175-176):
  hidden width 2 and linear3 ~ U(-hidden, hidden); "intended": hidden width `hidden`, init 3e-3;
- soft_update="as_written": SAC:290 calls soft_update(V_t, V) against soft_update(local, target), so V <- (1 - tau) V + tau V_t
  after V's step and V_t never leaves its initial value; "intended": V_t <- (1 - tau) V_t + tau V;
- learn() (SAC:231-290): two Normal.sample draws (forward()'s is thrown away, evaluate()'s counts), the three losses on the
  pre-update weights, Adam steps in the order Q, V, actor, then the soft update;
- checkpoints sac_{actor,critic_v,critic_soft_q}_model_ep<N>.pt, the V file holding V_t; load_models loads it into V and copies."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._fused import FusedLearner, mlp_of
from .td3 import DeviceReplay

INIT_W = 3e-3
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
LOGP_EPS = 1e-6          # Actor.evaluate's epsilon (SAC:78)
HALF_LOG_2PI = 0.9189385332046727


class Actor(nn.Module):
    def __init__(self, num_inputs=363, num_actions=2, hidden_size=256, max_lin_vel=0.22, max_ang_vel=2.0, init_w=INIT_W):
        super().__init__()
        self.linear1 = nn.Linear(num_inputs, hidden_size)
        self.linear2 = nn.Linear(hidden_size, hidden_size)
        self.mean_linear = nn.Linear(hidden_size, num_actions)
        self.mean_linear.weight.data.uniform_(-init_w, init_w)
        self.mean_linear.bias.data.uniform_(-init_w, init_w)
        self.log_std_linear = nn.Linear(hidden_size, num_actions)
        self.log_std_linear.weight.data.uniform_(-init_w, init_w)
        self.log_std_linear.bias.data.uniform_(-init_w, init_w)
        self.max_lin_vel, self.max_ang_vel = max_lin_vel, max_ang_vel

    def forward(self, state):
        """-> (mean, clamped log_std, raw log_std)"""
        x = F.relu(self.linear2(F.relu(self.linear1(state))))
        raw = self.log_std_linear(x)
        return self.mean_linear(x), torch.clamp(raw, LOG_STD_MIN, LOG_STD_MAX), raw

    def squash(self, z):
        """SAC:84-91: tanh, then the heads' squash on top of it."""
        t = torch.tanh(z)
        return torch.stack([torch.sigmoid(t[:, 0]) * self.max_lin_vel, torch.tanh(t[:, 1]) * self.max_ang_vel], 1), t


class SoftQNetwork(nn.Module):
    def __init__(self, num_inputs=363, num_actions=2, hidden_size=256, init_w=INIT_W):
        super().__init__()
        self.linear1 = nn.Linear(num_inputs + num_actions, hidden_size)
        self.linear2 = nn.Linear(hidden_size, hidden_size)
        self.linear3 = nn.Linear(hidden_size, 1)
        self.linear3.weight.data.uniform_(-init_w, init_w)
        self.linear3.bias.data.uniform_(-init_w, init_w)

    def forward(self, state, action):
        x = F.relu(self.linear1(torch.cat([state, action], 1)))
        return self.linear3(F.relu(self.linear2(x)))


class ValueNetwork(nn.Module):
    def __init__(self, state_dim=363, hidden_dim=2, init_w=256):
        super().__init__()
        self.linear1 = nn.Linear(state_dim, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, hidden_dim)
        self.linear3 = nn.Linear(hidden_dim, 1)
        self.linear3.weight.data.uniform_(-init_w, init_w)
        self.linear3.bias.data.uniform_(-init_w, init_w)

    def forward(self, state):
        return self.linear3(F.relu(self.linear2(F.relu(self.linear1(state)))))


class Agent:
    """SAC agent (SAC:146-324) acting on batches of observations that stay on the device."""

    def __init__(self, obs_dim=363, hidden=256, actor_lr=3e-4, v_lr=3e-4, q_lr=3e-4, batch_size=64, memory_size=1_000_000,
                 gamma=0.99, tau=5e-3, max_v=0.22, max_w=2.0, mean_lambda=1e-3, std_lambda=1e-3, z_lambda=0.0,
                 value_net="as_written", soft_update="as_written", deterministic=False, n_envs=1, device="cuda", seed=0,
                 replay_sample="with"):
        from . import _abi
        _abi.replay_sample_mode(replay_sample)      # "with" (replacement) | "without" (distinct rows, sac.py:34-35's random.sample)
        self.replay_sample = replay_sample
        if value_net not in ("as_written", "intended") or soft_update not in ("as_written", "intended"):
            raise ValueError("value_net / soft_update: 'as_written' or 'intended'")
        self.device = torch.device(device)
        torch.manual_seed(seed)
        # construction and draw order of SAC:169-181: actor, V, V_t, Q -- the same seed draws the reference's parameters
        self.actor = Actor(obs_dim, 2, hidden, max_v, max_w).to(self.device)
        vh, vw = (2, hidden) if value_net == "as_written" else (hidden, INIT_W)     # SAC:175-176: (state, action_size, hidden_size)
        self.v = ValueNetwork(obs_dim, vh, vw).to(self.device)
        self.v_t = ValueNetwork(obs_dim, vh, vw).to(self.device)
        self.q = SoftQNetwork(obs_dim, 2, hidden).to(self.device)
        self.v_t.load_state_dict(self.v.state_dict())                               # SAC:191
        kw = dict(fused=True) if self.device.type == "cuda" else {}
        self.opt_a = torch.optim.Adam(self.actor.parameters(), lr=actor_lr, **kw)
        self.opt_v = torch.optim.Adam(self.v.parameters(), lr=v_lr, **kw)
        self.opt_q = torch.optim.Adam(self.q.parameters(), lr=q_lr, **kw)
        self.memory = DeviceReplay(memory_size, obs_dim, self.device)
        self.obs_dim, self.hidden, self.hidden_v = obs_dim, hidden, vh
        self.batch_size, self.gamma, self.tau = batch_size, gamma, tau
        self.max_v, self.max_w = max_v, max_w
        self.mean_lambda, self.std_lambda, self.z_lambda = mean_lambda, std_lambda, z_lambda
        self.value_net, self.soft_update, self.deterministic, self.n_envs = value_net, soft_update, bool(deterministic), n_envs
        self._lo = torch.tensor([0.0, -max_w], device=self.device)
        self._hi = torch.tensor([max_v, max_w], device=self.device)
        self._act_seed = (0x9E3779B97F4A7C15 * (int(seed) + 1) ^ 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        self._act_calls = 0
        self._dev_index = self.device.index if self.device.type == "cuda" and self.device.index is not None else (
            torch.cuda.current_device() if self.device.type == "cuda" else -1)

    # ---- acting ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def act(self, obs, add_noise=True, eps=None, deterministic=None):
        """Agent.act (SAC:206-229) for a batch: z = eps std + mean (eps: unit normal [N, 2], default drawn), the double squash, the
        clip.  It samples whatever add_noise says, as the reference does; deterministic (default: the agent's) takes z = mean."""
        mean, log_std, _ = self.actor(obs[:, :self.obs_dim].to(self.actor.linear1.weight.dtype))      # (float32 unless the actor was cast)
        if self.deterministic if deterministic is None else deterministic:
            z = mean
        else:
            if eps is None:
                eps = torch.randn(mean.shape, device=mean.device)
            z = eps.to(mean.device) * log_std.exp() + mean
        a, _ = self.actor.squash(z)
        return torch.max(torch.min(a, self._hi), self._lo).contiguous()

    def actor_struct(self):
        from . import _abi
        a = self.actor
        ps = [a.linear1.weight, a.linear1.bias, a.linear2.weight, a.linear2.bias, a.mean_linear.weight, a.mean_linear.bias,
              a.log_std_linear.weight, a.log_std_linear.bias]
        assert all(p.is_contiguous() and p.dtype == torch.float32 and p.is_cuda for p in ps)
        return _abi.CnSacActor(*[p.data_ptr() for p in ps])

    def act_fused(self, obs, eps=None, deterministic=None, out=None, mean=None, log_std=None, z=None):
        """cn_sac_act: the whole of act() as one launch.  eps None = drawn on the device from (seed, call counter, row).
        mean / log_std / z: optional [N, 2] outputs.  -> twist [N, 2].
        The call counter travels as a kernel argument: a captured graph of this call would replay ONE draw.  Nothing captures
        it today; a capture must supply eps (or read the counter from device memory first)."""
        import ctypes as C
        from . import _abi
        L = _abi.lib()
        n = obs.shape[0]
        if obs.dtype != torch.float32 or obs.stride(1) != 1:
            obs = obs.float().contiguous()
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        if eps is not None:
            eps = eps.to(self.device).float().contiguous()
        ptr = lambda t: t.data_ptr() if t is not None else None
        io = _abi.CnSacActIO(obs=obs.data_ptr(), obs_ld=obs.stride(0), n=n, obs_dim=self.obs_dim, hidden=self.hidden,
                             deterministic=int(self.deterministic if deterministic is None else deterministic), actor=self.actor_struct(),
                             max_v=self.max_v, max_w=self.max_w, log_std_min=LOG_STD_MIN, log_std_max=LOG_STD_MAX, eps=ptr(eps),
                             seed=self._act_seed, counter=self._act_calls, twist=out.data_ptr(), mean=ptr(mean), log_std=ptr(log_std), z=ptr(z))
        self._act_calls += 1
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = L.cn_sac_act(C.byref(io), self._dev_index, st)
        if rc != 0:
            raise _abi.CrowdNavError("cn_sac_act: %s" % L.cn_td3_last_error().decode())
        self._keep_act = (obs, eps)
        return out

    # ---- the update --------------------------------------------------------------------------------------------------------
    def _update(self, s, a, r, s2, d, noise):
        """The arithmetic of one SAC update (SAC:253-290) on a given batch; noise = the unit normal eps [B, 2], z = eps std + mean."""
        q_sa, v_s = self.q(s, a), self.v(s)                                            # SAC:253-254
        mean, log_std, _ = self.actor(s)
        std = log_std.exp()
        z = (noise * std + mean).detach()                                              # Normal.sample: a value
        a_new, t = self.actor.squash(z)
        # Normal.log_prob(z) - log(1 - tanh(z)^2 + eps), summed over the two actions (SAC:86-87)
        log_prob = (-((z - mean) ** 2) / (2 * std ** 2) - std.log() - HALF_LOG_2PI - torch.log(1 - t.pow(2) + LOGP_EPS)).sum(-1, keepdim=True)
        with torch.no_grad():
            y = r + (1 - d) * self.gamma * self.v_t(s2)                                # :257-258
        lq = F.mse_loss(q_sa, y)                                                       # :259
        q_new = self.q(s, a_new.detach())                                              # :261
        lv = F.mse_loss(v_s, (q_new - log_prob).detach())                              # :262-263
        lp = (log_prob * (log_prob - (q_new - v_s)).detach()).mean()                   # :265-266
        lp = lp + self.mean_lambda * mean.pow(2).mean() + self.std_lambda * log_std.pow(2).mean() + self.z_lambda * z.pow(2).sum(1).mean()
        self.opt_q.zero_grad(set_to_none=True); lq.backward(); self.opt_q.step()       # :275-277
        self.opt_v.zero_grad(set_to_none=True); lv.backward(); self.opt_v.step()       # :280-282
        self.opt_a.zero_grad(set_to_none=True); lp.backward(); self.opt_a.step()       # :285-287
        with torch.no_grad():                                                          # :290
            moved, toward = (self.v, self.v_t) if self.soft_update == "as_written" else (self.v_t, self.v)
            for pm, pt in zip(moved.parameters(), toward.parameters()):
                pm.copy_(pm * (1.0 - self.tau) + pt * self.tau)
        return torch.stack([lq.detach(), lv.detach(), lp.detach()])

    def enable_fused_update(self):
        """Hand the update to cn_sac_update (10 launches, 11 with soft_update="as_written"; enqueue-only).  Adam's moments restart
        from zero inside the library: call this before training."""
        from . import _abi
        if self.device.type != "cuda":
            raise RuntimeError("enable_fused_update needs a HIP device")
        if getattr(self, "_fused", None):
            return
        og = self.opt_a.param_groups[0]
        cfg = _abi.CnSacConfig(obs_dim=self.obs_dim, hidden=self.hidden, hidden_v=self.hidden_v, batch=self.batch_size,
                               gamma=self.gamma, tau=self.tau, lr_actor=og["lr"], lr_v=self.opt_v.param_groups[0]["lr"],
                               lr_q=self.opt_q.param_groups[0]["lr"], beta1=og["betas"][0], beta2=og["betas"][1], eps=og["eps"],
                               max_v=self.max_v, max_w=self.max_w, log_std_min=LOG_STD_MIN, log_std_max=LOG_STD_MAX,
                               mean_lambda=self.mean_lambda, std_lambda=self.std_lambda, z_lambda=self.z_lambda, logp_eps=LOGP_EPS,
                               soft_update=0 if self.soft_update == "as_written" else 1, reserved=0,
                               actor=self.actor_struct(), q=mlp_of(self.q), v=mlp_of(self.v), v_t=mlp_of(self.v_t),
                               seed=self._act_seed ^ 0x5851F42D4C957F2D, **self.memory.ring_fields())
        self._fused = FusedLearner("sac", cfg, self.device, self._dev_index, loss_shape=(3,), replay_sample=self.replay_sample)

    def _fused_learn(self, batch=None, noise=None):
        from . import _abi
        bs = keep = None
        if batch is not None:
            keep = s, a, r, s2, d = [t.contiguous().float() for t in batch]
            B, D = self.batch_size, self.obs_dim
            if s.shape != (B, D) or s2.shape != (B, D) or a.shape != (B, 2) or r.numel() != B or d.numel() != B:
                raise ValueError("cn_sac_update was created for batches of %d x %d; got s %s a %s r %s s2 %s d %s" % (
                    B, D, tuple(s.shape), tuple(a.shape), tuple(r.shape), tuple(s2.shape), tuple(d.shape)))
            if noise is not None:
                noise = noise.to(self.device).contiguous().float()
                if noise.shape != (B, 2):
                    raise ValueError("noise must be [%d, 2]; got %s" % (B, tuple(noise.shape)))
                keep = keep + [noise]
            bs = _abi.CnTd3Batch(s.data_ptr(), a.data_ptr(), r.data_ptr(), s2.data_ptr(), d.data_ptr(), noise.data_ptr() if noise is not None else None)
        elif noise is not None:
            raise ValueError("noise needs an explicit batch")
        return self._fused.update(batch=bs, keep=keep)

    def fused_batch(self, what, shape):
        """A host copy of what the last fused update gathered or computed (cn_sac_batch_dev; synchronises)."""
        return self._fused.batch_dev(what, shape).cpu()

    def learn(self, step=None, batch=None, noise=None):
        """One SAC update (SAC:231-290).  batch = (s, a, r[B,1], s2, d[B,1]) overrides the replay sample; noise = the unit eps [B, 2]
        (default: drawn -- the PyTorch path draws twice and uses the second, as learn() does).  `step` is unused.  Returns
        [q_loss, value_loss, policy_loss] as one device tensor (no host synchronisation), or None while the replay holds no more
        than a batch (TRAIN_SAC:127)."""
        if batch is None and not self.memory.ready(self.batch_size):
            return None
        if getattr(self, "_fused", None):
            return self._fused_learn(batch, noise)
        if batch is None:
            batch = self.memory.sample(self.batch_size, replace=self.replay_sample == "with")
        s, a, r, s2, d = batch
        if noise is None:
            torch.randn((s.shape[0], 2), device=s.device)                    # forward()'s sample, thrown away (SAC:74, 79)
            noise = torch.randn((s.shape[0], 2), device=s.device)
        return self._update(s, a, r.reshape(-1, 1), s2, d.reshape(-1, 1), noise.to(s.device))

    # ---- checkpoints -------------------------------------------------------------------------------------------------------
    def noise_state(self):
        return self._act_seed, self._act_calls

    def set_noise_state(self, seed, calls):
        self._act_seed, self._act_calls = int(seed), int(calls)

    def save(self, outdir, ep):
        """sac_{actor,critic_v,critic_soft_q}_model_ep<N>.pt (TRAIN_SAC, SAC:309-316); the V file holds the TARGET value net."""
        os.makedirs(outdir, exist_ok=True)
        torch.save(self.actor.state_dict(), os.path.join(outdir, "sac_actor_model_ep%d.pt" % ep))
        torch.save(self.v_t.state_dict(), os.path.join(outdir, "sac_critic_v_model_ep%d.pt" % ep))
        torch.save(self.q.state_dict(), os.path.join(outdir, "sac_critic_soft_q_model_ep%d.pt" % ep))

    def load_models(self, actor_path, critic_v_path, critic_soft_q_path):
        """SAC:318-324 (its argument order is actor, soft_q, v; here the order of CHECKPOINT_NETS): V's file into the local V,
        hard-copied to V_t."""
        self.actor.load_state_dict(torch.load(actor_path, map_location=self.device))
        self.q.load_state_dict(torch.load(critic_soft_q_path, map_location=self.device))
        self.v.load_state_dict(torch.load(critic_v_path, map_location=self.device))
        self.v_t.load_state_dict(self.v.state_dict())
