"""DDPG, the reference's baseline learner (turtlebot3_rl_sim/src/ddpg.py, start_ddpg_training.py), in PyTorch-ROCm with the
update also available as libcrowdnav's cn_ddpg_update (csrc/crowdnav_ddpg.hip, 8 launches).

What it keeps from the reference:
- networks: td3.Actor / td3.Critic (the same 3 x Linear(256) and sigmoid*0.22 / tanh*2.0 heads as TD3, DDPG:67-109) with
  linear3's weight and bias of BOTH networks drawn from U(-3e-3, 3e-3) (DDPG:75-76, 102-103); the targets are hard copies
  (DDPG:150-151);
- hyper-parameters: batch 64, memory 1e6, hidden 256 (TRAIN_DDPG:53-58), actor lr 1e-4, critic lr 1e-3, gamma 0.99,
  tau 0.001 (configs/ddpg.yaml), torch.optim.Adam's defaults, nn.MSELoss;
- learn() (DDPG:198-243): y = r + (1 - d) gamma Q_t(s2, pi_t(s2)); critic loss mean((Q(s, a) - y)^2); actor loss -mean Q(s, pi(s))
  back-propagated and stepped BEFORE the critic's step, i.e. through the pre-update critic; then the critic's step (the
  actor loss's gradients on the critic are cleared by its zero_grad) and the soft updates of critic and actor;
- collection without exploration noise (TRAIN_DDPG:100, add_noise=False): explore_sigma = 0 in every fused actor path;
  Ornstein-Uhlenbeck noise (DDPG:44-64) as an opt-in term, with the reference's uniform (not Gaussian) increments: in PyTorch
  (act(add_noise=True)) or with the actor in one launch (act_ou_fused: cn_ddpg_act), on one shared state;
- checkpoints of the TARGET networks as ddpg_{actor,critic}_model_ep<N>.pt (DDPG:262-266); load_models loads the locals and
  hard-copies them to the targets (DDPG:268-272)."""
import os

import torch
import torch.nn.functional as F

from ._fused import FusedLearner, mlp_of
from .td3 import Actor, Critic, DeviceReplay, FusedActorMixin

INIT_W = 3e-3      # DDPG:68, 96: init_w of linear3


class OUNoise:
    """OUNoise (DDPG:44-64) with one state per environment: x <- x + theta (mu - x) + sigma U, U = random.random() per component
    -- uniform on [0, 1), not Gaussian, so the process drifts upwards; kept as the reference has it.  State in float64 like the
    reference's numpy arrays; reset() of the rows of finished episodes (TRAIN_DDPG:161)."""

    def __init__(self, n, action_dim=2, mu=0.0, theta=0.15, max_sigma=0.2, min_sigma=0.2, decay_period=100000, device="cpu", seed=0):
        self.mu, self.theta, self.sigma = float(mu), float(theta), float(max_sigma)
        self.max_sigma, self.min_sigma, self.decay_period = float(max_sigma), float(min_sigma), decay_period
        self.state = torch.full((n, action_dim), self.mu, dtype=torch.float64, device=device)
        self.gen = torch.Generator(device=device).manual_seed(seed)

    def reset(self, mask=None):
        """DDPG:53-54 for every row (mask None) or the rows where `mask` is set."""
        if mask is None:
            self.state.fill_(self.mu)
        else:
            self.state[mask.reshape(-1).bool()] = self.mu

    def sample(self, step=0, u=None):
        """DDPG:56-64.  u: the uniforms [n, action_dim] (default: drawn from this object's generator)."""
        x = self.state
        if u is None:
            u = torch.rand(x.shape, generator=self.gen, dtype=torch.float64, device=x.device)
        dx = self.theta * (self.mu - x) + self.sigma * u.to(torch.float64)
        self.state = x + dx
        self.decay(step)
        return self.state

    def decay(self, step):
        """DDPG:63: the sigma of the NEXT sample."""
        self.sigma = self.max_sigma - (self.max_sigma - self.min_sigma) * min(1.0, step / self.decay_period)


class Agent(FusedActorMixin):
    """DDPG agent (DDPG:112-272) acting on batches of observations that stay on the device."""

    def __init__(self, obs_dim=363, hidden=256, actor_lr=1e-4, critic_lr=1e-3, batch_size=64, memory_size=1_000_000,
                 gamma=0.99, tau=0.001, max_v=0.22, max_w=2.0, explore_sigma=0.0, n_envs=1, device="cuda", seed=0,
                 replay_sample="with"):
        from . import _abi
        _abi.replay_sample_mode(replay_sample)      # "with" (replacement) | "without" (distinct rows, ddpg.py:33-34's random.sample)
        self.replay_sample = replay_sample
        self.device = torch.device(device)
        torch.manual_seed(seed)

        def small_head(m):           # DDPG:75-76, 102-103, drawn right after the module's own nn.Linear draws as there
            with torch.no_grad():
                m.linear3.weight.uniform_(-INIT_W, INIT_W)
                m.linear3.bias.uniform_(-INIT_W, INIT_W)
            return m.to(self.device)
        # construction order of DDPG:131-143 (actor_local, actor_target, critic_local, critic_target): the same seed draws the
        # reference's parameters
        self.actor = small_head(Actor(obs_dim, 2, hidden, max_v, max_w))
        self.actor_t = small_head(Actor(obs_dim, 2, hidden, max_v, max_w))
        self.critic = small_head(Critic(obs_dim, 2, hidden))
        self.critic_t = small_head(Critic(obs_dim, 2, hidden))
        self.actor_t.load_state_dict(self.actor.state_dict())      # DDPG:150-151
        self.critic_t.load_state_dict(self.critic.state_dict())
        kw = dict(fused=True) if self.device.type == "cuda" else {}
        self.opt_a = torch.optim.Adam(self.actor.parameters(), lr=actor_lr, **kw)
        self.opt_c = torch.optim.Adam(self.critic.parameters(), lr=critic_lr, **kw)
        self.memory = DeviceReplay(memory_size, obs_dim, self.device)
        self.batch_size, self.gamma, self.tau = batch_size, gamma, tau
        self.max_v, self.max_w = max_v, max_w
        self.explore_sigma = explore_sigma      # the fused actor paths' Gaussian term: 0 = the reference's add_noise=False
        self.noise = OUNoise(n_envs, device=self.device, seed=seed)
        self._init_fused_actor(seed)

    # ---- acting ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def act(self, obs, add_noise=False, step=0):
        """Agent.act (DDPG:170-196) for a batch: the actor, + OU noise when asked (one state per row of obs), clip to
        v in [0, max_v], w in [-max_w, max_w].  The noise is float64 and the action float32, as numpy's `action += noise`."""
        a = self.actor(obs)
        if add_noise:
            if self.noise.state.shape[0] != a.shape[0]:
                raise ValueError("OU noise has %d states for %d observations (Agent(n_envs=...))" % (self.noise.state.shape[0], a.shape[0]))
            a = (a.double() + self.noise.sample(step)).float()
        return torch.max(torch.min(a, self._hi), self._lo).contiguous()

    def reset_noise(self, mask=None):
        """agent.noise.reset() at an episode's end (TRAIN_DDPG:161), for the rows where `mask` is set."""
        self.noise.reset(mask)

    def _ou_io(self, obs, out, reset, u, add_noise):
        """cn_ddpg_act's io for these buffers; state, sigma and counter are filled in per call."""
        from . import _abi
        ns = self.noise
        return _abi.CnDdpgActIO(obs=obs.data_ptr(), reset=None if reset is None else reset.data_ptr(), u=None if u is None else u.data_ptr(),
                                action=out.data_ptr(), noise_out=None, mu=ns.mu, theta=ns.theta, seed=self._noise_seed,
                                max_v=self.max_v, max_w=self.max_w, n=obs.shape[0], add_noise=1 if add_noise else 0)

    def _ou_check(self, obs, reset, u, add_noise):
        """The buffers as cn_ddpg_act reads them: the row count of act(), a byte per row of `reset`, float64 uniforms."""
        n, st = obs.shape[0], self.noise.state
        if add_noise and st.shape[0] != n:
            raise ValueError("OU noise has %d states for %d observations (Agent(n_envs=...))" % (st.shape[0], n))
        if reset is not None:
            reset = reset.reshape(-1)
            if reset.dtype not in (torch.uint8, torch.bool):
                reset = reset != 0
            reset = reset.contiguous()
            if reset.shape[0] != n:
                raise ValueError("reset has %d rows for %d observations" % (reset.shape[0], n))
        if u is not None:
            u = u.to(device=self.device, dtype=torch.float64).contiguous()
            if tuple(u.shape) != (n, 2):
                raise ValueError("u must be [%d, 2], not %s" % (n, tuple(u.shape)))
        return reset, u

    @torch.no_grad()
    def act_ou_fused(self, obs, reset=None, step=0, out=None, u=None, add_noise=True):
        """act(obs, add_noise=True, step=step) preceded by reset_noise(reset), as ONE kernel (cn_ddpg_act, csrc/crowdnav_ddpg.hip):
        act_mfma's actor tile with the Ornstein-Uhlenbeck update and numpy's float64 `action += noise` as its output stage.
        It updates `self.noise.state` itself, in place, so this path and act(add_noise=True) / reset_noise share one state and can be
        mixed call by call.  reset: [n] uint8 / bool (the previous step's `done`) or None; u: the uniforms [n, 2] float64, or None =
        drawn on the device from (the agent's noise seed, its call counter, row, component).  This call uses `self.noise.sigma`,
        then sets the next call's from `step` as OUNoise.sample does.  add_noise=False: the deterministic policy; the state, `reset`
        and sigma stay as they are."""
        import ctypes as C
        from . import _abi
        if not hasattr(self, "_fw_struct"):
            self.sync_fused_weights()
        obs = obs.contiguous()
        reset, u = self._ou_check(obs, reset, u, add_noise)
        if out is None:
            out = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        ns = self.noise
        state = ns.state if ns.state.is_contiguous() else ns.state.contiguous()
        io = self._ou_io(obs, out, reset, u, add_noise)
        self._fused_calls += 1
        io.state, io.sigma, io.counter = state.data_ptr(), ns.sigma, self._fused_calls
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _abi.check(_abi.lib().cn_ddpg_act(C.byref(self._fw_struct), C.byref(io), self._dev_index, st))
        if add_noise:
            ns.state = state
            ns.decay(step)
        return out

    def bind_act_ou_fused(self, obs, out, reset, u=None):
        """Pre-marshalled act_ou_fused for fixed obs / out / reset (and, optionally, u) buffers: a callable `call(step=0)` that only
        enqueues.  Each call reads where `self.noise.state` lives NOW (the torch path replaces that tensor), this call's sigma and the
        call counter on the host and passes them by value; `step` sets the next call's sigma.  So a call captured into a graph keeps
        the state's address, the sigma and the counter it was captured with: keep to the fused path while replaying (it updates the
        state in place), and give `u` -- a buffer refilled before every replay -- because the device draw of a frozen counter
        repeats."""
        import ctypes as C
        from . import _abi
        if not hasattr(self, "_fw_struct"):
            self.sync_fused_weights()
        assert obs.is_contiguous() and out.is_contiguous()
        reset_c, u_c = self._ou_check(obs, reset, u, True)
        assert (reset is None or reset_c.data_ptr() == reset.data_ptr()) and (u is None or u_c.data_ptr() == u.data_ptr()), \
            "reset must be contiguous uint8 / bool and u contiguous float64 on the agent's device: the call reads these buffers"
        io = self._ou_io(obs, out, reset_c, u_c, True)
        fn, check, w, pio = _abi.lib().cn_ddpg_act, _abi.check, C.byref(self._fw_struct), C.byref(io)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        ns, dv, n = self.noise, self._dev_index, obs.shape[0]
        keep = (obs, out, reset_c, u_c, io, self._fw_struct, self._fw)

        def call(step=0, _keep=keep):
            state = ns.state
            if state.shape[0] != n or not state.is_contiguous():
                raise ValueError("OU noise has %d states for %d observations (Agent(n_envs=...))" % (state.shape[0], n))
            self._fused_calls = c = self._fused_calls + 1
            io.state, io.sigma, io.counter = state.data_ptr(), ns.sigma, c
            rc = fn(w, pio, dv, st)
            if rc:
                check(rc)
            ns.decay(step)
        return call

    # ---- the update --------------------------------------------------------------------------------------------------------
    def _update(self, s, a, r, s2, d):
        """The arithmetic of one DDPG update (DDPG:198-243) on a given batch."""
        la = -self.critic(s, self.actor(s)).mean()                          # DDPG:216-217
        with torch.no_grad():
            y = r + (1.0 - d) * self.gamma * self.critic_t(s2, self.actor_t(s2))   # :219-222 (the clamp to +-inf is a no-op)
        lc = F.mse_loss(self.critic(s, a), y)                               # :228-230
        self.opt_a.zero_grad(set_to_none=True); la.backward(); self.opt_a.step()       # :233-235, through the pre-update critic
        self.opt_c.zero_grad(set_to_none=True); lc.backward(); self.opt_c.step()       # :237-239 (drops la's critic gradients)
        with torch.no_grad():
            for t, src in ((self.critic_t, self.critic), (self.actor_t, self.actor)):   # :241-242, soft_update :244-254
                for pt, ps in zip(t.parameters(), src.parameters()):
                    pt.copy_(pt * (1.0 - self.tau) + ps * self.tau)
        return lc.detach()

    def enable_fused_update(self):
        """Hand the update to cn_ddpg_update: the forward / backward GEMMs of the four networks on the f32 matrix cores, weight
        gradients and soft updates folded into the Adam steps, 8 launches per update.  The networks stay these nn.Modules (stepped
        in place); Adam's moments restart from zero inside the library, so call this before training."""
        from . import _abi
        if self.device.type != "cuda":
            raise RuntimeError("enable_fused_update needs a HIP device")
        if getattr(self, "_fused", None):
            return
        og = self.opt_a.param_groups[0]
        cfg = _abi.CnDdpgConfig(obs_dim=self.actor.linear1.in_features, hidden=self.actor.linear1.out_features, batch=self.batch_size,
                                gamma=self.gamma, tau=self.tau, lr_actor=og["lr"], lr_critic=self.opt_c.param_groups[0]["lr"],
                                beta1=og["betas"][0], beta2=og["betas"][1], eps=og["eps"], max_v=self.max_v, max_w=self.max_w,
                                actor=mlp_of(self.actor), actor_t=mlp_of(self.actor_t), critic=mlp_of(self.critic),
                                critic_t=mlp_of(self.critic_t), seed=self._noise_seed, **self.memory.ring_fields())
        self._fused = FusedLearner("ddpg", cfg, self.device, self._dev_index, replay_sample=self.replay_sample)

    def _fused_learn(self, batch=None):
        from . import _abi
        bs = keep = None
        if batch is not None:
            keep = s, a, r, s2, d = [t.contiguous().float() for t in batch]
            B, D = self.batch_size, self.actor.linear1.in_features
            if s.shape != (B, D) or s2.shape != (B, D) or a.shape != (B, 2) or r.numel() != B or d.numel() != B:
                raise ValueError("cn_ddpg_update was created for batches of %d x %d; got s %s a %s r %s s2 %s d %s" % (
                    B, D, tuple(s.shape), tuple(a.shape), tuple(r.shape), tuple(s2.shape), tuple(d.shape)))
            bs = _abi.CnTd3Batch(s.data_ptr(), a.data_ptr(), r.data_ptr(), s2.data_ptr(), d.data_ptr(), None)
        return self._fused.update(batch=bs, keep=keep)

    def learn(self, step=None, batch=None):
        """One DDPG update (DDPG:198-243).  `batch` = (s, a, r[B,1], s2, d[B,1]) overrides the replay sample (parity tests).
        `step` is accepted for the trainer's call signature and unused (no policy delay).  Returns the critic's loss as a 0-d
        tensor (no host synchronisation), or None while the replay holds no more than a batch (TRAIN_DDPG:111)."""
        if batch is None and not self.memory.ready(self.batch_size):
            return None
        if getattr(self, "_fused", None):
            return self._fused_learn(batch)
        if batch is None:
            batch = self.memory.sample(self.batch_size, replace=self.replay_sample == "with")
        s, a, r, s2, d = batch
        return self._update(s, a, r.reshape(-1, 1), s2, d.reshape(-1, 1))

    # ---- checkpoints -------------------------------------------------------------------------------------------------------
    def save(self, outdir, ep):
        """The TARGET networks as ddpg_{actor,critic}_model_ep<N>.pt (TRAIN_DDPG:150-152, DDPG:262-266)."""
        os.makedirs(outdir, exist_ok=True)
        torch.save(self.actor_t.state_dict(), os.path.join(outdir, "ddpg_actor_model_ep%d.pt" % ep))
        torch.save(self.critic_t.state_dict(), os.path.join(outdir, "ddpg_critic_model_ep%d.pt" % ep))

    def load_models(self, actor_path, critic_path):
        """DDPG:268-272: into the local networks (strict key match: linear{1,2,3}.{weight,bias}), then hard copies to the targets."""
        self.actor.load_state_dict(torch.load(actor_path, map_location=self.device))
        self.critic.load_state_dict(torch.load(critic_path, map_location=self.device))
        self.actor_t.load_state_dict(self.actor.state_dict())
        self.critic_t.load_state_dict(self.critic.state_dict())
        if hasattr(self, "_fw_struct"):
            self.sync_fused_weights()
