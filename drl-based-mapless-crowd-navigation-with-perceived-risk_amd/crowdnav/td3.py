"""TD3 pieces the rollout needs, in PyTorch-ROCm (the caller of the hot path).

Mirrors td3.py of the reference: Actor 3 x Linear(256) with sigmoid*max_lin_vel / tanh*max_ang_vel heads
(TD3:81-106), Critic (TD3:109-126), Gaussian exploration sigma = 1.0 (TD3:67-78), clipping to
v in [0, 0.22], w in [-2, 2] (TD3:214-215), and the TD3 update (TD3:225-285) with the hyper-parameters of
start_td3_training.py:62-72.  The replay buffer is a device-resident ring so a vectorised env never
leaves the GPU.  No custom kernels here: these are plain library GEMMs (hipBLASLt)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._fused import FusedLearner, FusedPopulation, _device_view, mlp_of


class Actor(nn.Module):
    def __init__(self, num_inputs=398, num_actions=2, hidden_size=256, max_lin_vel=0.22, max_ang_vel=2.0):
        super().__init__()
        self.linear1 = nn.Linear(num_inputs, hidden_size)
        self.linear2 = nn.Linear(hidden_size, hidden_size)
        self.linear3 = nn.Linear(hidden_size, num_actions)
        self.max_lin_vel, self.max_ang_vel = max_lin_vel, max_ang_vel

    def logits(self, state):
        x = F.relu(self.linear1(state))
        x = F.relu(self.linear2(x))
        return self.linear3(x)

    def forward(self, state):
        a = self.logits(state)
        return torch.stack([torch.sigmoid(a[:, 0]) * self.max_lin_vel, torch.tanh(a[:, 1]) * self.max_ang_vel], 1)


class Critic(nn.Module):
    def __init__(self, num_inputs=398, num_actions=2, hidden_size=256):
        super().__init__()
        self.linear1 = nn.Linear(num_inputs + num_actions, hidden_size)
        self.linear2 = nn.Linear(hidden_size, hidden_size)
        self.linear3 = nn.Linear(hidden_size, 1)

    def forward(self, state, action):
        x = torch.cat([state, action], 1)
        x = F.relu(self.linear1(x))
        x = F.relu(self.linear2(x))
        return self.linear3(x)


def _device_scalar_view(ptr, device):
    """A 0-d float32 tensor aliasing one device float owned by libcrowdnav (alive as long as its handle)."""
    return _device_view(ptr, (), torch.float32, device)


class DeviceReplay:
    """Ring buffer on the device (ReplayBuffer, TD3:19-37, without the Python list).  ONE source of truth for the write position
    and the fill level: the device scalars `pos_dev` / `size_dev`.  Every write -- add() and add_masked() alike -- indexes from
    `pos_dev` on the device, so the two can be mixed freely; rows that are not transitions go to a spare row past the end of the
    ring.  The host only keeps BOUNDS on the fill level (`_lb` <= size_dev <= `_ub`): add() moves both (every row is kept),
    add_masked() moves the upper one only.  `ready(n)` answers "more than n rows?" from the bounds and reads the device scalar
    only while they straddle n -- never again once the ring holds more than a batch -- and `len()` is exact (it reads the device
    when the bounds differ).  On a HIP device a write is libcrowdnav's cn_replay_write (two launches); `fused=False` keeps the
    PyTorch formulation (~15 kernels: cumulative sum, index arithmetic, five index_copy_), which is also what runs on the CPU
    and what the GPU tests compare the fused write against."""

    def __init__(self, capacity, obs_dim, device, fused=True):
        self.cap = int(capacity)
        self.obs_dim = int(obs_dim)
        self.fused = bool(fused) and torch.device(device).type == "cuda"
        self._ring = None
        cap1 = self.cap + 1                       # row `cap`: where add_masked() drops the rows it does not keep
        self.s = torch.zeros((cap1, obs_dim), dtype=torch.float32, device=device)
        self.s2 = torch.zeros((cap1, obs_dim), dtype=torch.float32, device=device)
        self.a = torch.zeros((cap1, 2), dtype=torch.float32, device=device)
        self.r = torch.zeros((cap1, 1), dtype=torch.float32, device=device)
        self.d = torch.zeros((cap1, 1), dtype=torch.float32, device=device)
        self.pos_dev = torch.zeros((), dtype=torch.int64, device=device)
        self.size_dev = torch.zeros((), dtype=torch.int64, device=device)
        self._lb, self._ub = 0, 0
        self._ar = None
        # sample(replace=False): the key of cn_replay_sample_indices and the number of such samples drawn so far
        self.sample_seed = (0xD6E8FEB86659FD93 * (self.cap + 1) ^ 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF
        self.sample_calls = 0

    def add(self, s, a, r, s2, d):
        """ReplayBuffer.add for a batch of transitions (all rows kept).  Same device-side path as add_masked()."""
        n = s.shape[0]
        self._write(s, a, r, s2, d, None)
        self._lb, self._ub = min(self.cap, self._lb + n), min(self.cap, self._ub + n)

    def add_masked(self, s, a, r, s2, d, keep):
        """add() for the rows where `keep` (bool [n]) is set -- the others are not transitions (an env's reset launch under the
        next-step reset convention).  No host synchronisation: kept rows go to consecutive ring slots after `pos_dev`, the
        rest to the spare row."""
        self._write(s, a, r, s2, d, keep)
        self._ub = min(self.cap, self._ub + s.shape[0])

    def _write_fused(self, s, a, r, s2, d, keep):
        import ctypes as C
        from . import _abi
        L = _abi.lib()
        n = s.shape[0]
        dev = self.s.device
        if self._ring is None:
            self._ring = self.ring_struct()
            self._slot = torch.zeros(0, dtype=torch.int32, device=dev)
        if self._slot.numel() < n:
            self._slot = torch.zeros(n, dtype=torch.int32, device=dev)
        f32 = lambda x, shape: x.reshape(shape).to(torch.float32).contiguous()        # (no-ops for what Env.step and Agent.act hand over)
        s, s2, a, r = f32(s, (n, self.obs_dim)), f32(s2, (n, self.obs_dim)), f32(a, (n, 2)), f32(r, (n,))
        d = d.reshape(n)
        d8 = d.contiguous() if d.dtype in (torch.uint8, torch.bool) else (d != 0)
        k8 = None
        if keep is not None:
            k8 = keep.reshape(n).contiguous() if keep.dtype in (torch.uint8, torch.bool) else (keep.reshape(n) != 0)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = L.cn_replay_write(C.byref(self._ring), C.c_void_p(s.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(r.data_ptr()),
                               C.c_void_p(s2.data_ptr()), C.c_void_p(d8.data_ptr()), C.c_void_p(k8.data_ptr() if k8 is not None else None),
                               n, C.c_void_p(self._slot.data_ptr()), dev.index if dev.index is not None else torch.cuda.current_device(), st)
        if rc != 0:
            raise _abi.CrowdNavError("cn_replay_write: %s" % L.cn_td3_last_error().decode())

    def _write(self, s, a, r, s2, d, keep):
        if self.fused:
            return self._write_fused(s, a, r, s2, d, keep)
        n = s.shape[0]
        if keep is None:
            c = torch.arange(1, n + 1, device=s.device)
            idx = (self.pos_dev + c - 1) % self.cap
        else:
            c = torch.cumsum(keep.to(torch.int64), 0)
            idx = torch.where(keep, (self.pos_dev + c - 1) % self.cap, torch.full_like(c, self.cap))
        self.s.index_copy_(0, idx, s); self.a.index_copy_(0, idx, a); self.s2.index_copy_(0, idx, s2)
        self.r.index_copy_(0, idx, r.reshape(n, 1).float()); self.d.index_copy_(0, idx, d.reshape(n, 1).float())
        tot = c[-1]
        self.pos_dev.copy_((self.pos_dev + tot) % self.cap)
        self.size_dev.copy_(torch.clamp(self.size_dev + tot, max=self.cap))

    def ring_struct(self):
        """The `cn_replay_ring` of this buffer (cn_replay_write, cn_pop_record_create): its five arrays, capacity, position and size."""
        from . import _abi
        return _abi.CnReplayRing(s=self.s.data_ptr(), a=self.a.data_ptr(), r=self.r.data_ptr(), s2=self.s2.data_ptr(), d=self.d.data_ptr(),
                                 capacity=self.cap, pos_dev=self.pos_dev.data_ptr(), size_dev=self.size_dev.data_ptr(),
                                 obs_dim=self.obs_dim, reserved=0)

    def ring_fields(self):
        """The six replay_* fields of a learner's configuration (cn_td3_config, cn_ddpg_config, cn_dqn_config)."""
        return dict(replay_s=self.s.data_ptr(), replay_a=self.a.data_ptr(), replay_r=self.r.data_ptr(), replay_s2=self.s2.data_ptr(),
                    replay_d=self.d.data_ptr(), replay_size_dev=self.size_dev.data_ptr())

    def sync_len(self):
        """The exact fill level (one host read); collapses the host-side bounds onto it."""
        self._lb = self._ub = int(self.size_dev.item())
        return self._lb

    def ready(self, n):
        """len() > n, without a host read whenever the bounds already decide it."""
        if self._lb > n:
            return True
        if self._ub <= n:
            return False
        return self.sync_len() > n

    @property
    def size(self):
        return len(self)

    @property
    def pos(self):
        return int(self.pos_dev.item())

    def sample_indices(self, batch, seed=None, counter=None, mode=1):
        """cn_replay_sample_indices: the ring rows [batch] (int64, on the device) that a fused update keyed (seed, counter) draws
        in `mode` (1 = distinct rows) from the fill level as it stands on the device when the launch runs.  seed / counter None =
        this buffer's own (`sample_seed`, and `sample_calls`, which then advances).  One launch, no host read."""
        import ctypes as C
        from . import _abi
        dev = self.s.device
        if dev.type != "cuda":
            raise RuntimeError("sampling without replacement is libcrowdnav's cn_replay_sample_indices: it needs a HIP device")
        if counter is None:
            counter, self.sample_calls = self.sample_calls, self.sample_calls + 1
        L = _abi.lib()
        idx = torch.empty(int(batch), dtype=torch.int64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = L.cn_replay_sample_indices(self.sample_seed if seed is None else int(seed), int(counter), int(batch),
                                        C.c_void_p(self.size_dev.data_ptr()), int(mode), C.c_void_p(idx.data_ptr()),
                                        dev.index if dev.index is not None else torch.cuda.current_device(), st)
        if rc != 0:
            raise _abi.CrowdNavError("cn_replay_sample_indices: %s" % L.cn_td3_last_error().decode())
        return idx

    def sample(self, batch, replace=True):
        """Uniform sample of the filled part; the indices are drawn on the device from the device-side fill level.  replace=False:
        `batch` distinct rows, as the reference's random.sample (td3.py:31-32) -- a keyed bijection of the filled part evaluated at
        0 .. batch-1 (include/crowdnav.h, cn_td3_batch_dev), O(batch) work and no host read; with batch > len() every row comes
        up floor or ceil(batch / len()) times instead of the reference's ValueError (callers gate on ready(batch))."""
        if not replace:
            idx = self.sample_indices(batch)
            return self.s[idx], self.a[idx], self.r[idx], self.s2[idx], self.d[idx]
        u = torch.rand(batch, device=self.s.device)
        idx = (u * self.size_dev.clamp(min=1).to(torch.float32)).long().clamp_(max=self.cap - 1)
        idx = torch.minimum(idx, (self.size_dev - 1).clamp(min=0))
        return self.s[idx], self.a[idx], self.r[idx], self.s2[idx], self.d[idx]

    def __len__(self):
        return self._lb if self._lb == self._ub else self.sync_len()


class FusedActorMixin:
    """The actor-side interface the collection paths use (rollout, collect_policy, rollout_groups, evaluate,
    VecEnv.rollout_policy): the packed-weight actor kernels of libcrowdnav and their exploration-noise bookkeeping.  Shared by
    the TD3 and the DDPG agent; the host class provides `actor`, `device`, `max_v`, `max_w` and `explore_sigma`."""

    def _init_fused_actor(self, seed):
        # exploration-noise key of the fused actor paths (cn_policy_tail / cn_actor_forward): derived from the Agent seed so that
        # --seed changes the noise; the call counter is part of checkpoints' bookkeeping (noise_state) so a resumed run
        # does not replay the stream
        self._noise_seed = (0x9E3779B97F4A7C15 * (int(seed) + 1) ^ 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        self._fused_calls = 0
        self._dev_index = self.device.index if self.device.type == "cuda" and self.device.index is not None else (
            torch.cuda.current_device() if self.device.type == "cuda" else -1)
        self._lo = torch.tensor([0.0, -self.max_w], device=self.device)
        self._hi = torch.tensor([self.max_v, self.max_w], device=self.device)

    @torch.no_grad()
    def act_fused(self, obs, out=None, add_noise=True):
        """Agent.act with the output stage (heads + exploration noise + clip) as ONE kernel of libcrowdnav
        (cn_policy_tail) instead of ~10 elementwise launches.  Same distribution as act(); the noise comes from
        a counter-based generator keyed by (seed, call counter, row)."""
        import ctypes as C
        from . import _abi
        lg = self.actor.logits(obs).contiguous()
        if out is None:
            out = torch.empty_like(lg)
        self._fused_calls += 1
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _abi.check(_abi.lib().cn_policy_tail(C.c_void_p(lg.data_ptr()), C.c_void_p(out.data_ptr()), lg.shape[0],
                                             self.max_v, self.max_w, self.explore_sigma if add_noise else 0.0,
                                             self._noise_seed, self._fused_calls, self._dev_index, st))
        return out

    def noise_state(self):
        """(seed, call counter) of the fused exploration noise -- persist it with a checkpoint and hand it back to
        set_noise_state() on resume so the noise stream continues instead of restarting."""
        return self._noise_seed, self._fused_calls

    def set_noise_state(self, seed, calls):
        self._noise_seed, self._fused_calls = int(seed), int(calls)

    def sync_fused_weights(self):
        """(Re)build the packed float32 copies cn_actor_forward / cn_rollout_policy read (cn_actor_pack_weights); call after the
        actor's weights change.  The packed buffers and the cn_actor_weights struct are allocated once and refreshed IN PLACE
        (two small copies + two pack kernels on the current stream), so pre-marshalled calls (bind_act_mfma,
        VecEnv.bind_rollout_policy) keep reading the current weights.  The refresh is ordered on torch's current stream: a caller
        that runs the actor on other streams (VecEnvGroups) orders this call after them (join) and their next launches after it (fork)."""
        import ctypes as C
        from . import _abi
        a = self.actor
        D = a.linear1.in_features
        Dp = (D + 31) // 32 * 32          # zero rows up to the packed layout's block of 32 inputs
        with torch.no_grad():
            st8 = getattr(self, "_fw_stage", None)
            if st8 is None or st8[0].shape != (Dp, 256):
                w1t = torch.zeros((Dp, 256), dtype=torch.float32, device=self.device)      # rows D..Dp stay zero
                w2t = torch.empty((256, 256), dtype=torch.float32, device=self.device)
                self._fw_stage = (w1t, w2t, torch.empty_like(w1t), torch.empty_like(w2t))
            w1t, w2t, w1p, w2p = self._fw_stage
            w1t[:D].copy_(a.linear1.weight.detach().t())
            w2t.copy_(a.linear2.weight.detach().t())
            L = _abi.lib()
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            # K-major -> the order the kernel's wavefronts consume (16-byte loads, 4 KB contiguous per wavefront and block)
            _abi.check(L.cn_actor_pack_weights(C.c_void_p(w1t.data_ptr()), Dp, C.c_void_p(w1p.data_ptr()), self._dev_index, st))
            _abi.check(L.cn_actor_pack_weights(C.c_void_p(w2t.data_ptr()), 256, C.c_void_p(w2p.data_ptr()), self._dev_index, st))
            # biases and linear3 are read where they live (float32, contiguous nn.Linear storages: .float().contiguous() is the tensor itself)
            self._fw = dict(w1p=w1p, b1=a.linear1.bias.detach().float().contiguous(),
                            w2p=w2p, b2=a.linear2.bias.detach().float().contiguous(),
                            w3=a.linear3.weight.detach().float().contiguous(), b3=a.linear3.bias.detach().float().contiguous())
        f = self._fw
        vals = dict(w1p=f["w1p"].data_ptr(), b1=f["b1"].data_ptr(), w2p=f["w2p"].data_ptr(), b2=f["b2"].data_ptr(), w3=f["w3"].data_ptr(),
                    b3=f["b3"].data_ptr(), obs_dim=D, obs_dim_padded=Dp, hidden=256, reserved=0)
        if hasattr(self, "_fw_struct"):
            for k, v in vals.items():
                setattr(self._fw_struct, k, v)          # same object: byref()s taken earlier stay valid
        else:
            self._fw_struct = _abi.CnActorWeights(**vals)

    @torch.no_grad()
    def act_mfma(self, obs, out=None, add_noise=True, stream=None, noise_seed=None):
        """Agent.act as ONE kernel (cn_actor_forward): the three Linear layers on the f32 matrix cores with the
        activations in LDS, plus heads, exploration noise and clip.  float32 throughout, like the reference.
        stream: torch stream to enqueue on (default: current).  The exploration noise is keyed by
        (noise_seed, call counter, row); noise_seed defaults to the Agent's own key, callers that split a batch over
        several calls pass `agent.group_noise_seed(g)` so that the groups draw different noise."""
        import ctypes as C
        from . import _abi
        if not hasattr(self, "_fw_struct"):
            self.sync_fused_weights()
        obs = obs.contiguous()
        if out is None:
            out = torch.empty((obs.shape[0], 2), dtype=torch.float32, device=self.device)
        self._fused_calls += 1
        st = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)
        seed = self._noise_seed if noise_seed is None else int(noise_seed)
        _abi.check(_abi.lib().cn_actor_forward(C.byref(self._fw_struct), C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()),
                                               obs.shape[0], self.max_v, self.max_w,
                                               self.explore_sigma if add_noise else 0.0, seed, self._fused_calls,
                                               self._dev_index, st))
        return out

    def group_noise_seed(self, g):
        """Noise key of stream group / rank `g` (distinct per group, derived from the Agent seed)."""
        return (self._noise_seed ^ (0xA0761D6478BD642F * (int(g) + 1))) & 0xFFFFFFFFFFFFFFFF

    def bind_act_mfma(self, obs, out, add_noise=True, stream=None, noise_seed=None):
        """Pre-marshalled act_mfma for fixed obs/out buffers: a zero-argument callable that only enqueues."""
        import ctypes as C
        from . import _abi
        if not hasattr(self, "_fw_struct"):
            self.sync_fused_weights()
        assert obs.is_contiguous() and out.is_contiguous()
        fn, check = _abi.lib().cn_actor_forward, _abi.check
        w = C.byref(self._fw_struct)
        po, pa, n = C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()), obs.shape[0]
        st = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)
        sigma = self.explore_sigma if add_noise else 0.0
        mv, mw, seed = self.max_v, self.max_w, self._noise_seed if noise_seed is None else int(noise_seed)
        keep = (obs, out, self._fw_struct, self._fw)
        dv = self._dev_index

        def call(_keep=keep):
            self._fused_calls = c = self._fused_calls + 1
            rc = fn(w, po, pa, n, mv, mw, sigma, seed, c, dv, st)
            if rc:
                check(rc)
        return call


class Agent(FusedActorMixin):
    """TD3 agent (TD3:129-319) acting on batches of observations that stay on the device."""

    def __init__(self, obs_dim=398, hidden=256, actor_lr=3e-4, critic_lr=3e-4, batch_size=128, memory_size=1_000_000,
                 gamma=0.99, tau=0.005, max_v=0.22, max_w=2.0, noise_std=0.2, noise_clip=0.5, policy_delay=2,
                 explore_sigma=1.0, device="cuda", seed=0, actor_final_init=None, replay_sample="with", n_step=1):
        from . import _abi
        _abi.replay_sample_mode(replay_sample)      # "with" (replacement) | "without" (distinct rows, the reference's random.sample)
        self.replay_sample = replay_sample
        self.device = torch.device(device)
        torch.manual_seed(seed)
        self.actor = Actor(obs_dim, 2, hidden, max_v, max_w).to(self.device)
        self.actor_t = Actor(obs_dim, 2, hidden, max_v, max_w).to(self.device)
        self.q1, self.q2 = Critic(obs_dim, 2, hidden).to(self.device), Critic(obs_dim, 2, hidden).to(self.device)
        self.q1_t, self.q2_t = Critic(obs_dim, 2, hidden).to(self.device), Critic(obs_dim, 2, hidden).to(self.device)
        if actor_final_init:
            # NOT the reference (td3.py:81-95 keeps nn.Linear's default U(+-1/sqrt(256)) everywhere): the DDPG paper's small uniform
            # initialisation of the actor's output layer, an opt-in for the seed sensitivity documented in profiles/r04/train/ (heads
            # that start near the middle of the sigmoid / tanh instead of wherever the default range leaves them)
            with torch.no_grad():
                self.actor.linear3.weight.uniform_(-float(actor_final_init), float(actor_final_init))
                self.actor.linear3.bias.uniform_(-float(actor_final_init), float(actor_final_init))
        for t, s in ((self.actor_t, self.actor), (self.q1_t, self.q1), (self.q2_t, self.q2)):
            t.load_state_dict(s.state_dict())
        fused = self.device.type == "cuda"        # one kernel per optimizer step instead of ~10 per parameter tensor;
        kw = dict(fused=True) if fused else {}
        self.opt_a = torch.optim.Adam(self.actor.parameters(), lr=actor_lr, **kw)
        self.opt_q1 = torch.optim.Adam(self.q1.parameters(), lr=critic_lr, **kw)
        self.opt_q2 = torch.optim.Adam(self.q2.parameters(), lr=critic_lr, **kw)
        self.memory = DeviceReplay(memory_size, obs_dim, self.device)
        self.batch_size, self.gamma, self.tau = batch_size, gamma, tau
        # n_step = W > 1: the replay holds W-step rows (an n-step recorder: Population.bind_record(n_step=W), cn_nstep_record), so the
        # target bootstraps with the recorder's gamma^W; gamma stays the one-step discount
        if not 1 <= int(n_step) <= _abi.CN_NSTEP_MAX:
            raise ValueError("n_step must be 1 ... %d, not %r" % (_abi.CN_NSTEP_MAX, n_step))
        self.n_step = int(n_step)
        self.max_v, self.max_w = max_v, max_w
        self.noise_std, self.noise_clip, self.policy_delay = noise_std, noise_clip, policy_delay
        self.explore_sigma = explore_sigma
        self.gen = torch.Generator(device=self.device).manual_seed(seed)
        self._init_fused_actor(seed)

    @property
    def bootstrap_gamma(self):
        """The discount on the target critics' value: gamma itself for one-step rows, cn_nstep_discount(gamma, n_step) -- the n-step
        recorder's own gamma^n_step, float64 products cast once -- for n-step rows."""
        if self.n_step == 1:
            return self.gamma
        from . import _abi
        return float(_abi.lib().cn_nstep_discount(self.gamma, self.n_step))

    @torch.no_grad()
    def act(self, obs, add_noise=True):
        """Agent.act (TD3:196-223) for a batch: actor, Gaussian noise sigma=1.0, clip."""
        a = self.actor(obs)
        if add_noise:
            a = a + torch.randn(a.shape, generator=self.gen, device=self.device) * self.explore_sigma
        return torch.max(torch.min(a, self._hi), self._lo).contiguous()

    def _update(self, s, a, r, s2, d, target_noise, do_actor):
        """The arithmetic of one TD3 update (TD3:225-285) on a given batch."""
        with torch.no_grad():
            noise = (target_noise * self.noise_std).clamp(-self.noise_clip, self.noise_clip)
            a2 = self.actor_t(s2) + noise                       # not re-clipped to the action bounds (TD3:244-247)
            q_t = torch.min(self.q1_t(s2, a2), self.q2_t(s2, a2))
            y = r + (1.0 - d) * self.bootstrap_gamma * q_t
        l1 = F.mse_loss(self.q1(s, a), y)
        l2 = F.mse_loss(self.q2(s, a), y)
        self.opt_q1.zero_grad(set_to_none=True); l1.backward(); self.opt_q1.step()
        self.opt_q2.zero_grad(set_to_none=True); l2.backward(); self.opt_q2.step()
        if do_actor:
            la = -self.q1(s, self.actor(s)).mean()
            self.opt_a.zero_grad(set_to_none=True); la.backward(); self.opt_a.step()
            with torch.no_grad():
                for t, src in ((self.q1_t, self.q1), (self.q2_t, self.q2), (self.actor_t, self.actor)):
                    pt, ps = list(t.parameters()), list(src.parameters())
                    torch._foreach_mul_(pt, 1.0 - self.tau)                      # TD3:287-299: target*(1-tau) + local*tau
                    torch._foreach_add_(pt, torch._foreach_mul(ps, self.tau))
        return l1.detach()

    # ---- the same update as ONE hipGraph launch (a TD3 update is ~150 small kernels: at batch 128 the eager path is bound by
    # launch overhead, 1.5 ms per update on an MI355X) ------------------------------------------------------------------------
    def enable_graphs(self):
        """Capture the update (replay sampling + target noise + _update) into two hipGraphs -- critics only, and critics +
        actor + soft updates -- which learn() then replays when it is called without an explicit batch.  The arithmetic is
        _update's; what differs from the eager path: the optimizers are rebuilt with capturable=True (step counters on the
        device), and the replay indices and the target noise come from torch's default CUDA generator inside the graph
        (seeded by Agent(seed=...)) instead of torch.randint / the Agent's own generator.  Parameters and optimizer state are
        left exactly as they were (the capture's warm-up runs on a copy of them)."""
        if self.device.type != "cuda":
            raise RuntimeError("enable_graphs needs a HIP device")
        if getattr(self, "_graphs", None):
            return
        if self.replay_sample != "with":
            raise RuntimeError("the captured PyTorch update draws its own indices with replacement; replay_sample='without' runs "
                               "eagerly or through enable_fused_update()")
        B, dev = self.batch_size, self.device
        nets = (self.actor, self.actor_t, self.q1, self.q1_t, self.q2, self.q2_t)
        saved = [[p.detach().clone() for p in m.parameters()] for m in nets]
        old_state = [o.state_dict() for o in (self.opt_a, self.opt_q1, self.opt_q2)]
        lr = [o.param_groups[0]["lr"] for o in (self.opt_a, self.opt_q1, self.opt_q2)]
        self.opt_a = torch.optim.Adam(self.actor.parameters(), lr=lr[0], fused=True, capturable=True)
        self.opt_q1 = torch.optim.Adam(self.q1.parameters(), lr=lr[1], fused=True, capturable=True)
        self.opt_q2 = torch.optim.Adam(self.q2.parameters(), lr=lr[2], fused=True, capturable=True)
        mem = self.memory

        def one(do_actor):
            # indices from the DEVICE-side fill level (DeviceReplay.size_dev): no host value is frozen into the graph, and an
            # index can never reach a row that was not written (float32 rounding of u * size is clamped to size - 1)
            u = torch.rand(B, device=dev)
            idx = torch.minimum((u * mem.size_dev.to(torch.float32)).long(), (mem.size_dev - 1).clamp(min=0))
            noise = torch.randn((B, 2), device=dev)
            return self._update(mem.s[idx], mem.a[idx], mem.r[idx], mem.s2[idx], mem.d[idx], noise, do_actor)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):                       # warm-up: allocator, optimizer state, autograd graphs of both shapes
                one(False); one(True)
        torch.cuda.current_stream(dev).wait_stream(side)
        self._graphs, self._g_loss = {}, {}
        for do_actor in (False, True):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._g_loss[do_actor] = one(do_actor)
            self._graphs[do_actor] = g
        # back to the state enable_graphs() was called in: parameters, and the optimizers' moments / step counters
        with torch.no_grad():
            for m, ps in zip(nets, saved):
                for p_, q_ in zip(m.parameters(), ps):
                    p_.copy_(q_)
            for o, st in zip((self.opt_a, self.opt_q1, self.opt_q2), old_state):
                for i, p_ in enumerate(o.param_groups[0]["params"]):
                    cur = o.state[p_]
                    prev = st["state"].get(i)
                    if prev is None:
                        cur["exp_avg"].zero_(); cur["exp_avg_sq"].zero_(); cur["step"].zero_()
                    else:
                        cur["exp_avg"].copy_(prev["exp_avg"]); cur["exp_avg_sq"].copy_(prev["exp_avg_sq"])
                        cur["step"].fill_(float(prev["step"]))
        torch.cuda.synchronize(dev)

    # ---- the same update as 7 (+ 5) hand-written launches: libcrowdnav's cn_td3_update (csrc/crowdnav_td3.hip) ----------------------
    def enable_fused_update(self):
        """Hand the update to cn_td3_update: forward / backward GEMMs of the six networks on the f32 matrix cores, weight gradients
        and soft updates folded into the Adam step, TD target / heads inside the GEMMs, replay indices and target noise
        drawn on the device -- 7 launches for the critic step, 5 more with the actor and the targets, against ~150 through PyTorch.  The
        networks stay these nn.Modules (the kernels step their parameter storages in place); Adam's moments restart from zero
        inside the library (torch.optim state is not carried over), so call this before training, not in the middle of it."""
        if self.device.type != "cuda":
            raise RuntimeError("enable_fused_update needs a HIP device")
        if getattr(self, "_fused", None):
            return
        self._fused = FusedLearner("td3", self.fused_config(), self.device, self._dev_index, replay_sample=self.replay_sample)

    def fused_config(self):
        """The cn_td3_config of this agent: its hyper-parameters, its six networks' storages, its replay ring and its seed."""
        from . import _abi
        og = self.opt_a.param_groups[0]
        return _abi.CnTd3Config(obs_dim=self.actor.linear1.in_features, hidden=self.actor.linear1.out_features, batch=self.batch_size,
                                policy_delay=self.policy_delay, gamma=self.bootstrap_gamma, tau=self.tau, lr_actor=og["lr"],
                                lr_critic=self.opt_q1.param_groups[0]["lr"], beta1=og["betas"][0], beta2=og["betas"][1], eps=og["eps"],
                                noise_std=self.noise_std, noise_clip=self.noise_clip, max_v=self.max_v, max_w=self.max_w, reserved=0.0,
                                actor=mlp_of(self.actor), actor_t=mlp_of(self.actor_t), q1=mlp_of(self.q1), q1_t=mlp_of(self.q1_t),
                                q2=mlp_of(self.q2), q2_t=mlp_of(self.q2_t), seed=self._noise_seed, **self.memory.ring_fields())

    def _fused_learn(self, step, batch=None, target_noise=None):
        from . import _abi
        bs = keep = None
        if batch is not None:
            s, a, r, s2, d = [t.contiguous().float() for t in batch]
            tn = target_noise.contiguous().float() if target_noise is not None else None
            # the kernels read exactly cn_td3_config.batch rows of every array (fixed at enable_fused_update)
            B, D = self.batch_size, self.actor.linear1.in_features
            if s.shape != (B, D) or s2.shape != (B, D) or a.shape != (B, 2) or r.numel() != B or d.numel() != B or (
                    tn is not None and tn.shape != (B, 2)):
                raise ValueError("cn_td3_update was created for batches of %d x %d; got s %s a %s r %s s2 %s d %s noise %s" % (
                    B, D, tuple(s.shape), tuple(a.shape), tuple(r.shape), tuple(s2.shape), tuple(d.shape),
                    None if tn is None else tuple(tn.shape)))
            keep = (s, a, r, s2, d, tn)
            bs = _abi.CnTd3Batch(s.data_ptr(), a.data_ptr(), r.data_ptr(), s2.data_ptr(), d.data_ptr(),
                                 tn.data_ptr() if tn is not None else None)
        return self._fused.update(int(step % self.policy_delay == 0), batch=bs, keep=keep)      # the first critic's loss

    def learn(self, step, batch=None, target_noise=None):
        """One TD3 update (TD3:225-285): clipped target-policy noise added to the target actor's action (the
        reference does not re-clip the noisy action to the action bounds, TD3:244-247), min of the two target
        critics, MSE critic losses with one Adam step each, and every `policy_delay` steps the actor step plus
        the three soft updates.  `batch` = (s, a, r[B,1], s2, d[B,1]) and `target_noise` [B,2] (before the clip)
        override the replay sample / the generator -- used by the parity test against the reference's update.
        Returns the first critic's loss as a 0-d tensor (no host synchronisation)."""
        if getattr(self, "_fused", None):
            if batch is None and not self.memory.ready(self.batch_size):
                return None
            return self._fused_learn(step, batch, target_noise)
        if batch is None:
            if not self.memory.ready(self.batch_size):
                return None
            if getattr(self, "_graphs", None) and target_noise is None:
                do_actor = step % self.policy_delay == 0
                self._graphs[do_actor].replay()
                return self._g_loss[do_actor]
            batch = self.memory.sample(self.batch_size, replace=self.replay_sample == "with")
        s, a, r, s2, d = batch
        if target_noise is None:
            target_noise = torch.randn(a.shape, generator=self.gen, device=self.device)
        return self._update(s, a, r, s2, d, target_noise, step % self.policy_delay == 0)

    def load_models(self, actor_path, critic1_path, critic2_path):
        """Agent.load_models (TD3:313-319): the reference's checkpoints are plain state_dicts with the same
        parameter names (linear1/2/3), so its published .pt files load unchanged; targets are hard-copied."""
        self.actor.load_state_dict(torch.load(actor_path, map_location=self.device))
        self.q1.load_state_dict(torch.load(critic1_path, map_location=self.device))
        self.q2.load_state_dict(torch.load(critic2_path, map_location=self.device))
        for t, src in ((self.actor_t, self.actor), (self.q1_t, self.q1), (self.q2_t, self.q2)):
            t.load_state_dict(src.state_dict())
        if hasattr(self, "_fw_struct"):
            self.sync_fused_weights()

    def save(self, outdir, ep):
        """Target-network checkpoints every 100 episodes (TRAIN:150-154, TD3:304-311)."""
        import os
        os.makedirs(outdir, exist_ok=True)
        torch.save(self.actor_t.state_dict(), os.path.join(outdir, "td3_actor_model_ep%d.pt" % ep))
        torch.save(self.q1_t.state_dict(), os.path.join(outdir, "td3_critic1_model_ep%d.pt" % ep))
        torch.save(self.q2_t.state_dict(), os.path.join(outdir, "td3_critic2_model_ep%d.pt" % ep))

    # ---- the whole training state, for a bit-for-bit resume (cn_td3_state_save / _load, include/crowdnav.h) ---------------------------
    def _side_state(self):
        """What the library does not own: the replay ring's live rows, position, fill level and host bounds, and the noise position."""
        import numpy as np
        m = self.memory
        n = int(m.size_dev.item())
        out = {"replay_" + k: getattr(m, k)[:n].cpu().numpy() for k in ("s", "a", "r", "s2", "d")}
        out.update(replay_pos=np.int64(m.pos_dev.item()), replay_size=np.int64(n), replay_sample_calls=np.int64(m.sample_calls),
                   replay_bounds=np.array([m._lb, m._ub], dtype=np.int64), replay_cap=np.int64(m.cap),
                   noise_state=np.array(self.noise_state(), dtype=np.uint64))
        return out

    def _load_side_state(self, z):
        m = self.memory
        n = int(z["replay_size"])
        if int(z["replay_cap"]) != m.cap or z["replay_s"].shape != (n, m.obs_dim):
            raise ValueError("the saved replay ring is %d x %d of capacity %d; this agent's is %d wide of capacity %d"
                             % (z["replay_s"].shape + (int(z["replay_cap"]), m.obs_dim, m.cap)))
        for k in ("s", "a", "r", "s2", "d"):
            getattr(m, k)[:n].copy_(torch.from_numpy(z["replay_" + k]))
        m.pos_dev.fill_(int(z["replay_pos"])); m.size_dev.fill_(n)
        m.sample_calls = int(z["replay_sample_calls"])
        m._lb, m._ub = (int(x) for x in z["replay_bounds"])
        self.set_noise_state(*(int(x) for x in z["noise_state"]))

    def save_state(self, path):
        """Everything a fused run continues from, as one .npz at `path`: the learner's blob (networks, Adam's moments, step counters,
        bias-correction products, update counter, loss: one launch), the replay ring's live rows [0, size) with its position, fill
        level, sample counter and host bounds, and the fused actor's noise position.  Needs enable_fused_update()."""
        import numpy as np
        if not getattr(self, "_fused", None):
            raise RuntimeError("Agent.save_state saves the fused learner's state: enable_fused_update() first")
        blob = self._fused.save_state().numpy().copy()
        with open(path, "wb") as f:
            np.savez(f, blob=blob, **self._side_state())

    def load_state(self, path):
        """Continue, bit for bit, where save_state(path) stood: the same Agent arguments and enable_fused_update() first.  The packed
        actor is re-packed when it exists."""
        import numpy as np
        if not getattr(self, "_fused", None):
            raise RuntimeError("Agent.load_state loads the fused learner's state: enable_fused_update() first")
        with np.load(path) as z:
            self._fused.load_state(z["blob"])
            self._load_side_state(z)
        if hasattr(self, "_fw_struct"):
            self.sync_fused_weights()


class RecorderMixin:
    """bind_record / record / resetting / record_pending over self.agents on self.device: the transitions and finished episodes of
    every agent's environments in one call of two launches (cn_pop_record; cn_nstep_record for n-step rows)."""
    _recorder = None

    def bind_record(self, envs, prev, obs, act, reward, done, elogs, n_step=1):
        """Create the cn_pop_record handle -- n_step = W > 1: the cn_nstep_record handle, whose ring rows are W-step transitions with
        member p's returns discounted by agents[p].gamma; every agent's n_step must then be W, so that its target bootstraps with
        gamma^W -- for fixed buffers.  Per member p: envs[p] its VecEnv (the finished episodes' counters and
        returns are read straight from its state records), prev[p] / obs[p] [n_p, obs_dim], act[p] [n_p, 2], reward[p] [n_p]
        (contiguous float32), done[p] [n_p] (uint8), all on the population's device, and elogs[p] its episode log (rows [>= max_rows,
        8] float32, n int64, tot [5] float64, max_rows: crowdnav.train.DeviceEpisodeLog).  The transitions go to agents[p].memory.
        prev[p] must hold the observation the first record()'s actions are computed from; every record() leaves obs[p] in it."""
        from . import _abi
        from ._fused import FusedNStepRecorder, FusedPopulationRecorder
        lists = [list(x) for x in (envs, prev, obs, act, reward, done, elogs)]
        if any(len(x) != len(self.agents) for x in lists):
            raise ValueError("bind_record takes one environment, one buffer of each kind and one episode log per member")
        n_step = int(n_step)
        differ = [p for p, a in enumerate(self.agents) if a.n_step != n_step]
        if differ:
            raise ValueError("bind_record(n_step=%d): member(s) %s were built with another n_step (%s): their targets would bootstrap "
                             "with another power of gamma than the rows span" % (n_step, differ, [self.agents[p].n_step for p in differ]))
        D, dev = self.agents[0].actor.linear1.in_features, self.agents[0]._dev_index
        members = []
        for p, (ag, e, pv, o, u, r, d, lg) in enumerate(zip(self.agents, *lists)):
            n = o.shape[0]
            f32 = [(pv, (n, D)), (o, (n, D)), (u, (n, 2)), (r, (n,))]
            ok = (all(tuple(t.shape) == sh and t.dtype == torch.float32 for t, sh in f32) and tuple(d.shape) == (n,) and d.dtype == torch.uint8
                  and all(t.is_contiguous() and t.is_cuda and t.get_device() == dev for t in (pv, o, u, r, d))
                  and lg.rows.dtype == torch.float32 and lg.rows.is_contiguous() and lg.rows.shape[0] >= lg.max_rows and lg.rows.shape[1] == 8
                  and lg.n.dtype == torch.int64 and lg.tot.dtype == torch.float64 and lg.tot.numel() == 5
                  and ag.memory.obs_dim == D and e.N == n)
            if not ok:
                raise ValueError("member %d: prev / obs must be [n, %d], act [n, 2], reward [n] (contiguous float32), done [n] (uint8) on %s "
                                 "for an environment of n rows, and the log a DeviceEpisodeLog's tensors" % (p, D, self.device))
            log = _abi.CnEpisodeLog(rows=lg.rows.data_ptr(), max_rows=lg.max_rows, n_dev=lg.n.data_ptr(), tot_dev=lg.tot.data_ptr())
            members.append(_abi.CnPopRecordMember(env=e.h.value, counters=None, last_return=None, prev=pv.data_ptr(), obs=o.data_ptr(),
                                                  action=u.data_ptr(), reward=r.data_ptr(), done=d.data_ptr(), ring=ag.memory.ring_struct(),
                                                  log=log, n=n, reserved=0))
        if n_step > 1:
            members = [_abi.CnNstepMember(rec=m, gamma=a.gamma, reserved_f=0.0) for m, a in zip(members, self.agents)]
            self._recorder = FusedNStepRecorder(members, n_step, D, self.device, dev, keep=lists)
        else:
            self._recorder = FusedPopulationRecorder(members, D, self.device, dev, keep=lists)
        self._record_n = [e.N * n_step for e in lists[0]]         # the most ring rows a call writes: every episode ends with a full window
        return self

    def record(self, launch):
        """Every member's transition and finished episodes of this launch as ONE call of two launches (cn_pop_record; cn_nstep_record
        when bound with n_step > 1) on torch's current stream: the replay write of the rows that are not reset launches, the episode
        log, prev <- obs.  Moves each member's host-side bound on its ring's fill level as DeviceReplay.add_masked does (by the most
        rows the call can have written: n, or n * n_step), so ready() / len() stay right."""
        if self._recorder is None:
            raise RuntimeError("Population.bind_record(envs, prev, obs, act, reward, done, elogs) first: the recorder works on fixed buffers")
        self._recorder.record(launch)
        for a, n in zip(self.agents, self._record_n):
            a.memory._ub = min(a.memory.cap, a.memory._ub + n)

    def resetting(self, p):
        """The recorder's flags of member p (uint8 [n_p], a view): set where the member's next record is a reset launch."""
        if self._recorder is None:
            raise RuntimeError("Population.bind_record first")
        return self._recorder.resetting(p)

    def record_pending(self, p):
        """The n-step recorder's pending store of member p -- views (s [n_p, W, obs_dim], a [n_p, W, 2], ret [n_p, W], count [n_p], clock
        [n_p]) -- which with resetting(p) is the recorder's whole state; () for the one-step recorder, which holds nothing back."""
        if self._recorder is None:
            raise RuntimeError("Population.bind_record first")
        return self._recorder.pending(p) if hasattr(self._recorder, "pending") else ()


class SoloRecorder(RecorderMixin):
    """The recorder of one agent that is updated on its own (Agent.learn): a population's record() for a population of one, which
    crowdnav.train's solo loop uses for n-step rows."""

    def __init__(self, agent):
        self.agents, self.device = [agent], agent.device


class Population(RecorderMixin):
    """P TD3 agents on one device whose updates run as ONE chain of 7 (+ 5) launches (cn_td3_pop_update): member p's update is, bit
    for bit, the update agents[p].enable_fused_update() would run alone.  The agents keep their networks, replay rings, seeds,
    learning rates, gamma and target-noise parameters; they must agree in obs_dim, hidden, batch_size, policy_delay, tau, max_v,
    max_w and Adam's betas / eps (the library names the field and the member otherwise).
    Acting: bind_act(obs_list, out_list) once, then act() is ONE launch for all members (cn_actor_pop_forward) and sync_actors() ONE
    re-pack of all their actors (cn_actor_pop_pack); member p's actions are, bit for bit, agents[p].act_mfma's, and both advance the
    same per-agent noise counter, so the two may be mixed.
    Recording: bind_record(...) once, then record(launch) is ONE call of two launches for all members (cn_pop_record) in place of P x
    (DeviceReplay.add_masked, VecEnv.counters, VecEnv.returns, DeviceEpisodeLog.add) and the copies around them; rings and logs are,
    bit for bit, what those leave.  bind_record(..., n_step=W) for agents built with n_step=W records W-step rows instead
    (cn_nstep_record: include/crowdnav.h), whose windows record_pending(p) shows.
    Evaluating: bind_eval(worlds, quota, metric) once, then evaluate() runs every member's greedy actor in every world -- three
    enqueues per launch for all of them (crowdnav.rollout.DeviceEvaluator, cn_eval_record) -- and returns the fitness [P] on the
    device, which exploit(fitness) takes; the members' noise counters do not move.
    replay_source: "own" (member p's batch comes from its own ring) | "shared" (from the union of all members' rings, uniformly over
    its live rows: include/crowdnav.h, cn_td3_pop_set_replay_source; the rings stay where they are and the recorder is the same)."""

    def __init__(self, agents, replay_sample=None, replay_source="own"):
        agents = list(agents)
        if not agents:
            raise ValueError("a population needs at least one agent")
        a0 = agents[0]
        if any(a.device != a0.device for a in agents) or a0.device.type != "cuda":
            raise ValueError("the agents of a population live on one HIP device")
        if any(getattr(a, "_fused", None) or getattr(a, "_graphs", None) for a in agents):
            raise ValueError("an agent of a population is not updated on its own (enable_fused_update / enable_graphs were called)")
        self.agents, self.device, self.policy_delay, self.batch_size = agents, a0.device, a0.policy_delay, a0.batch_size
        self._fused = FusedPopulation([a.fused_config() for a in agents], self.device, a0._dev_index,
                                      replay_sample=a0.replay_sample if replay_sample is None else replay_sample,
                                      replay_source=replay_source)
        self._actors = self._act_io = self._act_key = None

    def __len__(self):
        return len(self.agents)

    @property
    def replay_source(self):
        return self._fused.replay_source

    def ready(self):
        """Every member's ring holds more than a batch (a host read only while a member's bounds straddle it).  Shared source: the
        rings together hold more than a batch -- DeviceReplay.ready's inequality on the sum of the live sizes, from the sums of the
        rings' bounds, with host reads only while those straddle it.  All members start together either way."""
        if self.replay_source != "shared":
            return all(a.memory.ready(self.batch_size) for a in self.agents)
        n, mems = self.batch_size, [a.memory for a in self.agents]
        if sum(m._lb for m in mems) > n:
            return True
        if sum(m._ub for m in mems) <= n:
            return False
        return sum(m.sync_len() for m in mems) > n

    def learn(self, step):
        """One update of every member; the actor and the targets move when step % policy_delay == 0, as in Agent.learn.  Enqueue-only.
        Returns the members' first-critic losses [P] as a fresh tensor.  The caller gates on ready(): the kernels read each ring's
        live size on the device and do not refuse a ring shorter than the batch."""
        return self._fused.update(int(step % self.policy_delay == 0))

    def _noise_key(self):
        """What cn_actor_pop_create froze into the members' jobs besides the pointers."""
        return [(a._noise_seed, float(a.explore_sigma), float(a.max_v), float(a.max_w)) for a in self.agents]

    def bind_act(self, obs_list, out_list):
        """Create the cn_actor_pop handle for fixed buffers: obs_list[p] [n_p, obs_dim] and out_list[p] [n_p, 2] are member p's
        observations and actions (contiguous float32 on the population's device; n_p may differ and may be 0), read and written in
        place by every act().  Packs the actors once, on torch's current stream."""
        from . import _abi
        from ._fused import FusedPopulationActor, mlp_of
        obs_list, out_list = list(obs_list), list(out_list)
        if len(obs_list) != len(self.agents) or len(out_list) != len(self.agents):
            raise ValueError("bind_act takes one observation and one action buffer per member")
        D, dev = self.agents[0].actor.linear1.in_features, self.agents[0]._dev_index
        members = []
        for p, (a, o, u) in enumerate(zip(self.agents, obs_list, out_list)):
            ok = (o.dim() == 2 and o.shape[1] == D and tuple(u.shape) == (o.shape[0], 2) and o.is_contiguous() and u.is_contiguous()
                  and o.dtype == torch.float32 and u.dtype == torch.float32 and o.is_cuda and u.is_cuda and o.get_device() == dev == u.get_device())
            if not ok or a.actor.linear1.in_features != D or a.actor.linear1.out_features != 256:
                raise ValueError("member %d: obs must be [n, %d] and out [n, 2], contiguous float32 on %s, for an actor of hidden width 256"
                                 % (p, D, self.device))
            members.append(_abi.CnActorPopMember(actor=mlp_of(a.actor), obs=o.data_ptr(), action=u.data_ptr(), n=o.shape[0], reserved=0,
                                                 max_v=a.max_v, max_w=a.max_w, sigma=a.explore_sigma, reserved_f=0.0, seed=a._noise_seed))
        self._actors = FusedPopulationActor(members, D, self.device, self.agents[0]._dev_index, keep=(obs_list, out_list))
        self._act_io, self._act_key = (obs_list, out_list), self._noise_key()
        self._actors.pack()
        return self

    def _bound(self):
        if self._actors is None:
            raise RuntimeError("Population.bind_act(obs_list, out_list) first: the one-launch actor works on fixed buffers")
        if self._act_key != self._noise_key():       # set_noise_state / explore_sigma changed a member's key: the jobs are rebuilt
            self.bind_act(*self._act_io)
        return self._actors

    @torch.no_grad()
    def act(self, add_noise=True):
        """Every member's Agent.act on its bound observations as ONE launch (cn_actor_pop_forward) on torch's current stream; the
        actions land in the bound buffers, which are returned.  Each agent's call counter advances as in act_mfma (it keys the
        noise whether or not noise is added), so noise_state() / set_noise_state() cover both paths."""
        actors = self._bound()
        for a in self.agents:
            a._fused_calls += 1
        actors.forward([a._fused_calls for a in self.agents], add_noise)
        return self._act_io[1]

    def sync_actors(self):
        """Re-pack every member's actor from its nn.Linear storages (cn_actor_pop_pack: one launch on torch's current stream, no
        transposed staging copy); call after the weights change, as sync_fused_weights for one agent."""
        self._bound().pack()

    def actor_weights(self, p):
        """The CnActorWeights of member p (cn_actor_pop_weights): usable with cn_actor_forward / cn_rollout_policy while this
        population's binding lives."""
        return self._bound().weights(p)

    # ---- population-based training: cn_td3_pop_pbt_bind / cn_td3_pop_exploit (include/crowdnav.h) -----------------------------------
    PBT_BOUNDS = dict(lr_actor=(1e-5, 1e-2), lr_critic=(1e-5, 1e-2), gamma=(0.9, 0.9999), noise_std=(0.02, 1.0), noise_clip=(0.05, 2.0))

    def bind_pbt(self, n_replace, factor=(0.8, 1.2), explore=("lr_actor", "lr_critic", "noise_std"), bounds=None, min_episodes=10, seed=0,
                 elogs=None):
        """Set up exploit / explore: at every exploit() the n_replace worst members take over the networks and the optimizer state of
        members among the n_replace best, and the hyper-parameters named in `explore` (of lr_actor, lr_critic, gamma, noise_std,
        noise_clip) are multiplied by one of the two factors and clamped to bounds[name] = (lo, hi); the others are inherited.
        bounds: a dict overriding PBT_BOUNDS per name; a default bound is widened to hold every member's starting value.  elogs: the
        members' episode logs (as bind_record takes them; tot is read as CUMULATIVE totals) -- exploit() without a fitness then ranks
        by the mean return of the episodes finished since the last applied call and does nothing while a member has fewer than
        min_episodes new ones."""
        from . import _abi
        names = _abi.CN_PBT_HYPER_NAMES
        unknown = [n for n in tuple(explore) + tuple(bounds or ()) if n not in names]
        if unknown:
            raise ValueError("unknown hyper-parameter(s) %s: population-based training knows %s" % (", ".join(map(repr, unknown)), ", ".join(names)))
        if "gamma" in explore and any(a.n_step > 1 for a in self.agents):
            raise ValueError("gamma cannot be explored with n_step > 1: the device tables hold the bootstrap discount gamma^n_step, "
                             "and the recorder's window weights would not follow it")
        start = [self._pbt_hypers(a) for a in self.agents]
        lo, hi = [], []
        for k, n in enumerate(names):
            if bounds and n in bounds:
                l, h = bounds[n]
            else:
                l, h = self.PBT_BOUNDS[n]
                l, h = min([l] + [s[k] for s in start]), max([h] + [s[k] for s in start])
            lo.append(l); hi.append(h)
        cfg = _abi.CnTd3PbtConfig(n_replace=int(n_replace), min_episodes=int(min_episodes), explore_mask=sum(1 << names.index(n) for n in set(explore)),
                                  reserved=0, factor=tuple(float(f) for f in factor), lo=tuple(lo), hi=tuple(hi), seed=int(seed) & (2 ** 64 - 1))
        logs = None
        if elogs is not None:
            elogs = list(elogs)
            if len(elogs) != len(self.agents):
                raise ValueError("bind_pbt takes one episode log per member")
            logs = [_abi.CnEpisodeLog(rows=lg.rows.data_ptr(), max_rows=lg.max_rows, n_dev=lg.n.data_ptr(), tot_dev=lg.tot.data_ptr()) for lg in elogs]
        self._fused.pbt_bind(cfg, logs, keep=elogs)
        return self

    @staticmethod
    def _pbt_hypers(a):
        """An agent's five hyper-parameters in CN_PBT_* order, as fused_config() hands them to the library."""
        return [a.opt_a.param_groups[0]["lr"], a.opt_q1.param_groups[0]["lr"], a.bootstrap_gamma, a.noise_std, a.noise_clip]

    def exploit(self, fitness=None):
        """One exploit / explore step (cn_td3_pop_exploit: two launches on torch's current stream, no host read), then sync_actors()
        when the actors are bound: the re-pack reads the nn.Linear storages that were just overwritten.  fitness: float32 [P] on the
        device, higher is better; None = from the logs bound by bind_pbt."""
        self._fused.exploit(fitness)
        if self._actors is not None:
            self.sync_actors()

    def pbt_state(self):
        """One device-to-host copy of the PBT state -> dict(calls, applied, members=[dict(src, generation, fitness, lr_actor, lr_critic,
        gamma, noise_std, noise_clip)]).  Also brings the agents' Python-side hyper-parameters (the optimizers' lr, actor_lr,
        critic_lr, gamma, noise_std, noise_clip) up to what the device trains with, so that checkpoints and logs show those."""
        from . import _abi
        st = self._fused.pbt_state()
        members = []
        for p, a in enumerate(self.agents):
            m = st.member[p]
            row = dict(src=int(m.src), generation=int(m.generation), fitness=float(m.fitness))
            row.update({n: float(m.hyper[k]) for k, n in enumerate(_abi.CN_PBT_HYPER_NAMES)})
            members.append(row)
            gamma = a.gamma
            a.actor_lr, a.critic_lr, a.gamma, a.noise_std, a.noise_clip = (row[n] for n in _abi.CN_PBT_HYPER_NAMES)
            if a.n_step > 1:                       # the table's (and the row's) gamma is the bootstrap discount, which is not explored
                a.gamma = gamma
            a.opt_a.param_groups[0]["lr"] = a.actor_lr
            a.opt_q1.param_groups[0]["lr"] = a.opt_q2.param_groups[0]["lr"] = a.critic_lr
        return dict(calls=int(st.calls), applied=int(st.applied), members=members)

    # ---- the whole training state, for a bit-for-bit resume (cn_td3_pop_state_save / _load, include/crowdnav.h) ---------------------
    def save_state(self, outdir):
        """Everything the population continues from, into the directory `outdir`: learner.npz (the blob of all members -- networks,
        Adam's state, counters, losses, the hyper-parameters as the device tables hold them, and the PBT state when bind_pbt was
        called: one launch) and member<p>.npz (member p's replay ring and noise position, as Agent.save_state)."""
        import os
        import numpy as np
        os.makedirs(outdir, exist_ok=True)
        blob = self._fused.save_state().numpy().copy()
        with open(os.path.join(outdir, "learner.npz"), "wb") as f:
            np.savez(f, blob=blob)
        for p, a in enumerate(self.agents):
            with open(os.path.join(outdir, "member%d.npz" % p), "wb") as f:
                np.savez(f, **a._side_state())

    def load_state(self, outdir):
        """Continue, bit for bit, where save_state(outdir) stood: a population built from the same agents' arguments, with bind_pbt
        called (or not) as it was.  Re-packs the bound actors; with PBT bound, the agents' Python-side hyper-parameters follow the
        loaded ones (pbt_state())."""
        import os
        import numpy as np
        with np.load(os.path.join(outdir, "learner.npz")) as z:
            self._fused.load_state(z["blob"])
        for p, a in enumerate(self.agents):
            with np.load(os.path.join(outdir, "member%d.npz" % p)) as z:
                a._load_side_state(z)
        if self._actors is not None:
            self.sync_actors()
        if getattr(self._fused, "_pbt_state", None) is not None:
            self.pbt_state()

    # ---- evaluation on the device: cn_eval_* (include/crowdnav.h) through crowdnav.rollout.DeviceEvaluator -------------------------
    def bind_eval(self, specs, quota=1, metric="success", step="multi"):
        """Set up evaluate(): specs is a list of worlds (Config, ped_init | None, ped_preset_vel | None); job (p, s) is member p's
        greedy actor in world s and feeds group p, so every member is measured in the same worlds with the same seeds.  At most 64
        jobs.  quota: episodes counted per environment; metric: "success" | "return", what the fitness averages over a member's
        worlds.  step: "multi" | "group", how the jobs' environments are stepped (DeviceEvaluator)."""
        from . import _abi
        from .rollout import DeviceEvaluator
        specs = [tuple(s) for s in specs]
        if not specs:
            raise ValueError("bind_eval takes at least one world")
        if metric not in _abi.EVAL_METRIC:
            raise ValueError("metric must be 'success' or 'return', not %r" % (metric,))
        jobs = [(cfg, init, vel, a, p) for p, a in enumerate(self.agents) for (cfg, init, vel) in specs]
        self._evaluator = DeviceEvaluator(jobs, self.agents[0]._dev_index, n_groups=len(self.agents), step=step)
        self._eval_quota, self._eval_metric, self.eval_worlds = int(quota), metric, len(specs)
        return self

    def evaluate(self, poll=16):
        """Every member's greedy actor in every bound world (three enqueues per launch for all of them: DeviceEvaluator.run) -> the
        fitness [P] on the device, float32, ready for exploit(fitness).  The actors are re-packed from the current weights first; the
        members' noise counters are not touched.  evaluator().summary() / .stats(p * worlds + s) hold the details."""
        if getattr(self, "_evaluator", None) is None:
            raise RuntimeError("Population.bind_eval(specs, quota, metric) first")
        ev = self._evaluator
        ev.repack()
        ev.run(self._eval_quota, poll=poll)
        return ev.finish(self._eval_metric)

    def evaluator(self):
        """The DeviceEvaluator bind_eval built: job p * eval_worlds + s is member p in world s."""
        return getattr(self, "_evaluator", None)

    def set_replay_sample(self, replay_sample):
        self._fused.set_replay_sample(replay_sample)

    def set_replay_source(self, replay_source):
        self._fused.set_replay_source(replay_source)

    def batch_src(self, member):
        """{ring, row} [batch, 2] (int64, a view) of `member`'s rows in the last shared update."""
        return self._fused.batch_src(member, self.batch_size)

    def batch_dev(self, member, what, shape):
        return self._fused.batch_dev(member, what, shape)
