"""DQN, the reference's discrete learner (turtlebot3_rl_sim/src/deepq.py, memory.py, start_dqn_training.py), in PyTorch-ROCm with
action selection and the update also available as libcrowdnav's cn_dqn_act / cn_dqn_update (csrc/crowdnav_dqn.hip).

What it keeps from the reference:
- network (deepq.py:102-127, TRAIN_DQN:55-57): Linear(361, 300) - ReLU - Linear(300, 300) - ReLU - Linear(300, 3), weights
  lecun_uniform = U(+-sqrt(3 / fan_in)), biases zero (Keras's RNG stream is not reproduced, only the distribution); the target
  network is a second model, hard-copied every `target_update` updates (TRAIN_DQN:123-124, deepq.py:136-148);
- inputs: the first `obs_dim` = 361 columns of the obs_layout-1 observation (its 363-wide rows are read through a row stride);
- hyper-parameters: batch 64, learnStart 64, memory 1e6, target 10 000 (TRAIN_DQN:51-54), gamma 0.99, lr 2.5e-4, epsilon
  discount 0.995 (configs/dqn.yaml), RMSprop(rho 0.9, epsilon 1e-6) (deepq.py:124);
- learn() = learnOnMiniBatch (deepq.py:219-266): Y = Q(s) with Y[a] = r if final else r + gamma max Q'(s2), Q' = the online
  network until the first target copy (TRAIN_DQN:115-118); a final sample adds the row (s2, [r, r, r]); Keras's fit(batch_size = 64)
  shuffles the 64 + F rows and takes one RMSprop step on the first 64 and, when F > 0, a second on the other F, against the same Y;
- selectAction (deepq.py:178-184): with probability epsilon a uniform index, else argmax with ties to the lowest index; the index
  maps to the twists of environment_stage_1_original.py:412-425; epsilon *= 0.995 at the start of every episode while > 0.05.
Replay: td3.DeviceReplay with the action index in column 0 of its action rows; sampling with replacement by default,
replay_sample="without" draws distinct rows as the reference's random.sample does (memory.py:23)."""
import json
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._fused import FusedLearner, mlp_of
from .td3 import DeviceReplay

TWISTS = ((0.22, 0.0), (0.22, 2.0), (0.22, -2.0))     # environment_stage_1_original.py:412-425
PARAM_KEYS = ['nepisodes', 'nsteps', 'updateTargetNetwork', 'explorationRate', 'minibatch_size', 'learnStart', 'learningRate',
              'discountFactor', 'memorySize', 'network_inputs', 'network_outputs', 'network_structure', 'current_epoch']   # TRAIN_DQN:136-138


def epsilon_after(episodes, epsilon=1.0, discount=0.995, floor=0.05):
    """The exploration rate after `episodes` applications of TRAIN_DQN:89-90 (float64, as the reference's Python float)."""
    e = float(epsilon)
    for _ in range(int(episodes)):
        if e > floor:
            e *= discount
        else:
            break
    return e


class QNet(nn.Module):
    def __init__(self, obs_dim=361, hidden=(300, 300), n_actions=3):
        super().__init__()
        self.linear1 = nn.Linear(obs_dim, hidden[0])
        self.linear2 = nn.Linear(hidden[0], hidden[1])
        self.linear3 = nn.Linear(hidden[1], n_actions)
        with torch.no_grad():
            for m in (self.linear1, self.linear2, self.linear3):      # lecun_uniform, zero bias (Keras Dense defaults)
                lim = math.sqrt(3.0 / m.in_features)
                m.weight.uniform_(-lim, lim)
                m.bias.zero_()

    def forward(self, x):
        return self.linear3(F.relu(self.linear2(F.relu(self.linear1(x)))))


class Agent:
    """DQN agent (deepq.DeepQ + the collection side of start_dqn_training.py) on batches of observations that stay on the device."""

    def __init__(self, obs_dim=361, obs_ld=None, hidden=(300, 300), n_actions=3, batch_size=64, learn_start=64, gamma=0.99,
                 lr=2.5e-4, rho=0.9, eps=1e-6, target_update=10000, memory_size=1_000_000, epsilon=1.0, epsilon_discount=0.995,
                 epsilon_min=0.05, device="cuda", seed=0, replay_sample="with"):
        from . import _abi
        _abi.replay_sample_mode(replay_sample)      # "with" (replacement) | "without" (distinct rows, memory.py:23's random.sample)
        self.replay_sample = replay_sample
        self.device = torch.device(device)
        torch.manual_seed(seed)
        self.obs_dim = int(obs_dim)
        self.obs_ld = int(obs_ld if obs_ld is not None else obs_dim)
        if self.obs_ld < self.obs_dim:
            raise ValueError("obs_ld %d < obs_dim %d" % (self.obs_ld, self.obs_dim))
        if len(hidden) != 2 or hidden[0] != hidden[1]:
            raise ValueError("the fused paths take two equal hidden layers (the reference's [300, 300])")
        self.hidden, self.n_actions = tuple(int(h) for h in hidden), int(n_actions)
        self.q = QNet(obs_dim, hidden, n_actions).to(self.device)
        self.q_t = QNet(obs_dim, hidden, n_actions).to(self.device)        # TRAIN_DQN:60-61 builds a second model ...
        self.q_t.load_state_dict(self.q.state_dict())                      # (a copy here: unused until the first update anyway)
        self.opt = torch.optim.RMSprop(self.q.parameters(), lr=lr, alpha=rho, eps=eps)
        self.batch_size, self.learn_start, self.gamma = int(batch_size), int(learn_start), float(gamma)
        self.lr, self.rho, self.eps = float(lr), float(rho), float(eps)
        self.target_update = int(target_update)
        self.memory_size = int(memory_size)
        self.memory = DeviceReplay(memory_size, self.obs_ld, self.device)
        self.epsilon, self.epsilon0 = float(epsilon), float(epsilon)
        self.epsilon_discount, self.epsilon_min = float(epsilon_discount), float(epsilon_min)
        self.updates = 0                       # the PyTorch path's update counter (the fused path keeps its own on the device)
        self.seed = int(seed)
        self._act_seed = (0x9E3779B97F4A7C15 * (int(seed) + 1) ^ 0x5851F42D4C957F2D) & 0xFFFFFFFFFFFFFFFF
        self._replay_seed = (0xD1B54A32D192ED03 * (int(seed) + 1) ^ 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        self._act_calls = 0
        self._gen = torch.Generator(device="cpu").manual_seed(seed)
        self._twists = torch.tensor(TWISTS, dtype=torch.float32, device=self.device)
        self._dev_index = self.device.index if self.device.type == "cuda" and self.device.index is not None else (
            torch.cuda.current_device() if self.device.type == "cuda" else -1)

    # ---- epsilon -------------------------------------------------------------------------------------------------------------
    def start_episode(self):
        """TRAIN_DQN:89-90, at the start of an episode (before its first step)."""
        if self.epsilon > self.epsilon_min:
            self.epsilon *= self.epsilon_discount
        return self.epsilon

    # ---- acting --------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def q_values(self, obs):
        return self.q(obs[:, :self.obs_dim].float())

    @torch.no_grad()
    def select(self, obs, epsilon=None, u=None, pick=None):
        """selectAction (deepq.py:178-184) for a batch: -> action indices [N] (int64).  u / pick: pinned draws (tests)."""
        e = self.epsilon if epsilon is None else float(epsilon)
        idx = torch.argmax(self.q_values(obs), dim=1)                   # first maximum, as np.argmax
        n = idx.shape[0]
        if u is None:
            u = torch.rand(n, generator=self._gen, dtype=torch.float64).to(idx.device)
        if pick is None:
            pick = torch.randint(0, self.n_actions, (n,), generator=self._gen).to(idx.device)
        return torch.where(u.to(idx.device) < e, pick.to(idx.device), idx)

    def act(self, obs, add_noise=False):
        """The twist [N, 2] of selectAction's index (epsilon-greedy when add_noise, greedy otherwise) -- rollout.evaluate's call."""
        return self._twists[self.select(obs, epsilon=None if add_noise else 0.0)]

    def act_fused(self, obs, epsilon=None, episodes_dev=None, out_index=None, out_twist=None, q_out=None):
        """cn_dqn_act: Q on the matrix cores, argmax, the epsilon draw keyed by (seed, call counter, row), one launch.  epsilon None
        = this agent's; episodes_dev (int64 device scalar): the schedule from epsilon0 evaluated on the device for that many
        finished episodes (no host read).  -> (index int32 [N], twist [N, 2])."""
        import ctypes as C
        from . import _abi
        L = _abi.lib()
        n = obs.shape[0]
        if obs.dtype != torch.float32 or obs.stride(1) != 1:
            obs = obs.float().contiguous()
        if out_index is None:
            out_index = torch.empty(n, dtype=torch.int32, device=self.device)
        if out_twist is None:
            out_twist = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        io = _abi.CnDqnActIO(obs=obs.data_ptr(), obs_ld=obs.stride(0), n=n, obs_dim=self.obs_dim, hidden=self.hidden[0], reserved=0,
                             q=mlp_of(self.q),
                             epsilon=self.epsilon0 if episodes_dev is not None else (self.epsilon if epsilon is None else float(epsilon)),
                             epsilon_discount=self.epsilon_discount, epsilon_min=self.epsilon_min,
                             episodes_dev=episodes_dev.data_ptr() if episodes_dev is not None else None,
                             seed=self._act_seed, counter=self._act_calls, action=out_index.data_ptr(), twist=out_twist.data_ptr(),
                             q_out=q_out.data_ptr() if q_out is not None else None)
        self._act_calls += 1
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = L.cn_dqn_act(C.byref(io), self._dev_index, st)
        if rc != 0:
            raise _abi.CrowdNavError("cn_dqn_act: %s" % L.cn_td3_last_error().decode())
        return out_index, out_twist

    # ---- the update ----------------------------------------------------------------------------------------------------------
    def targets(self, s, a, r, s2, d, use_target=None):
        """deepq.py:228-262: (X_batch, Y_batch, source) -- X_batch rows in the reference's order, source[i] = the sample of row i
        (+ B for a final sample's extra s2 row)."""
        B = s.shape[0]
        s, s2 = s[:, :self.obs_dim].float(), s2[:, :self.obs_dim].float()
        a = a.reshape(-1).long(); r = r.reshape(-1).float(); d = d.reshape(-1).float()
        if use_target is None:
            use_target = self.updates >= self.target_update
        with torch.no_grad():
            q = self.q(s)
            qn = (self.q_t if use_target else self.q)(s2)
            t = torch.where(d != 0, r, r + self.gamma * qn.max(dim=1).values)
            Y = q.clone()
            Y[torch.arange(B, device=Y.device), a] = t
        ar = torch.arange(B, device=s.device)
        keep = torch.stack([torch.ones_like(d, dtype=torch.bool), d != 0], 1).reshape(-1)
        src = torch.stack([ar, ar + B], 1).reshape(-1)[keep]            # (one host synchronisation: the row count B + F)
        X = torch.cat([s, s2], 0)[src]
        Yall = torch.cat([Y, r[:, None].expand(B, self.n_actions)], 0)[src]
        return X, Yall, src

    def _update(self, s, a, r, s2, d, perm=None):
        X, Y, src = self.targets(s, a, r, s2, d)
        n = X.shape[0]
        if perm is None:
            perm = torch.randperm(n, generator=self._gen)
        perm = torch.as_tensor(perm, dtype=torch.long).to(X.device)
        losses = []
        for lo in range(0, n, self.batch_size):                    # Keras fit: consecutive chunks of the shuffled rows
            idx = perm[lo:lo + self.batch_size]
            loss = F.mse_loss(self.q(X[idx]), Y[idx])              # mean over the outputs and the chunk's rows
            self.opt.zero_grad(set_to_none=True); loss.backward(); self.opt.step()
            losses.append(loss.detach())
        self.updates += 1
        if self.updates % self.target_update == 0:
            self.q_t.load_state_dict(self.q.state_dict())
        return losses[0]

    def enable_fused_update(self):
        """Hand the update to cn_dqn_update (16 launches, enqueue-only).  RMSprop's accumulators restart from zero inside the
        library and the update counter from 0: call this before training."""
        from . import _abi
        if self.device.type != "cuda":
            raise RuntimeError("enable_fused_update needs a HIP device")
        if getattr(self, "_fused", None):
            return
        cfg = _abi.CnDqnConfig(obs_dim=self.obs_dim, obs_ld=self.obs_ld, hidden=self.hidden[0], batch=self.batch_size,
                               gamma=self.gamma, lr=self.lr, rho=self.rho, eps=self.eps, target_every=self.target_update,
                               learn_start=self.learn_start, q=mlp_of(self.q), q_t=mlp_of(self.q_t), seed=self._replay_seed,
                               **self.memory.ring_fields())
        self._fused = FusedLearner("dqn", cfg, self.device, self._dev_index, loss_shape=(2,), replay_sample=self.replay_sample)

    def _fused_learn(self, batch=None, perm=None):
        from . import _abi
        bs = keep = None
        if batch is not None:
            s, a, r, s2, d = batch
            B = self.batch_size
            s, s2 = s.float().contiguous(), s2.float().contiguous()
            if s.shape != (B, self.obs_ld) or s2.shape != (B, self.obs_ld):
                raise ValueError("cn_dqn_update was created for batches of %d x %d; got s %s s2 %s" % (B, self.obs_ld, tuple(s.shape), tuple(s2.shape)))
            a = a.reshape(-1).to(torch.int32).contiguous(); r = r.reshape(-1).float().contiguous(); d = d.reshape(-1).float().contiguous()
            p = None
            if perm is not None:                                     # the device reads B + F entries: check the count here
                p = torch.as_tensor(perm, dtype=torch.int32).to(self.device).contiguous()
                if p.numel() != B + int((d != 0).sum()):
                    raise ValueError("perm has %d entries; the batch has %d rows after its final samples' extra rows" % (
                        p.numel(), B + int((d != 0).sum())))
            keep = (s, a, r, s2, d, p)
            bs = _abi.CnDqnBatch(s.data_ptr(), a.data_ptr(), r.data_ptr(), s2.data_ptr(), d.data_ptr(),
                                 p.data_ptr() if p is not None else None)
        return self._fused.update(batch=bs, keep=keep)

    def fused_batch(self, what, shape, dtype=torch.float32):
        """A host copy of what the last fused update computed (cn_dqn_batch_dev; synchronises)."""
        return self._fused.batch_dev(what, shape, dtype).cpu()

    def learn(self, step=None, batch=None, perm=None):
        """One learnOnMiniBatch (deepq.py:219-266).  batch = (s [B, obs_ld], a [B] indices, r, s2, d) overrides the replay sample;
        perm = the shuffle of the B + F X_batch rows.  Returns the first chunk's loss as a 0-d tensor (fused: the two chunks'
        losses [2]), or None while the replay holds no more than learn_start rows (TRAIN_DQN:114, deepq.py:221)."""
        if batch is None and not self.memory.ready(self.learn_start):
            return None
        if getattr(self, "_fused", None):
            return self._fused_learn(batch, perm)
        if batch is None:
            s, a2, r, s2, d = self.memory.sample(self.batch_size, replace=self.replay_sample == "with")
            batch = (s, a2[:, 0].round().long(), r, s2, d)
        return self._update(*batch, perm=perm)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------
    def params(self, ep, nepisodes=1500, nsteps=250):
        """TRAIN_DQN:136-142's parameter record."""
        return dict(zip(PARAM_KEYS, [nepisodes, nsteps, self.target_update, self.epsilon, self.batch_size, self.learn_start, self.lr,
                                     self.gamma, self.memory_size, self.obs_dim, self.n_actions, list(self.hidden), int(ep)]))

    def save(self, outdir, ep, nepisodes=1500, nsteps=250):
        """dqn_model_ep<N>.pt (the online network, linear1/2/3) + dqn_model_ep<N>.json (TRAIN_DQN:134-144)."""
        os.makedirs(outdir, exist_ok=True)
        torch.save(self.q.state_dict(), os.path.join(outdir, "dqn_model_ep%d.pt" % ep))
        with open(os.path.join(outdir, "dqn_model_ep%d.json" % ep), "w") as f:
            json.dump(self.params(ep, nepisodes, nsteps), f)

    def load_models(self, path, params_json=None):
        """The online network from `path`, copied to the target (TRAIN_DQN:80-82).  With the json (TRAIN_DQN:63-68): epsilon resumes
        from its explorationRate, which also becomes the start of the schedule (epsilon0) for the episodes that follow."""
        self.q.load_state_dict(torch.load(path, map_location=self.device))
        self.q_t.load_state_dict(self.q.state_dict())
        if params_json and os.path.exists(params_json):
            with open(params_json) as f:
                self.epsilon = float(json.load(f).get("explorationRate", self.epsilon))
            self.epsilon0 = self.epsilon

