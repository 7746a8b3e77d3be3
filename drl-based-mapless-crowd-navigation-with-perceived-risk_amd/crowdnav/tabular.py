"""Q-learning and SARSA, the reference's tabular learners (turtlebot3_rl_sim/src/qlearn.py, sarsa.py with
start_qlearn_training.py, start_sarsa_training.py), for batches of environments that share ONE table; also available as
libcrowdnav's cn_tab_learn_act (csrc/crowdnav_tab.hip) after enable_fused().

What it keeps from the reference:
- the state: observation[-2] and observation[-1] (the last two columns of the obs_layout-1 row: round(x, 3), round(y, 3) of the
  robot, environment_stage_1_original.py:315-320; the scripts' comments call them distance and heading to goal), digitised with
  np.digitize against DISTANCE_BINS (30 edges, d in 0..30) and RADIAN_BINS (32 edges, h in 0..32), and keyed by the STRING
  str(d) + str(h) (start_sarsa_training.py:72): 977 distinct keys, 46 of them shared by two (d, h) pairs -- (1, 10) and (11, 0)
  are both '110'.  STATE_OF[d, h] numbers the keys in order of first appearance for d ascending, then h ascending;
- the table: {(key, action): float}; an absent entry reads 0.0 (getQ), learnQ sets an absent entry to `reward` and moves a
  present one to oldv + alpha * (value - oldv); an entry that holds 0.0 is present; count_same / count_diff count the two writes;
- QLearn.learn: value = reward + gamma * max_a getQ(s2, a);  Sarsa.learn: value = reward + gamma * getQ(s2, a2) with
  a2 = chooseAction(s2) drawn for the update alone (the next step draws its action afresh, start_sarsa_training.py:78, 98);
- chooseAction of both classes, with random.choice(seq) = seq[int(random() * len(seq))] (the reference's Python 2);
- epsilon: `if epsilon > 0.05: epsilon *= epsilon_discount` at the start of every episode; alpha 0.2, gamma 0.9,
  epsilon_discount 0.9986 (configs/qlearn.yaml, sarsa.yaml).

What is batched (n rows, one table).  One learn_act() call is, in this order:
  1. every bootstrap read of the learn phase (max_a Q(s2, a); SARSA: chooseAction(s2), then Q(s2, a2)) sees the table as it stood
     when the call began;
  2. the writes of the kept rows are applied per cell in ascending row order, each by learnQ's rule;
  3. the act phase reads the table after all writes.
For n = 1 that is the reference's loop.  Float64, every operation rounded on its own.

Draws.  Row i of a call takes five uniforms u[i, 0..4]; a slot always means the same draw whether it is consumed or not:
0 the epsilon test; 1-3 Q-learning's noise (1: SARSA's uniform choice); 4 the tie break.  u = None: device_draws(seed, counter,
n, phase), the function cn_tab_learn_act evaluates on the device -- both paths then agree without any array being passed."""
import os
import pickle

import numpy as np
import torch

from .dqn import TWISTS, epsilon_after

DISTANCE_BINS = np.array([round(i, 2) for i in np.arange(0, 3, 0.1)], dtype=np.float64)             # start_sarsa_training.py:41-42
RADIAN_BINS = np.array([round(i, 2) for i in np.arange(-3.14, 3.14, 0.19625)], dtype=np.float64)   # :44-45
N_ACTIONS = 3


def _build_keys():
    keys, index = [], {}
    state_of = np.zeros((len(DISTANCE_BINS) + 1, len(RADIAN_BINS) + 1), dtype=np.int32)
    for d in range(state_of.shape[0]):
        for h in range(state_of.shape[1]):
            k = str(d) + str(h)
            if k not in index:
                index[k] = len(keys)
                keys.append(k)
            state_of[d, h] = index[k]
    return keys, index, state_of


KEYS, KEY_INDEX, STATE_OF = _build_keys()
N_STATES = len(KEYS)                 # 977
K_LEARN, K_ACT = 0x6a09e667f3bcc909, 0xbb67ae8584caa73b      # the per-phase constants of the device draw


def _host(x, dtype=None):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    return x if dtype is None else x.astype(dtype, copy=False)


def digitize(x, bins):
    """np.digitize(x, bins) for float64 x.  A float32 x -- a double of the form round(v, 3) narrowed, as the env's rows are -- is
    compared against the edges NARROWED to float32: float32(0.7) < 0.7, so the double edges would give the wrong bin, while
    narrowing is monotone and two different multiples of 0.001 below 16 never narrow to the same float32, so e <= x on the
    doubles is float32(e) <= float32(x)."""
    x = _host(x)
    if x.dtype == np.float32:
        return np.digitize(x, np.asarray(bins, dtype=np.float64).astype(np.float32))
    return np.digitize(x.astype(np.float64, copy=False), bins)


def digitize_state(obs, return_dh=False):
    """obs [n, >= 2] (or [>= 2]): the state index 0..976 of every row from its last two columns; return_dh: (d, h, state)."""
    o = _host(obs)
    if o.dtype not in (np.float32, np.float64):
        o = o.astype(np.float64)
    o = o.reshape(-1, o.shape[-1])
    d, h = digitize(o[:, -2], DISTANCE_BINS), digitize(o[:, -1], RADIAN_BINS)
    s = STATE_OF[d, h]
    return (d, h, s) if return_dh else s


def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def device_draws(seed, counter, n, phase):
    """[n, 5] float64: u[i, j] = (x >> 11) * 2^-53, x = mix64(mix64(mix64(seed ^ mix64(counter ^ C)) ^ i) ^ j), C = K_LEARN / K_ACT
    for phase "learn" / "act" -- what cn_tab_learn_act draws when u_learn / u_act is NULL."""
    c = np.uint64(K_LEARN if phase == "learn" else K_ACT)
    with np.errstate(over="ignore"):
        base = _mix64(np.array([seed & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) ^ _mix64(np.array([counter & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) ^ c))
        row = _mix64(base ^ np.arange(n, dtype=np.uint64))
        x = _mix64(row[:, None] ^ np.arange(5, dtype=np.uint64)[None, :])
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _pymax(q):
    m = q[:, 0]
    m = np.where(q[:, 1] > m, q[:, 1], m)
    return np.where(q[:, 2] > m, q[:, 2], m)


def _pymin(q):
    m = q[:, 0]
    m = np.where(q[:, 1] < m, q[:, 1], m)
    return np.where(q[:, 2] < m, q[:, 2], m)


def _pick(u, count):
    """int(random() * len(seq)), kept inside the sequence."""
    return np.clip((u * count).astype(np.int64), 0, np.maximum(count - 1, 0))


def choose(table, states, u, epsilon, sarsa):
    """chooseAction for rows of states on `table` [977, 3] (absent = 0.0) -> (actions [n], the q rows it ended with [n, 3])."""
    q = table[states].copy()
    explore = u[:, 0] < epsilon
    if not sarsa:
        mx, mn = _pymax(q), _pymin(q)
        amx, amn = np.abs(mx), np.abs(mn)
        mag = np.where(amx > amn, amx, amn)
        noisy = (q + u[:, 1:4] * mag[:, None]) - (0.5 * mag)[:, None]
        q = np.where(explore[:, None], noisy, q)
    mx = _pymax(q)
    eq = q == mx[:, None]
    count = eq.sum(1)
    k = np.where(count > 1, _pick(u[:, 4], count), 0)
    a = np.argmax(eq & (np.cumsum(eq, 1) == (k + 1)[:, None]), 1)
    if sarsa:
        a = np.where(explore, _pick(u[:, 1], np.full(len(a), N_ACTIONS)), a)
    return a.astype(np.int64), q


class _Tabular:
    ALGO, NAME, SARSA = 0, "qlearn", False

    def __init__(self, epsilon=0.9, alpha=0.2, gamma=0.9, epsilon_discount=0.9986, epsilon_min=0.05, seed=0, device="cpu"):
        self.device = torch.device(device)
        self.alpha, self.gamma = float(alpha), float(gamma)
        self.epsilon, self.epsilon0 = float(epsilon), float(epsilon)
        self.epsilon_discount, self.epsilon_min = float(epsilon_discount), float(epsilon_min)
        self.actions = list(range(N_ACTIONS))
        self.seed = int(seed)
        self._seed = (0xD1B54A32D192ED03 * (int(seed) + 1) ^ 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF
        self._calls = 0
        self._q = np.zeros((N_STATES, N_ACTIONS), dtype=np.float64)
        self._present = np.zeros((N_STATES, N_ACTIONS), dtype=bool)
        self._counts = [0, 0]
        self._h = None
        self._twists = torch.tensor(TWISTS, dtype=torch.float32, device=self.device)

    # ---- the table -----------------------------------------------------------------------------------------------------------
    def table(self):
        """-> (q [977, 3] float64, present [977, 3] bool, (count_same, count_diff)) as host arrays (fused: cn_tab_get)."""
        if self._h is not None:
            from . import _abi
            q = np.zeros((N_STATES, N_ACTIONS), dtype=np.float64)
            p = np.zeros((N_STATES, N_ACTIONS), dtype=np.uint8)
            c = np.zeros(2, dtype=np.int64)
            self._check("cn_tab_get", _abi.lib().cn_tab_get(self._h, q.ctypes.data, p.ctypes.data, c.ctypes.data))
            return q, p.astype(bool), (int(c[0]), int(c[1]))
        return self._q.copy(), self._present.copy(), tuple(self._counts)

    def set_table(self, q, present, counts=(0, 0)):
        present = np.ascontiguousarray(_host(present).astype(bool).reshape(N_STATES, N_ACTIONS))
        q = np.where(present, _host(q, np.float64).reshape(N_STATES, N_ACTIONS), 0.0)
        if self._h is not None:
            from . import _abi
            q = np.ascontiguousarray(q); p8 = np.ascontiguousarray(present.astype(np.uint8)); c = np.array(counts, dtype=np.int64)
            self._check("cn_tab_set", _abi.lib().cn_tab_set(self._h, q.ctypes.data, p8.ctypes.data, c.ctypes.data))
        else:
            self._q, self._present, self._counts = q.copy(), present.copy(), [int(counts[0]), int(counts[1])]

    @property
    def count_same(self):
        return self.table()[2][0]

    @property
    def count_diff(self):
        return self.table()[2][1]

    def getQ(self, state, action):
        return float(self.table()[0][int(state), int(action)])

    def get_qtable(self):
        """The reference's dict {(key, action): value} of the present entries."""
        q, p, _ = self.table()
        return {(KEYS[s], int(a)): float(q[s, a]) for s, a in zip(*np.nonzero(p))}

    def set_q(self, new_q):
        q = np.zeros((N_STATES, N_ACTIONS), dtype=np.float64)
        p = np.zeros((N_STATES, N_ACTIONS), dtype=bool)
        for k, v in new_q.items():
            ok = isinstance(k, tuple) and len(k) == 2 and isinstance(k[0], str) and k[0] in KEY_INDEX
            if not ok or not isinstance(k[1], (int, np.integer)) or not 0 <= int(k[1]) < N_ACTIONS:
                raise ValueError("Q-table key %r is not (one of the %d discrete state strings, an action in 0..2); the reference's "
                                 "`continuous` tables (unbinned decimals as keys) are not supported" % (k, N_STATES))
            q[KEY_INDEX[k[0]], int(k[1])] = float(v)
            p[KEY_INDEX[k[0]], int(k[1])] = True
        self.set_table(q, p)

    def load_q(self, path):
        """utils.load_q: the reference's pickled dict (written by Python 2) becomes the table; the counters restart at 0."""
        with open(path, "rb") as f:
            d = pickle.load(f, encoding="latin1")
        if not isinstance(d, dict):
            raise ValueError("%s does not hold a Q-table dict" % path)
        self.set_q(d)

    def save_q(self, path):
        """save_q: the dict, pickle protocol 2 (the reference's utils.load_q reads it)."""
        with open(path, "wb") as f:
            pickle.dump(self.get_qtable(), f, protocol=2)
        return path

    def save(self, outdir, ep):
        """<algo>_qtable_ep<N>.txt (start_sarsa_training.py:105-108)."""
        os.makedirs(outdir, exist_ok=True)
        return self.save_q(os.path.join(outdir, "%s_qtable_ep%d.txt" % (self.NAME, int(ep))))

    # ---- epsilon -------------------------------------------------------------------------------------------------------------
    def start_episode(self):
        if self.epsilon > self.epsilon_min:
            self.epsilon *= self.epsilon_discount
        return self.epsilon

    def _epsilon_of(self, epsilon, episodes_dev):
        if episodes_dev is not None:
            return epsilon_after(int(episodes_dev) + 1, self.epsilon0, self.epsilon_discount, self.epsilon_min)
        return self.epsilon if epsilon is None else float(epsilon)

    # ---- the fused path ------------------------------------------------------------------------------------------------------
    def _check(self, what, rc):
        if rc != 0:
            from . import _abi
            raise _abi.CrowdNavError("%s: %s" % (what, _abi.lib().cn_tab_last_error().decode()))

    def enable_fused(self):
        """Hand the table to libcrowdnav (cn_tab_create + cn_tab_set): learn_act / learn / chooseAction become cn_tab_learn_act."""
        import ctypes as C
        from . import _abi
        if self.device.type != "cuda":
            raise RuntimeError("enable_fused needs a HIP device")
        if self._h is not None:
            return
        L = _abi.lib()
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        cfg = _abi.CnTabConfig(algo=self.ALGO, reserved=0, alpha=self.alpha, gamma=self.gamma, seed=self._seed)
        h = C.c_void_p()
        self._check("cn_tab_create", L.cn_tab_create(C.byref(cfg), self._dev_index, C.byref(h)))
        q, p, c = self._q, self._present, self._counts
        self._h = h
        self.set_table(q, p, c)

    def __del__(self):
        try:
            if self._h is not None:
                from . import _abi
                _abi.lib().cn_tab_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _fused(self, obs_prev, action_prev, reward, obs, keep, u_learn, u_act, learn, act, epsilon, episodes_dev, want):
        import ctypes as C
        from . import _abi
        dev = self.device

        def f32rows(x):
            x = torch.as_tensor(x, device=dev)
            if x.dim() == 1:
                x = x[None]
            return x if x.dtype == torch.float32 and x.stride(1) == 1 else x.float().contiguous()

        def vec(x, dtype):
            if x is None:
                return None
            x = torch.as_tensor(x, device=dev).reshape(-1)
            if dtype == torch.uint8 and x.dtype == torch.bool:
                return x.contiguous()
            return x.to(dtype).contiguous()
        obs = f32rows(obs)
        n = obs.shape[0]
        obs_prev = f32rows(obs_prev) if learn else None
        if learn and (obs_prev.shape[0] != n or obs_prev.stride(0) != obs.stride(0) or obs_prev.shape[1] != obs.shape[1]):
            obs_prev = obs_prev.contiguous(); obs = obs.contiguous()
            if obs_prev.shape != obs.shape:
                raise ValueError("obs_prev %s and obs %s differ in shape" % (tuple(obs_prev.shape), tuple(obs.shape)))
        ap, rw, kp = vec(action_prev, torch.int32), vec(reward, torch.float32), vec(keep, torch.uint8)

        def draws(u):
            if u is None:
                return None
            if not isinstance(u, torch.Tensor):
                u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64))
            return u.to(dev, torch.float64).reshape(n, 5).contiguous()
        ul, ua = draws(u_learn), draws(u_act)
        for name, t in (("action_prev", ap), ("reward", rw), ("keep", kp)):
            if t is not None and t.numel() != n:
                raise ValueError("%s has %d entries for %d rows" % (name, t.numel(), n))
        out = dict(action=torch.empty(n, dtype=torch.int32, device=dev), twist=torch.empty((n, 2), dtype=torch.float32, device=dev))
        if want:
            out.update(state=torch.empty(n, dtype=torch.int32, device=dev), state_prev=torch.empty(n, dtype=torch.int32, device=dev),
                       q_row=torch.empty((n, 3), dtype=torch.float64, device=dev))

        def ptr(t):
            return t.data_ptr() if t is not None else None
        io = _abi.CnTabIO(obs_prev=ptr(obs_prev), obs=obs.data_ptr(), obs_ld=obs.stride(0), n=n, col=obs.shape[1] - 2, learn=int(learn),
                          act=int(act), action_prev=ptr(ap), reward=ptr(rw), done=None, keep=ptr(kp),
                          epsilon=self.epsilon0 if episodes_dev is not None else (self.epsilon if epsilon is None else float(epsilon)),
                          epsilon_discount=self.epsilon_discount, epsilon_min=self.epsilon_min,
                          episodes_dev=episodes_dev.data_ptr() if episodes_dev is not None else None,
                          u_learn=ptr(ul), u_act=ptr(ua), counter=self._calls, action=out["action"].data_ptr(), twist=out["twist"].data_ptr(),
                          state=ptr(out.get("state")), state_prev=ptr(out.get("state_prev")), q_row=ptr(out.get("q_row")))
        self._keep = (obs_prev, obs, ap, rw, kp, ul, ua, episodes_dev, out)       # alive until the next call: the launch is asynchronous
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self._check("cn_tab_learn_act", _abi.lib().cn_tab_learn_act(self._h, C.byref(io), st))
        return out

    # ---- one launch ----------------------------------------------------------------------------------------------------------
    def learn_act(self, obs_prev, action_prev, reward, obs, keep=None, u_learn=None, u_act=None, learn=True, act=True,
                  epsilon=None, episodes_dev=None, want=False):
        """learn (the transitions (obs_prev, action_prev, reward, obs) of the rows with keep != 0), then chooseAction(obs) on the
        table after all writes.  -> dict(action int32 [n], twist [n, 2]; want: state, state_prev, q_row).  episodes_dev (an int64
        scalar tensor): epsilon = the schedule from this agent's initial epsilon after that many finished episodes + 1."""
        if not learn and not act:
            raise ValueError("neither learn nor act")
        counter = self._calls
        if self._h is not None:
            out = self._fused(obs_prev, action_prev, reward, obs, keep, u_learn, u_act, learn, act, epsilon, episodes_dev, want)
            self._calls += 1
            return out
        self._calls += 1
        eps = self._epsilon_of(epsilon, episodes_dev)
        o2 = _host(obs)
        o2 = o2.reshape(-1, o2.shape[-1])
        n = o2.shape[0]
        s2 = digitize_state(o2)
        out = {}
        if learn:
            s1 = digitize_state(_host(obs_prev))
            a1 = _host(action_prev).reshape(-1).astype(np.int64)
            r = _host(reward).reshape(-1).astype(np.float32).astype(np.float64)        # the env's float32 reward, widened
            kp = np.ones(n, dtype=bool) if keep is None else _host(keep).reshape(-1) != 0
            q0 = self._q.copy()                                                        # the table as the call began (absent = 0.0)
            if self.SARSA:
                ul = device_draws(self._seed, counter, n, "learn") if u_learn is None else _host(u_learn, np.float64).reshape(n, 5)
                a2, _ = choose(q0, s2, ul, eps, True)
                boot = q0[s2, a2]
            else:
                boot = _pymax(q0[s2])
            value = r + self.gamma * boot
            q, present, alpha = self._q, self._present, self.alpha
            for i in range(n):                                                         # learnQ, ascending rows
                if not kp[i] or not 0 <= a1[i] < N_ACTIONS:
                    continue
                s, a = s1[i], a1[i]
                if not present[s, a]:
                    q[s, a] = r[i]; present[s, a] = True
                    self._counts[0] += 1
                else:
                    old = float(q[s, a])
                    q[s, a] = old + alpha * (float(value[i]) - old)
                    self._counts[1] += 1
            if want:
                out["state_prev"] = torch.as_tensor(s1.astype(np.int32), device=self.device)
        if act:
            ua = device_draws(self._seed, counter, n, "act") if u_act is None else _host(u_act, np.float64).reshape(n, 5)
            a, qrow = choose(self._q, s2, ua, eps, self.SARSA)
            out["action"] = torch.as_tensor(a.astype(np.int32), device=self.device)
            out["twist"] = self._twists[out["action"].long()]
            if want:
                out["q_row"] = torch.as_tensor(qrow, device=self.device)
        if want:
            out["state"] = torch.as_tensor(s2.astype(np.int32), device=self.device)
        return out

    def chooseAction(self, obs, u=None, epsilon=None, return_q=False):
        """chooseAction for a batch of observations -> action indices int32 [n] (return_q: also the rows it ended with)."""
        out = self.learn_act(None, None, None, obs, u_act=u, learn=False, act=True, epsilon=epsilon, want=return_q)
        return (out["action"], out["q_row"]) if return_q else out["action"]

    def act(self, obs, add_noise=False):
        """The twist [n, 2] of chooseAction's index (greedy unless add_noise) -- rollout.evaluate's call."""
        return self.learn_act(None, None, None, obs, learn=False, act=True, epsilon=None if add_noise else 0.0)["twist"]

    def learn(self, obs_prev, action_prev, reward, obs, u=None, keep=None, epsilon=None):
        """learn for a batch of explicit transitions; u [n, 5]: the draws of SARSA's chooseAction(s2)."""
        self.learn_act(obs_prev, action_prev, reward, obs, keep=keep, u_learn=u, learn=True, act=False, epsilon=epsilon)


class QLearn(_Tabular):
    """qlearn.py's QLearn.  (The reference's constructor loads qlearn_qtable_ep3000.txt; here that is load_q().)"""
    ALGO, NAME, SARSA = 0, "qlearn", False


class Sarsa(_Tabular):
    """sarsa.py's Sarsa."""
    ALGO, NAME, SARSA = 1, "sarsa", True
