"""Batched counterpart of start_td3_training.py (TRAIN:40-168): TD3 on N environments of one MI355X.

    python -m crowdnav.train --scenario training_as_logged --waypoint-reward 0 --envs 16 --updates 16 --launches 25000 --csv --out runs/td3
    python -m crowdnav.train --evaluate --load runs/td3 --load-episode latest --scenario crossing_8

Checkpoints are labelled with the episode count the weights really have behind them (N envs finish episodes in batches, so the
count at a log interval is rarely a round number); every save also rewrites `latest_checkpoint.txt` with that count, and
`--load-episode latest` (the default) reads it -- resume / evaluate commands can be written before the run exists.

`--algo ddpg` trains the reference's baseline learner instead (start_ddpg_training.py, ddpg.py; crowdnav.ddpg): batch 64, actor
lr 1e-4, critic lr 1e-3, tau 0.001 unless --batch / --lr-actor / --lr-critic / --tau are given, no exploration noise
(TRAIN_DDPG:100) unless --ou-noise, checkpoints ddpg_{actor,critic}_model_ep<N>.pt, CSV ddpg_training.csv; `--learner fused` is
cn_ddpg_update.  `--obs-layout 1` is the 363-input observation of the shipped DDPG checkpoints.

`--algo dqn` trains the reference's discrete learner (start_dqn_training.py, deepq.py; crowdnav.dqn) on obs_layout 1 with
--max-steps 250 (dqn.yaml) unless given: the first --dqn-inputs (361) columns, the action index -> twist, epsilon from --epsilon
(1.0, the logged run; dqn.yaml's 0.0 by flag) discounted by --epsilon-discount per finished episode on the device, checkpoints
dqn_model_ep<N>.pt / .json, CSV dqn_training.csv; `--learner fused` is cn_dqn_update, `--evaluate` is greedy:

    python -m crowdnav.train --algo dqn --scenario training_as_logged --waypoint-reward 0 --envs 16 --updates 16 --csv --learner fused

    python -m crowdnav.train --algo ddpg --scenario training_as_logged --waypoint-reward 0 --envs 16 --updates 16 --csv --learner fused
    python -m crowdnav.train --algo ddpg --evaluate --load runs/ddpg --obs-layout 1 --scenario crossing_8

`--algo sac` trains the reference's SAC (sac.py; start_sac_training.py's values taken at their names; crowdnav.sac) on obs_layout 1
with --max-steps 1000 (sac.yaml): cn_sac_act -> env.step -> replay -> learn, batch 64, lr 3e-4, tau 5e-3; --sac-value-net /
--sac-soft-update choose between sac.py as committed (default) and what its calls intend; checkpoints
sac_{actor,critic_v,critic_soft_q}_model_ep<N>.pt, CSV sac_training.csv; `--learner fused` is cn_sac_update:

    python -m crowdnav.train --algo sac --scenario training_as_logged --waypoint-reward 0 --envs 16 --updates 16 --csv --learner fused

`--algo qlearn` / `--algo sarsa` train the reference's tabular learners (start_qlearn_training.py, start_sarsa_training.py; qlearn.py,
sarsa.py; crowdnav.tabular) on obs_layout 1 with --max-steps 200 (qlearn.yaml, sarsa.yaml): ONE Q-table shared by all envs, one
cn_tab_learn_act per launch (learn from the transitions of the launch with keep = ~resetting, then chooseAction on the table after
the writes); --alpha 0.2, --gamma 0.9, --epsilon 0.9 (the yamls' commented value) discounted by --epsilon-discount 0.9986 per
finished episode; checkpoints <algo>_qtable_ep<N>.txt (the reference's pickled dict), CSV <algo>_training.csv; --load-qtable
reads such a file (the published discrete tables included); `--evaluate` acts only (the committed start_qlearn_training.py: the
loaded table, epsilon as given, no learning).  --updates, --memory, --batch and --graphs do not apply and are rejected:

    python -m crowdnav.train --algo sarsa --scenario training_as_logged --waypoint-reward 0 --envs 16 --csv --learner fused

What it keeps from the reference loop: Agent hyper-parameters (TRAIN:62-72), exploration noise sigma = 1.0 with the
clip to v in [0, 0.22], w in [-2, 2], 1-based per-env step counters, `learn()` only once the replay holds more than a
batch, target-network checkpoints named td3_{actor,critic1,critic2}_model_ep<N>.pt, one CSV row per finished episode
(utils.record_data schema).  What is batched: N envs step per launch and `--updates` TD3 updates of `--batch` samples
follow each launch (the reference does one update of 128 per single env step: --envs E --updates E keeps its ratio).

The loop enqueues only -- no host synchronisation per launch: the policy is the whole actor as ONE kernel (cn_actor_forward on
the weights packed after the launch's updates), the env step is the fast kernel (next-step reset: a finished env spends its
next launch on Env.reset, and that launch is not a transition -- it is masked out of the replay on the device; the
observation a finished env returns is the terminal one, so it is the transition's s' as it stands), episode statistics and the
CSV rows accumulate in device tensors and are read once per `--log-every` launches.  `--reset-mode same` keeps the older
path (same-call reset + final_obs) for A/B runs."""
import argparse
import os
import time

import torch

from . import presets
from .config import Config
from .env import VecEnv, VecEnvGroups
from .rollout import EpisodeStats, evaluate
from . import ddpg, dqn, sac, tabular, td3

TABULAR = dict(qlearn=tabular.QLearn, sarsa=tabular.Sarsa)


def scenario_config(scenario, n_envs, max_steps, seed, ped_vmax=None, **switches):
    """-> (Config, ped_init or None, ped_preset_vel or None) of a scenario.  switches: cn_config fields applied on top of it
    (waypoint_reward, scan_f32, wheel_accel, ...)."""
    sw = {k: v for k, v in switches.items() if v is not None}
    if scenario in ("training", "training_as_logged"):
        # training_as_logged: without obstacles 7-14, which the world file creates at one point (presets.training's docstring)
        cfg, init = presets.training(n_envs=n_envs, max_steps=max_steps, seed=seed, drop_cospawned=scenario == "training_as_logged", **sw)
        if ped_vmax is not None:
            cfg.ped_vmax = ped_vmax
        vel = None
    elif scenario == "bench":
        cfg, init, vel = Config(n_envs=n_envs, max_steps=max_steps, seed=seed, ped_cycle_ms=1400, **sw), None, None
    else:
        kind, n = scenario.rsplit("_", 1)
        cfg, init, vel = presets.evaluation(kind, int(n), n_envs=n_envs, max_steps=max_steps, seed=seed, **sw)
    return cfg, init, vel


def make_env(scenario, n_envs, max_steps, seed, device, ped_vmax=None, **switches):
    cfg, init, vel = scenario_config(scenario, n_envs, max_steps, seed, ped_vmax, **switches)
    env = VecEnv(cfg, device=device)
    if init is not None:
        env.set_ped_init(init)
    if vel is not None:
        env.set_ped_preset_vel(vel)
    return env


class DeviceEpisodeLog:
    """Finished episodes, recorded on the device: running totals for the progress line and one row per episode for the CSV
    (success, failure, return, steps, ego / social violations, obstacle-present steps, launch index) -- appended with a
    cumulative-sum scatter, rows of envs that did not finish go to a spare row.  One host read per flush().  On a HIP device add()
    is libcrowdnav's cn_episode_log_add (one launch instead of ~20 PyTorch kernels); `fused=False` keeps the PyTorch formulation."""

    def __init__(self, device, max_rows, fused=True):
        self.max_rows = int(max_rows)
        self.fused = bool(fused) and torch.device(device).type == "cuda"
        self._log = None
        self.rows = torch.zeros((self.max_rows + 1, 8), dtype=torch.float32, device=device)
        self.n = torch.zeros((), dtype=torch.int64, device=device)
        self.tot = torch.zeros(5, dtype=torch.float64, device=device)     # episodes, successes, return sum, step sum, env-steps
        self._flushed = 0

    def _add_fused(self, done, counters, last_return, launch, transitions):
        import ctypes as C
        from . import _abi
        L = _abi.lib()
        dev = self.rows.device
        if self._log is None:
            self._log = _abi.CnEpisodeLog(rows=self.rows.data_ptr(), max_rows=self.max_rows, n_dev=self.n.data_ptr(), tot_dev=self.tot.data_ptr())
        n = done.shape[0]
        d8 = done.contiguous() if done.dtype in (torch.uint8, torch.bool) else (done != 0)
        t8 = transitions.contiguous() if transitions.dtype in (torch.uint8, torch.bool) else (transitions != 0)
        cnt = counters if counters.dtype == torch.int32 and counters.is_contiguous() else counters.to(torch.int32).contiguous()
        ret = last_return if last_return.dtype == torch.float32 and last_return.is_contiguous() else last_return.float().contiguous()
        rc = L.cn_episode_log_add(C.byref(self._log), C.c_void_p(d8.data_ptr()), C.c_void_p(cnt.data_ptr()), cnt.shape[1], C.c_void_p(ret.data_ptr()),
                                  C.c_void_p(t8.data_ptr()), float(launch), n, dev.index if dev.index is not None else torch.cuda.current_device(),
                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise _abi.CrowdNavError("cn_episode_log_add: %s" % L.cn_td3_last_error().decode())

    def add(self, done, counters, last_return, launch, transitions):
        if self.fused:
            return self._add_fused(done, counters, last_return, launch, transitions)
        d = done.bool()
        k = d.to(torch.int64)
        c = torch.cumsum(k, 0)
        idx = torch.where(d, torch.clamp(self.n + c - 1, max=self.max_rows), torch.full_like(c, self.max_rows))
        cf = counters.to(torch.float32)
        row = torch.stack([cf[:, 4], cf[:, 5], last_return, cf[:, 13], cf[:, 10], cf[:, 11], cf[:, 12],
                           torch.full_like(last_return, float(launch))], 1)
        self.rows.index_copy_(0, idx, row)
        self.n.add_(c[-1])
        df = d.to(torch.float64)
        self.tot.add_(torch.stack([df.sum(), (cf[:, 4].double() * df).sum(), (last_return.double() * df).sum(),
                                   (cf[:, 13].double() * df).sum(), transitions.sum().double()]))

    def flush(self):
        """-> (new rows as a CPU tensor, totals since the previous flush as a list); one synchronisation."""
        n = min(int(self.n.item()), self.max_rows)
        new = self.rows[self._flushed:n].cpu()
        self._flushed = n
        tot = self.tot.cpu().tolist()
        self.tot.zero_()
        return new, tot


def resolve_load_episode(load_dir, episode):
    """--load-episode: an integer, or "latest" = the count in <load_dir>/latest_checkpoint.txt (save_checkpoint writes it)."""
    if isinstance(episode, str) and episode.strip().lower() == "latest":
        path = os.path.join(load_dir, "latest_checkpoint.txt")
        if not os.path.exists(path):
            raise FileNotFoundError("--load-episode latest: %s does not exist (no checkpoint was saved into %s)" % (path, load_dir))
        return int(open(path).read().split()[0])
    return int(episode)


def save_checkpoint(agent, outdir, episodes):
    """TRAIN:150-154's checkpoint + the exploration-noise stream's position + the `latest` pointer."""
    agent.save(outdir, episodes)
    open(os.path.join(outdir, "noise_state_ep%d.txt" % episodes), "w").write("%d %d\n" % agent.noise_state())
    tmp = os.path.join(outdir, ".latest_checkpoint.txt.%d" % os.getpid())
    open(tmp, "w").write("%d\n" % episodes)
    os.replace(tmp, os.path.join(outdir, "latest_checkpoint.txt"))


CHECKPOINT_NETS = dict(td3=("actor", "critic1", "critic2"), ddpg=("actor", "critic"), sac=("actor", "critic_v", "critic_soft_q"))


def make_dqn_agent(a, obs_ld, device, memory_size):
    """The DQN learner with the reference's defaults (TRAIN_DQN:45-57); --batch / --target-update / --epsilon override them."""
    if a.dqn_inputs > obs_ld:
        raise ValueError("--dqn-inputs %d > the observation width %d (use --obs-layout 1)" % (a.dqn_inputs, obs_ld))
    return dqn.Agent(obs_dim=a.dqn_inputs, obs_ld=obs_ld, batch_size=a.batch or 64, memory_size=memory_size, epsilon=a.epsilon,
                     epsilon_discount=a.epsilon_discount, target_update=a.target_update, device=device, seed=a.seed,
                     replay_sample=getattr(a, "replay_sample", "with"))


def save_dqn_checkpoint(agent, a, outdir, episodes):
    agent.save(outdir, episodes, nsteps=a.max_steps)
    tmp = os.path.join(outdir, ".latest_checkpoint.txt.%d" % os.getpid())
    open(tmp, "w").write("%d\n" % episodes)
    os.replace(tmp, os.path.join(outdir, "latest_checkpoint.txt"))


def train_dqn(a):
    """start_dqn_training.py:84-152 for N environments: cn_dqn_act (epsilon from the device's count of finished episodes) ->
    env.step -> replay (the index in column 0) -> `--updates` learnOnMiniBatch calls per launch once the replay holds more than
    learnStart rows.  Enqueue-only between log intervals, like train()."""
    dev = a.device
    torch.cuda.set_device(dev)
    env = make_env(a.scenario, a.envs, a.max_steps, a.seed, dev, a.ped_vmax, **env_switches(a))
    agent = make_dqn_agent(a, env.D, "cuda:%d" % dev, a.memory)
    eps0 = a.epsilon
    if a.load:                                      # TRAIN_DQN:62-82: the weights, and epsilon from the parameter record
        a.load_episode = resolve_load_episode(a.load, a.load_episode)
        agent.load_models(os.path.join(a.load, "dqn_model_ep%d.pt" % a.load_episode),
                          os.path.join(a.load, "dqn_model_ep%d.json" % a.load_episode))
        eps0 = agent.epsilon0
    if a.learner == "fused":
        agent.enable_fused_update()
    stats = EpisodeStats()
    os.makedirs(a.out, exist_ok=True)
    resumed = bool(a.load) and os.path.abspath(a.load) == os.path.abspath(a.out)
    obs = env.reset()
    t0 = time.time()
    episodes, env_steps, updates_done = 0, 0, 0
    log = open(os.path.join(a.out, "progress.txt"), "a")
    N = env.N
    resetting = torch.zeros(N, dtype=torch.bool, device=obs.device)
    prev = torch.empty_like(obs)
    act2 = torch.zeros((N, 2), dtype=torch.float32, device=obs.device)
    elog = DeviceEpisodeLog(obs.device, a.max_csv_rows)
    learning = False
    next_ckpt = a.checkpoint_every
    step_s = (env.cfg.dt_ms + env.cfg.scan_latency_ms) / 1000.0
    for it in range(1, a.launches + 1):
        idx, twist = agent.act_fused(obs, episodes_dev=elog.n)               # TRAIN_DQN:89-90, 103-104
        act2[:, 0] = idx.float()
        prev.copy_(obs)
        obs, reward, done = env.step(twist, auto_reset="next")
        keep = ~resetting
        agent.memory.add_masked(prev, act2, reward, obs, done, keep)         # TRAIN_DQN:112
        resetting = done.bool()
        elog.add(done, env.counters(), env.returns()[0], it, keep)
        if not learning:
            learning = agent.memory.ready(agent.learn_start)                # TRAIN_DQN:114, deepq.py:221
        if learning:
            for u in range(a.updates):
                updates_done += 1
                agent.learn(updates_done)
        if it % a.log_every == 0 or it == a.launches:
            rows, tot = elog.flush()
            ne = int(tot[0])
            episodes += ne; env_steps += int(tot[4])
            for r in rows.tolist():
                seen = int(r[6])
                stats.add(int(r[0]), int(r[1]), r[2], int(r[3]), 1.0 - r[4] / seen if seen else float("nan"),
                          1.0 - r[5] / seen if seen else float("nan"), int(r[3]) * step_s)
            agent.epsilon = dqn.epsilon_after(episodes + 1, eps0, a.epsilon_discount)   # what the device used (the json records it)
            if ne:
                line = "launch %6d  env-steps %10d  updates %9d  episodes %8d  success %.3f  mean return %8.1f  epsilon %.3f  %.0f s" % (
                    it, env_steps, updates_done, episodes, tot[1] / ne, tot[2] / ne, agent.epsilon, time.time() - t0)
                print(line, flush=True); log.write(line + "\n"); log.flush()
            if a.csv:
                stats.append_csv(a.out, "dqn_training", resume=resumed)
            if episodes >= next_ckpt:                 # TRAIN_DQN:132-144 (every 100 episodes there), checked at log time
                save_dqn_checkpoint(agent, a, a.out, episodes)
                while next_ckpt <= episodes:
                    next_ckpt += a.checkpoint_every
            if a.time_limit and time.time() - t0 > a.time_limit:
                break
    agent.memory.sync_len()
    save_dqn_checkpoint(agent, a, a.out, episodes)
    last = stats.rows[-500:]
    if last:
        line = "last %d episodes: success %.3f  mean return %.1f  mean steps %.1f | %d updates, %d env-steps, %.0f s" % (
            len(last), sum(r[1] for r in last) / len(last), sum(r[3] for r in last) / len(last), sum(r[4] for r in last) / len(last),
            updates_done, env_steps, time.time() - t0)
        print(line, flush=True); log.write(line + "\n"); log.flush()
    return agent, episodes


def train_sac(a):
    """start_sac_training.py's loop for N environments, on train_dqn's pattern: cn_sac_act -> env.step -> replay -> `--updates`
    learn() calls per launch once the replay holds more than a batch (TRAIN_SAC:127).  Enqueue-only between log intervals."""
    dev = a.device
    torch.cuda.set_device(dev)
    env = make_env(a.scenario, a.envs, a.max_steps, a.seed, dev, a.ped_vmax, **env_switches(a))
    agent = make_agent(a, env.D, "cuda:%d" % dev, memory_size=a.memory)
    if a.load:
        load_checkpoint(agent, a)
        ns = os.path.join(a.load, "noise_state_ep%d.txt" % a.load_episode)
        if os.path.exists(ns):
            agent.set_noise_state(*[int(x) for x in open(ns).read().split()])
    if a.learner == "fused":
        agent.enable_fused_update()
    stats = EpisodeStats()
    os.makedirs(a.out, exist_ok=True)
    resumed = bool(a.load) and os.path.abspath(a.load) == os.path.abspath(a.out)
    obs = env.reset()
    t0 = time.time()
    episodes, env_steps, updates_done = 0, 0, 0
    log = open(os.path.join(a.out, "progress.txt"), "a")
    N = env.N
    resetting = torch.zeros(N, dtype=torch.bool, device=obs.device)
    prev = torch.empty_like(obs)
    elog = DeviceEpisodeLog(obs.device, a.max_csv_rows)
    learning = False
    next_ckpt = a.checkpoint_every
    step_s = (env.cfg.dt_ms + env.cfg.scan_latency_ms) / 1000.0
    for it in range(1, a.launches + 1):
        act = agent.act_fused(obs)                                           # Agent.act: samples, squashes twice, clips
        prev.copy_(obs)
        obs, reward, done = env.step(act, auto_reset="next")
        keep = ~resetting
        agent.memory.add_masked(prev, act, reward, obs, done, keep)
        resetting = done.bool()
        elog.add(done, env.counters(), env.returns()[0], it, keep)
        if not learning:
            learning = agent.memory.ready(agent.batch_size)
        if learning:
            for u in range(a.updates):
                updates_done += 1
                agent.learn(updates_done)
        last_launch = it == a.launches or (a.time_limit and it % a.log_every == 0 and time.time() - t0 > a.time_limit)
        if it % a.log_every == 0 or last_launch:
            rows, tot = elog.flush()
            ne = int(tot[0])
            episodes += ne; env_steps += int(tot[4])
            for r in rows.tolist():
                seen = int(r[6])
                stats.add(int(r[0]), int(r[1]), r[2], int(r[3]), 1.0 - r[4] / seen if seen else float("nan"),
                          1.0 - r[5] / seen if seen else float("nan"), int(r[3]) * step_s)
            if ne:
                line = "launch %6d  env-steps %10d  updates %9d  episodes %8d  success %.3f  mean return %8.1f  mean steps %6.1f  %.0f s" % (
                    it, env_steps, updates_done, episodes, tot[1] / ne, tot[2] / ne, tot[3] / ne, time.time() - t0)
                print(line, flush=True); log.write(line + "\n"); log.flush()
            if a.csv:
                stats.append_csv(a.out, "sac_training", resume=resumed)
            if episodes >= next_ckpt:
                save_checkpoint(agent, a.out, episodes)
                while next_ckpt <= episodes:
                    next_ckpt += a.checkpoint_every
            if last_launch:
                break
    agent.memory.sync_len()
    save_checkpoint(agent, a.out, episodes)
    last = stats.rows[-500:]
    if last:
        line = "last %d episodes: success %.3f  mean return %.1f  mean steps %.1f | %d updates, %.0f updates/s, %d env-steps, %.0f s" % (
            len(last), sum(r[1] for r in last) / len(last), sum(r[3] for r in last) / len(last), sum(r[4] for r in last) / len(last),
            updates_done, updates_done / max(1e-9, time.time() - t0), env_steps, time.time() - t0)
        print(line, flush=True); log.write(line + "\n"); log.flush()
    return agent, episodes


def save_tabular_checkpoint(agent, outdir, episodes):
    agent.save(outdir, episodes)
    tmp = os.path.join(outdir, ".latest_checkpoint.txt.%d" % os.getpid())
    open(tmp, "w").write("%d\n" % episodes)
    os.replace(tmp, os.path.join(outdir, "latest_checkpoint.txt"))


def train_tabular(a):
    """start_sarsa_training.py:48-116 / start_qlearn_training.py for N environments that share one Q-table, on train_dqn's pattern:
    chooseAction for every env after the reset, then per launch env.step -> ONE learn_act (learn the launch's transitions except
    the reset launches, then chooseAction on the table after the writes; epsilon from the device's count of finished episodes).
    --evaluate: the same loop without the learn phase (and no checkpoint: the table does not change)."""
    dev = a.device
    torch.cuda.set_device(dev)
    env = make_env(a.scenario, a.envs, a.max_steps, a.seed, dev, a.ped_vmax, **env_switches(a))
    if env.D < 2:
        raise ValueError("the tabular learners read the last two columns of the observation")
    agent = TABULAR[a.algo](epsilon=a.epsilon, alpha=a.alpha, gamma=a.gamma, epsilon_discount=a.epsilon_discount, seed=a.seed,
                            device="cuda:%d" % dev)
    if a.load_qtable:
        agent.load_q(a.load_qtable)                 # utils.load_q (qlearn.py:23)
    if a.learner == "fused":
        agent.enable_fused()
    learn = not a.evaluate
    stats = EpisodeStats()
    os.makedirs(a.out, exist_ok=True)
    obs = env.reset()
    t0 = time.time()
    episodes, env_steps = 0, 0
    log = open(os.path.join(a.out, "progress.txt"), "a")
    N = env.N
    resetting = torch.zeros(N, dtype=torch.bool, device=obs.device)
    prev = torch.empty_like(obs)
    elog = DeviceEpisodeLog(obs.device, a.max_csv_rows)
    next_ckpt = a.checkpoint_every
    step_s = (env.cfg.dt_ms + env.cfg.scan_latency_ms) / 1000.0
    name = "%s_training%s" % (a.algo, "_test" if a.evaluate else "")
    out = agent.learn_act(None, None, None, obs, learn=False, act=True, episodes_dev=elog.n)      # the first step of every first episode
    for it in range(1, a.launches + 1):
        action = out["action"]
        prev.copy_(obs)
        obs, reward, done = env.step(out["twist"], auto_reset="next")
        keep = ~resetting
        resetting = done.bool()
        elog.add(done, env.counters(), env.returns()[0], it, keep)
        out = agent.learn_act(prev, action, reward, obs, keep=keep, learn=learn, act=True, episodes_dev=elog.n)
        last_launch = it == a.launches or (a.time_limit and it % a.log_every == 0 and time.time() - t0 > a.time_limit)
        if it % a.log_every == 0 or last_launch:
            rows, tot = elog.flush()
            ne = int(tot[0])
            episodes += ne; env_steps += int(tot[4])
            for r in rows.tolist():
                seen = int(r[6])
                stats.add(int(r[0]), int(r[1]), r[2], int(r[3]), 1.0 - r[4] / seen if seen else float("nan"),
                          1.0 - r[5] / seen if seen else float("nan"), int(r[3]) * step_s)
            agent.epsilon = dqn.epsilon_after(episodes + 1, a.epsilon, a.epsilon_discount)      # what the device used
            if ne:
                line = "launch %6d  env-steps %10d  episodes %8d  success %.3f  mean return %8.1f  mean steps %6.1f  epsilon %.3f  %.0f s" % (
                    it, env_steps, episodes, tot[1] / ne, tot[2] / ne, tot[3] / ne, agent.epsilon, time.time() - t0)
                print(line, flush=True); log.write(line + "\n"); log.flush()
            if a.csv:
                stats.append_csv(a.out, name)
            if learn and episodes >= next_ckpt:            # start_sarsa_training.py:105-108 (every 100 episodes there)
                save_tabular_checkpoint(agent, a.out, episodes)
                while next_ckpt <= episodes:
                    next_ckpt += a.checkpoint_every
            if last_launch:
                break
    if learn:
        save_tabular_checkpoint(agent, a.out, episodes)
    last = stats.rows[-500:]
    if last:
        _, present, counts = agent.table()
        line = "last %d episodes: success %.3f  mean return %.1f  mean steps %.1f | %d table entries, %d first writes, %d blends, %d env-steps, %.0f s" % (
            len(last), sum(r[1] for r in last) / len(last), sum(r[3] for r in last) / len(last), sum(r[4] for r in last) / len(last),
            int(present.sum()), counts[0], counts[1], env_steps, time.time() - t0)
        print(line, flush=True); log.write(line + "\n"); log.flush()
    return agent, episodes


def make_agent(a, obs_dim, device, **kw):
    """The learner of --algo with its reference defaults; --batch / --lr-actor / --lr-critic / --tau override them when given."""
    over = {k: v for k, v in (("batch_size", getattr(a, "batch", None)), ("actor_lr", getattr(a, "lr_actor", None)),
                              ("critic_lr", getattr(a, "lr_critic", None)), ("tau", getattr(a, "tau", None))) if v is not None}
    over.update(kw)
    over["replay_sample"] = getattr(a, "replay_sample", "with")
    if getattr(a, "algo", "td3") == "sac":
        over = {dict(critic_lr="q_lr").get(k, k): v for k, v in over.items()}
        if "q_lr" in over:
            over["v_lr"] = over["q_lr"]
        return sac.Agent(obs_dim=obs_dim, device=device, seed=a.seed, n_envs=a.envs, value_net=a.sac_value_net.replace("-", "_"),
                         soft_update=a.sac_soft_update.replace("-", "_"), deterministic=getattr(a, "sac_deterministic", False), **over)
    if getattr(a, "algo", "td3") == "ddpg":
        return ddpg.Agent(obs_dim=obs_dim, device=device, seed=a.seed, n_envs=a.envs, **over)
    return td3.Agent(obs_dim=obs_dim, device=device, seed=a.seed, **over)


def load_checkpoint(agent, a):
    algo = getattr(a, "algo", "td3")
    a.load_episode = resolve_load_episode(a.load, a.load_episode)
    agent.load_models(*[os.path.join(a.load, "%s_%s_model_ep%d.pt" % (algo, n, a.load_episode)) for n in CHECKPOINT_NETS[algo]])


def env_switches(a):
    return dict(waypoint_reward=a.waypoint_reward, scan_f32=a.scan_f32, wheel_accel=a.wheel_accel,
                track_capacity=getattr(a, "track_capacity", None), obs_layout=getattr(a, "obs_layout", None))


def train(a):
    dev = a.device
    algo = getattr(a, "algo", "td3")
    torch.cuda.set_device(dev)        # policy kernels and torch ops of this process all target the env's GPU
    env = make_env(a.scenario, a.envs, a.max_steps, a.seed, dev, a.ped_vmax, **env_switches(a))
    extra = dict(memory_size=a.memory)
    if algo == "td3":
        extra["actor_final_init"] = getattr(a, "actor_final_init", None)
    agent = make_agent(a, env.D, "cuda:%d" % dev, **extra)
    batch = agent.batch_size
    ou = algo == "ddpg" and getattr(a, "ou_noise", False)      # OU noise: the act -> step loop (DDPG:170-196, add_noise=True)
    if a.load:
        load_checkpoint(agent, a)
        ns = os.path.join(a.load, "noise_state_ep%d.txt" % a.load_episode)
        if os.path.exists(ns):           # continue the exploration-noise stream instead of replaying it
            agent.set_noise_state(*[int(x) for x in open(ns).read().split()])
    if a.learner == "fused":
        agent.enable_fused_update()   # cn_td3_update: the update as 7 (+ 5) hand-written launches; cn_ddpg_update: 8
    elif a.graphs and algo == "td3":
        agent.enable_graphs()         # a TD3 update as one hipGraph launch (the eager update is launch-bound at batch 128)
    stats = EpisodeStats()
    os.makedirs(a.out, exist_ok=True)
    # a run continued into the directory it was loaded from appends to that run's CSV (as progress.txt always did)
    resumed = bool(a.load) and os.path.abspath(a.load) == os.path.abspath(a.out)
    obs = env.reset()
    t0 = time.time()
    episodes = 0
    env_steps = 0
    next_ckpt = a.checkpoint_every
    log = open(os.path.join(a.out, "progress.txt"), "a")
    N = env.N
    same = a.reset_mode == "same"
    resetting = torch.zeros(N, dtype=torch.bool, device=obs.device)   # envs whose NEXT launch is their Env.reset
    all_rows = torch.ones(N, dtype=torch.bool, device=obs.device)
    prev = torch.empty_like(obs)
    elog = DeviceEpisodeLog(obs.device, a.max_csv_rows)
    learning = False
    updates_done = 0
    agent.sync_fused_weights()
    step_s = (env.cfg.dt_ms + env.cfg.scan_latency_ms) / 1000.0
    win = []                                                           # (successes, episodes) of the recent log windows
    warned_overflow = False
    for it in range(1, a.launches + 1):
        if ou:
            act = agent.act(obs, add_noise=True, step=it - 1)
        else:
            act = agent.act_mfma(obs, add_noise=True)                  # TD3:196-223 as one kernel, sigma = 1.0 (DDPG: 0), clipped
        prev.copy_(obs)
        if same:
            obs, reward, done = env.step(act, auto_reset="same", want_final=True)
            agent.memory.add_masked(prev, act, reward, env.final_obs, done, all_rows)
            keep = all_rows
        else:
            obs, reward, done = env.step(act, auto_reset="next")
            keep = ~resetting
            agent.memory.add_masked(prev, act, reward, obs, done, keep)    # TRAIN:129-131; s' of a finished env = its terminal obs
            resetting = done.bool()
        if ou:
            agent.reset_noise(done)                                    # TRAIN_DDPG:161
        elog.add(done, env.counters(), env.returns()[0], it, keep)
        if not learning:                                               # TRAIN:132: only once the replay holds more than a batch
            learning = agent.memory.ready(batch)                     # (a host read only while the bounds straddle it; none afterwards)
        if learning:
            for u in range(a.updates):
                updates_done += 1
                agent.learn(updates_done)                              # TRAIN:133-136
            agent.sync_fused_weights()                                 # the actor the next launch acts with
        last_launch = it == a.launches or (a.time_limit and it % a.log_every == 0 and time.time() - t0 > a.time_limit)
        if it % a.log_every == 0 or last_launch:
            rows, tot = elog.flush()
            ne = int(tot[0])
            episodes += ne; env_steps += int(tot[4])
            for r in rows.tolist():
                seen = int(r[6])
                stats.add(int(r[0]), int(r[1]), r[2], int(r[3]), 1.0 - r[4] / seen if seen else float("nan"),
                          1.0 - r[5] / seen if seen else float("nan"), int(r[3]) * step_s)
            if ne:
                win.append((tot[1], ne))
                line = "launch %6d  env-steps %10d  updates %9d  episodes %8d  success %.3f  mean return %8.1f  mean steps %6.1f  %.0f s" % (
                    it, env_steps, updates_done, episodes, tot[1] / ne, tot[2] / ne, tot[3] / ne, time.time() - t0)
                print(line, flush=True); log.write(line + "\n"); log.flush()
            if not warned_overflow:
                sc_ = env.status_counts()
                if sc_["track_overflow"] or sc_["conf_overflow"]:
                    warned_overflow = True
                    line = ("WARNING: %d env(s) outgrew the track table and %d the confirmed-object table (status bits CN_ST_TRACK_OVERFLOW / "
                            "CN_ST_CONF_OVERFLOW): their risk features use the tracks that fit and differ from the reference's unbounded "
                            "lists from there on; --track-capacity 256 (or 128 / 512 / 1024: a wide table in HBM, slower) keeps the "
                            "track list equal to the reference's up to that many tracks" % (sc_["track_overflow"], sc_["conf_overflow"]))
                    print(line, flush=True); log.write(line + "\n"); log.flush()
            if a.csv:
                stats.append_csv(a.out, "%s_training" % algo, resume=resumed)   # incremental: a killed run keeps its rows up to here
            if episodes >= next_ckpt:                                    # TRAIN:150-154 (every 100 episodes there)
                # labelled with the episode count the weights really have behind them (checked at log time, so it can be past
                # the threshold that triggered it)
                save_checkpoint(agent, a.out, episodes)
                while next_ckpt <= episodes:
                    next_ckpt += a.checkpoint_every
            if last_launch:
                break
    agent.memory.sync_len()
    save_checkpoint(agent, a.out, episodes)
    last = stats.rows[-500:]
    if last:
        line = "last %d episodes: success %.3f  mean return %.1f  mean steps %.1f  ego %.3f  social %.3f  | %d updates, %.0f updates/s, %.0f env-steps/s overall" % (
            len(last), sum(r[1] for r in last) / len(last), sum(r[3] for r in last) / len(last), sum(r[4] for r in last) / len(last),
            sum(r[5] for r in last if r[5] == r[5]) / max(1, sum(1 for r in last if r[5] == r[5])),
            sum(r[6] for r in last if r[6] == r[6]) / max(1, sum(1 for r in last if r[6] == r[6])),
            updates_done, updates_done / max(1e-9, time.time() - t0), env_steps / max(1e-9, time.time() - t0))
        print(line, flush=True); log.write(line + "\n"); log.flush()
    if a.csv:
        stats.append_csv(a.out, "%s_training" % algo, resume=resumed)
    return agent, episodes


class MemberEnvs(VecEnvGroups):
    """The environments of a population: group p is member p's own environment handle -- its own seed, the same env indices as a solo
    run's -- instead of a slice of one configuration, so cn_step_multi steps all members with one call and member p sees the
    trajectory of VecEnv(cfgs[p])."""

    def __init__(self, cfgs, device):
        import dataclasses
        self._cfgs = list(cfgs)
        super().__init__(dataclasses.replace(self._cfgs[0], n_envs=self._cfgs[0].n_envs * len(self._cfgs)), groups=len(self._cfgs), device=device)

    def _group_cfg(self, g):
        return self._cfgs[g]


def train_population(a):
    """--population P: P independent TD3 runs, seeds a.seed ... a.seed + P - 1, whose updates are ONE cn_td3_pop_update per update
    (crowdnav.td3.Population) instead of P processes.  Member p has what `train()` with --seed <seed + p> has -- its environment
    handle of --envs environments, its Agent, replay, episode log, statistics -- and writes what that run writes into
    <out>/member<p>/.  Per launch: ONE act launch for all members (--population-act one-launch, Population.act; per-member: P
    act_mfma calls), one grouped environment step (cn_step_multi), P replay writes and P log adds; once EVERY member's replay holds more
    than a batch, --updates population updates and ONE re-pack of the P actors (per-member: P sync_fused_weights, 4 launches each).
    The two --population-act values give the same run, bit for bit.
    Member p's run IS the solo run --seed <seed + p> --learner fused (same parameters, same CSV rows) as long as the members' rings pass
    the batch size on the same launch: a member whose ring is not ready yet (it lost rows to reset launches) holds the others back, so
    that the update counters -- which key the sampling and drive policy_delay -- stay aligned; from then on that member's solo run
    would have started its updates earlier."""
    dev = a.device
    P = a.population
    torch.cuda.set_device(dev)
    members = []
    for p in range(P):
        m = argparse.Namespace(**vars(a))
        m.seed, m.out = a.seed + p, os.path.join(a.out, "member%d" % p)
        members.append(m)
    specs = [scenario_config(a.scenario, a.envs, a.max_steps, m.seed, a.ped_vmax, **env_switches(a)) for m in members]
    envs = MemberEnvs([sp[0] for sp in specs], dev)
    for e, (_, init, vel) in zip(envs.envs, specs):
        if init is not None:
            e.set_ped_init(init)
        if vel is not None:
            e.set_ped_preset_vel(vel)
    agents = [make_agent(m, envs.D, "cuda:%d" % dev, memory_size=a.memory, actor_final_init=getattr(a, "actor_final_init", None)) for m in members]
    pop = td3.Population(agents)
    batch = agents[0].batch_size
    stats = [EpisodeStats() for _ in range(P)]
    logs = []
    for m in members:
        os.makedirs(m.out, exist_ok=True)
        logs.append(open(os.path.join(m.out, "progress.txt"), "a"))
    obs = envs.reset()
    t0 = time.time()
    episodes, env_steps, next_ckpt = [0] * P, [0] * P, [a.checkpoint_every] * P
    N, rows = envs.N, [envs.rows(p) for p in range(P)]
    resetting = torch.zeros(N, dtype=torch.bool, device=obs.device)
    prev = torch.empty_like(obs)
    act = torch.zeros((N, 2), dtype=torch.float32, device=obs.device)
    step_all = envs.bind_step_all(act, auto_reset="next")
    elogs = [DeviceEpisodeLog(obs.device, a.max_csv_rows) for _ in range(P)]
    learning = False
    updates_done = 0
    one_launch = getattr(a, "population_act", "one-launch") == "one-launch"
    if one_launch:
        pop.bind_act([obs[r] for r in rows], [act[r] for r in rows])      # (packs the actors)
    else:
        for ag in agents:
            ag.sync_fused_weights()
    step_s = (envs.cfg.dt_ms + envs.cfg.scan_latency_ms) / 1000.0
    reward, done = envs.reward, envs.done
    for it in range(1, a.launches + 1):
        if one_launch:
            pop.act(add_noise=True)
        else:
            for ag, r in zip(agents, rows):
                ag.act_mfma(obs[r], out=act[r], add_noise=True)
        prev.copy_(obs)
        envs.fork()                                                    # the members' steps wait for the actions ...
        step_all()
        cnt = [e.counters() for e in envs.envs]
        ret = [e.returns()[0] for e in envs.envs]
        envs.join()                                                    # ... and everything below for the steps
        keep = ~resetting
        for p, (ag, r) in enumerate(zip(agents, rows)):
            ag.memory.add_masked(prev[r], act[r], reward[r], obs[r], done[r], keep[r])
            elogs[p].add(done[r], cnt[p], ret[p], it, keep[r])
        resetting = done.bool()
        if not learning:
            learning = pop.ready()                                     # every member: the update counters stay aligned
        if learning:
            for u in range(a.updates):
                updates_done += 1
                pop.learn(updates_done)
            if one_launch:
                pop.sync_actors()
            else:
                for ag in agents:
                    ag.sync_fused_weights()
        last_launch = it == a.launches or (a.time_limit and it % a.log_every == 0 and time.time() - t0 > a.time_limit)
        if it % a.log_every == 0 or last_launch:
            for p, m in enumerate(members):
                new, tot = elogs[p].flush()
                ne = int(tot[0])
                episodes[p] += ne; env_steps[p] += int(tot[4])
                for r in new.tolist():
                    seen = int(r[6])
                    stats[p].add(int(r[0]), int(r[1]), r[2], int(r[3]), 1.0 - r[4] / seen if seen else float("nan"),
                                 1.0 - r[5] / seen if seen else float("nan"), int(r[3]) * step_s)
                if ne:
                    line = "launch %6d  env-steps %10d  updates %9d  episodes %8d  success %.3f  mean return %8.1f  mean steps %6.1f  %.0f s" % (
                        it, env_steps[p], updates_done, episodes[p], tot[1] / ne, tot[2] / ne, tot[3] / ne, time.time() - t0)
                    print("member %2d  %s" % (p, line), flush=True); logs[p].write(line + "\n"); logs[p].flush()
                if a.csv:
                    stats[p].append_csv(m.out, "td3_training")
                if episodes[p] >= next_ckpt[p]:
                    save_checkpoint(agents[p], m.out, episodes[p])
                    while next_ckpt[p] <= episodes[p]:
                        next_ckpt[p] += a.checkpoint_every
            if last_launch:
                break
    for p, m in enumerate(members):
        agents[p].memory.sync_len()
        save_checkpoint(agents[p], m.out, episodes[p])
        last = stats[p].rows[-500:]
        if last:
            line = "last %d episodes: success %.3f  mean return %.1f  mean steps %.1f  | %d updates, %.0f updates/s (x %d members)" % (
                len(last), sum(r[1] for r in last) / len(last), sum(r[3] for r in last) / len(last), sum(r[4] for r in last) / len(last),
                updates_done, updates_done / max(1e-9, time.time() - t0), P)
            print("member %2d  %s" % (p, line), flush=True); logs[p].write(line + "\n"); logs[p].flush()
        if a.csv:
            stats[p].append_csv(m.out, "td3_training")
        logs[p].close()
    return agents, episodes


def run_evaluation(a):
    torch.cuda.set_device(a.device)
    env = make_env(a.scenario, a.envs, a.max_steps, a.seed, a.device, a.ped_vmax, **env_switches(a))
    if getattr(a, "algo", "td3") == "dqn":           # greedy: Agent.act(add_noise=False) takes epsilon = 0
        agent = make_dqn_agent(a, env.D, "cuda:%d" % a.device, 16)
        a.load_episode = resolve_load_episode(a.load, a.load_episode)
        agent.load_models(os.path.join(a.load, "dqn_model_ep%d.pt" % a.load_episode))
    else:
        agent = make_agent(a, env.D, "cuda:%d" % a.device, memory_size=16)
        load_checkpoint(agent, a)
    st = evaluate(env, agent, episodes_per_env=a.episodes_per_env)
    n = len(st.rows)
    print("%s: %d episodes, success %.3f, failure %.3f, mean return %.1f, mean steps %.1f, ego %.3f, social %.3f" % (
        a.scenario, n, sum(r[1] for r in st.rows) / n, sum(r[2] for r in st.rows) / n, sum(r[3] for r in st.rows) / n, sum(r[4] for r in st.rows) / n,
        sum(r[5] for r in st.rows if r[5] == r[5]) / max(1, sum(1 for r in st.rows if r[5] == r[5])),
        sum(r[6] for r in st.rows if r[6] == r[6]) / max(1, sum(1 for r in st.rows if r[6] == r[6]))))
    if a.out:
        print("wrote", st.write_csv(a.out, "%s_training_test_%s" % (getattr(a, "algo", "td3"), a.scenario)))
    return st


def parse_args(argv=None):
    """The command line with the algorithm's defaults resolved (max_steps, obs_layout, out)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenario", default="training", help="training | training_as_logged | bench | {crossing,towards,ahead,random}_{4,8,12,20}")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=3000)
    ap.add_argument("--time-limit", type=float, default=0.0, help="stop after this many seconds (checked at log time); 0 = run all launches")
    ap.add_argument("--max-steps", type=int, default=None, help="nsteps: configs/td3.yaml 1000; configs/dqn.yaml 250 (--algo dqn)")
    ap.add_argument("--updates", type=int, default=4, help="TD3 updates per launch (not qlearn / sarsa: one table update per transition)")
    ap.add_argument("--algo", default="td3", choices=["td3", "ddpg", "dqn", "sac", "qlearn", "sarsa"],
                    help="td3: start_td3_training.py; ddpg: start_ddpg_training.py (crowdnav.ddpg); dqn: start_dqn_training.py (crowdnav.dqn); "
                         "sac: sac.py with start_sac_training.py's values at their names (crowdnav.sac); qlearn / sarsa: the tabular learners "
                         "of start_qlearn_training.py / start_sarsa_training.py (crowdnav.tabular) -- --updates, --memory, --batch and "
                         "--graphs do not apply to them and are rejected")
    ap.add_argument("--alpha", type=float, default=0.2, help="qlearn / sarsa: the learning rate (qlearn.yaml, sarsa.yaml)")
    ap.add_argument("--gamma", type=float, default=0.9, help="qlearn / sarsa: the discount (qlearn.yaml, sarsa.yaml)")
    ap.add_argument("--load-qtable", default=None, help="qlearn / sarsa: a <algo>_qtable_ep<N>.txt to start from (the reference's pickled dict)")
    ap.add_argument("--sac-value-net", default="as-written", choices=["as-written", "intended"], help="sac: the value nets as sac.py:175-176 "
                    "constructs them (hidden width 2, linear3 ~ U(+-hidden)) or as intended (hidden width --hidden, 3e-3)")
    ap.add_argument("--sac-soft-update", default="as-written", choices=["as-written", "intended"], help="sac: sac.py:290 as written (V is pulled "
                    "towards its frozen copy) or as intended (the target follows V)")
    ap.add_argument("--sac-deterministic", action="store_true", help="sac: act with z = mean (the reference's act() always samples)")
    ap.add_argument("--epsilon", type=float, default=None, help="dqn: the initial exploration rate (default 1.0, the logged run; dqn.yaml: 0.0); "
                    "qlearn / sarsa: default 0.9 (sarsa.yaml; qlearn.yaml's commented value)")
    ap.add_argument("--epsilon-discount", type=float, default=None, help="epsilon_discount, applied per episode while > 0.05: dqn.yaml 0.995; "
                    "qlearn.yaml / sarsa.yaml 0.9986")
    ap.add_argument("--target-update", type=int, default=10000, help="dqn: updates between hard target copies (TRAIN_DQN:51)")
    ap.add_argument("--dqn-inputs", type=int, default=361, choices=[361, 363], help="dqn: network inputs (TRAIN_DQN:55: 361 = the first "
                    "361 columns of the obs_layout-1 observation)")
    ap.add_argument("--batch", type=int, default=None, help="TRAIN:62 -> 128 (td3); TRAIN_DDPG:55 -> 64 (ddpg) (not qlearn / sarsa)")
    ap.add_argument("--lr-actor", type=float, default=None, help="default: the algorithm's (td3 3e-4, ddpg 1e-4)")
    ap.add_argument("--lr-critic", type=float, default=None, help="default: the algorithm's (td3 3e-4, ddpg 1e-3)")
    ap.add_argument("--tau", type=float, default=None, help="default: the algorithm's (td3 0.005, ddpg 0.001)")
    ap.add_argument("--ou-noise", action="store_true", help="ddpg only: Agent.act(add_noise=True)'s Ornstein-Uhlenbeck noise (DDPG:44-64), "
                    "host-side, one state per env; collection goes act -> step.  Off by default, as in TRAIN_DDPG:100")
    ap.add_argument("--obs-layout", type=int, default=None, choices=[0, 1, 2], help="cn_config.obs_layout: 0 = 366 + 4K inputs (default); "
                    "1 = environment_stage_1_original's 363 (the shipped DDPG checkpoints); 2 = 370")
    ap.add_argument("--memory", type=int, default=1_000_000, help="TRAIN:63 (not qlearn / sarsa: no replay)")
    ap.add_argument("--replay-sample", default="with", choices=["with", "without"], help="how an update draws its mini-batch from the replay: "
                    "with replacement (default), or without -- distinct rows, as the reference's random.sample (td3.py:31-32, ddpg.py:33-34, "
                    "sac.py:34-35, memory.py:23); not qlearn / sarsa (no replay), and with --algo td3 --learner torch it needs --graphs 0")
    ap.add_argument("--checkpoint-every", type=int, default=100000, help="episodes between checkpoints (TRAIN:150: 100); checked at log time")
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--ped-vmax", type=float, default=None, help="training world only: walker speed bound (CROWD:101 -> 0.2)")
    ap.add_argument("--waypoint-reward", type=int, default=None, help="cn_config.waypoint_reward: ENV:1116's 200 (default) or 0 = the published log's reward")
    ap.add_argument("--scan-f32", type=int, default=None, help="cn_config.scan_f32")
    ap.add_argument("--wheel-accel", type=float, default=None, help="cn_config.wheel_accel (XACRO:70: 1.0)")
    ap.add_argument("--track-capacity", type=int, default=None, choices=[0, 32, 64, 128, 256, 512, 1024],
                    help="cn_config.track_capacity: 0 = auto (32 / 64, LDS); 128 ... 1024 = a wide table in HBM for long runs whose track "
                         "list outgrows 64 (slower; CN_ST_TRACK_OVERFLOW otherwise)")
    ap.add_argument("--reset-mode", default="next", choices=["next", "same"], help="next: the fast kernel, reset launches masked out of the replay; same: same-call reset + final_obs")
    ap.add_argument("--graphs", type=int, default=1, help="1: capture the TD3 update into hipGraphs (Agent.enable_graphs; td3 only; rejected for qlearn / sarsa)")
    ap.add_argument("--learner", default="torch", choices=["torch", "fused"], help="torch: the PyTorch update (td3: eager / hipGraph; ddpg: eager); "
                    "fused: cn_td3_update / cn_ddpg_update (csrc/crowdnav_td3.hip)")
    ap.add_argument("--actor-final-init", type=float, default=None, help="NOT the reference: U(+-x) initialisation of the actor's output layer (e.g. 0.003)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--population", type=int, default=0, help="P > 0: train P independent TD3 agents, seeds --seed ... --seed + P - 1, their updates "
                    "as one cn_td3_pop_update (1 ... 64; --algo td3 --learner fused only, not with --evaluate or --load); member p has its own "
                    "--envs environments and writes into <out>/member<p>/ what the solo run --seed <seed + p> writes into <out>")
    ap.add_argument("--population-act", default=None, choices=["one-launch", "per-member"], help="--population only: one-launch (default) = all "
                    "members act in one cn_actor_pop_forward and re-pack in one cn_actor_pop_pack per training launch; per-member = one "
                    "cn_actor_forward and one 4-launch re-pack per member.  Same results, bit for bit")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="default: runs/<algo>")
    ap.add_argument("--csv", action="store_true", help="one CSV row per finished episode in the reference's 8-column schema (recorded on the device, appended to the file at "
                    "every log interval); `timelapse` = the episode's own virtual duration, steps x (0.15 s + scan wait) -- TRAIN:141 "
                    "measures wall time since the episode's start, which the reference's time.sleep(0.15) makes the same quantity")
    ap.add_argument("--max-csv-rows", type=int, default=2_000_000)
    ap.add_argument("--load", default=None)
    ap.add_argument("--load-episode", default="latest", help="the <N> of td3_*_model_ep<N>.pt, or `latest` = the count in <load>/latest_checkpoint.txt")
    ap.add_argument("--evaluate", action="store_true")
    ap.add_argument("--episodes-per-env", type=int, default=1)
    a = ap.parse_args(argv)
    tab = a.algo in TABULAR
    if tab:           # flags of the replay learners: rejected when given, whatever their value
        probe = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
        for flag in ("--updates", "--memory", "--batch", "--graphs", "--replay-sample"):
            probe.add_argument(flag, default=None)
        given = [k for k, v in vars(probe.parse_known_args(argv)[0]).items() if v is not None]
        if given:
            ap.error("--algo %s has no replay, batch or update count: %s do(es) not apply" % (a.algo, ", ".join("--" + g.replace("_", "-") for g in given)))
    if a.epsilon is None:
        a.epsilon = 0.9 if tab else 1.0
    if a.epsilon_discount is None:
        a.epsilon_discount = 0.9986 if tab else 0.995
    if a.out is None:
        a.out = "runs/%s" % a.algo
    if a.max_steps is None:
        a.max_steps = 250 if a.algo == "dqn" else 200 if tab else 1000
    if (a.algo in ("dqn", "sac") or tab) and a.obs_layout is None:
        a.obs_layout = 1
    if (a.algo in ("dqn", "sac") or tab) and a.reset_mode != "next":
        ap.error("--algo %s collects with the next-step reset only (--reset-mode next)" % a.algo)
    if a.replay_sample == "without" and a.algo == "td3" and a.learner == "torch" and a.graphs and not a.evaluate:
        ap.error("--replay-sample without: the captured PyTorch TD3 update draws its own indices with replacement; use --learner fused or --graphs 0")
    if a.population:
        if not 1 <= a.population <= 64:
            ap.error("--population must be 1 ... 64")
        if a.algo != "td3":
            ap.error("--population trains TD3 agents (--algo td3), not --algo %s" % a.algo)
        if a.learner != "fused":
            ap.error("--population is cn_td3_pop_update: it needs --learner fused")
        if a.evaluate:
            ap.error("--population does not apply to --evaluate (evaluate a member's checkpoints from <out>/member<p>)")
        if a.load:
            ap.error("--population starts its members fresh: --load is not supported")
        if a.reset_mode != "next":
            ap.error("--population collects with the next-step reset only (--reset-mode next)")
    if a.population_act is not None and not a.population:
        ap.error("--population-act selects how a --population acts: it needs --population")
    if a.population_act is None:
        a.population_act = "one-launch"
    if a.ou_noise and a.algo != "ddpg":
        ap.error("--ou-noise is DDPG's exploration (--algo ddpg)")
    return a


def main(argv=None):
    a = parse_args(argv)
    if a.algo in TABULAR:
        return train_tabular(a)
    if a.evaluate:
        return run_evaluation(a)
    if a.population:
        return train_population(a)
    if a.algo == "dqn":
        return train_dqn(a)
    if a.algo == "sac":
        return train_sac(a)
    return train(a)


if __name__ == "__main__":
    main()
