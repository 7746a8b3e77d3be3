"""Batched counterpart of start_td3_training.py (TRAIN:40-168): TD3 on N environments of one MI355X.

    python -m crowdnav.train --scenario training_as_logged --waypoint-reward 0 --envs 16 --updates 16 --launches 25000 --csv --out runs/td3
    python -m crowdnav.train --evaluate --load runs/td3 --load-episode latest --scenario crossing_8
    python -m crowdnav.train --evaluate --evaluate-on device --load runs/td3 --eval-scenarios crossing_8,towards_8,random_8

`--evaluate-on device` (td3 / ddpg) runs the evaluation with its bookkeeping on the device (rollout.DeviceEvaluator: the f32-MFMA
actor, cn_eval_record, no host read until the end), all worlds of --eval-scenarios in one run; `--population P --eval-every L`
evaluates all members that way while they train (<out>/eval_log.csv) and `--pbt-fitness eval` ranks population-based training by it.

`--state-every L` (--algo td3 --learner fused, solo or --population) writes the run's WHOLE state at the end of every L-th launch --
the learner's blob (cn_td3_state_save / cn_td3_pop_state_save: networks, Adam's moments and counters, the update counter, a
population's hyper-parameters and PBT state, one launch), the replays, the environments, the loop's tensors, logs and counts -- into
<out>/state/launch<it>/, and `--resume DIR` with the same command line continues that run at the next launch, bit for bit: the CSVs,
the checkpoints and pbt_log.csv are those of the run that was never stopped.

    python -m crowdnav.train --learner fused --population 8 --envs 64 --pbt-every 500 --csv --state-every 1000 --out runs/pop
    python -m crowdnav.train --learner fused --population 8 --envs 64 --pbt-every 500 --csv --state-every 1000 --resume runs/pop

`--n-step W` (--algo td3, --reset-mode next; solo, or --population with the one-call recorder) fills the replay with W-step rows --
the discounted sum of W rewards and the observation W steps on, accumulated on the device by cn_nstep_record (two launches per
training launch); rows that an episode's end cuts short carry d = 1 -- and the target bootstraps with gamma^W.  W = 1, the default,
is the run without the switch.

Checkpoints are labelled with the episode count the weights really have behind them (N envs finish episodes in batches, so the
count at a log interval is rarely a round number); every save also rewrites `latest_checkpoint.txt` with that count, and
`--load-episode latest` (the default) reads it -- resume / evaluate commands can be written before the run exists.

`--algo ddpg` trains the reference's baseline learner instead (start_ddpg_training.py, ddpg.py; crowdnav.ddpg): batch 64, actor
lr 1e-4, critic lr 1e-3, tau 0.001 unless --batch / --lr-actor / --lr-critic / --tau are given, no exploration noise
(TRAIN_DDPG:100) unless --ou-noise (with --ou-act fused: actor and Ornstein-Uhlenbeck noise in one cn_ddpg_act launch), checkpoints ddpg_{actor,critic}_model_ep<N>.pt, CSV ddpg_training.csv; `--learner fused` is
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
import json
import os
import time

import numpy as np
import torch

from . import presets
from .config import Config
from .env import MemberEnvs, VecEnv
from .rollout import DeviceEvaluator, EpisodeStats, evaluate
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
    COLS = (0, 1, 4, 5, 6, 3)         # a row's success, failure, ego / social violations, obstacle-present steps, steps (EpisodeStats.add_from_counters)

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


def write_latest(outdir, episodes):
    """The `latest` pointer, replaced atomically: a reader never sees a half-written count."""
    tmp = os.path.join(outdir, ".latest_checkpoint.txt.%d" % os.getpid())
    open(tmp, "w").write("%d\n" % episodes)
    os.replace(tmp, os.path.join(outdir, "latest_checkpoint.txt"))


# ---- --state-every / --resume: the whole state of a fused TD3 run or population, for a bit-for-bit continuation -------------------
# <out>/state/launch<it>/ holds what the run at the end of launch `it` consists of: the learner's blob and the replays (Agent.save_state
# -> agent.npz; Population.save_state -> learner.npz, member<p>.npz), every environment handle's snapshot (env<g>.npy) and loop.npz:
# the loop's device tensors, every episode log's unflushed rows, n, totals and flushed count, PBT's running totals, the host scalars
# and the byte sizes of the files the run appends to.  A directory is written under another name and renamed when complete;
# <out>/state/latest then names it (replaced atomically, as write_latest), and only then are older directories pruned.
STATE_DIR = "state"


def resolve_resume(run_dir):
    """--resume DIR -> the state directory DIR/state/latest names."""
    pointer = os.path.join(run_dir, STATE_DIR, "latest")
    if not os.path.exists(pointer):
        raise FileNotFoundError("--resume %s: %s does not exist (no --state-every run wrote a complete state there)" % (run_dir, pointer))
    path = os.path.join(run_dir, STATE_DIR, open(pointer).read().split()[0])
    if not os.path.isdir(path):
        raise FileNotFoundError("--resume %s: the latest pointer names %s, which does not exist" % (run_dir, path))
    return path


def elog_state(e, key):
    n = min(int(e.n.item()), e.max_rows)
    return {key + "_n": np.int64(e.n.item()), key + "_flushed": np.int64(e._flushed), key + "_tot": e.tot.cpu().numpy(),
            key + "_rows": e.rows[e._flushed:n].cpu().numpy()}


def set_elog_state(e, z, key):
    rows = torch.from_numpy(z[key + "_rows"])
    e._flushed = int(z[key + "_flushed"])
    e.n.fill_(int(z[key + "_n"]))
    e.tot.copy_(torch.from_numpy(z[key + "_tot"]))
    e.rows[e._flushed:e._flushed + rows.shape[0]].copy_(rows)


def write_state(a, it, save_learner, runs, counts, env_handles, tensors, scalars, files):
    """One complete <out>/state/launch<it>/, then the `latest` pointer, then the pruning (--state-keep).  save_learner(dir) writes the
    learner's files; tensors: name -> device tensor; counts, scalars: name -> host number; files: the files this run appends to."""
    import re
    import shutil
    root = os.path.join(a.out, STATE_DIR)
    final = os.path.join(root, "launch%d" % it)
    tmp = final + ".tmp%d" % os.getpid()
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(tmp)
    torch.cuda.synchronize()
    save_learner(tmp)
    for g, e in enumerate(env_handles):
        np.save(os.path.join(tmp, "env%d.npy" % g), e.snapshot())
    loop = {"t_" + k: t.cpu().numpy() for k, t in tensors.items()}
    loop.update({"s_" + k: np.asarray(v) for k, v in dict(counts, **scalars).items()})
    for p, run in enumerate(runs):
        loop.update(elog_state(run.elog, "elog%d" % p))
        loop["run%d" % p] = np.array([run.episodes, run.env_steps, run.next_ckpt], dtype=np.int64)
    loop["file_names"] = np.array([os.path.relpath(f, a.out) for f in files])
    loop["file_sizes"] = np.array([os.path.getsize(f) if os.path.exists(f) else 0 for f in files], dtype=np.int64)
    with open(os.path.join(tmp, "loop.npz"), "wb") as f:
        np.savez(f, **loop)
    shutil.rmtree(final, ignore_errors=True)
    os.rename(tmp, final)
    pointer = os.path.join(root, ".latest.%d" % os.getpid())
    open(pointer, "w").write("launch%d\n" % it)
    os.replace(pointer, os.path.join(root, "latest"))
    kept = sorted((int(m.group(1)), d) for d in os.listdir(root) for m in [re.fullmatch(r"launch(\d+)", d)] if m)
    for _, d in kept[:-max(1, getattr(a, "state_keep", 1))]:
        if d != "launch%d" % it:
            shutil.rmtree(os.path.join(root, d), ignore_errors=True)


def read_state(a, path, env_handles, tensors, runs):
    """What write_state wrote at `path`, but the learner's files, back into the environments, the tensors and the runs -> the scalars.
    The files the run appends to are cut back to the sizes they had when the state was written (a run killed after it may have
    appended more)."""
    for g, e in enumerate(env_handles):
        e.restore(np.load(os.path.join(path, "env%d.npy" % g)))
    with np.load(os.path.join(path, "loop.npz")) as z:
        for k, t in tensors.items():
            t.copy_(torch.from_numpy(z["t_" + k]))
        for p, run in enumerate(runs):
            set_elog_state(run.elog, z, "elog%d" % p)
            run.episodes, run.env_steps, run.next_ckpt = (int(x) for x in z["run%d" % p])
        for name, size in zip(z["file_names"].tolist(), z["file_sizes"].tolist()):
            f = os.path.join(a.out, name)
            if os.path.exists(f) and os.path.getsize(f) > size:
                os.truncate(f, size)
        return {k[2:]: z[k] for k in z.files if k.startswith("s_")}


def save_checkpoint(agent, outdir, episodes):
    """TRAIN:150-154's checkpoint + the exploration-noise stream's position + the `latest` pointer."""
    agent.save(outdir, episodes)
    open(os.path.join(outdir, "noise_state_ep%d.txt" % episodes), "w").write("%d %d\n" % agent.noise_state())
    write_latest(outdir, episodes)


CHECKPOINT_NETS = dict(td3=("actor", "critic1", "critic2"), ddpg=("actor", "critic"), sac=("actor", "critic_v", "critic_soft_q"))


def make_dqn_agent(a, obs_ld, device, memory_size):
    """The DQN learner with the reference's defaults (TRAIN_DQN:45-57); --batch / --target-update / --epsilon override them."""
    if a.dqn_inputs > obs_ld:
        raise ValueError("--dqn-inputs %d > the observation width %d (use --obs-layout 1)" % (a.dqn_inputs, obs_ld))
    return dqn.Agent(obs_dim=a.dqn_inputs, obs_ld=obs_ld, batch_size=a.batch or 64, memory_size=memory_size, epsilon=a.epsilon,
                     epsilon_discount=a.epsilon_discount, target_update=a.target_update, device=device, seed=a.seed,
                     replay_sample=a.replay_sample)


def make_agent(a, obs_dim, device, **kw):
    """The learner of --algo with its reference defaults; --batch / --lr-actor / --lr-critic / --tau override them when given."""
    over = {k: v for k, v in (("batch_size", a.batch), ("actor_lr", a.lr_actor), ("critic_lr", a.lr_critic), ("tau", a.tau)) if v is not None}
    over.update(kw)
    over["replay_sample"] = a.replay_sample
    if a.algo == "sac":
        over = {dict(critic_lr="q_lr").get(k, k): v for k, v in over.items()}
        if "q_lr" in over:
            over["v_lr"] = over["q_lr"]
        return sac.Agent(obs_dim=obs_dim, device=device, seed=a.seed, n_envs=a.envs, value_net=a.sac_value_net.replace("-", "_"),
                         soft_update=a.sac_soft_update.replace("-", "_"), deterministic=a.sac_deterministic, **over)
    if a.algo == "ddpg":
        return ddpg.Agent(obs_dim=obs_dim, device=device, seed=a.seed, n_envs=a.envs, **over)
    return td3.Agent(obs_dim=obs_dim, device=device, seed=a.seed, n_step=getattr(a, "n_step", 1), **over)


def load_checkpoint(agent, a):
    a.load_episode = resolve_load_episode(a.load, a.load_episode)
    agent.load_models(*[os.path.join(a.load, "%s_%s_model_ep%d.pt" % (a.algo, n, a.load_episode)) for n in CHECKPOINT_NETS[a.algo]])


def env_switches(a):
    return dict(waypoint_reward=a.waypoint_reward, scan_f32=a.scan_f32, wheel_accel=a.wheel_accel,
                track_capacity=a.track_capacity, obs_layout=a.obs_layout)


class Learner:
    """What the collection loop asks of a learner, with the answers TD3, DDPG, SAC and a population's member share: the replay
    write, `learn()` once the replay holds more than a batch (TRAIN:132), save_checkpoint, the progress line with mean steps."""
    consume_after_log = False         # the transition is consumed before the episode log's add
    checkpoints = True
    line_updates = True               # the progress line shows the update count ...
    line_steps = True                 # ... and the mean episode length

    def __init__(self, a, agent):
        self.a, self.agent = a, agent
        self.learn = agent.learn      # TRAIN:133-136; bound here: the loop calls it --updates times per launch
        self.csv_name = "%s_training" % a.algo
        # a run continued into the directory it was loaded from appends to that run's CSV (as progress.txt always did)
        # (--resume continues the run of --out: it appends as well)
        self.resume = (bool(a.load) and os.path.abspath(a.load) == os.path.abspath(a.out)) or bool(getattr(a, "resume", None))

    def load(self):
        """--load: the networks, and the exploration-noise stream continued instead of replayed."""
        if self.a.load:
            load_checkpoint(self.agent, self.a)
            ns = os.path.join(self.a.load, "noise_state_ep%d.txt" % self.a.load_episode)
            if os.path.exists(ns):
                self.agent.set_noise_state(*[int(x) for x in open(ns).read().split()])

    def start(self, obs, elog):
        """Before launch 1."""

    def consume(self, prev, act, reward, obs, done, keep):
        self.agent.memory.add_masked(prev, act, reward, obs, done, keep)    # TRAIN:129-131; s' of a finished env = its terminal obs

    def ready(self):
        return self.agent.memory.ready(self.agent.batch_size)   # (a host read only while the bounds straddle it; none afterwards)

    def after_updates(self):
        """After the launch's --updates updates."""

    def epsilon_at(self, episodes):
        """At log time, before the progress line: the exploration rate the line shows, None = none."""

    def warn(self, run):
        """At log time, after the progress line."""

    def checkpoint(self, outdir, episodes):
        save_checkpoint(self.agent, outdir, episodes)

    def close(self):
        self.agent.memory.sync_len()

    def summary(self, run, last, updates, t):
        return " | %d updates, %.0f updates/s, %d env-steps, %.0f s" % (updates, updates / max(1e-9, t), run.env_steps, t)


class Td3(Learner):
    """--algo td3 / ddpg: the whole actor as ONE kernel on the weights packed after the launch's updates."""

    def __init__(self, a, env):
        extra = dict(actor_final_init=a.actor_final_init) if a.algo == "td3" else {}
        super().__init__(a, make_agent(a, env.D, "cuda:%d" % a.device, memory_size=a.memory, **extra))
        self.env = env
        self.load()
        if a.learner == "fused":
            self.agent.enable_fused_update()   # cn_td3_update: the update as 7 (+ 5) hand-written launches; cn_ddpg_update: 8
        elif a.graphs and a.algo == "td3":
            self.agent.enable_graphs()         # a TD3 update as one hipGraph launch (the eager update is launch-bound at batch 128)
        self.warned_overflow = False
        if a.algo == "ddpg" and a.ou_noise and a.ou_act == "fused":    # the same loop, actor + OU noise + noise.reset() as ONE launch (cn_ddpg_act)
            self.act = self.act_ou_fused
        elif a.algo == "ddpg" and a.ou_noise:  # OU noise: the act -> step loop (DDPG:170-196, add_noise=True)
            self.act, self.consume = self.act_ou, self.consume_ou

    def start(self, obs, elog):
        self.agent.sync_fused_weights()

    def act(self, obs, it):
        return self.agent.act_mfma(obs, add_noise=True)      # TD3:196-223 as one kernel, sigma = 1.0 (DDPG: 0), clipped

    def act_ou(self, obs, it):
        return self.agent.act(obs, add_noise=True, step=it - 1)

    def act_ou_fused(self, obs, it):
        # TRAIN_DDPG:161's noise.reset() rides in the act launch: env.done still holds the previous step's flags here
        return self.agent.act_ou_fused(obs, reset=self.env.done if it > 1 else None, step=it - 1)

    def consume_ou(self, prev, act, reward, obs, done, keep):
        self.agent.memory.add_masked(prev, act, reward, obs, done, keep)
        self.agent.reset_noise(done)                         # TRAIN_DDPG:161

    def after_updates(self):
        self.agent.sync_fused_weights()                      # the actor the next launch acts with

    def warn(self, run):
        if self.warned_overflow:
            return
        sc_ = self.env.status_counts()
        if sc_["track_overflow"] or sc_["conf_overflow"]:
            self.warned_overflow = True
            run.say("WARNING: %d env(s) outgrew the track table and %d the confirmed-object table (status bits CN_ST_TRACK_OVERFLOW / "
                    "CN_ST_CONF_OVERFLOW): their risk features use the tracks that fit and differ from the reference's unbounded "
                    "lists from there on; --track-capacity 256 (or 128 / 512 / 1024: a wide table in HBM, slower) keeps the "
                    "track list equal to the reference's up to that many tracks" % (sc_["track_overflow"], sc_["conf_overflow"]))

    def summary(self, run, last, updates, t):
        return "  ego %.3f  social %.3f  | %d updates, %.0f updates/s, %.0f env-steps/s overall" % (
            sum(r[5] for r in last if r[5] == r[5]) / max(1, sum(1 for r in last if r[5] == r[5])),
            sum(r[6] for r in last if r[6] == r[6]) / max(1, sum(1 for r in last if r[6] == r[6])),
            updates, updates / max(1e-9, t), run.env_steps / max(1e-9, t))


class Dqn(Learner):
    """--algo dqn, start_dqn_training.py:84-152: cn_dqn_act (epsilon from the device's count of finished episodes) -> env.step ->
    replay (the index in column 0) -> learnOnMiniBatch once the replay holds more than learnStart rows."""
    line_steps = False

    def __init__(self, a, env):
        super().__init__(a, make_dqn_agent(a, env.D, "cuda:%d" % a.device, a.memory))
        self.eps0 = a.epsilon
        if a.load:                                      # TRAIN_DQN:62-82: the weights, and epsilon from the parameter record
            a.load_episode = resolve_load_episode(a.load, a.load_episode)
            self.agent.load_models(os.path.join(a.load, "dqn_model_ep%d.pt" % a.load_episode),
                                   os.path.join(a.load, "dqn_model_ep%d.json" % a.load_episode))
            self.eps0 = self.agent.epsilon0
        if a.learner == "fused":
            self.agent.enable_fused_update()

    def start(self, obs, elog):
        self.episodes_dev = elog.n
        self.act2 = torch.zeros((obs.shape[0], 2), dtype=torch.float32, device=obs.device)

    def act(self, obs, it):
        idx, twist = self.agent.act_fused(obs, episodes_dev=self.episodes_dev)     # TRAIN_DQN:89-90, 103-104
        self.act2[:, 0] = idx.float()
        return twist

    def consume(self, prev, act, reward, obs, done, keep):
        self.agent.memory.add_masked(prev, self.act2, reward, obs, done, keep)     # TRAIN_DQN:112

    def ready(self):
        return self.agent.memory.ready(self.agent.learn_start)                    # TRAIN_DQN:114, deepq.py:221

    def epsilon_at(self, episodes):
        self.agent.epsilon = dqn.epsilon_after(episodes + 1, self.eps0, self.a.epsilon_discount)   # what the device used (the json records it)
        return self.agent.epsilon

    def checkpoint(self, outdir, episodes):
        self.agent.save(outdir, episodes, nsteps=self.a.max_steps)
        write_latest(outdir, episodes)

    def summary(self, run, last, updates, t):
        return " | %d updates, %d env-steps, %.0f s" % (updates, run.env_steps, t)


class Sac(Learner):
    """--algo sac, start_sac_training.py's loop: cn_sac_act -> env.step -> replay -> learn() (TRAIN_SAC:127)."""

    def __init__(self, a, env):
        super().__init__(a, make_agent(a, env.D, "cuda:%d" % a.device, memory_size=a.memory))
        self.load()
        if a.learner == "fused":
            self.agent.enable_fused_update()

    def act(self, obs, it):
        return self.agent.act_fused(obs)                     # Agent.act: samples, squashes twice, clips


class Tabular(Learner):
    """--algo qlearn / sarsa, start_sarsa_training.py:48-116 / start_qlearn_training.py for N environments that share one Q-table:
    chooseAction for every env after the reset, then per launch env.step -> ONE learn_act (learn the launch's transitions except
    the reset launches, then chooseAction on the table after the writes; epsilon from the device's count of finished episodes).
    --evaluate: the same loop without the learn phase (and no checkpoint: the table does not change)."""
    consume_after_log = True          # learn_act's epsilon reads the episode count the log's add has just advanced
    line_updates = False

    def __init__(self, a, env):
        if env.D < 2:
            raise ValueError("the tabular learners read the last two columns of the observation")
        self.a = a
        self.agent = TABULAR[a.algo](epsilon=a.epsilon, alpha=a.alpha, gamma=a.gamma, epsilon_discount=a.epsilon_discount, seed=a.seed,
                                     device="cuda:%d" % a.device)
        if a.load_qtable:
            self.agent.load_q(a.load_qtable)            # utils.load_q (qlearn.py:23)
        if a.learner == "fused":
            self.agent.enable_fused()
        self.learning = self.checkpoints = not a.evaluate
        self.csv_name = "%s_training%s" % (a.algo, "_test" if a.evaluate else "")
        self.resume = False

    def start(self, obs, elog):
        self.episodes_dev = elog.n
        self.out = self.agent.learn_act(None, None, None, obs, learn=False, act=True, episodes_dev=elog.n)   # the first step of every first episode

    def act(self, obs, it):
        self.action = self.out["action"]
        return self.out["twist"]

    def consume(self, prev, act, reward, obs, done, keep):
        self.out = self.agent.learn_act(prev, self.action, reward, obs, keep=keep, learn=self.learning, act=True, episodes_dev=self.episodes_dev)

    def ready(self):
        return False                  # no replay, no --updates loop

    def epsilon_at(self, episodes):
        self.agent.epsilon = dqn.epsilon_after(episodes + 1, self.a.epsilon, self.a.epsilon_discount)      # what the device used
        return self.agent.epsilon

    def checkpoint(self, outdir, episodes):            # start_sarsa_training.py:105-108 (every 100 episodes there)
        self.agent.save(outdir, episodes)
        write_latest(outdir, episodes)

    def close(self):
        pass

    def summary(self, run, last, updates, t):
        _, present, counts = self.agent.table()
        return " | %d table entries, %d first writes, %d blends, %d env-steps, %.0f s" % (int(present.sum()), counts[0], counts[1], run.env_steps, t)


class Member(Learner):
    """Member p of a --population: PopulationSide acts, stores and learns for all members at once; this is its log-time side."""

    def summary(self, run, last, updates, t):
        return "  | %d updates, %.0f updates/s (x %d members)" % (updates, updates / max(1e-9, t), self.a.population)


SOLO = dict(td3=Td3, ddpg=Td3, dqn=Dqn, sac=Sac, qlearn=Tabular, sarsa=Tabular)


class RunLog:
    """One run's bookkeeping: the device's episode log, the EpisodeStats rows it becomes, progress.txt, the episode and env-step
    counts, the checkpoint cadence.  log() is the whole log-interval block, finish() the tail; `learner` answers what differs
    between the algorithms (a Learner).  prefix goes in front of the lines on stdout only."""

    def __init__(self, a, out, elog, step_s, learner, prefix=""):
        self.a, self.out, self.elog, self.step_s, self.learner, self.prefix = a, out, elog, step_s, learner, prefix
        self.stats = EpisodeStats()
        os.makedirs(out, exist_ok=True)
        self.file = open(os.path.join(out, "progress.txt"), "a")
        self.episodes, self.env_steps, self.next_ckpt = 0, 0, a.checkpoint_every
        self.t0 = time.time()

    def say(self, line):
        print(self.prefix + line, flush=True); self.file.write(line + "\n"); self.file.flush()

    def log(self, it, updates):
        """One host read of the device's log, then: rows -> stats, the progress line, the CSV's new rows (a killed run keeps its
        rows up to here), a checkpoint once the episode count has reached the next multiple of --checkpoint-every."""
        L = self.learner
        rows, tot = self.elog.flush()
        ne = int(tot[0])
        self.episodes += ne; self.env_steps += int(tot[4])
        for r in rows.tolist():
            self.stats.add_from_counters(r, r[2], step_seconds=self.step_s, cols=DeviceEpisodeLog.COLS)
        eps = L.epsilon_at(self.episodes)
        if ne:
            self.say("launch %6d  env-steps %10d%s  episodes %8d  success %.3f  mean return %8.1f%s%s  %.0f s" % (
                it, self.env_steps, "  updates %9d" % updates if L.line_updates else "", self.episodes, tot[1] / ne, tot[2] / ne,
                "  mean steps %6.1f" % (tot[3] / ne) if L.line_steps else "", "" if eps is None else "  epsilon %.3f" % eps,
                time.time() - self.t0))
        L.warn(self)
        if self.a.csv:
            self.stats.append_csv(self.out, L.csv_name, resume=L.resume)
        if L.checkpoints and self.episodes >= self.next_ckpt:       # TRAIN:150-154 (every 100 episodes there)
            # labelled with the episode count the weights really have behind them (checked at log time, so it can be past
            # the threshold that triggered it)
            L.checkpoint(self.out, self.episodes)
            while self.next_ckpt <= self.episodes:
                self.next_ckpt += self.a.checkpoint_every

    def finish(self, updates):
        """The final checkpoint and the summary of the last 500 episodes."""
        L = self.learner
        L.close()
        if L.checkpoints:
            L.checkpoint(self.out, self.episodes)
        last = self.stats.rows[-500:]
        if last:
            self.say("last %d episodes: success %.3f  mean return %.1f  mean steps %.1f%s" % (
                len(last), sum(r[1] for r in last) / len(last), sum(r[3] for r in last) / len(last), sum(r[4] for r in last) / len(last),
                L.summary(self, last, updates, time.time() - self.t0)))
        self.file.close()


def open_csv(path, columns):
    """A CSV file the run appends to; the header goes in while the file is still empty."""
    f = open(path, "a")
    if f.tell() == 0:
        f.write(",".join(columns) + "\n")
    return f


def run_loop(a, side):
    """The training loop of every run; `side` (SoloSide, PopulationSide) answers what differs.  Per launch side.launch(it) -- act ->
    step -> record --, then, once side.ready() has turned true (it is not asked again), `--updates` side.learn(n), n = 1, 2, 3 ..., and
    side.after_updates(); then side.after_launch(it, learning).  Every --log-every launches and at the last one (--time-limit is
    checked there) side.before_log() and side.runs' log(); at the end side.close() and their finish().  --state-every writes
    side.state() -> (env handles, loop tensors, extra scalars, files appended to) and side.save_state(dir); --resume is read_state,
    the side's load_state(dir, scalars), then the loop's three scalars.  Enqueue-only between log intervals.  -> side"""
    state_every, resume = getattr(a, "state_every", 0), getattr(a, "resume", None)     # (collect() takes Namespaces built by hand, which have neither: Args)
    first, updates_done, learning = 1, 0, False
    if resume:
        path = resolve_resume(resume)
        sc = read_state(a, path, *side.state()[:2], side.runs)
        side.load_state(path, sc)
        first, updates_done, learning = int(sc["it"]) + 1, int(sc["updates_done"]), bool(sc["learning"])
    for it in range(first, a.launches + 1):
        side.launch(it)
        if not learning:
            learning = side.ready()
        if learning:
            for u in range(a.updates):
                updates_done += 1
                side.learn(updates_done)
            side.after_updates()
        side.after_launch(it, learning)
        last_launch = it == a.launches or (a.time_limit and it % a.log_every == 0 and time.time() - side.runs[0].t0 > a.time_limit)
        if it % a.log_every == 0 or last_launch:
            side.before_log()
            for run in side.runs:
                run.log(it, updates_done)
        if state_every and it % state_every == 0:
            write_state(a, it, side.save_state, side.runs, dict(it=it, updates_done=updates_done, learning=learning), *side.state())
        if last_launch:
            break
    side.close()
    for run in side.runs:
        run.finish(updates_done)
    return side


PENDING_NAMES = ("s", "a", "ret", "count", "clock")      # Population.record_pending's tensors, as a state names them


class SoloSide:
    """One environment handle and one learner (TRAIN:104-168 for N environments): per launch act -> env.step -> the learner consumes
    the transition -> episode log.  elog: the episode log (default: DeviceEpisodeLog on the observation's device).  --n-step W > 1: the
    transition and the episode log are ONE call of a one-member n-step recorder (td3.SoloRecorder, cn_nstep_record) on fixed buffers,
    which also keeps `prev` and the reset-launch flags."""
    after_launch = before_log = close = staticmethod(lambda *args: None)      # (what follows the updates: a population's business)

    def __init__(self, a, env, learner, elog=None):
        self.a, self.env, self.learner = a, env, learner
        self.obs = obs = env.reset()
        self.runs = [RunLog(a, a.out, elog or DeviceEpisodeLog(obs.device, a.max_csv_rows), (env.cfg.dt_ms + env.cfg.scan_latency_ms) / 1000.0, learner)]
        self.same, self.late = a.reset_mode == "same", learner.consume_after_log
        self.resetting = torch.zeros(env.N, dtype=torch.bool, device=obs.device)   # envs whose NEXT launch is their Env.reset
        self.all_rows = torch.ones(env.N, dtype=torch.bool, device=obs.device)
        self.prev, self.act = torch.empty_like(obs), None
        self.ready, self.learn, self.after_updates = learner.ready, getattr(learner, "learn", None), learner.after_updates   # (Tabular: never ready, no learn)
        self.save_state = lambda d: learner.agent.save_state(os.path.join(d, "agent.npz"))
        self.load_state = lambda d, scalars: learner.agent.load_state(os.path.join(d, "agent.npz"))      # (re-packs the actor)
        self.rec = None
        if getattr(a, "n_step", 1) > 1:                                 # (parse_args: --algo td3 --reset-mode next)
            self.prev.copy_(obs)                                       # once: every record() leaves the new observation in prev
            self.act = torch.zeros((env.N, 2), dtype=torch.float32, device=obs.device)
            self.rec = td3.SoloRecorder(learner.agent).bind_record([env], [self.prev], [obs], [self.act], [env.reward], [env.done],
                                                                  [self.runs[0].elog], n_step=a.n_step)
            self.launch = self.launch_nstep
        learner.start(obs, self.runs[0].elog)

    def launch_nstep(self, it):
        self.learner.agent.act_mfma(self.obs, out=self.act, add_noise=True)
        self.env.step(self.act, auto_reset="next")
        self.rec.record(it)

    def launch(self, it):
        env, learner, obs = self.env, self.learner, self.obs
        act = self.act = learner.act(obs, it)
        self.prev.copy_(obs)
        if self.same:
            obs, reward, done = env.step(act, auto_reset="same", want_final=True)
            keep, nxt = self.all_rows, env.final_obs
        else:
            obs, reward, done = env.step(act, auto_reset="next")
            keep, nxt = ~self.resetting, obs
        if not self.late:
            learner.consume(self.prev, act, reward, nxt, done, keep)
        if not self.same:
            self.resetting = done.bool()
        self.runs[0].elog.add(done, env.counters(), env.returns()[0], it, keep)
        if self.late:
            learner.consume(self.prev, act, reward, nxt, done, keep)
        self.obs = obs

    def state(self):                                                   # (parse_args: --algo td3 --learner fused --reset-mode next)
        t = dict(obs=self.obs, prev=self.prev, reward=self.env.reward, done=self.env.done, resetting=self.resetting,
                 **({} if self.act is None else dict(act=self.act)))     # (act: for the record; every launch computes its own)
        if self.rec:                                                   # the recorder's flags in place of the loop's, and its pending store
            t.update(resetting=self.rec.resetting(0), **{"record_pending_" + k: v for k, v in zip(PENDING_NAMES, self.rec.record_pending(0))})
        return [self.env], t, {}, [os.path.join(self.a.out, self.learner.csv_name + ".csv")] if self.a.csv else []


def collect(a, env, learner, elog=None):
    """The collection loop of every solo run: run_loop around (env, learner) -> (the learner's agent, finished episodes)."""
    return learner.agent, run_loop(a, SoloSide(a, env, learner, elog)).runs[0].episodes


def train(a):
    """One solo run of --algo on N environments of one GPU -> (agent, finished episodes)."""
    fill_defaults(a)
    torch.cuda.set_device(a.device)        # policy kernels and torch ops of this process all target the env's GPU
    env = make_env(a.scenario, a.envs, a.max_steps, a.seed, a.device, a.ped_vmax, **env_switches(a))
    return collect(a, env, SOLO[a.algo](a, env))


PBT_CSV_COLUMNS = ("launch", "call", "member", "src", "generation", "fitness", "lr_actor", "lr_critic", "gamma", "noise_std", "noise_clip")
PBT_HYPERS = PBT_CSV_COLUMNS[6:]
EVAL_POPULATION_FLAGS = ("eval_every", "eval_envs", "eval_episodes", "eval_max_steps", "eval_seed", "eval_metric")      # refused without --population
EVAL_SUMMARY_COLUMNS = ("episodes", "success_rate", "failure_rate", "timeout_rate", "mean_return", "mean_steps", "mean_ego", "mean_social")
EVAL_CSV_COLUMNS = ("launch", "member", "world") + EVAL_SUMMARY_COLUMNS


def _mix64(z):
    """splitmix64's finaliser on Python integers (include/crowdnav.h: mix64)."""
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def pbt_spread_factors(seed, member, spread):
    """--pbt-spread S: member p's factors for (lr_actor, lr_critic, noise_std), log-uniform in [1/S, S], a function of (seed, p) alone."""
    key = _mix64((int(seed) & ((1 << 64) - 1)) ^ 0x504254)
    return [float(spread) ** (2.0 * ((_mix64(key ^ (8 * member + k)) >> 11) * 2.0 ** -53) - 1.0) for k in range(3)]


def build_members(a):
    """-> (members, envs, agents, pop) of --population P: per member its Namespace (seed + p, <out>/member<p>/), its handle in one
    MemberEnvs and its Agent; pop: their td3.Population.  --pbt-spread S > 0 starts member p with lr_actor, lr_critic and noise_std
    multiplied by a keyed log-uniform factor in [1/S, S]: the sweep PBT then acts on.  --population-replay shared: every update
    samples the union of all members' rings (replay_source="shared") and the updates begin once the rings together hold more than a
    batch; the rings are written and saved per member as before, so --state-every / --resume hold a shared run as any other (give the
    switch again on --resume, like --replay-sample).  <out>/run.json records the switches that shape the run."""
    members = [argparse.Namespace(**dict(vars(a), seed=a.seed + p, out=os.path.join(a.out, "member%d" % p), resume=a.resume, n_step=getattr(a, "n_step", 1)))
               for p in range(a.population)]                          # (resume, by name: the member's CSV is appended to; n_step: the member's Agent)
    specs = [scenario_config(a.scenario, a.envs, a.max_steps, m.seed, a.ped_vmax, **env_switches(a)) for m in members]
    envs = MemberEnvs([sp[0] for sp in specs], a.device)
    for e, (_, init, vel) in zip(envs.envs, specs):
        if init is not None:
            e.set_ped_init(init)
        if vel is not None:
            e.set_ped_preset_vel(vel)
    spread = [{} for _ in members]
    for p, m in enumerate(members if a.pbt_spread > 0 else []):
        f = pbt_spread_factors(a.seed, p, a.pbt_spread)
        m.lr_actor, m.lr_critic = (a.lr_actor or 3e-4) * f[0], (a.lr_critic or 3e-4) * f[1]
        spread[p] = dict(noise_std=0.2 * f[2])
    agents = [make_agent(m, envs.D, "cuda:%d" % a.device, memory_size=a.memory, actor_final_init=a.actor_final_init, **kw) for m, kw in zip(members, spread)]
    pop = td3.Population(agents, replay_source=a.population_replay)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "run.json"), "w") as f:
        json.dump({k: getattr(a, k) for k in ("population", "population_replay", "population_act", "population_record", "population_step",
                                              "replay_sample", "n_step")}, f, indent=1, sort_keys=True)
        f.write("\n")
    return members, envs, agents, pop


class Pbt:
    """--pbt-every L > 0 (population-based training): after the updates of every L-th launch, once learning has begun, ONE
    Population.exploit() -- two launches that rank the members by the mean return of the episodes each finished since the last applied
    call, copy the best members' networks and optimizer state over the worst --pbt-fraction of them, and perturb the hyper-parameters
    of --pbt-explore by one of --pbt-factor -- then one read of the PBT state (the only host read PBT adds), rows to <out>/pbt_log.csv.
    The logs' totals restart at every flush; PBT ranks on totals that never do: what was flushed so far + the running ones."""

    def __init__(self, a, pop, elogs, sync_unbound):
        self.pop, self.elogs, self.sync_unbound, self.applied, self.path = pop, elogs, sync_unbound, 0, os.path.join(a.out, "pbt_log.csv")
        self.flushed, self.tot = (torch.zeros((len(elogs), 5), dtype=torch.float64, device=elogs[0].tot.device) for _ in range(2))
        pop.bind_pbt(a.pbt_n_replace, factor=a.pbt_factor, explore=a.pbt_explore, min_episodes=a.pbt_min_episodes, seed=a.seed,
                     elogs=[argparse.Namespace(rows=e.rows, max_rows=e.max_rows, n=e.n, tot=self.tot[p]) for p, e in enumerate(elogs)])
        open_csv(self.path, PBT_CSV_COLUMNS).close()                   # (a run without an applied exploit leaves the header)

    def exploit(self, it, fitness):
        torch.add(self.flushed, torch.stack([e.tot for e in self.elogs]), out=self.tot)
        self.pop.exploit(fitness)                                      # (re-packs the bound actors)
        self.sync_unbound()
        st = self.pop.pbt_state()                                      # the one host read PBT adds: once per --pbt-every launches
        if st["applied"] > self.applied:
            self.applied = st["applied"]
            with open_csv(self.path, PBT_CSV_COLUMNS) as f:
                for p, m in enumerate(st["members"]):
                    f.write(",".join(["%d" % it, "%d" % (st["calls"] - 1), "%d" % p, "%d" % m["src"], "%d" % m["generation"]] +
                                     ["%.9g" % m[k] for k in PBT_CSV_COLUMNS[5:]]) + "\n")

    def before_log(self):
        self.flushed.add_(torch.stack([e.tot for e in self.elogs]))     # (RunLog.log flushes: the totals restart)


class Evaluation:
    """--eval-every L > 0: after the updates and the re-pack of every L-th launch, ONE evaluation of all members on the device
    (Population.evaluate: every member's greedy actor in the --eval-scenarios worlds with --eval-seed, --eval-envs environments and
    --eval-episodes episodes each, job (p, w) on its own handle; three enqueues per evaluation launch for all of them) and one read of
    its summaries, whose rows go to <out>/eval_log.csv.  It has its own environment and actor handles and draws no noise, so the
    training run is, bit for bit, the run without it.  --pbt-fitness eval: every exploit is preceded by such an evaluation and ranks
    by its fitness (--eval-metric) instead of the training episodes' returns."""

    def __init__(self, a, pop, step):
        self.pop, self.worlds, self.runs, self.seconds, self.path = pop, a.eval_scenarios, 0, 0.0, os.path.join(a.out, "eval_log.csv")
        pop.bind_eval([scenario_config(s, a.eval_envs, a.eval_max_steps, a.eval_seed, a.ped_vmax, **env_switches(a)) for s in a.eval_scenarios],
                      quota=a.eval_episodes, metric=a.eval_metric, step=step)
        open_csv(self.path, EVAL_CSV_COLUMNS).close()

    def run(self, it):
        t = time.time()
        fitness = self.pop.evaluate()                                  # [P], on the device; the summary below is the one host read
        with open_csv(self.path, EVAL_CSV_COLUMNS) as f:
            for j, row in enumerate(self.pop.evaluator().summary().tolist()):
                f.write(",".join(["%d" % it, "%d" % (j // len(self.worlds)), self.worlds[j % len(self.worlds)]] + ["%.9g" % v for v in row]) + "\n")
        self.runs, self.seconds = self.runs + 1, self.seconds + time.time() - t
        return fitness

    def close(self, t0):
        print("evaluation: %d runs of %d jobs, %.1f s of %.1f s (host clock, from the first enqueue to the summary's read)"
              % (self.runs, len(self.pop.evaluator().jobs), self.seconds, time.time() - t0))
        self.pop.evaluator().close()


class PopulationSide:
    """What build_members built, bound for run_loop: every switch is resolved here, once, into the calls a launch makes, and the two
    values of each give the same run, bit for bit.  --population-act one-launch: ONE act launch for all members (Population.act) and
    ONE re-pack of the P actors (sync_actors); per-member: P act_mfma calls and P sync_fused_weights, 4 launches each.
    --population-record one-call: ONE record call of two launches for all members' replay writes and episode logs (Population.record);
    per-member: P x (add_masked, counters, returns, log add) and the copies around them.  --population-step per-member: one grouped
    step (cn_step_multi), a kernel per member on its stream between two rounds of stream waits; one-launch: ONE launch on the loop's
    stream (MemberEnvs.bind_step_group, cn_step_group_step), for the jobs of the bound evaluation too.  The start gate: the updates
    begin once EVERY member's replay holds more than a batch -- a member whose ring is not ready yet (it lost rows to reset launches)
    holds the others back, so that the update counters, which key the sampling and drive policy_delay, stay aligned."""

    def __init__(self, a, members, envs, agents, pop):
        self.a, self.envs, self.agents, self.pop = a, envs, agents, pop
        group_step, self.one_call = a.population_step == "one-launch", a.population_record == "one-call"
        self.act = act = torch.zeros((envs.N, 2), dtype=torch.float32, device=envs.device)
        step_all = envs.bind_step_group(act, auto_reset="next") if group_step else envs.bind_step_all(act, auto_reset="next")
        self.obs = obs = envs.reset(group=group_step)                  # (one-launch: the reset is the group's, one launch too)
        self.runs = [RunLog(m, m.out, DeviceEpisodeLog(obs.device, a.max_csv_rows), (envs.cfg.dt_ms + envs.cfg.scan_latency_ms) / 1000.0, Member(m, ag),
                            prefix="member %2d  " % p) for p, (m, ag) in enumerate(zip(members, agents))]
        self.rows = rows = [envs.rows(p) for p in range(len(agents))]
        self.resetting = torch.zeros(envs.N, dtype=torch.bool, device=obs.device)
        self.prev = prev = torch.empty_like(obs)
        self.elogs = [r.elog for r in self.runs]
        if a.population_act == "one-launch":
            pop.bind_act([obs[r] for r in rows], [act[r] for r in rows])  # (packs the actors)
            act_all, self.sync_all, self.sync_unbound = (lambda: pop.act(add_noise=True)), pop.sync_actors, (lambda: None)
        else:
            act_all = lambda: [ag.act_mfma(obs[r], out=act[r], add_noise=True) for ag, r in zip(agents, rows)]
            self.sync_all = self.sync_unbound = lambda: [ag.sync_fused_weights() for ag in agents]    # (unbound: those Population does not re-pack itself)
            self.sync_all()
        keep_prev = lambda: prev.copy_(obs)
        if self.one_call:
            keep_prev()                                                # once: every record() leaves the new observation in prev
            pop.bind_record(envs.envs, *[[x[r] for r in rows] for x in (prev, obs, act, envs.reward, envs.done)], self.elogs,
                            **(dict(n_step=a.n_step) if getattr(a, "n_step", 1) > 1 else {}))      # (--n-step 1: the call as it always was)
        # a launch: these calls, then record(it).  fork: the members' streams wait for the loop's (the actions, or the group's step);
        # join: the loop's waits for theirs (record_members joins after its reads on their streams)
        self.calls = [act_all] + {(True, True): [step_all],            # one launch on this stream: no wait before it, none behind it
                                  (True, False): [envs.fork, step_all, envs.join],
                                  (False, True): [keep_prev, step_all, envs.fork],
                                  (False, False): [keep_prev, envs.fork, step_all]}[self.one_call, group_step]
        self.record = pop.record if self.one_call else self.record_members
        self.pbt = Pbt(a, pop, self.elogs, self.sync_unbound) if a.pbt_every else None
        self.eval_fitness = bool(a.pbt_every) and a.pbt_fitness == "eval"
        self.evaluation = Evaluation(a, pop, "group" if group_step else "multi") if a.eval_every or self.eval_fitness else None
        self.ready, self.learn, self.after_updates, self.save_state = pop.ready, pop.learn, self.sync_all, pop.save_state
        self.before_log = self.pbt.before_log if self.pbt else (lambda: None)
        self.close = (lambda: self.evaluation.close(self.runs[0].t0)) if self.evaluation else (lambda: None)

    def launch(self, it):
        for call in self.calls:
            call()
        self.record(it)

    def record_members(self, it):
        envs, reward, done = self.envs, self.envs.reward, self.envs.done
        cnt = [e.counters() for e in envs.envs]
        ret = [e.returns()[0] for e in envs.envs]
        envs.join()
        keep = ~self.resetting
        for p, (ag, r) in enumerate(zip(self.agents, self.rows)):
            ag.memory.add_masked(self.prev[r], self.act[r], reward[r], self.obs[r], done[r], keep[r])
            self.elogs[p].add(done[r], cnt[p], ret[p], it, keep[r])
        self.resetting = done.bool()

    def after_launch(self, it, learning):                              # the evaluation, if due or if the exploit ranks by it; then the exploit
        exploiting = learning and self.a.pbt_every and it % self.a.pbt_every == 0
        due = (self.a.eval_every and it % self.a.eval_every == 0) or (exploiting and self.eval_fitness)
        fitness = self.evaluation.run(it) if due else None             # (its own handles and no noise draw)
        if exploiting:
            self.pbt.exploit(it, fitness if self.eval_fitness else None)

    def state(self):                                                   # (parse_args: not with an evaluation's handles)
        t = dict(obs=self.obs, prev=self.prev, act=self.act, reward=self.envs.reward, done=self.envs.done, resetting=self.resetting)
        t.update({"record_resetting%d" % p: self.pop.resetting(p) for p in range(len(self.agents))} if self.one_call else {})
        if getattr(self.a, "n_step", 1) > 1:                           # the n-step recorder's pending store
            t.update({"record_pending%d_%s" % (p, k): v for p in range(len(self.agents)) for k, v in zip(PENDING_NAMES, self.pop.record_pending(p))})
        t.update(dict(pbt_flushed=self.pbt.flushed, pbt_tot=self.pbt.tot) if self.pbt else {})
        files = [os.path.join(r.out, r.learner.csv_name + ".csv") for r in self.runs] if self.a.csv else []
        return self.envs.envs, t, dict(pbt_applied=self.pbt.applied if self.pbt else 0), files + ([self.pbt.path] if self.pbt else [])

    def load_state(self, d, scalars):
        self.pop.load_state(d)                                         # (re-packs the bound actors; the agents' hyper-parameters follow)
        self.sync_unbound()
        if self.pbt:
            self.pbt.applied = int(scalars["pbt_applied"])


def train_population(a):
    """--population P: P independent TD3 runs, seeds a.seed ... a.seed + P - 1, whose updates are ONE cn_td3_pop_update per update
    (crowdnav.td3.Population) instead of P processes.  Member p has what `train()` with --seed <seed + p> has -- its environment
    handle of --envs environments, its Agent, replay, RunLog -- and writes what that run writes into <out>/member<p>/.  While PBT is
    off (--pbt-every 0, --pbt-spread 0: the default), member p's run IS the solo run --seed <seed + p> --learner fused (same parameters,
    same CSV rows) as long as the members' rings pass the batch size on the same launch (PopulationSide's start gate); from then on a
    member that was held back would, solo, have started its updates earlier."""
    fill_defaults(a)
    torch.cuda.set_device(a.device)
    side = run_loop(a, PopulationSide(a, *build_members(a)))
    return side.agents, [run.episodes for run in side.runs]


def report_evaluation(a, scenario, st):
    """--evaluate's printed line and CSV for one world."""
    n = len(st.rows)
    print("%s: %d episodes, success %.3f, failure %.3f, mean return %.1f, mean steps %.1f, ego %.3f, social %.3f" % (
        scenario, n, sum(r[1] for r in st.rows) / n, sum(r[2] for r in st.rows) / n, sum(r[3] for r in st.rows) / n, sum(r[4] for r in st.rows) / n,
        sum(r[5] for r in st.rows if r[5] == r[5]) / max(1, sum(1 for r in st.rows if r[5] == r[5])),
        sum(r[6] for r in st.rows if r[6] == r[6]) / max(1, sum(1 for r in st.rows if r[6] == r[6]))))
    if a.out:
        print("wrote", st.write_csv(a.out, "%s_training_test_%s" % (a.algo, scenario)))


def run_evaluation_device(a):
    """--evaluate --evaluate-on device: the loaded actor in every world of --eval-scenarios (default: --scenario) as ONE
    DeviceEvaluator run, a job per world -> the worlds' EpisodeStats."""
    specs = [scenario_config(s, a.envs, a.max_steps, a.seed, a.ped_vmax, **env_switches(a)) for s in a.eval_scenarios]
    agent = make_agent(a, specs[0][0].obs_dim, "cuda:%d" % a.device, memory_size=16)
    load_checkpoint(agent, a)
    ev = DeviceEvaluator([(cfg, init, vel, agent, w) for w, (cfg, init, vel) in enumerate(specs)], a.device)
    ev.run(a.episodes_per_env)
    ev.finish("success")
    table = ev.summary().tolist()
    stats = [ev.stats(w) for w in range(len(specs))]
    for s, st in zip(a.eval_scenarios, stats):
        report_evaluation(a, s, st)
    if a.out and a.eval_summary:
        path = os.path.join(a.out, "eval_summary.csv")
        with open(path, "w") as fp:
            fp.write(",".join(("world",) + EVAL_SUMMARY_COLUMNS) + "\n")
            for s, row in zip(a.eval_scenarios, table):
                fp.write(",".join([s] + ["%.9g" % v for v in row]) + "\n")
        print("wrote", path)
    ev.close()
    return stats[0] if len(stats) == 1 else stats


def run_evaluation(a):
    fill_defaults(a)
    torch.cuda.set_device(a.device)
    if a.evaluate_on == "device":
        return run_evaluation_device(a)
    env = make_env(a.scenario, a.envs, a.max_steps, a.seed, a.device, a.ped_vmax, **env_switches(a))
    if a.algo == "dqn":           # greedy: Agent.act(add_noise=False) takes epsilon = 0
        agent = make_dqn_agent(a, env.D, "cuda:%d" % a.device, 16)
        a.load_episode = resolve_load_episode(a.load, a.load_episode)
        agent.load_models(os.path.join(a.load, "dqn_model_ep%d.pt" % a.load_episode))
    else:
        agent = make_agent(a, env.D, "cuda:%d" % a.device, memory_size=16)
        load_checkpoint(agent, a)
    st = evaluate(env, agent, episodes_per_env=a.episodes_per_env)
    report_evaluation(a, a.scenario, st)
    return st


def build_parser():
    """The command line's parser: every flag and its default."""
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
    ap.add_argument("--ou-act", default=None, choices=["torch", "fused"], help="--ou-noise only: torch (default) = Agent.act(add_noise=True) "
                    "and reset_noise, eager PyTorch; fused = Agent.act_ou_fused: actor, OU update, noise.reset() and clip in one cn_ddpg_act launch")
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
                    "fused: cn_td3_update / cn_ddpg_update (csrc/crowdnav_td3.hip, crowdnav_ddpg.hip)")
    ap.add_argument("--actor-final-init", type=float, default=None, help="NOT the reference: U(+-x) initialisation of the actor's output layer (e.g. 0.003)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--population", type=int, default=0, help="P > 0: train P independent TD3 agents, seeds --seed ... --seed + P - 1, their updates "
                    "as one cn_td3_pop_update (1 ... 64; --algo td3 --learner fused only, not with --evaluate or --load); member p has its own "
                    "--envs environments and writes into <out>/member<p>/ what the solo run --seed <seed + p> writes into <out>")
    ap.add_argument("--population-act", default=None, choices=["one-launch", "per-member"], help="--population only: one-launch (default) = all "
                    "members act in one cn_actor_pop_forward and re-pack in one cn_actor_pop_pack per training launch; per-member = one "
                    "cn_actor_forward and one 4-launch re-pack per member.  Same results, bit for bit")
    ap.add_argument("--population-record", default=None, choices=["one-call", "per-member"], help="--population only: one-call (default) = all "
                    "members' replay writes and episode logs in one cn_pop_record (two launches) per training launch; per-member = one "
                    "cn_replay_write, cn_get_counters, cn_get_returns and cn_episode_log_add per member.  Same results, bit for bit")
    ap.add_argument("--n-step", type=int, default=1, help="W > 1: the replay holds W-step transitions -- R = sum_{k<W} gamma^k r_{t+k} and the "
                    "observation W steps on, accumulated on the device by cn_nstep_record (two launches per training launch) -- and the TD3 "
                    "target bootstraps with gamma^W; rows that an episode's end cuts short carry d = 1.  1 ... 16, default 1 = one-step rows, "
                    "the calls and the results of a run without the switch.  --algo td3 with --reset-mode next; solo runs, and --population "
                    "with --population-record one-call; not with gamma in --pbt-explore.  --memory must hold --envs * W rows.  Give it "
                    "again on --resume")
    ap.add_argument("--population-replay", default=None, choices=["own", "shared"], help="--population only: own (default) = every member's "
                    "update samples its own replay ring; shared = every member samples the union of all members' rings, uniformly over its "
                    "live rows (cn_td3_pop_set_replay_source: the rings stay where they are, only the update's first launch reads "
                    "differently); the updates begin once the rings together hold more than a batch.  <out>/run.json records it")
    ap.add_argument("--population-step", default=None, choices=["per-member", "one-launch"], help="--population only: per-member (default) = "
                    "one step kernel per member on the member's stream (cn_step_multi) between two rounds of stream waits; one-launch = "
                    "all members' environments in ONE launch on the loop's stream (cn_step_group_step), for the training members and for "
                    "the jobs of --eval-every / --pbt-fitness eval.  Same results, bit for bit.  <out>/run.json records it")
    ap.add_argument("--pbt-every", type=int, default=None, help="--population only: L > 0 = population-based training, one Population.exploit() "
                    "(cn_td3_pop_exploit) after the updates of every L-th launch once learning has begun: the worst members copy the best "
                    "members' networks and optimizer state and perturb their hyper-parameters, on the device; rows go to <out>/pbt_log.csv.  "
                    "Default 0 = off (needs --population >= 2)")
    ap.add_argument("--pbt-fraction", type=float, default=None, help="--population only: the fraction f of the members replaced per exploit, "
                    "n_replace = max(1, floor(P f)) <= P / 2 (default 0.25)")
    ap.add_argument("--pbt-factor", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="--population only: an explored "
                    "hyper-parameter is multiplied by one of these two (default 0.8 1.2)")
    ap.add_argument("--pbt-explore", default=None, help="--population only: comma-separated names of the hyper-parameters a replaced member "
                    "perturbs, of " + ", ".join(PBT_HYPERS) + " (default lr_actor,lr_critic,noise_std); the others are inherited unchanged")
    ap.add_argument("--pbt-min-episodes", type=int, default=None, help="--population only: an exploit changes nothing while a member has "
                    "finished fewer than this many episodes since the last one that applied (default 10)")
    ap.add_argument("--pbt-spread", type=float, default=None, help="--population only: S > 0 = member p starts with lr_actor, lr_critic and "
                    "noise_std multiplied by a keyed log-uniform factor in [1/S, S] (default 0 = all members start alike)")
    ap.add_argument("--pbt-fitness", default=None, choices=["log", "eval"], help="--pbt-every only: what an exploit ranks the members by.  log "
                    "(default) = the mean return of the exploration-noise training episodes each finished since the last applied exploit; eval = "
                    "every exploit is preceded by one evaluation on the device (greedy actors, identical worlds: the --eval-* flags) and is "
                    "called with its fitness")
    ap.add_argument("--evaluate-on", default=None, choices=["host", "device"], help="--evaluate with --algo td3 / ddpg: host (default) = "
                    "rollout.evaluate, the PyTorch actor and one host read per launch; device = rollout.DeviceEvaluator, the f32-MFMA actor "
                    "and cn_eval_record, three enqueues per launch and no read until the end (the same CSV file name and printed line)")
    ap.add_argument("--eval-scenarios", default=None, help="comma-separated worlds.  With --evaluate --evaluate-on device: all of them in one run, "
                    "one CSV per world and <out>/eval_summary.csv with one row per world (default: --scenario alone, no summary file).  With "
                    "--population: the worlds every member is evaluated in (default crossing_8)")
    ap.add_argument("--eval-every", type=int, default=None, help="--population only: L > 0 = after the updates of every L-th launch all members "
                    "are evaluated once on the device; rows launch, member, world and the 8 summary columns go to <out>/eval_log.csv (one "
                    "host read per evaluation).  Default 0 = off")
    ap.add_argument("--eval-envs", type=int, default=None, help="--population only: environments per member and world of an evaluation (default 16)")
    ap.add_argument("--eval-episodes", type=int, default=None, help="--population only: episodes counted per evaluation environment (default 1)")
    ap.add_argument("--eval-max-steps", type=int, default=None, help="--population only: nsteps of the evaluation worlds (default: --max-steps)")
    ap.add_argument("--eval-seed", type=int, default=None, help="--population only: the evaluation worlds' seed, one for all members (default: --seed)")
    ap.add_argument("--eval-metric", default=None, choices=["success", "return"], help="--population only: what a member's fitness averages over "
                    "its worlds: the success rate (default) or the mean return")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="default: runs/<algo>")
    ap.add_argument("--csv", action="store_true", help="one CSV row per finished episode in the reference's 8-column schema (recorded on the device, appended to the file at "
                    "every log interval); `timelapse` = the episode's own virtual duration, steps x (0.15 s + scan wait) -- TRAIN:141 "
                    "measures wall time since the episode's start, which the reference's time.sleep(0.15) makes the same quantity")
    ap.add_argument("--max-csv-rows", type=int, default=2_000_000)
    ap.add_argument("--load", default=None)
    ap.add_argument("--load-episode", default="latest", help="the <N> of td3_*_model_ep<N>.pt, or `latest` = the count in <load>/latest_checkpoint.txt")
    ap.add_argument("--state-every", type=int, default=0, help="L > 0: at the end of every L-th launch the run's whole state goes to "
                    "<out>/state/launch<it>/ (the learner's blob -- networks, Adam's state, counters, a population's hyper-parameters and PBT "
                    "state: one launch -- the replays, the environments' snapshots, the loop's tensors, logs and counts) and <out>/state/latest "
                    "names it; --algo td3 --learner fused, solo or --population, --reset-mode next, without --eval-every / --pbt-fitness eval")
    ap.add_argument("--state-keep", type=int, default=1, help="--state-every: how many state directories stay (older ones are removed once the "
                    "new one is complete)")
    ap.add_argument("--resume", default=None, metavar="DIR", help="continue the run whose --out was DIR from the state DIR/state/latest names, "
                    "at the launch after it, bit for bit: give the command line of that run (--launches may be larger); CSVs and pbt_log.csv "
                    "are appended, checkpoint labels go on growing.  --out defaults to DIR")
    ap.add_argument("--evaluate", action="store_true")
    ap.add_argument("--episodes-per-env", type=int, default=1)
    return ap


class Args(argparse.Namespace):
    """What parse_args returns.  The state switches (--state-every, --state-keep, --resume), --population-replay, --population-step and --n-step are attributes like
    every other switch, but they are held beside vars(): the namespace vars() gives for a command line stays, key for key, what it was
    before these switches (tests/test_eval_layout.py holds it to a record), and a Namespace built by hand or copied from vars() simply
    has none -- getattr(a, "state_every", 0) -- so the members of a population are handed `resume` by name."""
    __slots__ = ("_state",)
    STATE = dict(state_every=0, state_keep=1, resume=None, population_replay=None, population_step=None, n_step=1)

    def __init__(self, **kw):
        object.__setattr__(self, "_state", dict(self.STATE))
        super().__init__(**kw)


for _name in Args.STATE:
    setattr(Args, _name, property(lambda self, n=_name: self._state[n], lambda self, v, n=_name: self._state.__setitem__(n, v)))


def parse_args(argv=None):
    """The command line with the algorithm's defaults resolved (max_steps, obs_layout, out)."""
    ap = build_parser()
    a = ap.parse_args(argv, namespace=Args())
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
        a.out = a.resume if a.resume else "runs/%s" % a.algo
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
            ap.error("--population starts its members fresh: --load is not supported (a population continues from its whole state: "
                     "--state-every while it runs, then --resume)")
        if a.reset_mode != "next":
            ap.error("--population collects with the next-step reset only (--reset-mode next)")
    if a.population_act is not None and not a.population:
        ap.error("--population-act selects how a --population acts: it needs --population")
    if a.population_act is None:
        a.population_act = "one-launch"
    if a.population_record is not None and not a.population:
        ap.error("--population-record selects how a --population records its transitions: it needs --population")
    if a.population_record is None:
        a.population_record = "one-call"
    if a.population_replay is not None and not a.population:
        ap.error("--population-replay selects whose replay rings a --population's updates sample: it needs --population")
    if a.population_replay is None:
        a.population_replay = "own"
    if a.population_step is not None and not a.population:
        ap.error("--population-step selects how a --population's environments are stepped: it needs --population")
    if a.population_step is None:
        a.population_step = "per-member"
    pbt_given = [k for k in ("pbt_every", "pbt_fraction", "pbt_factor", "pbt_explore", "pbt_min_episodes", "pbt_spread") if getattr(a, k) is not None]
    if pbt_given and not a.population:
        ap.error("%s: population-based training acts on a --population: it needs --population" % ", ".join("--" + k.replace("_", "-") for k in pbt_given))
    for k, v in (("pbt_every", 0), ("pbt_fraction", 0.25), ("pbt_factor", [0.8, 1.2]), ("pbt_explore", "lr_actor,lr_critic,noise_std"),
                 ("pbt_min_episodes", 10), ("pbt_spread", 0.0)):
        if getattr(a, k) is None:
            setattr(a, k, v)
    a.pbt_factor = tuple(a.pbt_factor)
    a.pbt_explore = tuple(n for n in a.pbt_explore.split(",") if n)
    a.pbt_n_replace = 0
    if pbt_given:
        if a.pbt_every < 0 or a.pbt_min_episodes < 1 or a.pbt_spread < 0 or not all(0 < f < float("inf") for f in a.pbt_factor):
            ap.error("--pbt-every and --pbt-spread must be >= 0, --pbt-min-episodes >= 1 and both --pbt-factor values finite and > 0")
        unknown = [n for n in a.pbt_explore if n not in PBT_HYPERS]
        if unknown:
            ap.error("--pbt-explore: unknown hyper-parameter(s) %s; known: %s" % (", ".join(unknown), ", ".join(PBT_HYPERS)))
        if not 0 <= a.pbt_fraction <= 1:
            ap.error("--pbt-fraction must be a fraction of the population, 0 ... 1")
    if a.pbt_every:
        if a.population < 2:
            ap.error("--pbt-every needs --population >= 2: the worst member copies from another")
        a.pbt_n_replace = max(1, int(a.population * a.pbt_fraction))
        if a.pbt_n_replace > a.population // 2:
            ap.error("--pbt-fraction %g of --population %d replaces %d members: at most half (%d) can be replaced, the others are the sources"
                     % (a.pbt_fraction, a.population, a.pbt_n_replace, a.population // 2))
    if a.n_step != 1:
        if not 1 <= a.n_step <= 16:
            ap.error("--n-step must be 1 ... 16 (CN_NSTEP_MAX)")
        if a.algo != "td3":
            ap.error("--n-step records n-step rows for TD3's target (--algo td3), not --algo %s" % a.algo)
        if a.reset_mode != "next":
            ap.error("--n-step accumulates along the next-step reset's loop (--reset-mode next), not --reset-mode %s" % a.reset_mode)
        if a.population and a.population_record != "one-call":
            ap.error("--n-step is cn_nstep_record, the one-call recorder's sibling: it needs --population-record one-call, not %s" % a.population_record)
        if a.pbt_every and "gamma" in a.pbt_explore:
            ap.error("--n-step does not go with gamma in --pbt-explore: the learner's tables hold gamma^W, which an explore step would move "
                     "away from the recorder's window weights")
        if a.memory < a.envs * a.n_step:
            ap.error("--n-step %d: a launch can write --envs * W = %d rows, more than --memory %d holds" % (a.n_step, a.envs * a.n_step, a.memory))
    if a.pbt_fitness is not None and not a.pbt_every:
        ap.error("--pbt-fitness selects what an exploit ranks by: it needs --pbt-every")
    if a.pbt_fitness is None:
        a.pbt_fitness = "log"
    if a.evaluate_on is not None and not (a.evaluate and a.algo in ("td3", "ddpg")):
        ap.error("--evaluate-on selects how --evaluate runs a td3 / ddpg actor: it needs --evaluate with --algo td3 or ddpg")
    if a.evaluate_on is None:
        a.evaluate_on = "host"
    eval_given = [k for k in EVAL_POPULATION_FLAGS if getattr(a, k) is not None]
    if eval_given and not a.population:
        ap.error("%s: the evaluation of a population during its training: it needs --population" % ", ".join("--" + k.replace("_", "-") for k in eval_given))
    if a.eval_scenarios is not None and not (a.population or a.evaluate_on == "device"):
        ap.error("--eval-scenarios names the worlds of an evaluation on the device: it needs --population or --evaluate --evaluate-on device")
    a.eval_summary = a.eval_scenarios is not None and a.evaluate_on == "device"      # (eval_summary.csv: only when the worlds were listed)
    if a.eval_scenarios is None:
        a.eval_scenarios = a.scenario if a.evaluate_on == "device" else "crossing_8"
    a.eval_scenarios = tuple(s for s in a.eval_scenarios.split(",") if s)
    for k, v in (("eval_every", 0), ("eval_envs", 16), ("eval_episodes", 1), ("eval_max_steps", a.max_steps), ("eval_seed", a.seed), ("eval_metric", "success")):
        if getattr(a, k) is None:
            setattr(a, k, v)
    if a.eval_every < 0 or a.eval_envs < 1 or a.eval_episodes < 1 or a.eval_max_steps < 1:
        ap.error("--eval-every must be >= 0 and --eval-envs, --eval-episodes and --eval-max-steps >= 1")
    if not a.eval_scenarios or len(set(a.eval_scenarios)) != len(a.eval_scenarios):
        ap.error("--eval-scenarios: at least one world, each named once")
    if max(1, a.population) * len(a.eval_scenarios) > 64:
        ap.error("--eval-scenarios: %d worlds for %d actor(s) are %d jobs: one evaluation takes at most 64"
                 % (len(a.eval_scenarios), max(1, a.population), max(1, a.population) * len(a.eval_scenarios)))
    if a.state_every or a.resume or a.state_keep != 1:
        which = "--resume" if a.resume else "--state-every" if a.state_every else "--state-keep"
        if a.state_every < 0 or a.state_keep < 1:
            ap.error("--state-every must be >= 0 and --state-keep >= 1")
        if not (a.state_every or a.resume):
            ap.error("--state-keep says how many --state-every directories stay: it needs --state-every")
        if a.algo != "td3":
            ap.error("%s saves and loads the fused TD3 learner's state (--algo td3), not --algo %s" % (which, a.algo))
        if a.learner != "fused":
            ap.error("%s is cn_td3_state_save / _load, the fused learner's state: it needs --learner fused" % which)
        if a.evaluate:
            ap.error("%s continues a training run: it does not apply to --evaluate" % which)
        if a.eval_every or a.pbt_fitness == "eval":
            ap.error("%s does not cover an evaluation's handles (--eval-every, --pbt-fitness eval): they keep their simulator clock "
                     "across resets, which no state holds yet" % which)
        if a.reset_mode != "next":
            ap.error("%s holds the next-step reset's loop (--reset-mode next), not --reset-mode %s" % (which, a.reset_mode))
        if a.resume and a.load:
            ap.error("--resume restores the networks with everything else: --load does not apply")
        if a.resume:
            try:
                resolve_resume(a.resume)
            except FileNotFoundError as ex:
                ap.error(str(ex))
    if a.ou_noise and a.algo != "ddpg":
        ap.error("--ou-noise is DDPG's exploration (--algo ddpg)")
    if a.ou_act is not None and not a.ou_noise:
        ap.error("--ou-act selects how --ou-noise acts: it needs --ou-noise")
    if a.ou_act is None:
        a.ou_act = "torch"
    return a


def fill_defaults(a):
    """Give a Namespace that a caller built by hand every option it lacks, at the value the command line without that flag gives
    (the algorithm's own defaults resolved for a.algo); what it sets stays untouched."""
    for k, v in vars(parse_args(["--algo", vars(a).get("algo", build_parser().get_default("algo"))])).items():
        if not hasattr(a, k):
            setattr(a, k, v)
    return a


def main(argv=None):
    a = parse_args(argv)
    if a.evaluate and a.algo not in TABULAR:
        return run_evaluation(a)
    if a.population:
        return train_population(a)
    return train(a)


if __name__ == "__main__":
    main()
