"""BASELINE.json configs 2, 3, 4 and 5 at their FULL sizes against the CPU oracle, through the C-ABI (`-m gpu`).

  config 2   4096 envs x 20 pedestrians x 360 rays, K = 8, one MI355X
  config 3   4096 envs, the TD3 actor in the loop (cn_actor_forward -> cn_step chains on 4 stream groups)
  config 4   envs sharded over ranks by global index, all-gather of episode returns: two ranks with the REAL kernel
             (two processes sharing cuda:0, gloo) against one handle
  config 5   4096 envs x 100 pedestrians x 720 rays (dense crowd, the LDS-pressure case)

Envs are independent, so the oracle needs < 1 s per config here (OpenMP over envs).  Bar: equality -- done flags, top-K
indices, observations, rewards, returns and counters equal the oracle's (float32 outputs: its float64 values cast to float32)."""
import os
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, load_seq

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _one_oracle_thread_afterwards(oracle_mod):
    yield
    oracle_mod.set_num_threads(1)


def test_config2_full_size_4096_envs(oracle_mod):
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    N, STEPS = 4096, 40
    cfg = Config(n_envs=N, n_peds=20, n_rays=360, k_obstacles=8, max_steps=30, seed=1234, ped_cycle_ms=1400)
    env = VecEnv(cfg); env.enable_f64_obs()
    orc = oracle_mod.Oracle(cfg.as_dict())
    oracle_mod.set_num_threads()      # every usable CPU (cgroup-aware), back to 1 in the fixture below
    env.reset(); torch.cuda.synchronize()
    assert np.array_equal(env.obs_f64.cpu().numpy(), orc.reset())
    g = torch.Generator(device="cpu").manual_seed(7)
    n_done = exact = 0
    for t in range(STEPS):
        act = torch.stack([torch.rand(N, generator=g) * 0.22, torch.rand(N, generator=g) * 4 - 2], 1)
        mode = "next" if t >= STEPS // 2 else "same"       # both reset conventions at full size
        env.step(act.cuda(), auto_reset=mode, want_final=True); torch.cuda.synchronize()
        oc, rc, dc, ic, fc = orc.step(act.numpy().astype(np.float64), auto_reset=mode, want_final=True)
        assert np.array_equal(env.done.cpu().numpy(), dc), t                      # bit-exact
        assert np.array_equal(env.topk_idx.cpu().numpy(), ic), t                  # bit-exact
        assert np.array_equal(env.reward.cpu().numpy(), rc.astype(np.float32)), t
        og = env.obs_f64.cpu().numpy()
        assert np.array_equal(og, oc), t
        assert np.array_equal(env.obs.cpu().numpy(), oc.astype(np.float32)), t
        exact += int((og == oc).all(1).sum()); n_done += int(dc.sum())
    assert np.array_equal(env.counters().cpu().numpy()[:, :6], orc.counters())
    assert n_done > N // 2 and exact == STEPS * N


def test_config5_full_size_dense_crowd_4096_envs(oracle_mod):
    """4096 envs x 100 pedestrians x 720 rays in the 4.8 m room: every env every step against the oracle (the oracle needs
    ~1 ms per env-step here, so 30 steps with OpenMP over the envs)."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    N, STEPS = 4096, 30
    cfg = Config(n_envs=N, n_peds=100, n_rays=720, k_obstacles=8, room_half=2.4, max_steps=12, seed=4321, ped_cycle_ms=1400)
    env = VecEnv(cfg); env.enable_f64_obs()
    orc = oracle_mod.Oracle(cfg.as_dict())
    oracle_mod.set_num_threads()
    env.reset(); torch.cuda.synchronize()
    assert np.array_equal(env.obs_f64.cpu().numpy(), orc.reset())
    g = torch.Generator(device="cpu").manual_seed(9)
    n_done = exact = 0
    for t in range(STEPS):
        act = torch.stack([torch.rand(N, generator=g) * 0.22, torch.rand(N, generator=g) * 4 - 2], 1)
        mode = "next" if t >= STEPS // 2 else "same"
        env.step(act.cuda(), auto_reset=mode, want_final=True); torch.cuda.synchronize()
        oc, rc, dc, ic, fc = orc.step(act.numpy().astype(np.float64), auto_reset=mode, want_final=True)
        assert np.array_equal(env.done.cpu().numpy(), dc), t
        assert np.array_equal(env.topk_idx.cpu().numpy(), ic), t
        assert np.array_equal(env.reward.cpu().numpy(), rc.astype(np.float32)), t
        og = env.obs_f64.cpu().numpy()
        assert np.array_equal(og, oc), t
        exact += int((og == oc).all(1).sum()); n_done += int(dc.sum())
    assert np.array_equal(env.counters().cpu().numpy()[:, :6], orc.counters())
    assert (env.counters().cpu().numpy()[:, 6] == 0).all()          # status: no track / segment overflow in the dense crowd
    assert n_done > N // 4 and exact == STEPS * N


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_config3_actor_in_the_loop_4096_envs(oracle_mod, sigma):
    """The act -> step chain of rollout_groups at full size: 4 stream groups, each running cn_actor_forward then cn_step
    on its own stream.  Every step the GPU's actions are copied to the host and drive the oracle; the trajectory the
    policy sees (observations -> actions -> observations ...) must then be the oracle's, for 50 steps."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnvGroups
    from crowdnav.rollout import rollout_groups
    from crowdnav.td3 import Agent
    N, STEPS = 4096, 50
    cfg = Config(n_envs=N, n_peds=20, max_steps=25, seed=77, ped_cycle_ms=1400)
    envs = VecEnvGroups(cfg, groups=4)
    agent = Agent(obs_dim=envs.D, device="cuda", seed=5, memory_size=16, explore_sigma=sigma)
    with torch.no_grad():                 # spread the random-init actor's outputs so that the robots really move
        agent.actor.linear1.weight.mul_(4.0); agent.actor.linear3.weight.mul_(10.0)
    orc = oracle_mod.Oracle(cfg.as_dict())
    oracle_mod.set_num_threads()      # every usable CPU (cgroup-aware), back to 1 in the fixture below
    o0 = envs.reset(); torch.cuda.synchronize()
    oc = orc.reset()
    assert np.array_equal(o0.cpu().numpy(), oc.astype(np.float32))
    envs._started = True
    n_done = 0
    acts_seen = []
    for t in range(STEPS):
        rollout_groups(envs, agent, 1, add_noise=sigma > 0, auto_reset="next")
        torch.cuda.synchronize()
        act = envs._act.cpu().numpy()
        assert act[:, 0].min() >= 0.0 and act[:, 0].max() <= 0.22 and np.abs(act[:, 1]).max() <= 2.0
        oc, rc, dc, ic = orc.step(act.astype(np.float64), auto_reset="next")
        assert np.array_equal(envs.done.cpu().numpy(), dc), t
        assert np.array_equal(envs.topk_idx.cpu().numpy(), ic), t
        assert np.array_equal(envs.reward.cpu().numpy(), rc.astype(np.float32)), t
        assert np.array_equal(envs.obs.cpu().numpy(), oc.astype(np.float32)), t
        n_done += int(dc.sum()); acts_seen.append(act[:64].copy())
    assert n_done > N
    a = np.stack(acts_seen)
    assert a[:, :, 1].std() > 1e-4                                   # the policy reacts to what it observes
    if sigma > 0:                              # groups draw different noise; steps draw different noise
        assert not np.array_equal(acts_seen[0], acts_seen[1])
    envs.close()


def test_training_return_rises(tmp_path):
    """Does the return rise?  The as-logged training run -- presets.training(drop_cospawned=True), the reference's
    hyper-parameters and its one update of 128 per env-step (16 envs x 16 updates per launch), the reward the published log shows
    (waypoint_reward 0), cn_td3_update, the next-step reset kernel, seed 0 -- for 30 000 launches (~40 s): nothing is learnt during
    the first 6 000 launches, and by the end the policy reaches the goal in a good part of its episodes.  The run is bit-reproducible
    (counter-based sampling and noise, no atomics in the update), so this is a fixed trajectory, not a statistical test: the same
    command as profiles/r05/train/td3_as_logged_fused_e16_u16_wp0_seed0.txt, whose launch-30000 line reads 2712 episodes and whose
    success rate passes 0.4 between launches 16 000 and 18 000.  (Every change of the update's summation order is another
    trajectory -- round 4's kernels passed 0.4 at launch 16 000 with 1069 episodes at 18 000 -- and which seeds escape the reward's
    local optimum within a minute changes with it: profiles/r05/train/README.md.  The bounds below are this tree's.)"""
    import re
    from crowdnav import train as T
    a = T.main.__globals__["argparse"].Namespace(scenario="training_as_logged", envs=16, launches=30000, max_steps=1000, updates=16, batch=128,
                                                 memory=1_000_000, checkpoint_every=10 ** 9, log_every=1000, ped_vmax=None, seed=0, device=0,
                                                 out=str(tmp_path / "run"), csv=False, load=None, load_episode=0, evaluate=False,
                                                 episodes_per_env=1, graphs=1, waypoint_reward=0, scan_f32=None, wheel_accel=None,
                                                 reset_mode="next", max_csv_rows=100000, time_limit=0.0, learner="fused")
    agent, episodes = T.train(a)
    lines = [l for l in open(os.path.join(a.out, "progress.txt")).read().splitlines() if l.startswith("launch")]
    win = [(int(m.group(1)), float(m.group(2)), float(m.group(3))) for m in
           (re.search(r"launch\s+(\d+) .* success ([0-9.]+)  mean return\s+(-?[0-9.]+)", l) for l in lines) if m]
    assert len(win) == 30 and 2300 <= episodes <= 3100, (episodes, lines)     # 2712 on every box so far
    early, late = [w for w in win if w[0] <= 6000], [w for w in win if w[0] > 25000]
    assert max(w[1] for w in early) <= 0.15, lines                     # sigma = 1 exploration alone rarely reaches the goal
    assert max(w[1] for w in late) >= 0.4, lines                       # ... the trained policy does
    assert max(w[2] for w in late) > max(w[2] for w in early) + 100.0, lines


def test_fused_replay_write_and_episode_log_equal_the_pytorch_formulation():
    """cn_replay_write / cn_episode_log_add (the collection loop's bookkeeping, TRAIN:129-149 + ReplayBuffer.add TD3:24-31, as two
    and one launches) against the PyTorch formulation they replace (DeviceReplay / DeviceEpisodeLog with fused=False): the same
    calls on both -- masked and plain adds mixed, row counts below and above one scan chunk (1024), the ring wrapping several times,
    the episode log running past its capacity -- leave the same ring, position, fill level, rows, row count and totals."""
    import torch
    from crowdnav.td3 import DeviceReplay
    from crowdnav.train import DeviceEpisodeLog
    g = torch.Generator(device="cuda").manual_seed(5)
    cap, D = 5003, 11
    A, B = DeviceReplay(cap, D, "cuda"), DeviceReplay(cap, D, "cuda", fused=False)
    assert A.fused and not B.fused
    EA, EB = DeviceEpisodeLog(torch.device("cuda"), 700), DeviceEpisodeLog(torch.device("cuda"), 700, fused=False)
    assert EA.fused and not EB.fused
    rnd = lambda *sh: torch.randn(sh, generator=g, device="cuda")
    coin = lambda n, p: torch.rand(n, generator=g, device="cuda") < p
    for it in range(14):
        n = [5, 16, 1, 1024, 2050, 1025, 333][it % 7]
        s, a, r, s2 = rnd(n, D), rnd(n, 2), rnd(n), rnd(n, D)
        d = coin(n, 0.3).to(torch.uint8) if it % 2 else coin(n, 0.3)
        keep = coin(n, 0.7)
        for R in (A, B):
            if it % 3 == 2: R.add(s, a, r, s2, d)
            else: R.add_masked(s, a, r, s2, d, keep)
        cnt = torch.randint(0, 50, (n, 14), generator=g, device="cuda", dtype=torch.int32)
        ret = rnd(n) * 100
        for E in (EA, EB):
            E.add(d, cnt, ret, it + 1, keep)
        torch.cuda.synchronize()
        assert int(A.pos_dev) == int(B.pos_dev) and int(A.size_dev) == int(B.size_dev), it
        for x, y in ((A.s, B.s), (A.a, B.a), (A.r, B.r), (A.s2, B.s2), (A.d, B.d)):
            assert torch.equal(x[:cap], y[:cap]), it
        assert len(A) == len(B)
        assert int(EA.n) == int(EB.n)
        assert torch.equal(EA.rows[:700], EB.rows[:700]), it
        assert torch.allclose(EA.tot, EB.tot, rtol=1e-12, atol=0), (EA.tot, EB.tot)
    assert int(A.size_dev) == cap and int(EA.n) > 700                # the ring wrapped; the log ran past its capacity
    ra, ta = EA.flush(); rb, tb = EB.flush()
    assert torch.equal(ra, rb) and ra.shape[0] == 700 and ta[0] == tb[0]


@pytest.mark.parametrize("reset_mode", ["next", "same"])
def test_batched_trainer_runs_on_the_next_step_reset_kernel(tmp_path, reset_mode):
    """crowdnav.train (TRAIN:40-168 batched) without a host synchronisation per launch: the actor as one kernel
    (cn_actor_forward), the replay's masked add and the episode log on the device.  reset_mode "next" (the fast
    one-observation kernel): a finished env's next launch is its reset and is masked out of the replay, so the buffer holds
    exactly the env-steps taken; "same" (the older path, kept for A/B runs): every launch is a transition and s' of a finished
    env is final_obs.  Terminal transitions carry done = 1 and the terminal observation; the CSV has one row per episode in the
    reference's 8-column schema; evaluation rows carry the episode's duration (TRAIN:141 timelapse)."""
    import torch
    from crowdnav import train as T
    a = T.main.__globals__["argparse"].Namespace(scenario="bench", envs=64, launches=120, max_steps=25, updates=1, batch=64, memory=20000,
                                                 checkpoint_every=10 ** 9, log_every=50, ped_vmax=None, seed=3, device=0,
                                                 out=str(tmp_path / "run"), csv=True, load=None, load_episode=0, evaluate=False,
                                                 episodes_per_env=1, graphs=1, waypoint_reward=0, scan_f32=None, wheel_accel=None,
                                                 reset_mode=reset_mode, max_csv_rows=100000, time_limit=0.0,
                                                 learner="fused" if reset_mode == "next" else "torch")
    agent, episodes = T.train(a)
    m = agent.memory
    assert episodes > 64 and len(m) == m.size == int(m.size_dev.item())
    if reset_mode == "next":
        # 120 launches x 64 envs, minus one launch per finished episode (except episodes that finished in the very last launch)
        assert 120 * 64 - episodes <= len(m) <= 120 * 64 - episodes + 64
    else:
        assert len(m) == 120 * 64
    d = m.d[:m.size, 0]
    assert 0 < int(d.sum().item()) <= episodes
    # a terminal transition's s' is the terminal observation, not a fresh episode's first one: the robot is where the episode
    # ended, i.e. either inside the goal box, at max_steps, or with a scan below min_scan_range (0.12)
    term = torch.nonzero(d > 0).flatten()[:50]
    assert (m.s2[term, :359].min(1).values < 0.6).any()
    assert float(m.r[:m.size].max()) <= 200.0            # waypoint_reward = 0: nothing above the goal reward
    import csv
    rows = list(csv.reader(open(os.path.join(a.out, "td3_training.csv"))))
    assert rows[0] == ["episode_number", "success_episode", "failure_episode", "episode_reward", "episode_step", "ego_safety_score",
                       "social_safety_score", "timelapse"] and len(rows) - 1 == episodes
    assert all(1 <= int(r[4]) <= 25 for r in rows[1:]) and any(int(r[4]) == 25 for r in rows[1:])
    from crowdnav.env import VecEnv
    from crowdnav import Config
    from crowdnav.rollout import evaluate
    st = evaluate(VecEnv(Config(n_envs=32, max_steps=20, seed=4)), agent)
    assert len(st.rows) == 32 and all(abs(r[7] - r[4] * 0.16) < 1e-9 and r[7] > 0 for r in st.rows)


def test_device_replay_masked_add_without_a_host_read():
    """DeviceReplay.add_masked: kept rows land in consecutive ring slots after the device-side position (wrapping), the others in
    the spare row; sample() never returns an unwritten row."""
    import torch
    from crowdnav.td3 import DeviceReplay
    m = DeviceReplay(10, 3, "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    want = []
    for it in range(7):
        s = torch.rand((4, 3), generator=g, device="cuda") + it
        keep = torch.tensor([it % 2 == 0, True, it % 3 != 0, False], device="cuda")
        m.add_masked(s, s[:, :2], s[:, 0], s + 100, keep, keep)
        want += [s[i] for i in range(4) if bool(keep[i])]
    n = m.sync_len()
    assert n == 10 and len(want) > 10 and m.pos == len(want) % 10
    for j, row in enumerate(want[-10:]):
        slot = (len(want) - 10 + j) % 10
        assert torch.equal(m.s[slot], row) and torch.equal(m.s2[slot], row + 100) and float(m.r[slot]) == float(row[0])
    m2 = DeviceReplay(100, 3, "cuda")
    m2.add_masked(torch.ones((4, 3), device="cuda"), torch.ones((4, 2), device="cuda"), torch.ones(4, device="cuda"),
                  torch.ones((4, 3), device="cuda"), torch.zeros(4, device="cuda"), torch.tensor([True, False, True, True], device="cuda"))
    assert m2.sync_len() == 3 and bool((m2.sample(64)[0] == 1).all())


def test_graphed_td3_update_equals_the_eager_update():
    """Agent.enable_graphs: the TD3 update captured into two hipGraphs (critics only / critics + actor + soft updates).
    (a) enable_graphs leaves parameters and optimizer state untouched (its warm-up runs on a copy);
    (b) the graphs compute _update's arithmetic: fed the same replay rows and target noise through the eager path of an
        identically built agent (capturable Adam on both sides), six updates give the same parameters bit for bit;
    (c) the golden vectors of the REFERENCE's learn() still hold after enable_graphs (explicit batches take the eager path
        with the capturable optimizers)."""
    import torch
    from crowdnav.td3 import Agent

    def build():
        ag = Agent(device="cuda", memory_size=4096, obs_dim=46, hidden=32, batch_size=16, seed=5)
        g = torch.Generator(device="cuda").manual_seed(11)
        n = 600
        ag.memory.add(torch.randn((n, 46), generator=g, device="cuda"), torch.rand((n, 2), generator=g, device="cuda"),
                      torch.randn(n, generator=g, device="cuda"), torch.randn((n, 46), generator=g, device="cuda"),
                      (torch.rand(n, generator=g, device="cuda") < 0.1))
        return ag
    a, b = build(), build()
    before = [p.detach().clone() for m in (a.actor, a.q1, a.q2, a.actor_t, a.q1_t, a.q2_t) for p in m.parameters()]
    a.enable_graphs(); b.enable_graphs()
    after = [p for m in (a.actor, a.q1, a.q2, a.actor_t, a.q1_t, a.q2_t) for p in m.parameters()]
    assert all(torch.equal(x, y) for x, y in zip(before, after))                       # (a)
    assert all(float(st["step"]) == 0.0 and not st["exp_avg"].any() for o in (a.opt_a, a.opt_q1, a.opt_q2) for st in o.state.values())
    # (b) a: graph replays; b: the eager path on exactly the rows / noise a's graph drew (re-drawn from the same generator state)
    for step in range(6):
        st = torch.cuda.get_rng_state("cuda")
        a.learn(step)
        torch.cuda.synchronize()
        torch.cuda.set_rng_state(st, "cuda")
        u = torch.rand(16, device="cuda")
        idx = (u * float(len(b.memory))).long().clamp_(max=len(b.memory) - 1)
        noise = torch.randn((16, 2), device="cuda")
        m = b.memory
        b.learn(step, batch=(m.s[idx], m.a[idx], m.r[idx], m.s2[idx], m.d[idx]), target_noise=noise)
    for ma, mb in ((a.actor, b.actor), (a.q1, b.q1), (a.q2, b.q2), (a.actor_t, b.actor_t), (a.q1_t, b.q1_t), (a.q2_t, b.q2_t)):
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(pa, pb)
    # (c) the reference's learn() goldens through an agent that has graphs enabled
    G = np.load(os.path.join(ROOT, "tests", "golden", "td3.npz"))
    ag = Agent(device="cuda", memory_size=64, obs_dim=46, hidden=32, batch_size=16)
    nets = dict(actor=ag.actor, actor_t=ag.actor_t, q1=ag.q1, q1_t=ag.q1_t, q2=ag.q2, q2_t=ag.q2_t)
    for k, m_ in nets.items():
        m_.load_state_dict({n: torch.from_numpy(G["init.%s.%s" % (k, n)]).cuda() for n in m_.state_dict()})
    ag.memory.add(torch.zeros((32, 46), device="cuda"), torch.zeros((32, 2), device="cuda"), torch.zeros(32, device="cuda"),
                  torch.zeros((32, 46), device="cuda"), torch.zeros(32, device="cuda", dtype=torch.bool))
    ag.enable_graphs()
    dev = lambda x: torch.from_numpy(x).cuda()
    batch = (dev(G["upd_s"]), dev(G["upd_a"]), dev(G["upd_r"])[:, None], dev(G["upd_s2"]), dev(G["upd_d"])[:, None])
    for step in range(4):
        ag.learn(step, batch=batch, target_noise=dev(G["upd_noise"][step]))
        for k, m_ in nets.items():
            for n, v in m_.state_dict().items():
                np.testing.assert_allclose(v.cpu().numpy(), G["step%d.%s.%s" % (step, k, n)], rtol=5e-4, atol=2e-6, err_msg="step %d %s.%s" % (step, k, n))


@pytest.mark.parametrize("shape", [(398, 256, 128), (46, 32, 16), (370, 64, 48), (45, 24, 10), (131, 72, 37), (7, 5, 3)])
def test_fused_td3_update_matches_the_pytorch_update(shape):
    """cn_td3_update (csrc/crowdnav_td3.hip: the TD3 update as 7 + 5 hand-written launches -- MFMA GEMMs forward and backward,
    weight gradients and soft updates folded into Adam, TD target / heads evaluated inside the GEMMs) against crowdnav.td3.Agent._update (the
    PyTorch restatement of td3.py:225-285, itself pinned on the reference's learn() goldens): two identically initialised agents,
    the same explicit batches and target-policy noise, six updates (three with the actor step and the soft updates) -- every
    parameter of the six networks agrees up to float32 summation order.  Shapes: the product's (398 -> 256 -> 256, batch 128), the
    goldens' (46 -> 32, batch 16), and four with ragged tile edges (odd row lengths, a batch smaller than a tile, a batch that is
    not a multiple of the reduction step)."""
    import torch
    from crowdnav.td3 import Agent
    obs_dim, hidden, B = shape
    a = Agent(obs_dim=obs_dim, hidden=hidden, batch_size=B, seed=3, memory_size=4 * B, device="cuda")
    b = Agent(obs_dim=obs_dim, hidden=hidden, batch_size=B, seed=3, memory_size=4 * B, device="cuda")
    nets = lambda ag: (ag.actor, ag.actor_t, ag.q1, ag.q1_t, ag.q2, ag.q2_t)
    for ma, mb in zip(nets(a), nets(b)):
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(pa, pb)
    a.enable_fused_update()
    g = torch.Generator(device="cuda").manual_seed(17)
    for step in range(6):
        batch = (torch.randn((B, obs_dim), generator=g, device="cuda") * 0.5,
                 torch.rand((B, 2), generator=g, device="cuda") * torch.tensor([0.22, 4.0], device="cuda") - torch.tensor([0.0, 2.0], device="cuda"),
                 torch.randn((B, 1), generator=g, device="cuda") * 3.0, torch.randn((B, obs_dim), generator=g, device="cuda") * 0.5,
                 (torch.rand((B, 1), generator=g, device="cuda") < 0.2).float())
        noise = torch.randn((B, 2), generator=g, device="cuda")
        a.learn(step, batch=batch, target_noise=noise)
        b.learn(step, batch=batch, target_noise=noise)
        torch.cuda.synchronize()
        worst = 0.0
        for ma, mb in zip(nets(a), nets(b)):
            for (n_, pa), pb in zip(ma.named_parameters(), mb.parameters()):
                diff = (pa - pb).abs()
                # Adam's first steps move every weight by ~lr whatever the gradient's size, so a gradient that cancels to ~0 can
                # land on the other side of zero in another summation order: allow a handful of such weights (<= 2 lr apart)
                bad = diff > (2e-6 + 2e-4 * pb.abs())
                assert int(bad.sum()) <= max(2, pa.numel() // 2000), (step, n_, int(bad.sum()), float(diff.max()))
                assert float(diff.detach().max()) <= 2.5 * 3e-4 * (step + 1), (step, n_, float(diff.detach().max()))
                worst = max(worst, float(diff.detach().max()))
    # the fused path also samples the replay and draws the target noise on the device: it runs and changes the networks
    a.memory.add(batch[0], batch[1], batch[2][:, 0], batch[3], batch[4][:, 0] > 0)
    a.memory.add(batch[0], batch[1], batch[2][:, 0], batch[3], batch[4][:, 0] > 0)
    before = [p.detach().clone() for p in a.q1.parameters()]
    for step in range(4):
        a.learn(step)
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for m in nets(a) for p in m.parameters())
    assert any(not torch.equal(x, y) for x, y in zip(before, a.q1.parameters()))


def test_fused_td3_update_on_the_reference_learn_goldens():
    """The golden vectors of the REFERENCE's own td3.Agent.learn() (tests/golden/td3.npz, oracle/make_goldens_td3.py) through
    cn_td3_update: four updates with the pinned batch and target-policy noise."""
    import torch
    from crowdnav.td3 import Agent
    G = np.load(os.path.join(ROOT, "tests", "golden", "td3.npz"))
    ag = Agent(device="cuda", memory_size=64, obs_dim=46, hidden=32, batch_size=16)
    nets = dict(actor=ag.actor, actor_t=ag.actor_t, q1=ag.q1, q1_t=ag.q1_t, q2=ag.q2, q2_t=ag.q2_t)
    for k, m in nets.items():
        m.load_state_dict({n: torch.from_numpy(G["init.%s.%s" % (k, n)]).cuda() for n in m.state_dict()})
    ag.enable_fused_update()
    dev = lambda x: torch.from_numpy(x).cuda()
    batch = (dev(G["upd_s"]), dev(G["upd_a"]), dev(G["upd_r"])[:, None], dev(G["upd_s2"]), dev(G["upd_d"])[:, None])
    losses = []
    for step in range(4):
        losses.append(ag.learn(step, batch=batch, target_noise=dev(G["upd_noise"][step])))
        torch.cuda.synchronize()
        for k, m_ in nets.items():
            for n, v in m_.state_dict().items():
                np.testing.assert_allclose(v.cpu().numpy(), G["step%d.%s.%s" % (step, k, n)], rtol=5e-4, atol=2e-6, err_msg="step %d %s.%s" % (step, k, n))
    # every call returns its own loss tensor (a collected list keeps four values, not four aliases of the last one),
    # and the tensors outlive the handle
    vals = [float(l) for l in losses]
    assert len({l.data_ptr() for l in losses}) == 4 and len(set(vals)) > 1 and all(np.isfinite(vals))
    del ag
    assert [float(l) for l in losses] == vals


@pytest.mark.parametrize("reset_mode", ["next", "same"])
def test_episode_stats_rows_match_the_reference_run(reset_mode):
    """SURVEY 8a A33 "pinned by": the batched loop's per-episode rows (EpisodeStats: success, failure, return, steps,
    ego / social safety scores) equal the tuples of the golden run the REFERENCE's Python produced (`train20`: five
    episodes), the recorded actions replayed through crowdnav.rollout.rollout under both reset conventions."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.rollout import EpisodeStats, rollout
    z, kw = load_seq("train20")
    steps = [i for i in range(len(z["now"])) if not z["is_reset"][i]]
    acts = torch.tensor(np.stack([z["action"][i] for i in steps]), dtype=torch.float32, device="cuda")
    env = VecEnv(Config(n_envs=1, **kw))
    env.set_ped_init(z["ped_init"])
    stats = EpisodeStats()
    if reset_mode == "same":
        rollout(env, None, len(steps), stats=stats, policy=lambda obs, t: acts[t:t + 1].contiguous(), auto_reset="same")
    else:
        # next-step reset (rollout's default): the launch after a finished episode is the env's Env.reset and ignores its action,
        # so the recorded action stream pauses for that launch
        used = [0]

        def policy(obs, t):
            if t > 0 and bool(env.done[0].item()):
                return torch.zeros((1, 2), device="cuda")
            used[0] += 1
            return acts[used[0] - 1:used[0]].contiguous()
        n_eps = int(sum(bool(z["done"][i]) for i in steps))
        rollout(env, None, len(steps) + n_eps - 1, stats=stats, policy=policy)
        assert used[0] == len(steps)
    # the reference's tuples, episode by episode (TRAIN:142-161)
    want, ret, n = [], 0.0, 0
    for i in steps:
        ret += float(z["reward"][i]); n += 1
        if z["done"][i]:
            ego_v, soc_v, seen = (int(c) for c in z["counters"][i])
            want.append((bool(z["status"][i][0]), bool(z["status"][i][1]), ret, n,
                         1.0 - ego_v * 1.0 / seen if seen else float("nan"), 1.0 - soc_v * 1.0 / seen if seen else float("nan")))
            ret, n = 0.0, 0
    assert len(want) == 5 and len(stats.rows) == len(want)
    for row, w in zip(stats.rows, want):
        assert (row[1], row[2]) == (w[0], w[1])
        assert row[3] == pytest.approx(w[2], abs=1e-3) and row[4] == w[3]        # return (float32 on the device), steps
        for got, exp in ((row[5], w[4]), (row[6], w[5])):
            assert (got != got and exp != exp) or got == pytest.approx(exp, abs=1e-12)


def _rank_worker(rank, world, port, n_total, steps, q):
    for p_ in (ROOT, PKG):
        sys.path.insert(0, p_)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.rollout import gather_returns, shard_range
    base, n = shard_range(n_total, rank, world)
    env = VecEnv(Config(n_envs=n, env_index_base=base, max_steps=15, seed=77))     # both ranks share cuda:0
    env.reset()
    g = torch.Generator(device="cpu").manual_seed(123)
    done_count = 0
    for t in range(steps):
        act = torch.stack([torch.rand(n_total, generator=g) * 0.22, torch.rand(n_total, generator=g) * 4 - 2], 1)
        _, _, d = env.step(act[base:base + n].contiguous().cuda(), auto_reset=True)
        done_count += int(d.sum().item())
    allr = gather_returns(env.returns()[0].cpu())            # gloo: host tensors
    obs = [torch.empty_like(env.obs.cpu()) for _ in range(world)]
    dist.all_gather(obs, env.obs.cpu())
    total = torch.tensor([done_count]); dist.all_reduce(total)
    if rank == 0:
        q.put((allr.numpy(), torch.cat(obs).numpy(), int(total.item())))
    dist.barrier()
    dist.destroy_process_group()


def test_config4_two_ranks_with_the_real_kernel():
    """World size 2 with the HIP kernel (not the oracle) as the environment: rank r owns global envs [r N/2, (r+1) N/2)
    with env_index_base = r N/2; the gathered returns and observations equal a single handle of N envs."""
    import torch
    import torch.multiprocessing as mp
    from crowdnav import Config
    from crowdnav.env import VecEnv
    N_TOTAL, STEPS = 256, 40
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, N_TOTAL, STEPS, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    allr, allobs, total = q.get(timeout=300)
    for p_ in procs:
        p_.join(timeout=120)
        assert p_.exitcode == 0
    env = VecEnv(Config(n_envs=N_TOTAL, max_steps=15, seed=77))
    env.reset()
    g = torch.Generator(device="cpu").manual_seed(123)
    dc = 0
    for t in range(STEPS):
        act = torch.stack([torch.rand(N_TOTAL, generator=g) * 0.22, torch.rand(N_TOTAL, generator=g) * 4 - 2], 1)
        _, _, d = env.step(act.cuda(), auto_reset=True)
        dc += int(d.sum().item())
    assert total == dc and dc >= N_TOTAL
    assert np.array_equal(allr, env.returns()[0].cpu().numpy())
    assert np.array_equal(allobs, env.obs.cpu().numpy())


def test_config4_full_workload_16384_envs_as_8_shards(oracle_mod):
    """BASELINE configs[3] at ITS workload on one GPU: 16384 envs x 20 pedestrians x 360 rays as the 8 shards the 8 ranks
    would own (8 handles x 2048 envs, env_index_base = 2048 r, each on its own stream), every env every step against the
    oracle (one 16384-env oracle, OpenMP over envs) and against ONE 16384-env handle, in both reset conventions; then the
    host-side equivalent of the path's one exchange: the concatenated per-shard returns equal the single handle's."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    N, S, STEPS = 16384, 8, 24
    n = N // S
    cfg = Config(n_envs=N, n_peds=20, n_rays=360, k_obstacles=8, max_steps=18, seed=4321, ped_cycle_ms=1400)
    import dataclasses
    shards = [VecEnv(dataclasses.replace(cfg, n_envs=n, env_index_base=r * n), stream=torch.cuda.Stream()) for r in range(S)]
    one = VecEnv(cfg)
    orc = oracle_mod.Oracle(cfg.as_dict())
    oracle_mod.set_num_threads()
    for e in shards:
        e.reset()
    one.reset()
    torch.cuda.synchronize()
    oc = orc.reset()
    assert np.array_equal(torch.cat([e.obs for e in shards]).cpu().numpy(), oc.astype(np.float32))
    assert np.array_equal(one.obs.cpu().numpy(), oc.astype(np.float32))
    g = torch.Generator(device="cpu").manual_seed(17)
    n_done = 0
    for t in range(STEPS):
        act = torch.stack([torch.rand(N, generator=g) * 0.22, torch.rand(N, generator=g) * 4 - 2], 1)
        mode = "next" if t >= STEPS // 2 else "same"
        ad = act.cuda()
        torch.cuda.synchronize()
        for r, e in enumerate(shards):
            e.step(ad[r * n:(r + 1) * n], auto_reset=mode)
        one.step(ad, auto_reset=mode)
        torch.cuda.synchronize()
        oc, rc, dc, ic = orc.step(act.numpy().astype(np.float64), auto_reset=mode)
        dg = torch.cat([e.done for e in shards]).cpu().numpy()
        assert np.array_equal(dg, dc), t                                                       # bit-exact
        assert np.array_equal(torch.cat([e.topk_idx for e in shards]).cpu().numpy(), ic), t    # bit-exact
        assert np.array_equal(torch.cat([e.reward for e in shards]).cpu().numpy(), rc.astype(np.float32)), t
        og = torch.cat([e.obs for e in shards])
        assert np.array_equal(og.cpu().numpy(), oc.astype(np.float32)), t
        assert torch.equal(og, one.obs) and torch.equal(torch.cat([e.done for e in shards]), one.done), t
        n_done += int(dc.sum())
    assert n_done > N // 2
    rets = [e.returns()[0] for e in shards]          # each on its shard's stream
    cnts = [e.counters() for e in shards]
    torch.cuda.synchronize()
    ret = torch.cat(rets)
    assert torch.equal(ret, one.returns()[0])
    assert np.array_equal(ret.cpu().numpy(), orc.returns().astype(np.float32))
    assert np.array_equal(torch.cat(cnts).cpu().numpy()[:, :6], orc.counters())


def test_step_sequence_at_the_bench_shape_4096_envs_20_steps_equals_step_by_step():
    """The exact launches bench.py's sequence legs time (VERDICT r04 "weak" 1): cn_env_kernel_seq_s360 over 4096 envs x T = 20
    after the bench's pre-roll -- in place (bind_step_sequence) and into trajectory buffers (the round-5 `sequence_traj` leg) --
    against 20 calls of cn_step (cn_env_kernel_fair_s360_w4: four environments per workgroup since round 5): every step's observation / reward / done in the trajectory, the final
    outputs, the whole state record, counters and returns.  Same seed, pedestrian cycle and open-loop action law as bench.py."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    N, T, PRE = 4096, 20, 60
    cfg = Config(n_envs=N, n_peds=20, n_rays=360, k_obstacles=8, max_steps=1000, seed=1234, ped_cycle_ms=1400)
    ref, inplace, tr = VecEnv(cfg), VecEnv(cfg), VecEnv(cfg)
    assert ref.kernel_name("sequence") == "cn_env_kernel_seq_s360" and ref.kernel_name("step") == "cn_env_kernel_fair_s360_w4"
    g = torch.Generator(device="cuda").manual_seed(1234)
    acts = torch.stack([torch.rand((PRE + 2 * T, N), generator=g, device="cuda") * 0.22,
                        torch.rand((PRE + 2 * T, N), generator=g, device="cuda") * 4.0 - 2.0], 2).contiguous()
    for e in (ref, inplace, tr):
        e.reset()
        e.bind_step_sequence(acts[:PRE])()             # pre-roll: de-phased envs, live tracks, some finished episodes
    torch.cuda.synchronize()
    assert np.array_equal(ref.snapshot(), inplace.snapshot())
    D = ref.D
    traj = dict(obs=torch.zeros((T, N, D), device="cuda"), reward=torch.zeros((T, N), device="cuda"),
                done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"))
    for rnd in range(2):                                # two consecutive 20-step launches, as consecutive bench samples are
        a = acts[PRE + rnd * T:PRE + (rnd + 1) * T]
        inplace.bind_step_sequence(a)()
        tr.bind_step_sequence(a, traj=traj)()
        n_done = 0
        for t in range(T):
            ref.step(a[t], auto_reset="next")
            torch.cuda.synchronize()
            assert torch.equal(traj["obs"][t], ref.obs) and torch.equal(traj["reward"][t], ref.reward), (rnd, t)
            assert torch.equal(traj["done"][t], ref.done), (rnd, t)
            n_done += int(ref.done.sum())
        assert n_done > 0
        assert torch.equal(inplace.obs, ref.obs) and torch.equal(inplace.reward, ref.reward) and torch.equal(inplace.done, ref.done)
        assert torch.equal(inplace.topk_idx, ref.topk_idx)
        for other in (inplace, tr):
            assert np.array_equal(other.snapshot(), ref.snapshot())
            assert torch.equal(other.counters(), ref.counters()) and torch.equal(other.returns()[0], ref.returns()[0])


@pytest.mark.parametrize("risk_mode", [0, 1])
def test_step_sequence_kernel_equals_step_by_step(oracle_mod, risk_mode):
    """cn_step_sequence -- T open-loop steps in ONE launch, every wavefront keeping its env and walking the T steps at its own
    pace -- leaves the trajectory T calls of cn_step (next-step reset) leave: observations, rewards, done flags and indices of
    EVERY step (trajectory buffers), the final state record (snapshot), counters and returns; in place and into trajectory
    buffers, with per-step actions and with one action held for T steps, across consecutive calls.  The step-by-step run is
    checked against the oracle at every step as well."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    N, T = 640, 45
    cfg = Config(n_envs=N, n_peds=20, max_steps=18, seed=43, ped_cycle_ms=1400, risk_mode=risk_mode)
    ref, seq, inplace = VecEnv(cfg), VecEnv(cfg), VecEnv(cfg)
    orc = oracle_mod.Oracle(cfg.as_dict())
    oracle_mod.set_num_threads()
    o0 = ref.reset(); seq.reset(); inplace.reset(); torch.cuda.synchronize()
    assert np.array_equal(o0.cpu().numpy(), orc.reset().astype(np.float32))
    g = torch.Generator(device="cpu").manual_seed(6)
    D, K = ref.D, ref.K
    for call in range(3):
        acts = torch.stack([torch.rand((T, N), generator=g) * 0.22, torch.rand((T, N), generator=g) * 4 - 2], 2).cuda().contiguous()
        if call == 2:
            acts = acts[:1].expand(T, N, 2)                   # action repeat: one [N, 2] held for T steps (stride 0)
        traj = dict(obs=torch.zeros((T, N, D), device="cuda"), reward=torch.zeros((T, N), device="cuda"),
                    done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"), topk_idx=torch.zeros((T, N, K), dtype=torch.int32, device="cuda"))
        seq.step_sequence(acts, traj=traj)
        if call == 2:
            inplace.step_sequence(acts)
        else:
            inplace.bind_step_sequence(acts)()
        n_done = 0
        for t in range(T):
            ref.step(acts[t].contiguous(), auto_reset="next")
            torch.cuda.synchronize()
            assert torch.equal(traj["obs"][t], ref.obs) and torch.equal(traj["reward"][t], ref.reward), (call, t)
            assert torch.equal(traj["done"][t], ref.done) and torch.equal(traj["topk_idx"][t], ref.topk_idx), (call, t)
            oc, rc, dc, ic = orc.step(acts[t].cpu().numpy().astype(np.float64), auto_reset="next")
            assert np.array_equal(ref.done.cpu().numpy(), dc) and np.array_equal(ref.topk_idx.cpu().numpy(), ic), (call, t)
            assert np.array_equal(ref.obs.cpu().numpy(), oc.astype(np.float32)), (call, t)
            n_done += int(dc.sum())
        assert n_done > N
        for other in (seq, inplace):
            assert torch.equal(other.obs, ref.obs) and torch.equal(other.reward, ref.reward) and torch.equal(other.done, ref.done)
            assert np.array_equal(other.snapshot(), ref.snapshot())
            assert torch.equal(other.counters(), ref.counters()) and torch.equal(other.returns()[0], ref.returns()[0])
        assert torch.equal(inplace.topk_idx, ref.topk_idx)
    # (round 6: the other observation layouts and the contact ticks have the one-launch forms too --
    #  test_one_launch_paths_of_the_other_simulators_equal_step_by_step)
    import crowdnav
    with pytest.raises(crowdnav.CrowdNavError):
        _abi_check_negative_stride(VecEnv(Config(n_envs=16)))


def _abi_check_negative_stride(env):
    """cn_step_sequence still validates its arguments: a negative stride is CN_ERR_ARG"""
    import ctypes as C
    from crowdnav import _abi
    import torch
    a = torch.zeros((2, env.N, 2), device="cuda")
    io = _abi.CnSequenceIO()
    io.action, io.action_stride, io.n_steps = a.data_ptr(), -1, 2
    io.obs, io.reward, io.done, io.topk_idx = env.obs.data_ptr(), env.reward.data_ptr(), env.done.data_ptr(), env.topk_idx.data_ptr()
    _abi.check(env.L.cn_step_sequence(env.h, C.byref(io), env._stream()))


def test_step_sequence_kernel_of_the_dense_shape_equals_step_by_step():
    """cn_env_kernel_seq_s720 (BASELINE configs[4]: 100 pedestrians x 720 rays, the sequence kernel compiled for that shape):
    every step's outputs and the final state record equal T calls of cn_step."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    N, T = 96, 40
    cfg = Config(n_envs=N, n_peds=100, n_rays=720, room_half=2.4, max_steps=15, seed=5, ped_cycle_ms=1400)
    ref, seq = VecEnv(cfg), VecEnv(cfg)
    assert seq.kernel_name("sequence") == "cn_env_kernel_seq_s720" and ref.kernel_name("step") in ("cn_env_kernel_s720", "cn_env_kernel_fair_s720")
    ref.reset(); seq.reset()
    g = torch.Generator(device="cpu").manual_seed(8)
    acts = torch.stack([torch.rand((T, N), generator=g) * 0.22, torch.rand((T, N), generator=g) * 4 - 2], 2).cuda().contiguous()
    D, K = ref.D, ref.K
    traj = dict(obs=torch.zeros((T, N, D), device="cuda"), reward=torch.zeros((T, N), device="cuda"),
                done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"), topk_idx=torch.zeros((T, N, K), dtype=torch.int32, device="cuda"))
    seq.step_sequence(acts, traj=traj)
    n_done = 0
    for t in range(T):
        ref.step(acts[t].contiguous(), auto_reset="next")
        torch.cuda.synchronize()
        assert torch.equal(traj["obs"][t], ref.obs) and torch.equal(traj["reward"][t], ref.reward), t
        assert torch.equal(traj["done"][t], ref.done) and torch.equal(traj["topk_idx"][t], ref.topk_idx), t
        n_done += int(ref.done.sum())
    assert n_done > N and np.array_equal(seq.snapshot(), ref.snapshot())


@pytest.mark.parametrize("shape", ["s360", "generic", "gt"])
def test_policy_rollout_kernel_equals_act_then_step(oracle_mod, shape):
    """cn_rollout_policy -- T control periods with the TD3 actor INSIDE the step kernel (16 environments per workgroup, the
    actor on their CU's matrix cores between two steps, no launch in between) -- leaves exactly what T pairs of
    (cn_actor_forward with exploration noise, cn_step with the next-step reset) leave: the actions of every period, the
    observations / rewards / done flags / indices of every period, the final state record, counters, returns and the agent's
    noise counter; into trajectory buffers and in place, across consecutive calls, for env counts that are not multiples of
    16, for the headline-shape kernel, the generic one and the gt (risk_mode 1) one.  The step-by-step run is checked against the oracle (fed the same actions) at every step."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.td3 import Agent
    N, T = (648, 30) if shape == "s360" else (200, 24)
    cfg = (Config(n_envs=N, n_peds=20, max_steps=14, seed=47, ped_cycle_ms=1400) if shape == "s360" else
           Config(n_envs=N, n_peds=12, n_rays=300, k_obstacles=6, max_steps=14, seed=48, ped_cycle_ms=1400) if shape == "generic" else
           Config(n_envs=N, n_peds=20, max_steps=14, seed=49, ped_cycle_ms=1400, risk_mode=1))
    ref, pol, inplace = VecEnv(cfg), VecEnv(cfg), VecEnv(cfg)
    assert pol.kernel_name("policy") == {"s360": "cn_policy_kernel_s360", "generic": "cn_policy_kernel", "gt": "cn_policy_kernel_gt"}[shape]
    orc = oracle_mod.Oracle(cfg.as_dict())
    oracle_mod.set_num_threads()
    agents = [Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=5, memory_size=16) for _ in range(3)]
    for ag in agents:
        ag.sync_fused_weights()
    a_ref, a_pol, a_inp = agents
    ref.reset(); pol.reset(); inplace.reset(); torch.cuda.synchronize()
    orc.reset()
    D, K = ref.D, ref.K
    act = torch.zeros((N, 2), device="cuda")
    n_done = 0
    for call in range(3):
        traj = dict(action=torch.zeros((T, N, 2), device="cuda"), obs=torch.zeros((T, N, D), device="cuda"),
                    reward=torch.zeros((T, N), device="cuda"), done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"),
                    topk_idx=torch.zeros((T, N, K), dtype=torch.int32, device="cuda"))
        pol.rollout_policy(a_pol, T, traj=traj, add_noise=(call != 2))
        if call == 1:
            inplace.bind_rollout_policy(a_inp, T)()
        else:
            inplace.rollout_policy(a_inp, T, add_noise=(call != 2))
        for t in range(T):
            a_ref.act_mfma(ref.obs, out=act, add_noise=(call != 2))
            torch.cuda.synchronize()
            assert torch.equal(traj["action"][t], act), (call, t)
            ref.step(act, auto_reset="next")
            torch.cuda.synchronize()
            assert torch.equal(traj["obs"][t], ref.obs) and torch.equal(traj["reward"][t], ref.reward), (call, t)
            assert torch.equal(traj["done"][t], ref.done) and torch.equal(traj["topk_idx"][t], ref.topk_idx), (call, t)
            oc, rc, dc, ic = orc.step(act.cpu().numpy().astype(np.float64), auto_reset="next")
            assert np.array_equal(ref.done.cpu().numpy(), dc) and np.array_equal(ref.topk_idx.cpu().numpy(), ic), (call, t)
            assert np.array_equal(ref.obs.cpu().numpy(), oc.astype(np.float32)), (call, t)
            n_done += int(dc.sum())
        assert a_pol.noise_state() == a_ref.noise_state() == a_inp.noise_state()
        for other in (pol, inplace):
            assert torch.equal(other.obs, ref.obs) and torch.equal(other.reward, ref.reward) and torch.equal(other.done, ref.done)
            assert np.array_equal(other.snapshot(), ref.snapshot())
            assert torch.equal(other.counters(), ref.counters()) and torch.equal(other.returns()[0], ref.returns()[0])
        assert torch.equal(inplace.topk_idx, ref.topk_idx) and torch.equal(inplace.last_policy_action, act)
    assert n_done > N // 2
    import crowdnav
    with pytest.raises(crowdnav.CrowdNavError):      # an actor of another observation width (K = 4 -> 382 inputs) is refused
        VecEnv(Config(n_envs=16, k_obstacles=4)).rollout_policy(a_ref, 2)


def test_small_grids_run_two_wavefronts_per_environment_with_identical_results(oracle_mod):
    """Round 5: up to 8 x CUs environments of the 360-ray shape run cn_env_kernel_s360_x2 -- a workgroup of two
    wavefronts per environment: wave 1 advances the pedestrians while wave 0 advances the robot, then takes every other 64-ray block
    of the ray loop, half of the gradient / flag-word entries and half of the association blocks; the hand-offs are LDS + s_barrier.
    Same arithmetic, same order: observations, rewards, done flags, indices and the whole state record equal the one-wave kernel's
    (CN_X2=0 at creation) step for step, and the oracle's, across resets (both reset paths of the pair)."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv, VecEnvGroups
    N = 300
    cfg = Config(n_envs=N, n_peds=20, max_steps=25, seed=71, ped_cycle_ms=1400)
    two = VecEnv(cfg)
    os.environ["CN_X2"] = "0"
    try:
        one = VecEnv(cfg)
    finally:
        del os.environ["CN_X2"]
    assert two.kernel_name("step") == "cn_env_kernel_s360_x2" and one.kernel_name("step") == "cn_env_kernel_s360_w4"
    orc = oracle_mod.Oracle(cfg.as_dict())
    oracle_mod.set_num_threads()
    o2 = two.reset(); o1 = one.reset(); torch.cuda.synchronize()
    assert torch.equal(o1, o2) and np.array_equal(o2.cpu().numpy(), orc.reset().astype(np.float32))
    g = torch.Generator(device="cpu").manual_seed(9)
    n_done = 0
    for t in range(90):
        a = torch.stack([torch.rand(N, generator=g) * 0.22, torch.rand(N, generator=g) * 4 - 2], 1).cuda().contiguous()
        two.step(a, auto_reset="next", want_final=True); one.step(a, auto_reset="next", want_final=True)
        torch.cuda.synchronize()
        assert torch.equal(two.obs, one.obs) and torch.equal(two.reward, one.reward) and torch.equal(two.done, one.done), t
        assert torch.equal(two.topk_idx, one.topk_idx) and torch.equal(two.final_obs, one.final_obs), t
        oc, rc, dc, ic = orc.step(a.cpu().numpy().astype(np.float64), auto_reset="next")
        assert np.array_equal(two.done.cpu().numpy(), dc) and np.array_equal(two.topk_idx.cpu().numpy(), ic), t
        assert np.array_equal(two.obs.cpu().numpy(), oc.astype(np.float32)), t
        n_done += int(dc.sum())
    assert n_done > N
    assert np.array_equal(two.snapshot(), one.snapshot())
    assert torch.equal(two.counters(), one.counters()) and torch.equal(two.returns()[0], one.returns()[0])
    # which kernel a launch gets: two waves per environment up to 8 x CUs environments in flight, four environments per workgroup up
    # to 16 x CUs, one wavefront per workgroup beyond -- stream groups count together (cn_set_group_envs)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert VecEnv(Config(n_envs=8 * ncu)).kernel_name("step") == "cn_env_kernel_s360_x2"
    assert VecEnv(Config(n_envs=8 * ncu + 1)).kernel_name("step") == "cn_env_kernel_fair_s360_w4"
    assert VecEnv(Config(n_envs=16 * ncu + 64)).kernel_name("step") == "cn_env_kernel_fair_s360"
    grp = VecEnvGroups(Config(n_envs=16 * ncu), groups=4)
    assert grp.envs[0].kernel_name("multi") == "cn_env_kernel_s360_w4"
    grp = VecEnvGroups(Config(n_envs=8 * ncu), groups=2)
    assert grp.envs[0].kernel_name("multi") == "cn_env_kernel_s360_x2"


ONE_LAUNCH_WORLDS = {
    # name: (config keywords, cn_step_sequence kernel, cn_rollout_policy kernel, environments per policy workgroup)
    "sf": (dict(n_peds=20, ped_mode=2), "cn_env_kernel_seq_sf", "cn_policy_kernel_sf"),
    "gt_sf": (dict(n_peds=20, ped_mode=2, risk_mode=1), "cn_env_kernel_gt_seq_sf", "cn_policy_kernel_gt_sf"),
    "sfd": (dict(n_peds=60, ped_mode=2, room_half=2.40), "cn_env_kernel_seq_sfd", "cn_policy_kernel_sfd"),
    "gt_sfd": (dict(n_peds=60, ped_mode=2, room_half=2.40, risk_mode=1), "cn_env_kernel_gt_seq_sfd", "cn_policy_kernel_gt_sfd"),
    "wa": (dict(n_peds=20, wheel_accel=1.0, scan_f32=1), "cn_env_kernel_seq_wa", "cn_policy_kernel_wa"),
    "gt_wa": (dict(n_peds=20, wheel_accel=1.0, risk_mode=1), "cn_env_kernel_gt_seq_wa", "cn_policy_kernel_gt_wa"),
    "s720": (dict(n_peds=100, n_rays=720, room_half=2.40), "cn_env_kernel_seq_s720", "cn_policy_kernel_s720"),
    # round 6: the worlds round 5 still refused -- the contact ticks (both risk modes) and the two older observation layouts
    "ct": (dict(n_peds=20, ped_contact=1), "cn_env_kernel_seq_ct", "cn_policy_kernel_ct"),
    "gt_ct": (dict(n_peds=20, ped_contact=1, risk_mode=1), "cn_env_kernel_gt_seq_ct", "cn_policy_kernel_gt_ct"),
    "orig": (dict(n_peds=20, obs_layout=1), "cn_env_kernel_seq_orig", "cn_policy_kernel_orig"),
    "rw": (dict(n_peds=20, obs_layout=2, dt_ms=50), "cn_env_kernel_seq_rw", "cn_policy_kernel_rw"),
}


@pytest.mark.parametrize("world", sorted(ONE_LAUNCH_WORLDS))
def test_one_launch_paths_of_the_other_simulators_equal_step_by_step(world):
    """Round 5: cn_step_sequence and cn_rollout_policy exist for social-force pedestrians (pair-matrix and dense
    kernels), the diff-drive plugin's wheel ramp, both risk modes -- and for BASELINE configs[4]'s shape, whose 16 working sets do
    not fit one CU's LDS: there the policy kernel runs 8 environments per workgroup.  Round 6: and for the contact ticks and the two
    older observation layouts (363 / 370 actor inputs), so every configuration cn_create accepts has both forms.  Each leaves exactly what T calls of cn_step (resp. T pairs of cn_actor_forward, cn_step) leave: every period's
    actions / observations / rewards / done flags / indices, the final state record, counters and returns, across two calls,
    with an env count that is not a multiple of the workgroup size.  (The step-by-step kernels of these worlds, and these sequence
    and policy kernels themselves, are pinned against the oracle by name in tests/test_gpu_kernel_matrix.py.)"""
    import torch
    import crowdnav
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.td3 import Agent
    kw, kseq, kpol = ONE_LAUNCH_WORLDS[world]
    N, T = (76, 8) if world == "s720" else (148, 12)
    cfg = Config(n_envs=N, max_steps=9, seed=61, ped_cycle_ms=1400, **kw)
    ref, seq, ref2, pol = VecEnv(cfg), VecEnv(cfg), VecEnv(cfg), VecEnv(cfg)
    assert seq.kernel_name("sequence") == kseq and pol.kernel_name("policy") == kpol
    D, K = ref.D, ref.K
    for e in (ref, seq, ref2, pol):
        e.reset()
    torch.cuda.synchronize()
    # ---- cn_step_sequence (open loop) against T calls of cn_step
    g = torch.Generator(device="cpu").manual_seed(3)
    n_done = 0
    for call in range(2):
        acts = torch.stack([torch.rand((T, N), generator=g) * 0.22, torch.rand((T, N), generator=g) * 4 - 2], 2).cuda().contiguous()
        traj = dict(obs=torch.zeros((T, N, D), device="cuda"), reward=torch.zeros((T, N), device="cuda"),
                    done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"), topk_idx=torch.zeros((T, N, K), dtype=torch.int32, device="cuda"))
        seq.step_sequence(acts, traj=traj)
        for t in range(T):
            ref.step(acts[t].contiguous(), auto_reset="next")
            torch.cuda.synchronize()
            assert torch.equal(traj["obs"][t], ref.obs) and torch.equal(traj["reward"][t], ref.reward), (call, t)
            assert torch.equal(traj["done"][t], ref.done) and torch.equal(traj["topk_idx"][t], ref.topk_idx), (call, t)
            n_done += int(ref.done.sum())
        assert np.array_equal(seq.snapshot(), ref.snapshot())
        assert torch.equal(seq.counters(), ref.counters()) and torch.equal(seq.returns()[0], ref.returns()[0])
    assert n_done > N // 2
    # ---- cn_rollout_policy (the actor inside the step kernel) against T pairs of (cn_actor_forward, cn_step)
    a_ref, a_pol = [Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=6, memory_size=16) for _ in range(2)]
    a_ref.sync_fused_weights(); a_pol.sync_fused_weights()
    act = torch.zeros((N, 2), device="cuda")
    for call in range(2):
        traj = dict(action=torch.zeros((T, N, 2), device="cuda"), obs=torch.zeros((T, N, D), device="cuda"),
                    reward=torch.zeros((T, N), device="cuda"), done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"),
                    topk_idx=torch.zeros((T, N, K), dtype=torch.int32, device="cuda"))
        pol.rollout_policy(a_pol, T, traj=traj)
        for t in range(T):
            a_ref.act_mfma(ref2.obs, out=act, add_noise=True)
            torch.cuda.synchronize()
            assert torch.equal(traj["action"][t], act), (call, t)
            ref2.step(act, auto_reset="next")
            torch.cuda.synchronize()
            assert torch.equal(traj["obs"][t], ref2.obs) and torch.equal(traj["reward"][t], ref2.reward), (call, t)
            assert torch.equal(traj["done"][t], ref2.done) and torch.equal(traj["topk_idx"][t], ref2.topk_idx), (call, t)
        assert a_pol.noise_state() == a_ref.noise_state()
        assert np.array_equal(pol.snapshot(), ref2.snapshot())
        assert torch.equal(pol.counters(), ref2.counters()) and torch.equal(pol.returns()[0], ref2.returns()[0])
    # an actor packed for another observation width is refused (the check reads the handle's own width, whatever the layout)
    wrong = Agent(obs_dim=cfg.obs_dim + 1, device="cuda:0", seed=6, memory_size=16)
    wrong.sync_fused_weights()
    with pytest.raises(crowdnav.CrowdNavError):
        pol.rollout_policy(wrong, 2)


def test_collect_policy_fills_the_replay_like_the_per_step_loop():
    """crowdnav.rollout.collect_policy -- cn_rollout_policy launches of `periods` periods, one masked replay add per launch --
    leaves the replay ring, its device-side position / fill level and the env exactly where the per-step loop (act_mfma ->
    step(next-step reset) -> add_masked, TRAIN:104-168) leaves them, for a period count that does not divide the step count."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.rollout import collect_policy
    from crowdnav.td3 import Agent
    N, steps = 96, 53
    cfg = Config(n_envs=N, max_steps=12, seed=21, ped_cycle_ms=1400)
    e1, e2 = VecEnv(cfg), VecEnv(cfg)
    a1 = Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=3, memory_size=4000)
    a2 = Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=3, memory_size=4000)
    assert collect_policy(e1, a1, steps, periods=8) == steps * N
    a2.sync_fused_weights()
    obs = e2.reset()
    act = torch.zeros((N, 2), device="cuda")
    resetting = torch.zeros(N, dtype=torch.bool, device="cuda")
    for t in range(steps):
        a2.act_mfma(obs, out=act)
        prev = obs.clone()
        obs, reward, done = e2.step(act, auto_reset="next")
        a2.memory.add_masked(prev, act, reward, obs, done, ~resetting)
        resetting = done.bool()
    torch.cuda.synchronize()
    m1, m2 = a1.memory, a2.memory
    assert m1.sync_len() == m2.sync_len() and 0 < len(m2) < steps * N and m1.pos == m2.pos
    n = len(m2)
    for x, y in ((m1.s, m2.s), (m1.a, m2.a), (m1.r, m2.r), (m1.s2, m2.s2), (m1.d, m2.d)):
        assert torch.equal(x[:n], y[:n])
    assert float(m2.d[:n].sum()) > N // 2                       # episodes ended inside the run (max_steps 12)
    assert torch.equal(e1.obs, e2.obs) and torch.equal(e1.done, e2.done) and np.array_equal(e1.snapshot(), e2.snapshot())
    assert torch.equal(e1._resetting, resetting) and a1.noise_state() == a2.noise_state()


def test_bind_step_sequence_equals_step_by_step():
    """VecEnvGroups.bind_step_sequence -- the path bench.py's timed region goes through (K steps x G groups behind ONE
    cn_step_multi call, a C loop over the launches) -- leaves every env where K calls of VecEnv.step leave it: observations,
    rewards, done flags, indices, counters, returns, and the snapshot of the whole state."""
    import torch
    from crowdnav import Config
    from crowdnav.env import VecEnv, VecEnvGroups
    cfg = Config(n_envs=256, seed=9, max_steps=25, ped_cycle_ms=1400)
    Ksteps = 40
    g = torch.Generator(device="cpu").manual_seed(3)
    acts = torch.stack([torch.rand((16, 256), generator=g) * 0.22, torch.rand((16, 256), generator=g) * 4 - 2], 2).cuda().contiguous()
    for G, mode in ((4, "next"), (2, "same"), (1, "next")):
        full = VecEnv(cfg)
        grp = VecEnvGroups(cfg, groups=G)
        assert torch.equal(full.reset(), grp.reset())
        seq = [acts[i % 16] for i in range(Ksteps)]
        call = grp.bind_step_sequence(seq, auto_reset=mode)
        torch.cuda.synchronize()
        call()
        grp.join()
        for a_ in seq:
            full.step(a_, auto_reset=mode)
        torch.cuda.synchronize()
        assert torch.equal(grp.obs, full.obs) and torch.equal(grp.reward, full.reward) and torch.equal(grp.done, full.done)
        assert torch.equal(grp.topk_idx, full.topk_idx)
        assert torch.equal(grp.counters(), full.counters())
        assert torch.equal(grp.returns()[0], full.returns()[0])
        assert int(full.counters()[:, 8].sum().item()) > 0                 # episodes really ended inside the sequence
        # a second sequence call continues from there (the bench repeats its timed call)
        call(); grp.join()
        for a_ in seq:
            full.step(a_, auto_reset=mode)
        torch.cuda.synchronize()
        assert torch.equal(grp.obs, full.obs) and torch.equal(grp.counters(), full.counters())
        grp.close(); full.close()


def test_bench_self_launches_two_ranks():
    """`python bench.py --gpus 2` with no launcher environment re-executes itself under torch.distributed.run and prints
    ONE JSON line with n_gpus = 2 and a measured all-gather (dry run: both ranks share cuda:0 over gloo, so the numbers
    mean nothing -- the launch path, the sharding arguments and the JSON contract are what is checked), in both the
    weak-scaling and the --envs-total (BASELINE config 4) forms."""
    import json
    import subprocess
    env = dict(os.environ, CN_BENCH_DRYRUN_GLOO="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    for extra, per_gpu, scaling in ((["--envs", "256"], 256, "weak"), (["--envs-total", "512"], 256, "strong")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2",
                            "--preroll", "5", "--groups", "2", "--repeats", "2", "--no-cpu-baseline"] + extra,
                           capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["n_gpus"] == 2 and out["scaling"] == scaling
        assert out["config"]["envs_per_gpu"] == per_gpu and out["config"]["envs_total"] == 2 * per_gpu
        ga = out["config"]["returns_allgather"]
        assert ga["ms"] is not None and ga["ranks_seen"] == 2 and ga["all_ranks_agree"] and out["value"] > 0
        pr = out["config"]["per_rank"]
        assert [p_["rank"] for p_ in pr] == [0, 1] and all(p_["value"] > 0 for p_ in pr)


def test_bench_under_the_launcher_runs_the_rccl_path_at_world_size_one():
    """The driver launches `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` on an 8-GPU node; with the
    one GPU a round can lease, the same command at N = 1 still takes the NON-gloo branch of bench.py: process group "nccl"
    (= RCCL) bound to the device, communicator init, barrier, the sample all-reduces / all-gathers on device buffers and the
    all_gather_into_tensor of the per-env episode returns -- every collective call an 8-rank run makes, executed on real
    hardware here.  (Scaling itself is the driver's 8-GPU tier; DESIGN.md section 7 holds the expected curve.)"""
    import json
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CN_BENCH_DRYRUN_GLOO", "CN_BENCH_NO_DIST"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--preroll", "20", "--repeats", "2", "--no-cpu-baseline", "--no-plateau", "--no-other-configs", "--sustained-seconds", "0.5"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    print(lines[0][:6000])            # (shown by pytest only if an assertion below fails)
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["scaling"] == "weak"
    ga = out["config"]["returns_allgather"]
    assert ga is not None and ga["collective"] == "rccl" and ga["rccl_version"] and ga["ranks_seen"] == 1 and ga["all_ranks_agree"]
    assert ga["bytes_per_rank"] == 4 * 4096 and ga["ms"] > 0 and ga["nonzero_returns"] > 0
    pr = out["config"]["per_rank"]
    assert [p_["rank"] for p_ in pr] == [0] and abs(pr[0]["value"] - out["value"]) <= 1e-6 * out["value"]
    assert out["roofline"]["kernel"].startswith("cn_env_kernel") and out["roofline"]["kernel"] == out["roofline"]["legs_kernels"][out["config"]["decomposition"]]
    # round 5: the headline is a decomposition that can serve a policy (one cn_step launch per step) -- never a cn_step_sequence leg --
    # the open-loop legs stay as comparables, flat scalar copies exist, and the sustained leg reports a rate and a shader clock
    c = out["config"]
    assert c["decomposition"] in ("4_groups", "2_groups", "1_groups") and "sequence" not in out["roofline"]["kernel"]
    assert c["leg_sequence_env_steps_s"] > 0 and c["leg_sequence_traj_env_steps_s"] > 0 and c["leg_1_groups_env_steps_s"] > 0
    assert c["leg_sequence_kernel"] == "cn_env_kernel_seq_s360"
    assert c["sustained_env_steps_s"] > 0 and c["sustained_seconds"] >= 0.4 and 500 < c["sustained_clock_mhz"] < 4000
    assert 0.1 < c["burst_over_sustained"] < 10.0      # (a sanity bound: the burst here is 5 steps, 0.2 ms, on a box that just ran 40 other tests)
    assert out["roofline"]["vector_peak_f64_tflops"] == 78.6 and out["roofline"]["frac_valu_f64"] > 0


def test_td3_update_on_the_gpu_matches_reference_learn():
    """SURVEY 8f N1 on the device path: crowdnav.td3.Agent on cuda (fused Adam, _foreach soft updates, hipBLASLt GEMMs)
    against the golden vectors of the REFERENCE's own td3.Agent.learn() (tests/golden/td3.npz, generated by
    oracle/make_goldens_td3.py from turtlebot3_rl_sim/src/td3.py): four updates with pinned replay order and
    target-policy noise.  float32 with a different summation order than the CPU run that made the goldens, hence the
    tolerance (the CPU test in test_td3_parity.py holds 2e-5)."""
    import torch
    from crowdnav.td3 import Agent
    G = np.load(os.path.join(ROOT, "tests", "golden", "td3.npz"))
    ag = Agent(device="cuda", memory_size=64, obs_dim=46, hidden=32, batch_size=16)
    nets = dict(actor=ag.actor, actor_t=ag.actor_t, q1=ag.q1, q1_t=ag.q1_t, q2=ag.q2, q2_t=ag.q2_t)
    for k, m in nets.items():
        m.load_state_dict({n: torch.from_numpy(G["init.%s.%s" % (k, n)]).cuda() for n in m.state_dict()})
    dev = lambda a: torch.from_numpy(a).cuda()
    batch = (dev(G["upd_s"]), dev(G["upd_a"]), dev(G["upd_r"])[:, None], dev(G["upd_s2"]), dev(G["upd_d"])[:, None])
    worst = 0.0
    for step in range(4):
        ag.learn(step, batch=batch, target_noise=dev(G["upd_noise"][step]))
        for k, m in nets.items():
            for n, v in m.state_dict().items():
                ref = G["step%d.%s.%s" % (step, k, n)]
                worst = max(worst, float(np.abs(v.cpu().numpy() - ref).max()))
                np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=5e-4, atol=2e-6, err_msg="step %d %s.%s" % (step, k, n))
    print("td3 cuda vs reference learn(): max abs deviation %.3g" % worst)
    # Actor forward + Agent.act clip on the device against the reference's actor outputs
    from crowdnav.td3 import Actor
    torch.manual_seed(int(G["actor_seed"]))
    actor = Actor(398, 2, 256, 0.22, 2.0)
    ag2 = Agent(device="cuda", memory_size=16, obs_dim=398)
    ag2.actor.load_state_dict(actor.state_dict())
    out = ag2.actor(dev(G["actor_obs"])).detach().cpu().numpy()
    np.testing.assert_allclose(out, G["actor_out"], rtol=0, atol=2e-6)
    for fn in (ag2.act, ag2.act_fused, ag2.act_mfma):
        a = fn(dev(G["actor_obs"][:8]), add_noise=False).cpu().numpy()
        np.testing.assert_allclose(a, G["act_single"], rtol=0, atol=3e-6)


def test_env_wrapper_get_state_and_compute_reward_replay_the_reference_run():
    """B1: Env.get_state(scan, step_counter, action) and Env.compute_reward(state, step_counter, done) called
    SEPARATELY, as Env.step does at ENV:1222-1223, on what Gazebo handed the reference in the golden run `train20`
    (recorded /scan, /odom, clock; deque append of ENV:1208-1209 through append_agent_pose): states, rewards and done
    flags are the reference's, call by call."""
    from crowdnav.env import Env

    class Scan:                           # sensor_msgs/LaserScan as far as get_state looks at it
        def __init__(self, r):
            self.ranges = list(r)

    z, kw = load_seq("train20")
    env = Env(action_dim=2, max_step=int(kw.pop("max_steps")), **kw)
    for i in range(len(z["now"])):
        env.odom_callback(z["px"][i], z["py"][i], z["yaw"][i], z["v"][i], z["w"][i], now=z["now"][i])
        if z["is_reset"][i]:
            # Env.reset (ENV:1243-1262): the library runs previous_distance / counters; then TRAIN:116
            env._v.observe_external(z["ranges"][i][None, :], [env._odom()], step_counter=[0], is_reset=True)
            import torch
            torch.cuda.synchronize()
            state = env._v.obs_f64[0].cpu().numpy()
            env.done = False
        else:
            sc = int(z["step_counter"][i])
            env.append_agent_pose(z["deque_x"][i], z["deque_y"][i], z["end_timestep"][i])
            state, done = env.get_state(Scan(z["ranges"][i]), sc, z["action"][i])
            assert isinstance(state, list) and len(state) == 398 and isinstance(done, bool)
            reward, done = env.compute_reward(state, sc, done)
            assert isinstance(reward, float) and reward == z["reward"][i], (i, reward, z["reward"][i])
            assert done == bool(z["done"][i]), i
            state = np.asarray(state)
        assert np.array_equal(state, z["obs"][i]), (i, np.nonzero(state != z["obs"][i])[0][:8])
        c = env._v.counters()[0].cpu().tolist()
        assert tuple(c[:3]) == tuple(int(x) for x in z["counters"][i]), i

