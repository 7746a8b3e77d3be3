"""One case per cell of tests/kernel_matrix.py (`-m gpu`): every kernel of csrc/crowdnav_variants.h by name.  A case creates its
handle under the cell's forcing, asserts that the handle launches the cell's kernel, and then drives it next to the CPU oracle on
the same seeded actions: 22 environments (a partial last workgroup of every launch geometry), 40 steps across four resets per
environment.  Equality, no tolerance: done, top-K indices, reward, the float32 observation, the float64 observation and the final
observation where the form writes them, the whole state record of every environment (after every step; after every launch of the
sequence and policy forms), counters and returns.  What the cells are, why their forcings select their kernels on any device, that
the oracle stays the reference over these runs and that the comparers reject a one-ulp change: tests/test_kernel_matrix.py, on the
CPU.  The oracle runs of a case take 0.01 to 0.4 s (sfd, s720), so every case keeps its own."""
import pytest

import kernel_matrix as M

pytestmark = pytest.mark.gpu


def _create(cell, monkeypatch, cfg=None):
    """the cell's handle: CN_X2 / CN_WPB are as the forcing says (absent unless named) while cn_create reads them, and only then"""
    from crowdnav import Config
    from crowdnav.env import VecEnv
    cfg = cfg or Config(**M.config_kw(cell.world))
    with monkeypatch.context() as m:
        for name in ("CN_X2", "CN_WPB"):
            m.delenv(name, raising=False)
        for name, value in cell.forcing.env.items():
            m.setenv(name, value)
        env = VecEnv(cfg, arbitration=cell.forcing.arbitration)
    return cfg, env


def _host(src, names, t=None):
    return {k: (src[k] if isinstance(src, dict) else getattr(src, k))[slice(None) if t is None else t].cpu().numpy() for k in names}


OUT = ("done", "topk_idx", "reward", "obs")


def _assert_state(env, orc, cfg, where):
    d = M.first_state_record_difference(env.snapshot(), orc, cfg.risk_mode)
    assert d is None, "%s: %s" % (where, d)


def _assert_end_of_run(env, orc, cfg):
    import torch
    counters, last = env.counters().cpu().numpy(), env.returns()[0].cpu().numpy()
    torch.cuda.synchronize()
    d = M.first_final_difference(counters, last, orc)
    assert d is None, d
    episodes, status = M.oracle_episodes_and_status(orc)
    assert episodes.min() >= 2 and not (status & (M.ST_TRACK_OVERFLOW | M.ST_CONF_OVERFLOW)).any()      # the premise held in this run


def _reset_both(env, orc, cfg, form):
    import torch
    env.reset()
    torch.cuda.synchronize()
    d = M.first_reset_difference(_host(env, ("obs",) + (("obs_f64",) if env.obs_f64 is not None else ())), orc.reset(), form)
    assert d is None, "reset launch: %s" % d
    _assert_state(env, orc, cfg, "after the reset launch")


def _run_steps(cell, cfg, env, orc):
    import torch
    mode = "next" if cell.form == "step" else "same"
    env.enable_f64_obs()
    _reset_both(env, orc, cfg, cell.form)
    for t, a in enumerate(M.actions()):
        env.step(torch.from_numpy(a).cuda(), auto_reset=mode, want_final=True)
        torch.cuda.synchronize()
        d = M.first_output_difference(_host(env, OUT + ("obs_f64", "final_obs")), M.oracle_step(orc, a, mode), cell.form)
        assert d is None, "step %d: %s" % (t, d)
        _assert_state(env, orc, cfg, "after step %d" % t)


def _traj(env, with_action):
    import torch
    T, N = M.T_LAUNCH, env.N
    traj = dict(obs=torch.zeros((T, N, env.D), device="cuda"), reward=torch.zeros((T, N), device="cuda"),
                done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"), topk_idx=torch.zeros((T, N, env.K), dtype=torch.int32, device="cuda"))
    if with_action:
        traj["action"] = torch.zeros((T, N, 2), device="cuda")
    return traj


def _run_sequence(cell, cfg, env, orc):
    import torch
    _reset_both(env, orc, cfg, cell.form)
    for launch, acts in enumerate(M.sequence_actions()):
        a = torch.from_numpy(acts).cuda().contiguous()
        if launch == M.HELD_LAUNCH:
            a = a[:1].expand(M.T_LAUNCH, env.N, 2)               # one [N, 2] action held for the whole launch: action_stride 0
            assert a.stride(0) == 0
        traj = _traj(env, False)
        env.step_sequence(a, traj=traj)
        torch.cuda.synchronize()
        for t in range(M.T_LAUNCH):
            d = M.first_output_difference(_host(traj, OUT, t), M.oracle_step(orc, acts[t], "next"), cell.form)
            assert d is None, "launch %d step %d: %s" % (launch, t, d)
        _assert_state(env, orc, cfg, "after launch %d" % launch)


def _run_policy(cell, cfg, env, orc):
    import torch
    from crowdnav.td3 import Agent
    agent, twin = [Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=M.AGENT_SEED, memory_size=16) for _ in range(2)]
    agent.sync_fused_weights(); twin.sync_fused_weights()
    _reset_both(env, orc, cfg, cell.form)
    prev = env.obs.clone()                       # the observation the next action is computed from: the oracle has confirmed it
    act = torch.zeros((env.N, 2), device="cuda")
    for launch in range(M.LAUNCHES):
        traj = _traj(env, True)
        env.rollout_policy(agent, M.T_LAUNCH, traj=traj)
        torch.cuda.synchronize()
        for t in range(M.T_LAUNCH):
            twin.act_mfma(prev, out=act, add_noise=True)
            torch.cuda.synchronize()
            assert torch.equal(traj["action"][t], act), "launch %d step %d: the action is not the actor's on the previous observation" % (launch, t)
            want = M.oracle_step(orc, traj["action"][t].cpu().numpy(), "next")
            d = M.first_output_difference(_host(traj, OUT, t), want, cell.form)
            assert d is None, "launch %d step %d: %s" % (launch, t, d)
            prev = traj["obs"][t]
        _assert_state(env, orc, cfg, "after launch %d" % launch)
    assert agent.noise_state() == twin.noise_state() and agent.noise_state()[1] == M.LAUNCHES * M.T_LAUNCH


def _check_external(cell, cfg, env, monkeypatch):
    """the replay itself is cell.held_by's: it asserts this kernel's name on the golden's handle and holds every recorded call to the
    reference.  Here: the cell's world and the golden's configuration both launch the cell's kernel."""
    import test_gpu_external as X
    from crowdnav import Config
    golden = M.EXTERNAL_GOLDEN[cell.kernel]
    assert cell.held_by == M.EXTERNAL_TEST % golden and X.KERNEL[golden] == cell.kernel
    assert hasattr(X, cell.held_by.split("::")[1].split("[")[0])
    _, other = _create(cell, monkeypatch, Config(n_envs=1, **X.load_golden(golden)[1]))
    assert other.kernel_name("external") == cell.kernel
    other.close()


@pytest.mark.parametrize("cell", M.CELLS, ids=[c.kernel for c in M.CELLS])
def test_kernel_equals_the_oracle(oracle_mod, monkeypatch, cell):
    cfg, env = _create(cell, monkeypatch)
    assert env.kernel_name(cell.form) == cell.kernel
    if cell.form == "external":
        _check_external(cell, cfg, env, monkeypatch)
        env.close()
        return
    orc = oracle_mod.Oracle(cfg.as_dict())
    {"step": _run_steps, "same": _run_steps, "sequence": _run_sequence, "policy": _run_policy}[cell.form](cell, cfg, env, orc)
    _assert_end_of_run(env, orc, cfg)
    env.close()
