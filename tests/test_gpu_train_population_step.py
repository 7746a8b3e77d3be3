"""crowdnav.train --population-step per-member | one-launch, and DeviceEvaluator(step="multi" | "group"): the members' (the jobs')
environments stepped by one kernel per handle between two rounds of stream waits (cn_step_multi), against ONE launch on the loop's
stream (cn_step_group_step).  The same run: byte-equal member CSVs, checkpoints and final state directories; equal evaluation logs and
summaries.  No tolerance."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_train_resume import checkpoint_files, read, same_state

pytestmark = pytest.mark.gpu

COMMON = ["--algo", "td3", "--learner", "fused", "--scenario", "training_as_logged", "--waypoint-reward", "0", "--population", "2", "--envs", "4",
          "--updates", "1", "--memory", "256", "--batch", "16", "--max-steps", "9", "--log-every", "10", "--checkpoint-every", "1", "--csv",
          "--seed", "5"]
CSVS = ["member%d/td3_training.csv" % p for p in range(2)]


def counted(monkeypatch):
    """How often each stepping path was bound and each stream wait entered."""
    from crowdnav import env as E
    calls = {"bind_step_group": 0, "bind_step_all": 0, "fork": 0, "join": 0}
    for name in calls:
        orig = getattr(E.MemberEnvs, name)

        def wrapped(self, *a, _orig=orig, _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(E.MemberEnvs, name, wrapped)
    return calls


@pytest.mark.parametrize("record, launches", [("one-call", 60), ("per-member", 30)])
def test_the_two_population_step_paths_give_the_same_run(record, launches, tmp_path, monkeypatch):
    from crowdnav import train
    calls = counted(monkeypatch)
    seen = {}
    for mode in ("per-member", "one-launch"):
        before = dict(calls)
        train.main(COMMON + ["--population-record", record, "--population-step", mode, "--launches", str(launches),
                             "--state-every", str(launches), "--out", str(tmp_path / mode)])
        torch.cuda.synchronize()
        seen[mode] = {k: calls[k] - before[k] for k in calls}
    per, one = str(tmp_path / "per-member"), str(tmp_path / "one-launch")
    # each run took its own path; with the one-call recorder the one-launch run has no stream wait at all
    assert seen["per-member"]["bind_step_all"] == 1 and seen["per-member"]["bind_step_group"] == 0
    assert seen["one-launch"]["bind_step_group"] == 1 and seen["one-launch"]["bind_step_all"] == 0
    assert seen["per-member"]["fork"] >= launches and seen["per-member"]["join"] >= launches
    if record == "one-call":
        assert seen["one-launch"]["fork"] == 0 and seen["one-launch"]["join"] == 0
    for rel in CSVS:
        assert read(os.path.join(per, rel)) == read(os.path.join(one, rel)), rel
        assert len(read(os.path.join(per, rel)).splitlines()) > 1, rel
    want, got = checkpoint_files(per), checkpoint_files(one)
    assert want and set(want) == set(got)
    for rel, b in want.items():
        assert got[rel] == b, rel
    same_state(os.path.join(per, "state", "launch%d" % launches), os.path.join(one, "state", "launch%d" % launches))
    assert json.load(open(os.path.join(per, "run.json")))["population_step"] == "per-member"
    assert json.load(open(os.path.join(one, "run.json")))["population_step"] == "one-launch"


def test_device_evaluator_group_equals_multi():
    """J = 4 jobs (two actors x two seeds) of 4 environments in crossing_8, quota 1."""
    from crowdnav import train
    from crowdnav.rollout import DeviceEvaluator
    from crowdnav.td3 import Agent
    specs = [train.scenario_config("crossing_8", 4, 30, 40 + w) for w in range(2)]
    agents = [Agent(obs_dim=specs[0][0].obs_dim, device="cuda:0", seed=3 + p, memory_size=16) for p in range(2)]
    jobs = [(cfg, init, vel, ag, p) for p, ag in enumerate(agents) for (cfg, init, vel) in specs]
    out = {}
    for step in ("multi", "group"):
        ev = DeviceEvaluator(jobs, 0, step=step)
        launches = ev.run(1, poll=0)
        fitness = ev.finish("return").clone()
        torch.cuda.synchronize()
        out[step] = (launches, fitness.cpu(), ev.summary(), [lg.rows[:int(lg.n.item())].cpu() for lg in ev.logs], ev.remaining(),
                     [e.snapshot() for e in ev.envs.envs])
        ev.close()
    m, g = out["multi"], out["group"]
    assert m[0] == g[0] and torch.equal(m[1], g[1]) and torch.equal(m[4], g[4])
    assert m[2].shape == (4, 8) and np.array_equal(m[2].numpy(), g[2].numpy(), equal_nan=True)       # (a score with no sample is nan)
    assert int(m[4].sum()) == 0 and all(len(r) == 4 for r in m[3])          # every environment's first episode was counted
    for j, (x, y) in enumerate(zip(m[3], g[3])):
        assert torch.equal(x, y), j
    for j, (x, y) in enumerate(zip(m[5], g[5])):
        assert (x == y).all(), j
    with pytest.raises(ValueError, match="step must be"):
        DeviceEvaluator(jobs, 0, step="fused")


def test_an_evaluation_over_worlds_of_different_kernels_is_refused_with_the_librarys_message():
    from crowdnav import Config, _abi
    from crowdnav.rollout import DeviceEvaluator
    from crowdnav.td3 import Agent
    cfgs = [Config(n_envs=2, max_steps=6, seed=1), Config(n_envs=2, max_steps=6, seed=1, risk_mode=1)]
    agent = Agent(obs_dim=cfgs[0].obs_dim, device="cuda:0", seed=3, memory_size=16)
    jobs = [(c, None, None, agent, 0) for c in cfgs]
    with pytest.raises(_abi.CrowdNavError, match="job 1: its group kernel is cn_env_kernel_gt_grp"):
        DeviceEvaluator(jobs, 0, step="group")
    DeviceEvaluator(jobs, 0, step="multi").close()                           # cn_step_multi takes any mix
