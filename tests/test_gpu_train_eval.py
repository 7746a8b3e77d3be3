"""crowdnav.train with the evaluation on the device: --population with --eval-every writes <out>/eval_log.csv and leaves the training run,
byte for byte, the run without it; --pbt-fitness eval ranks by what eval_log.csv shows; --evaluate --evaluate-on device writes the files
--evaluate-on host writes, with the rows of the per-handle loop on the f32-MFMA actor."""
import csv
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POP = ["--algo", "td3", "--learner", "fused", "--population", "2", "--envs", "8", "--updates", "1", "--launches", "60", "--max-steps", "20",
       "--csv", "--log-every", "20", "--seed", "7"]
EVAL = ["--eval-every", "20", "--eval-envs", "8", "--eval-max-steps", "20"]


def _files(d):
    """{relative path: bytes} of the checkpoints, their bookkeeping and the CSVs below d (not progress.txt: it holds wall-clock rates)."""
    out = {}
    for root, _, names in os.walk(d):
        for n in names:
            if n.endswith((".pt", ".csv", ".txt")) and n != "progress.txt":
                out[os.path.relpath(os.path.join(root, n), d)] = open(os.path.join(root, n), "rb").read()
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from crowdnav import train
    base = tmp_path_factory.mktemp("train_eval")
    for name, extra in (("plain", []), ("eval", EVAL)):
        train.main(POP + extra + ["--out", str(base / name)])
        torch.cuda.synchronize()
    return base


def test_eval_log_has_a_row_per_launch_member_and_world_and_training_is_untouched(runs):
    from crowdnav import train
    rows = list(csv.reader(open(runs / "eval" / "eval_log.csv")))
    assert tuple(rows[0]) == train.EVAL_CSV_COLUMNS and len(train.EVAL_CSV_COLUMNS) == 3 + 8
    worlds = train.parse_args(POP + EVAL).eval_scenarios
    assert len(rows) - 1 == 3 * 2 * len(worlds)
    assert [(int(r[0]), int(r[1]), r[2]) for r in rows[1:]] == [(it, p, w) for it in (20, 40, 60) for p in range(2) for w in worlds]
    for r in rows[1:]:
        v = [float(x) for x in r[3:]]
        assert v[0] == 8 and 0 <= v[1] <= 1 and 0 <= v[2] <= 1 and v[1] + v[2] + v[3] == 1 and 1 <= v[5] <= 20      # 8 envs x 1 episode
    assert not os.path.exists(runs / "plain" / "eval_log.csv")
    plain, ev = _files(runs / "plain"), _files(runs / "eval")
    assert set(ev) == set(plain) | {"eval_log.csv"}
    assert any(k.endswith(".pt") for k in plain) and sum(k.endswith("td3_training.csv") for k in plain) == 2
    for k, v in plain.items():
        assert ev[k] == v, k                                               # checkpoints, noise state and training CSVs: byte for byte


def test_pbt_ranks_by_the_evaluations_fitness(tmp_path):
    from crowdnav import train
    out = tmp_path / "pbt"
    train.main(POP + EVAL + ["--pbt-every", "20", "--pbt-fitness", "eval", "--eval-metric", "return", "--pbt-fraction", "0.5", "--out", str(out)])
    torch.cuda.synchronize()
    ev = list(csv.reader(open(out / "eval_log.csv")))
    col = ev[0].index("mean_return")
    shown = {(int(r[0]), int(r[1])): float(r[col]) for r in ev[1:]}
    assert sorted({k[0] for k in shown}) == [20, 40, 60]                   # one evaluation per launch, shared by the log and the exploit
    pbt = list(csv.reader(open(out / "pbt_log.csv")))
    fit = pbt[0].index("fitness")
    assert len(pbt) > 1 and (len(pbt) - 1) % 2 == 0
    for r in pbt[1:]:
        want, got = shown[(int(r[0]), int(r[2]))], float(r[fit])
        assert got == want or (got != got and want != want), r


def test_evaluate_on_device_writes_what_host_writes_with_the_mfma_loops_rows(runs, tmp_path):
    from crowdnav import train
    from crowdnav.rollout import EpisodeStats
    load = str(runs / "plain" / "member0")
    common = ["--evaluate", "--load", load, "--scenario", "crossing_4", "--envs", "8", "--max-steps", "20", "--episodes-per-env", "2", "--seed", "3"]
    train.main(common + ["--out", str(tmp_path / "host")])
    st = train.main(common + ["--evaluate-on", "device", "--out", str(tmp_path / "device")])
    torch.cuda.synchronize()
    assert sorted(os.listdir(tmp_path / "device")) == sorted(os.listdir(tmp_path / "host")) == ["td3_training_test_crossing_4.csv"]
    # the loop DeviceEvaluator replaces, on the actor it runs
    a = train.fill_defaults(train.parse_args(common))
    env = train.make_env(a.scenario, a.envs, a.max_steps, a.seed, a.device, a.ped_vmax, **train.env_switches(a))
    agent = train.make_agent(a, env.D, "cuda:0", memory_size=16)
    train.load_checkpoint(agent, a)
    env.reset()
    obs, want, finished = env.obs, EpisodeStats(), [0] * 8
    step_s = (env.cfg.dt_ms + env.cfg.scan_latency_ms) / 1000.0
    for _ in range(2 * 21):
        obs, _, done = env.step(agent.act_mfma(obs, add_noise=False), auto_reset="next")
        d = done.cpu().numpy()
        if d.any():
            c, ret = env.counters().cpu(), env.returns()[0].cpu()
            for e in np.nonzero(d)[0].tolist():
                if finished[e] < 2:
                    want.add_from_counters(c[e], ret[e].item(), step_seconds=step_s)
                    finished[e] += 1
    env.close()
    assert finished == [2] * 8 and len(st.rows) == 16
    same = lambda x, y: x == y or (x != x and y != y)
    assert all(same(x, y) for r, s in zip(st.rows, want.rows) for x, y in zip(r, s))
    assert open(tmp_path / "device" / "td3_training_test_crossing_4.csv").read() == open(want.write_csv(str(tmp_path / "loop"), "rows")).read()
    # several worlds in one run: a CSV per world and the summary table
    many = tmp_path / "many"
    train.main(common + ["--evaluate-on", "device", "--eval-scenarios", "crossing_4,towards_4", "--out", str(many)])
    assert sorted(os.listdir(many)) == ["eval_summary.csv", "td3_training_test_crossing_4.csv", "td3_training_test_towards_4.csv"]
    assert open(many / "td3_training_test_crossing_4.csv").read() == open(tmp_path / "device" / "td3_training_test_crossing_4.csv").read()
    table = list(csv.reader(open(many / "eval_summary.csv")))
    assert tuple(table[0]) == ("world",) + train.EVAL_SUMMARY_COLUMNS and [r[0] for r in table[1:]] == ["crossing_4", "towards_4"]
    assert [float(r[1]) for r in table[1:]] == [16.0, 16.0]
    assert float(table[1][2]) == sum(r[1] for r in st.rows) / 16 and float(table[1][6]) == np.float32(sum(r[4] for r in st.rows) / 16)
