"""crowdnav.train --population with --pbt-every: the run completes, <out>/pbt_log.csv carries a row for every member of every applied
exploit call, every row agrees with the NumPy restatement (tests/pbt_ref.py) fed the logged fitness, the members' checkpoints load, and a
run with --pbt-every 0 writes no such file (what that run computes: tests/test_gpu_train_population.py)."""
import argparse
import csv
import os

import numpy as np
import pytest
import torch

import pbt_ref as R

pytestmark = pytest.mark.gpu

P, SEED, EVERY = 4, 23, 10
SWITCHES = ["--algo", "td3", "--learner", "fused", "--scenario", "training_as_logged", "--waypoint-reward", "0", "--envs", "4", "--updates", "2",
            "--launches", "40", "--max-steps", "9", "--memory", "64", "--batch", "8", "--log-every", "15", "--csv", "--population", str(P),
            "--seed", str(SEED)]


def test_a_pbt_run_logs_what_the_statement_says_and_its_checkpoints_load(tmp_path):
    from crowdnav import td3, train
    out = tmp_path / "pbt"
    a = train.parse_args(SWITCHES + ["--pbt-every", str(EVERY), "--pbt-min-episodes", "1", "--pbt-spread", "2", "--out", str(out)])
    assert a.pbt_n_replace == 1
    agents, episodes = train.train_population(a)
    torch.cuda.synchronize()
    rows = list(csv.reader(open(out / "pbt_log.csv")))
    assert tuple(rows[0]) == train.PBT_CSV_COLUMNS
    calls = {}
    for r in rows[1:]:
        calls.setdefault((int(r[0]), int(r[1])), []).append(r)
    order = sorted(calls)
    assert len(order) >= 2 and all(launch % EVERY == 0 and 0 <= call < launch // EVERY for launch, call in order)
    assert [c for _, c in order] == sorted({c for _, c in order})             # one applied call per logged launch, in order
    lo, hi = zip(*[td3.Population.PBT_BOUNDS[n] for n in R.HYPERS])
    cfg = R.make_config(1, min_episodes=1, explore=("lr_actor", "lr_critic", "noise_std"), factor=(0.8, 1.2), lo=lo, hi=hi, seed=SEED)
    generation = [0] * P
    hyper = None
    for (launch, call), group in sorted(calls.items()):
        assert [int(r[2]) for r in group] == list(range(P))                # a row for every member
        fitness = np.array([float(r[5]) for r in group], np.float32)
        now = np.array([[float(x) for x in r[6:]] for r in group], np.float32)
        assert np.isfinite(fitness).all()
        (dst, src), = R.plan(fitness, 1, SEED, call)
        generation[dst] += 1
        assert [int(r[3]) for r in group] == [src if p == dst else p for p in range(P)], (launch, call)
        assert [int(r[4]) for r in group] == generation
        assert now[dst].tolist() == R.explore(now[src], dst, cfg, call).tolist()
        if hyper is not None:
            for p in range(P):
                assert p == dst or now[p].tolist() == hyper[p].tolist()    # a survivor keeps its values
        hyper = now
    spread = np.array([train.pbt_spread_factors(SEED, p, 2.0) for p in range(P)])
    assert len({tuple(r) for r in spread.tolist()}) == P
    # the Python side shows what the device trains with, and the checkpoints are the members' target networks
    for p, ag in enumerate(agents):
        want = hyper[p].tolist()
        got = [ag.opt_a.param_groups[0]["lr"], ag.opt_q1.param_groups[0]["lr"], ag.gamma, ag.noise_std, ag.noise_clip]
        assert np.asarray(got, np.float32).tolist() == want, p
        mdir = out / ("member%d" % p)
        fresh = td3.Agent(obs_dim=ag.actor.linear1.in_features, memory_size=16, device="cuda:0", seed=99)
        train.load_checkpoint(fresh, argparse.Namespace(load=str(mdir), load_episode="latest", algo="td3"))
        for x, y in zip(fresh.actor.parameters(), ag.actor_t.parameters()):
            assert torch.equal(x, y), p
        assert episodes[p] > 0 and os.path.exists(mdir / "td3_training.csv")


def test_pbt_every_zero_writes_no_pbt_log(tmp_path):
    from crowdnav import train
    out = tmp_path / "off"
    train.train_population(train.parse_args(SWITCHES + ["--pbt-every", "0", "--launches", "12", "--out", str(out)]))
    torch.cuda.synchronize()
    assert os.path.isdir(out / "member0") and not os.path.exists(out / "pbt_log.csv")
