"""crowdnav.train --state-every / --resume: a run stopped at its midpoint and continued by fresh objects is, byte for byte, the run
that was never stopped -- the episode CSVs, every checkpoint file, pbt_log.csv, and the whole final state (learner blob, replays,
environment snapshots, the loop's tensors and counts).  progress.txt and the printed lines carry wall-clock times and are not
compared.  The solo case stops and resumes `python -m crowdnav.train` as child processes; the population runs in this process.  No
tolerance."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

COMMON = ["--algo", "td3", "--learner", "fused", "--scenario", "training_as_logged", "--waypoint-reward", "0", "--envs", "16", "--updates", "4",
          "--max-steps", "20", "--log-every", "20", "--checkpoint-every", "1", "--csv", "--seed", "5", "--state-every", "60"]
SOLO = COMMON + ["--memory", "4096"]
POPULATION = COMMON + ["--population", "3", "--memory", "512", "--pbt-every", "20", "--pbt-spread", "3", "--pbt-min-episodes", "1"]
FULL, HALF = 120, 60


def read(path):
    with open(path, "rb") as f:
        return f.read()


def checkpoint_files(run_dir):
    """{relative path: bytes} of every checkpoint file below run_dir: the networks, the noise positions, the latest pointers."""
    out = {}
    for base, _, names in os.walk(run_dir):
        if os.sep + "state" in base[len(str(run_dir)):]:
            continue
        for n in names:
            if n.endswith(".pt") or n.startswith("noise_state_ep") or n == "latest_checkpoint.txt":
                out[os.path.relpath(os.path.join(base, n), run_dir)] = read(os.path.join(base, n))
    return out


def labels(run_dir):
    """{directory: (sorted checkpoint labels, the latest pointer's label)}"""
    out = {}
    for rel in checkpoint_files(run_dir):
        d, n = os.path.split(rel)
        if n.startswith("td3_actor_model_ep"):
            out.setdefault(d, []).append(int(n[len("td3_actor_model_ep"):-3]))
    return {d: (sorted(v), int(read(os.path.join(run_dir, d, "latest_checkpoint.txt")).split()[0])) for d, v in out.items()}


def same_state(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "loop.npz" in names and "env0.npy" in names
    for n in names:
        if n.endswith(".npy"):
            x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), n
            continue
        with np.load(os.path.join(a, n)) as x, np.load(os.path.join(b, n)) as y:
            assert sorted(x.files) == sorted(y.files), n
            for k in x.files:
                assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), (n, k)


def same_run(whole, resumed, csvs):
    for rel in csvs:
        assert read(os.path.join(whole, rel)) == read(os.path.join(resumed, rel)), rel
    want, got = checkpoint_files(whole), checkpoint_files(resumed)
    assert want and set(want) <= set(got)          # (the stopped run's own final checkpoint may be one more file)
    for rel, b in want.items():
        assert got[rel] == b, rel
    assert sorted(os.listdir(os.path.join(whole, "state"))) == sorted(os.listdir(os.path.join(resumed, "state"))) == ["latest", "launch%d" % FULL]
    same_state(os.path.join(whole, "state", "launch%d" % FULL), os.path.join(resumed, "state", "launch%d" % FULL))


def labels_only_grow(before, after):
    assert before and set(before) <= set(after)
    for d, (old, latest) in before.items():
        new, latest_now = after[d]
        assert set(old) <= set(new) and latest_now >= latest and latest_now == max(new) and all(x >= latest for x in set(new) - set(old)), d


@pytest.fixture(scope="module")
def solo(tmp_path_factory):
    """whole: 120 launches, in this process; resumed: 60, then --resume to 120 -- a child process each, as a run that did not survive
    its process is continued."""
    from crowdnav import train
    root = tmp_path_factory.mktemp("solo")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))

    def run(args):
        r = subprocess.run([sys.executable, "-m", "crowdnav.train"] + SOLO + args, cwd=str(root), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    whole, resumed = str(root / "whole"), str(root / "resumed")
    train.main(SOLO + ["--launches", str(FULL), "--out", whole])
    run(["--launches", str(HALF), "--out", resumed])
    at_stop = dict(labels=labels(resumed), state=sorted(os.listdir(os.path.join(resumed, "state"))), rows=len(read(os.path.join(resumed, "td3_training.csv")).splitlines()))
    run(["--launches", str(FULL), "--resume", resumed])               # --out defaults to the run it continues
    return whole, resumed, at_stop


def test_solo_resumed_run_is_the_uninterrupted_run(solo):
    whole, resumed, at_stop = solo
    assert at_stop["state"] == ["latest", "launch%d" % HALF] and at_stop["rows"] > 1
    same_run(whole, resumed, ["td3_training.csv"])
    rows = list(csv.reader(open(os.path.join(resumed, "td3_training.csv"))))
    assert len(rows) > at_stop["rows"] and [int(r[0]) for r in rows[1:]] == list(range(1, len(rows)))      # appended, numbered on
    with np.load(os.path.join(resumed, "state", "launch%d" % FULL, "agent.npz")) as z:
        assert 0 < int(z["replay_size"]) < 4096 and int(z["replay_size"]) == int(z["replay_pos"])          # the ring has not wrapped
    with np.load(os.path.join(resumed, "state", "launch%d" % FULL, "loop.npz")) as z:
        assert int(z["s_it"]) == FULL and int(z["s_updates_done"]) > 4 * HALF and bool(z["s_learning"])


def test_solo_checkpoint_labels_only_grow(solo):
    whole, resumed, at_stop = solo
    labels_only_grow(at_stop["labels"], labels(resumed))


@pytest.fixture(scope="module")
def population(tmp_path_factory):
    from crowdnav import train
    root = tmp_path_factory.mktemp("population")
    whole, resumed = str(root / "whole"), str(root / "resumed")
    train.main(POPULATION + ["--launches", str(FULL), "--out", whole])
    train.main(POPULATION + ["--launches", str(HALF), "--out", resumed])
    at_stop = dict(labels=labels(resumed), pbt=read(os.path.join(resumed, "pbt_log.csv")))
    with np.load(os.path.join(resumed, "state", "launch%d" % HALF, "member0.npz")) as z:
        at_stop["ring"] = (int(z["replay_size"]), int(z["replay_pos"]))
    train.main(POPULATION + ["--launches", str(FULL), "--out", resumed, "--resume", resumed])
    return whole, resumed, at_stop


def test_population_resumed_run_is_the_uninterrupted_run(population):
    whole, resumed, at_stop = population
    csvs = ["member%d/td3_training.csv" % p for p in range(3)]
    same_run(whole, resumed, csvs + ["pbt_log.csv"])
    # not vacuous: exploits were applied on each side of the stop, every member finished episodes, the ring had wrapped at the stop
    rows = list(csv.reader(open(os.path.join(resumed, "pbt_log.csv"))))[1:]
    launches = sorted({int(r[0]) for r in rows})
    assert any(x <= HALF for x in launches) and any(x > HALF for x in launches), launches
    assert read(os.path.join(resumed, "pbt_log.csv")).startswith(at_stop["pbt"]) and len(at_stop["pbt"].splitlines()) > 1
    assert any(int(r[4]) > 0 for r in rows)                           # a member was replaced
    for rel in csvs:
        assert len(read(os.path.join(resumed, rel)).splitlines()) > 1, rel
    size, pos = at_stop["ring"]
    assert size == 512 and pos < 512 and 16 * HALF > 512
    with np.load(os.path.join(resumed, "state", "launch%d" % FULL, "loop.npz")) as z:
        assert int(z["s_pbt_applied"]) >= 2 and int(z["s_it"]) == FULL


def test_population_checkpoint_labels_only_grow(population):
    whole, resumed, at_stop = population
    labels_only_grow(at_stop["labels"], labels(resumed))
