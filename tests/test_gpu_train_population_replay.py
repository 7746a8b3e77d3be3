"""crowdnav.train --population-replay shared: the run ends and <out>/run.json names the switch; a run stopped by --state-every and
resumed by fresh processes is, byte for byte, the run that was never stopped (test_gpu_train_resume's comparison and its
child-process pattern); --population-replay own is the run without the switch.  No tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from test_gpu_train_resume import checkpoint_files, read, same_state

pytestmark = pytest.mark.gpu

COMMON = ["--algo", "td3", "--learner", "fused", "--scenario", "training_as_logged", "--waypoint-reward", "0", "--population", "2", "--envs", "4",
          "--updates", "1", "--memory", "256", "--batch", "16", "--max-steps", "9", "--log-every", "10", "--checkpoint-every", "1", "--csv",
          "--seed", "5"]
SHARED = COMMON + ["--population-replay", "shared", "--state-every", "20"]
# --max-steps 9 under --log-every 10: an episode and its reset launch are at most 10 launches, so every member finishes episodes
# between two log lines, and the checkpoint the stopped run writes as its last carries the label the uninterrupted run gives its
# checkpoint of the same launch (with no new episode it would overwrite an older checkpoint of that label with later weights).
FULL, HALF = 40, 20
CSVS = ["member%d/td3_training.csv" % p for p in range(2)]


def same_files(whole, other):
    for rel in CSVS:
        assert read(os.path.join(whole, rel)) == read(os.path.join(other, rel)), rel
        assert len(read(os.path.join(whole, rel)).splitlines()) > 1, rel
    want, got = checkpoint_files(whole), checkpoint_files(other)
    assert want and set(want) <= set(got)          # (a stopped run's own final checkpoint may be one more file)
    for rel, b in want.items():
        assert got[rel] == b, rel


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    """whole: 40 launches in this process; resumed: 20, then --resume to 40 -- a child process each."""
    from crowdnav import train
    root = tmp_path_factory.mktemp("shared")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))

    def run(args):
        r = subprocess.run([sys.executable, "-m", "crowdnav.train"] + SHARED + args, cwd=str(root), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    whole, resumed = str(root / "whole"), str(root / "resumed")
    train.main(SHARED + ["--launches", str(FULL), "--out", whole])
    run(["--launches", str(HALF), "--out", resumed])
    at_stop = sorted(os.listdir(os.path.join(resumed, "state")))
    run(["--launches", str(FULL), "--resume", resumed])               # --out defaults to the run it continues
    return whole, resumed, at_stop


def test_the_shared_run_ends_and_its_json_names_the_switch(shared):
    whole, resumed, _ = shared
    for d in (whole, resumed):
        rec = json.load(open(os.path.join(d, "run.json")))
        assert rec["population_replay"] == "shared" and rec["population"] == 2
    with np.load(os.path.join(whole, "state", "launch%d" % FULL, "loop.npz")) as z:
        assert int(z["s_it"]) == FULL and bool(z["s_learning"]) and int(z["s_updates_done"]) > FULL - HALF      # updates on both sides of the stop


def test_the_resumed_shared_run_is_the_uninterrupted_run(shared):
    whole, resumed, at_stop = shared
    assert at_stop == ["latest", "launch%d" % HALF]
    same_files(whole, resumed)
    assert sorted(os.listdir(os.path.join(whole, "state"))) == sorted(os.listdir(os.path.join(resumed, "state"))) == ["latest", "launch%d" % FULL]
    same_state(os.path.join(whole, "state", "launch%d" % FULL), os.path.join(resumed, "state", "launch%d" % FULL))


def test_own_is_the_run_without_the_switch_and_shared_is_not(shared, tmp_path):
    from crowdnav import train
    plain, own = str(tmp_path / "plain"), str(tmp_path / "own")
    train.main(COMMON + ["--launches", str(FULL), "--out", plain])
    train.main(COMMON + ["--population-replay", "own", "--launches", str(FULL), "--out", own])
    same_files(plain, own)
    assert json.load(open(os.path.join(plain, "run.json")))["population_replay"] == "own"
    assert json.load(open(os.path.join(own, "run.json"))) == json.load(open(os.path.join(plain, "run.json")))
    a, b = checkpoint_files(plain), checkpoint_files(shared[0])
    assert any(a[k] != b[k] for k in set(a) & set(b) if k.endswith(".pt"))      # the shared run learned from other rows
