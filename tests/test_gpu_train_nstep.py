"""crowdnav.train --n-step on tiny shapes (4 environments, episodes of at most 9 steps, a ring of 64 rows, batches of 8, 40 launches):
--n-step 1 writes, byte for byte, what the command without the switch writes; member p of an n-step population is the n-step solo run
of seed + p; an n-step run stopped by --state-every and continued by --resume is the run that was never stopped; and the learner
bootstraps with cn_nstep_discount(gamma, W).  progress.txt carries wall-clock times and is not compared.  No tolerance but the last
test's, which is the fused / PyTorch parity test's own."""
import csv
import os

import numpy as np
import pytest
import torch

from learner_handle import lib

pytestmark = pytest.mark.gpu

SEED = 11
SWITCHES = ["--algo", "td3", "--learner", "fused", "--scenario", "training_as_logged", "--waypoint-reward", "0", "--envs", "4", "--updates", "2",
            "--launches", "40", "--max-steps", "9", "--memory", "64", "--batch", "8", "--log-every", "10", "--csv", "--checkpoint-every", "1"]
NETS = ("actor", "actor_t", "q1", "q1_t", "q2", "q2_t")


def _files(run_dir):
    """{relative path: bytes} of everything a run wrote but progress.txt."""
    out = {}
    for base, _, names in os.walk(run_dir):
        for n in names:
            if not n.startswith("progress"):
                with open(os.path.join(base, n), "rb") as f:
                    out[os.path.relpath(os.path.join(base, n), run_dir)] = f.read()
    return out


def _state_files(d):
    """A state directory's arrays: {file/key: (dtype, shape, bytes)}."""
    out = {}
    for n in sorted(os.listdir(d)):
        if n.endswith(".npy"):
            x = np.load(os.path.join(d, n))
            out[n] = (str(x.dtype), x.shape, x.tobytes())
            continue
        with np.load(os.path.join(d, n)) as z:
            for k in z.files:
                out[n + "/" + k] = (str(z[k].dtype), z[k].shape, z[k].tobytes())
    return out


@pytest.mark.parametrize("population", ([], ["--population", "2"]), ids=("solo", "population"))
def test_n_step_one_is_the_run_without_the_switch(tmp_path, population):
    from crowdnav import train
    base = SWITCHES + population + ["--seed", str(SEED)]
    train.main(base + ["--out", str(tmp_path / "plain")])
    train.main(base + ["--n-step", "1", "--out", str(tmp_path / "one")])
    torch.cuda.synchronize()
    plain, one = _files(tmp_path / "plain"), _files(tmp_path / "one")
    assert sorted(plain) == sorted(one) and any(k.endswith("td3_training.csv") for k in plain) and any(k.endswith(".pt") for k in plain)
    for k in plain:
        assert plain[k] == one[k], k


def test_member_p_of_an_n_step_population_is_the_n_step_solo_run_of_seed_plus_p(tmp_path):
    from crowdnav import train
    nstep = SWITCHES + ["--n-step", "3"]
    agents, episodes = train.train_population(train.parse_args(nstep + ["--population", "2", "--seed", str(SEED), "--out", str(tmp_path / "pop")]))
    torch.cuda.synchronize()
    plain, _ = train.train(train.parse_args(SWITCHES + ["--seed", str(SEED), "--out", str(tmp_path / "plain")]))
    for p in range(2):
        out = tmp_path / ("solo%d" % p)
        solo, solo_eps = train.train(train.parse_args(nstep + ["--seed", str(SEED + p), "--out", str(out)]))
        torch.cuda.synchronize()
        assert solo.n_step == agents[p].n_step == 3 and len(solo.memory) > 8       # updates started within the run
        for net in NETS:
            for x, y in zip(getattr(agents[p], net).parameters(), getattr(solo, net).parameters()):
                assert torch.equal(x, y), (p, net, float((x - y).abs().max()))
        for k in ("s", "s2", "a", "r", "d", "pos_dev", "size_dev"):
            assert torch.equal(getattr(agents[p].memory, k), getattr(solo.memory, k)), (p, k)
        mdir = tmp_path / "pop" / ("member%d" % p)
        got, want = list(csv.reader(open(mdir / "td3_training.csv"))), list(csv.reader(open(out / "td3_training.csv")))
        assert len(want) > 1 and got == want and episodes[p] == solo_eps == len(want) - 1
    # ... and the window is in the ring: rows of both kinds, returns that are sums (the one-step run of the same seed learned otherwise)
    d = solo.memory.d[:int(solo.memory.size_dev)]
    assert (d == 0).any() and (d == 1).any()
    assert any(not torch.equal(x, y) for x, y in zip(plain.q1.parameters(), agents[0].q1.parameters()))


@pytest.mark.parametrize("population", ([], ["--population", "2"]), ids=("solo", "population"))
def test_an_n_step_run_resumed_is_the_uninterrupted_run(tmp_path, population):
    """Stopped at launch 15 of 40, in the middle of the episodes (they last 9 steps and a reset launch): windows are open at the stop and
    the pending store travels in the state.  Both runs write their last state at launch 30.  A run checkpoints when it ends: the stopped
    run's last checkpoint carries the episode count of launch 15, which no launch has changed since the checkpoint of launch 10, and
    replaces that one; those files are the only ones left out.  (tests/test_gpu_train_resume.py stops where the label is a new one.)"""
    import re
    from crowdnav import train
    base = SWITCHES + population + ["--n-step", "3", "--seed", str(SEED), "--state-every", "15"]
    whole, resumed = str(tmp_path / "whole"), str(tmp_path / "resumed")
    train.main(base + ["--out", whole])
    train.main([x if x != "40" else "15" for x in base] + ["--out", resumed])
    with np.load(os.path.join(resumed, "state", "launch15", "loop.npz")) as z:
        pending = [k for k in z.files if "record_pending" in k]
        assert len(pending) == 5 * (2 if population else 1) and any(z[k].any() for k in pending if k.endswith("count"))
        assert any("resetting" in k for k in z.files)
    label = lambda k: re.search(r"_ep(\d+)\.(pt|txt)$", k)
    last = {}                                                          # directory -> the stopped run's last checkpoint label
    for k in _files(resumed):
        if label(k):
            last[os.path.dirname(k)] = max(last.get(os.path.dirname(k), 0), int(label(k).group(1)))
    train.main(base + ["--out", resumed, "--resume", resumed])
    torch.cuda.synchronize()
    a, b = _files(whole), _files(resumed)
    a = {k: v for k, v in a.items() if not (label(k) and int(label(k).group(1)) == last[os.path.dirname(k)])}
    assert sum(1 for k in a if label(k)) >= 3 * 3                      # later checkpoints are compared
    csvs = [k for k in a if k.endswith("td3_training.csv")]
    assert csvs and all(len(a[k].splitlines()) > 1 for k in csvs)
    for k in a:
        if not k.startswith("state"):
            assert b[k] == a[k], k                                     # CSVs, every checkpoint file, run.json
    sa, sb = _state_files(os.path.join(whole, "state", "launch30")), _state_files(os.path.join(resumed, "state", "launch30"))
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert sa[k] == sb[k], k


def test_the_learner_bootstraps_with_the_recorders_discount():
    """fused_config() carries cn_nstep_discount(0.99, 3); one explicit-batch update through cn_td3_update against the PyTorch _update
    of a twin, with the bound tests/test_gpu_configs.py holds that pair to at this shape (46 -> 32, batch 16) after one update; and the
    PyTorch update's loss is the one-step formula with that discount, not with gamma."""
    from crowdnav.td3 import Agent
    _, L = lib()
    obs_dim, hidden, B = 46, 32, 16
    mk = lambda **kw: Agent(obs_dim=obs_dim, hidden=hidden, batch_size=B, seed=3, memory_size=4 * B, device="cuda", **kw)
    a, b, one = mk(n_step=3), mk(n_step=3), mk()
    g3 = L.cn_nstep_discount(0.99, 3)
    assert np.float32(a.fused_config().gamma) == np.float32(g3) != np.float32(0.99) and a.gamma == 0.99
    assert np.float32(one.fused_config().gamma) == np.float32(0.99)
    a.enable_fused_update()
    g = torch.Generator(device="cuda").manual_seed(17)
    batch = (torch.randn((B, obs_dim), generator=g, device="cuda") * 0.5,
             torch.rand((B, 2), generator=g, device="cuda") * torch.tensor([0.22, 4.0], device="cuda") - torch.tensor([0.0, 2.0], device="cuda"),
             torch.randn((B, 1), generator=g, device="cuda") * 3.0, torch.randn((B, obs_dim), generator=g, device="cuda") * 0.5,
             (torch.rand((B, 1), generator=g, device="cuda") < 0.2).float())
    noise = torch.randn((B, 2), generator=g, device="cuda")
    s, act, r, s2, d = batch
    with torch.no_grad():
        a2 = b.actor_t(s2) + (noise * b.noise_std).clamp(-b.noise_clip, b.noise_clip)
        q_t = torch.min(b.q1_t(s2, a2), b.q2_t(s2, a2))
        want = {k: torch.nn.functional.mse_loss(b.q1(s, act), r + (1.0 - d) * k * q_t) for k in (g3, 0.99)}
    a.learn(0, batch=batch, target_noise=noise)
    lb = b.learn(0, batch=batch, target_noise=noise)
    torch.cuda.synchronize()
    # the same float32 operations in the same order: a few units in the last place at most (2^-20 relative), against a discount that is
    # 2 % away
    near, far = abs(float(lb) - float(want[g3])), abs(float(lb) - float(want[0.99]))
    assert near <= 2.0 ** -20 * abs(float(lb)) and far > 8 * max(near, 2.0 ** -20 * abs(float(lb))), (float(lb), near, far)
    for ma, mb in zip([getattr(a, n) for n in NETS], [getattr(b, n) for n in NETS]):
        for (n_, pa), pb in zip(ma.named_parameters(), mb.parameters()):
            diff = (pa - pb).abs()
            bad = diff > (2e-6 + 2e-4 * pb.abs())
            assert int(bad.sum()) <= max(2, pa.numel() // 2000), (n_, int(bad.sum()), float(diff.max()))
            assert float(diff.detach().max()) <= 2.5 * 3e-4, (n_, float(diff.detach().max()))
