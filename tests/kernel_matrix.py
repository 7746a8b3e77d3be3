"""The kernel matrix: every kernel of csrc/crowdnav_variants.h (the 68 names of tests/kernel_table_ref.py::UNIT) in ONE cell that
names it, forces its selection whatever the device's CU count, and says how it is driven; and the comparers that hold a cell's
outputs and state records to the CPU oracle, bit for bit.  No tests here: tests/test_kernel_matrix.py checks the cells, the
selection, the premise and the comparers without a GPU; tests/test_gpu_kernel_matrix.py runs one case per cell.

A cell is (kernel, world, form, forcing[, held_by]):
  world    a row of kernel_table_ref.WORLDS; its configuration is test_gpu_kernel_table.CONFIGS[world] on top of COMMON
  form     step | same | external | sequence | policy -- what VecEnv.kernel_name(form) is asked and how the handle is driven
  forcing  (env, arbitration): the environment variables present while the handle is created (cn_create reads CN_X2 and CN_WPB once;
           a variable that is not named is absent) and VecEnv's arbitration argument.  Every forcing is explicit: with CN_X2 and CN_WPB
           pinned, nothing in cn_select_kernel depends on the CU count at 22 environments.
  held_by  external cells only: the existing test that replays a golden of that layout through cn_observe_external and asserts
           exactly this kernel's name (tests/test_gpu_external.py); the cell points at it instead of running the replay twice.

Every cell runs N_ENVS = 22 environments: a partial last workgroup for the four-environments-per-workgroup kernels (5 full, then
2), for the 16-per-workgroup policy kernels (1 full, then 6) and for the 8-per-workgroup ones (2 full, then 6).  max_steps = 9 ends an
episode every 10 calls at the latest, so 40 steps cross four resets per environment under both reset conventions; the premise -- the
oracle alone ends episodes in every environment and never outgrows its own tables, so it stays the reference for the whole run -- is
checked on the CPU."""
import os
import sys
from collections import namedtuple

import numpy as np

import kernel_table_ref as T
from conftest import ROOT
from test_gpu_kernel_table import CONFIGS

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bisect_divergence import first_env_state_difference  # noqa: E402

COMMON = dict(n_envs=22, max_steps=9, seed=61, ped_cycle_ms=1400)
N_ENVS, STEPS = COMMON["n_envs"], 40
LAUNCHES, T_LAUNCH, HELD_LAUNCH = 5, 8, 2          # sequence / policy: 5 launches of 8 steps; the third holds one action (stride 0)
ACTION_SEED, AGENT_SEED = 61, 6
FORMS = ("step", "same", "external", "sequence", "policy")
ARBITRATION = {"auto": T.ARB_AUTO, "oldest_first": T.ARB_OLDEST_FIRST, "fair": T.ARB_FAIR}
ST_TRACK_OVERFLOW, ST_CONF_OVERFLOW = 1, 8        # include/crowdnav.h CN_ST_*
SI_STATUS, SI_EPISODES = 9, 15                     # include/crowdnav.h CN_SI_*

Forcing = namedtuple("Forcing", "env arbitration")
Cell = namedtuple("Cell", "kernel world form forcing held_by", defaults=(None,))

E = T.E
PLAIN = Forcing({}, "oldest_first")
# the step kernels of the three plain tracker worlds: the forcing of each
HEADLINE = {
    E + "_s360_x2":      ("s360", Forcing({"CN_X2": "1"}, "oldest_first")),
    E + "_s360_w4":      ("s360", Forcing({"CN_X2": "0", "CN_WPB": "4"}, "oldest_first")),
    E + "_fair_s360_w4": ("s360", Forcing({"CN_X2": "0", "CN_WPB": "4"}, "fair")),
    E + "_s360":         ("s360", Forcing({"CN_X2": "0", "CN_WPB": "0"}, "oldest_first")),
    E + "_fair_s360":    ("s360", Forcing({"CN_X2": "0", "CN_WPB": "0"}, "fair")),
    E:                   ("generic", PLAIN),
    E + "_fair":         ("generic", Forcing({}, "fair")),
    E + "_s720":         ("s720", PLAIN),
    E + "_fair_s720":    ("s720", Forcing({}, "fair")),
}
# a kernel several worlds launch (USE rows of CN_WORLDS) runs under the world whose row defines it
OWNER = {E + "_same": "generic", E + "_ext": "generic"}
# external: kernel -> (golden, the test that replays it and asserts the kernel's name).  The smallest golden of each layout
# that tests/test_external_worlds_helpers.py::PHASE_GOLDENS has.
EXTERNAL_TEST = "tests/test_gpu_external.py::test_pre_get_state_reward_one_by_one_equal_the_whole_flow[%s]"
EXTERNAL_GOLDEN = {E + "_ext": "timeout", E + "_orig_ext": "orig20", E + "_rw_ext": "rw_goal", E + "_wide_ext": "wide_tracks"}


def _cells():
    cells = [Cell(k, w, "step", f) for k, (w, f) in HEADLINE.items()]
    cells += [Cell(row[1], w, "step", PLAIN) for w, row in T.WORLDS.items() if w not in T.PLAIN_TRACKER]
    for col, form in ((2, "same"), (3, "external"), (4, "sequence"), (5, "policy")):
        for w, row in T.WORLDS.items():
            k = row[col]
            if k is None or OWNER.get(k, w) != w:
                continue
            held = EXTERNAL_TEST % EXTERNAL_GOLDEN[k] if form == "external" else None
            cells.append(Cell(k, w, form, PLAIN, held))
    return cells


CELLS = _cells()


def config_kw(world):
    """Config keywords of a cell's world"""
    return dict(COMMON, **CONFIGS[world])


def launch_facts(forcing):
    """(arbitration, x2, wpb) of kernel_table_ref.want_step / CnLaunchFacts for a forcing, as cn_create reads the variables:
    CN_X2 unset -1, else 0 / 1; CN_WPB unset 4, else its value if that is 2, 4, 8 or 16 and 0 otherwise"""
    x2 = -1 if "CN_X2" not in forcing.env else (1 if int(forcing.env["CN_X2"]) else 0)
    wpb = 4 if "CN_WPB" not in forcing.env else int(forcing.env["CN_WPB"])
    return ARBITRATION[forcing.arbitration], x2, wpb if wpb in (2, 4, 8, 16) else 0


def actions(steps=STEPS, n=N_ENVS, seed=ACTION_SEED):
    """[steps, n, 2] float32 (v, w): the seeded actions of every cell that is not a policy cell"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, 0.22, (steps, n)), rng.uniform(-2, 2, (steps, n))], 2).astype(np.float32)


def sequence_actions():
    """[LAUNCHES, T_LAUNCH, N, 2] float32; launch HELD_LAUNCH holds its first action for all its steps"""
    a = actions(LAUNCHES * T_LAUNCH).reshape(LAUNCHES, T_LAUNCH, N_ENVS, 2).copy()
    a[HELD_LAUNCH] = a[HELD_LAUNCH, :1]
    return a


def oracle_step(orc, act, mode):
    """One oracle step as the dict the comparers take: float64 obs / reward / final, done, topk_idx"""
    oc, rc, dc, ic, fc = orc.step(np.asarray(act, dtype=np.float64), auto_reset=mode, want_final=True)
    return dict(obs=oc, reward=rc, done=dc, topk_idx=ic, final=fc)


# ---- comparers: plain functions of "got" arrays (host copies of what a launch wrote) and oracle arrays ----------------------------------
# what a form writes besides done, topk_idx, reward and the float32 observation
FORM_WRITES = {"step": ("obs_f64",), "same": ("obs_f64", "final_obs"), "sequence": (), "policy": ()}


def _first(name, g, w):
    g, w = np.asarray(g), np.asarray(w)
    if g.shape != w.shape or g.dtype != w.dtype:
        return "%s: got %s %s, want %s %s" % (name, g.dtype, g.shape, w.dtype, w.shape)
    bad = np.argwhere(g != w)                         # np.array_equal's rule, as in tests/test_gpu_parity.py: a NaN equals nothing
    if bad.size:
        i = tuple(int(x) for x in bad[0])
        return "%s%s: got %r, oracle %r (%d elements differ)" % (name, list(i), g[i].item(), w[i].item(), len(bad))
    return None


def first_output_difference(got, want, form):
    """got: done [N] uint8, topk_idx [N, K] int32, reward [N] float32, obs [N, D] float32, and what FORM_WRITES[form] names (obs_f64
    float64, final_obs float32) -- a missing one is a KeyError, never a skipped comparison.  want: oracle_step().  Equality; the
    float32 outputs are the oracle's float64 values cast to float32.  Returns None or a description of the first difference."""
    checks = [("done", got["done"], want["done"]), ("topk_idx", got["topk_idx"], want["topk_idx"]),
              ("reward", got["reward"], want["reward"].astype(np.float32)), ("obs", got["obs"], want["obs"].astype(np.float32))]
    if "obs_f64" in FORM_WRITES[form]:
        checks.append(("obs_f64", got["obs_f64"], want["obs"]))
    if "final_obs" in FORM_WRITES[form]:
        checks.append(("final_obs", got["final_obs"], want["final"].astype(np.float32)))
    for name, g, w in checks:
        d = _first(name, g, w)
        if d:
            return d
    return None


def first_reset_difference(got, obs, form):
    """the reset launch: float32 observation, and float64 where the form's handle has one, against the oracle's reset()"""
    d = _first("obs", got["obs"], obs.astype(np.float32))
    if d is None and "obs_f64" in FORM_WRITES[form]:
        d = _first("obs_f64", got["obs_f64"], obs)
    return d


def first_state_record_difference(snapshot, orc, risk_mode):
    """the whole state record of every environment (a cn_snapshot blob) against the oracle stepped alongside:
    tools/bisect_divergence.py::first_env_state_difference, the one rule of the parity tests.  None or a description."""
    d = first_env_state_difference(snapshot, orc, risk_mode=risk_mode)
    return None if d is None else "state of env %d, %s: got %r, oracle %r" % d


def first_final_difference(counters, last_returns, orc):
    """end of run: counters[:, :6] int32 and the last finished episodes' returns float32"""
    return (_first("counters", np.asarray(counters)[:, :6], orc.counters()) or
            _first("last_return", last_returns, orc.returns().astype(np.float32)))


def oracle_episodes_and_status(orc):
    """(episodes finished [N], status word [N]) of an oracle"""
    si = np.stack([orc.get_state(e)["si"] for e in range(orc.N)])
    return si[:, SI_EPISODES], si[:, SI_STATUS]
