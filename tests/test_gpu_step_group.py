"""cn_step_group_*: J handles' environments in ONE launch (job j in the grid's z dimension, its argument block row j of a device table)
against the same handles stepped by cn_step_multi.  The yardstick is always a twin set of handles of the same configurations and seeds:
after every launch obs, reward, done and topk_idx are equal, after the last one the twins' cn_snapshot blobs are byte-equal.  There is no
tolerance.  A case runs 20 launches with max_steps = 6, so time-outs and next-step resets fall inside the run; the actions come from a
fixed-seed generator."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LAUNCHES, MAX_STEPS = 20, 6
E_ = "cn_env_kernel"


class Twins:
    """Two sets of handles of `cfgs`: `a` stepped by cn_step_multi, `b` by a step group.  Both read rows of one action layout."""

    def __init__(self, cfgs, seed=11, reset=True):
        from crowdnav import _abi
        from crowdnav import env as E
        self.L, self.check, self.E = _abi.lib(), _abi.check, E
        self.a, self.b = [E.VecEnv(c) for c in cfgs], [E.VecEnv(c) for c in cfgs]
        self.N = sum(c.n_envs for c in cfgs)
        self.act_a, self.act_b = (torch.zeros((self.N, 2), dtype=torch.float32, device="cuda") for _ in range(2))
        self.multi, self._keep_a = E.multi_io(self.a, [self.act_a], "next")
        self.gen = torch.Generator(device="cpu").manual_seed(seed)
        self.groups, self.n_done, self.n_first = [], 0, 0
        if reset:
            for e in self.a + self.b:
                e.reset()
            torch.cuda.synchronize()

    def group_args(self, envs=None, auto_reset="next", action=None):
        (n, hs, ios), keep = self.E.group_io(self.b if envs is None else envs, self.act_b if action is None else action, auto_reset)
        self._keep_b = keep
        return n, hs, ios

    def create(self, n, hs, ios):
        """cn_step_group_create -> (return code, message, handle)"""
        g = C.c_void_p()
        rc = self.L.cn_step_group_create(n, hs, ios, C.byref(g))
        if rc == 0:
            self.groups.append(g)
        return rc, self.L.cn_last_error().decode(), g

    def group(self):
        rc, msg, g = self.create(*self.group_args())
        assert rc == 0, msg
        assert self.L.cn_step_group_jobs(g) == len(self.b)
        return g

    def name(self, g):
        return self.L.cn_step_group_kernel_name(g).decode()

    def compare(self, what):
        torch.cuda.synchronize()
        for j, (x, y) in enumerate(zip(self.a, self.b)):
            for k in ("obs", "reward", "done", "topk_idx"):
                assert np.array_equal(getattr(x, k).cpu().numpy(), getattr(y, k).cpu().numpy()), (what, j, k)

    def launch(self, g, what=None):
        act = torch.stack([torch.rand(self.N, generator=self.gen) * 0.22, torch.rand(self.N, generator=self.gen) * 4 - 2], 1)
        self.act_a.copy_(act)
        self.act_b.copy_(act)
        was_done = torch.cat([e.done for e in self.b]).bool().cpu()
        self.check(self.L.cn_step_multi(*self.multi))
        self.check(self.L.cn_step_group_step(g, None))
        self.compare(what)
        self.n_done += int(sum(int(e.done.sum()) for e in self.b))
        self.n_first += int(was_done.sum())          # launches an environment spent on its next-step reset

    def run(self, g, launches=LAUNCHES):
        for t in range(launches):
            self.launch(g, t)

    def snapshots_equal(self):
        torch.cuda.synchronize()
        for j, (x, y) in enumerate(zip(self.a, self.b)):
            assert np.array_equal(x.snapshot(), y.snapshot()), j

    def close(self):
        for g in self.groups:                         # a group goes before its handles
            self.L.cn_step_group_destroy(g)
        for e in self.a + self.b:
            e.close()


def configs(kws, n_envs, seed=70):
    from crowdnav import Config
    return [Config(n_envs=n, max_steps=MAX_STEPS, seed=seed + j, **kw) for j, (kw, n) in enumerate(zip(kws, n_envs))]


def whole_run(cfgs, kernel, launches=LAUNCHES):
    t = Twins(cfgs)
    g = t.group()
    assert t.name(g) == kernel
    t.run(g, launches)
    t.snapshots_equal()
    assert t.n_done > 0 and t.n_first > 0            # episodes ended inside the run, and environments spent launches on their reset
    t.step_kernels = [e.kernel_name("step") for e in t.b]
    t.shapes = [(e.R, e.P) for e in t.b]
    t.close()
    return t


def test_generic_world_ragged_jobs():
    """J = 3 PLAIN handles of 5, 1 and 9 environments and three shapes (none the headline one): the grid's tail rows, the launch's LDS
    from the largest job, R and P per job."""
    cfgs = configs([dict(n_rays=360, n_peds=8), dict(n_rays=128, n_peds=3), dict(n_rays=360, n_peds=12)], [5, 1, 9])
    t = whole_run(cfgs, E_ + "_grp")
    assert t.step_kernels == [E_] * 3 and t.shapes == [(360, 8), (128, 3), (360, 12)]


@pytest.mark.parametrize("x2", ["selected", "off"])
def test_headline_shape(x2, monkeypatch):
    """J = 3 handles of 360 rays x 20 pedestrians x K = 8, 4 environments each: the two-wavefront group kernel as selected (12
    environments <= 8 x compute units), and the one-wavefront one with the library's CN_X2 switch off."""
    if x2 == "off":
        monkeypatch.setenv("CN_X2", "0")
    else:
        monkeypatch.delenv("CN_X2", raising=False)
    t = whole_run(configs([{}] * 3, [4] * 3), E_ + ("_s360_x2_grp" if x2 == "selected" else "_s360_grp"))
    # (on their own the handles run the headline shape's kernels too: the two-wavefront one, or with the switch off one without it)
    assert all(k.startswith(E_ + "_s360") and k.endswith("_x2") == (x2 == "selected") for k in t.step_kernels), t.step_kernels


OTHER_WORLDS = {
    # name: (config keywords, environments per job)
    "s720": (dict(n_peds=100, n_rays=720, room_half=2.40), (2, 3)),
    "gt": (dict(risk_mode=1), (3, 2)),
    "wide": (dict(track_capacity=128), (2, 3)),
    "sf": (dict(ped_mode=2), (3, 2)),
    "sfd": (dict(n_peds=60, ped_mode=2, room_half=2.40), (2, 3)),
    "wa": (dict(wheel_accel=1.0, scan_f32=1), (3, 2)),
    "ct": (dict(ped_contact=1), (2, 3)),
    "gt_sf": (dict(ped_mode=2, risk_mode=1), (3, 2)),
    "gt_sfd": (dict(n_peds=60, ped_mode=2, room_half=2.40, risk_mode=1), (2, 3)),
    "gt_wa": (dict(wheel_accel=1.0, risk_mode=1), (3, 2)),
    "gt_ct": (dict(ped_contact=1, risk_mode=1), (2, 3)),
    "orig": (dict(obs_layout=1), (3, 2)),
    "rw": (dict(obs_layout=2, dt_ms=50), (2, 3)),
}


@pytest.mark.parametrize("world", sorted(OTHER_WORLDS))
def test_every_other_world(world):
    kw, n_envs = OTHER_WORLDS[world]
    t = whole_run(configs([kw, kw], n_envs), "%s_%s_grp" % (E_, world))
    assert t.step_kernels == [E_ + "_" + world] * 2


def test_one_job_and_sixty_four_jobs():
    small = dict(n_rays=128, n_peds=3)
    whole_run(configs([small], [3]), E_ + "_grp")
    t = Twins(configs([small] * 64, [1] * 64))
    n, hs, ios = t.group_args()
    more_h, more_io = (C.c_void_p * 65)(*[hs[j % 64] for j in range(65)]), (type(ios[0]) * 65)(*[ios[j % 64] for j in range(65)])
    rc, msg, _ = t.create(65, more_h, more_io)
    assert rc != 0 and "65 jobs" in msg and "1 ... 64" in msg
    g = t.group()
    assert t.L.cn_step_group_jobs(g) == 64 and t.name(g) == E_ + "_grp"
    t.run(g)
    t.snapshots_equal()
    assert t.n_done > 0 and t.n_first > 0
    t.close()


def test_group_reset_with_masks():
    """cn_step_group_reset against cn_reset on the twins: some environments of some jobs, every environment of the others (a NULL
    mask), in the middle of a run; then masks NULL for all, and the same masks again (nothing to copy)."""
    cfgs = configs([dict(n_rays=360, n_peds=8), dict(n_rays=128, n_peds=3), dict(n_rays=360, n_peds=12)], [5, 3, 4])
    t = Twins(cfgs, reset=False)
    g = t.group()

    def reset(masks):
        for x, m in zip(t.a, masks or [None] * 3):
            x.reset(m)
        ptrs = None if masks is None else (C.c_void_p * 3)(*[m.data_ptr() if m is not None else None for m in masks])
        t.check(t.L.cn_step_group_reset(g, ptrs, None))
        t.compare(("reset", masks is None))

    reset(None)                                                        # the first observation: every environment of every job
    t.run(g, 7)
    m0 = torch.tensor([1, 0, 0, 1, 1], dtype=torch.uint8, device="cuda")
    m2 = torch.tensor([0, 0, 1, 0], dtype=torch.uint8, device="cuda")
    before = [e.obs.clone() for e in t.b]
    reset([m0, None, m2])
    assert not torch.equal(before[1], t.b[1].obs) and not torch.equal(before[0][0], t.b[0].obs[0])
    t.run(g, 5)
    reset([m0, None, m2])                                              # the rows hold these addresses already
    t.run(g, 2)
    reset(None)
    t.run(g, 5)
    t.snapshots_equal()
    assert t.n_done > 0
    t.close()


def test_refusals_by_message():
    """Every refusal of cn_step_group_create names the job; after each one a valid group on the same handles still steps equal to
    the twins."""
    from crowdnav.env import VecEnv
    small = dict(n_rays=128, n_peds=3)
    t = Twins(configs([small] * 3, [2, 3, 2]))
    other = VecEnv(configs([dict(risk_mode=1)], [2])[0])               # a handle of another world

    def args(envs=None):
        return t.group_args(envs)

    def refused(n, hs, ios, *words):
        rc, msg, _ = t.create(n, hs, ios)
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)
        g = t.group()                                                  # nothing was left behind: the same handles, a valid group
        t.launch(g, words)
        t.launch(g, words)

    n, hs, ios = args()
    refused(0, hs, ios, "0 jobs", "1 ... 64")
    refused(65, hs, ios, "65 jobs", "1 ... 64")
    n, hs, ios = args()
    hs[1] = None
    refused(n, hs, ios, "job 1", "null handle")
    for field in ("action", "obs", "reward", "done"):
        n, hs, ios = args()
        setattr(ios[2], field, None)
        refused(n, hs, ios, "job 2", "null action, obs, reward or done")
    n, hs, ios = args()
    ios[1].auto_reset = 1
    refused(n, hs, ios, "job 1", "auto_reset 1")
    n, hs, ios = args()
    hs[2] = hs[0]
    refused(n, hs, ios, "job 2", "the same handle as job 0")
    n, hs, ios = args(envs=t.b[:2] + [other])
    refused(n, hs, ios, "job 2", E_ + "_gt_grp", E_ + "_grp")
    if torch.cuda.device_count() > 1:
        far = VecEnv(configs([small], [2])[0], device=1)
        with torch.cuda.device(1):
            far_act = torch.zeros((2, 2), device="cuda:1")
        n, hs, ios = args()
        from crowdnav.env import step_io
        hs[1], ios[1] = far.h.value, step_io(far, far_act, None, "next")
        refused(n, hs, ios, "job 1", "on device 1", "job 0 on device 0")
        far.close()
    t.snapshots_equal()
    t.close()
    other.close()


def test_refusal_of_handles_whose_group_kernels_differ(monkeypatch):
    """Headline-shape handles with and without the CN_X2 switch select different group kernels: one launch runs one kernel."""
    from crowdnav.env import VecEnv
    monkeypatch.delenv("CN_X2", raising=False)
    t = Twins(configs([{}] * 2, [2, 2]))
    monkeypatch.setenv("CN_X2", "0")
    off = VecEnv(configs([{}], [2])[0])
    monkeypatch.delenv("CN_X2")
    rc, msg, _ = t.create(*t.group_args(t.b + [off], action=torch.zeros((6, 2), device="cuda")))
    assert rc != 0 and "job 2" in msg and E_ + "_s360_grp" in msg and E_ + "_s360_x2_grp" in msg, msg
    g = t.group()
    t.launch(g)
    t.snapshots_equal()
    t.close()
    off.close()


def test_refusal_of_handles_with_stage_timing_or_ablation(monkeypatch):
    """The profiling build (its own library, with cn_debug_set_timing / cn_debug_set_ablate): a handle with either set is refused; with
    both cleared the group kernels of that build step equal to its twins."""
    from crowdnav import _abi
    monkeypatch.setattr(_abi, "LIB_PATH", _abi.build_timing())
    monkeypatch.setattr(_abi, "_lib", None)
    t = Twins(configs([dict(n_rays=128, n_peds=3)] * 2, [2, 3]))
    L = t.L
    L.cn_debug_set_timing.argtypes = [C.c_void_p, C.c_void_p]
    L.cn_debug_set_ablate.argtypes = [C.c_void_p, C.c_int]
    stamps = torch.zeros((3, 32), dtype=torch.int64, device="cuda")
    assert L.cn_debug_set_timing(t.b[1].h, stamps.data_ptr()) == 0
    rc, msg, _ = t.create(*t.group_args())
    assert rc != 0 and "job 1" in msg and "timing" in msg, msg
    assert L.cn_debug_set_timing(t.b[1].h, None) == 0 and L.cn_debug_set_ablate(t.b[0].h, 1) == 0
    rc, msg, _ = t.create(*t.group_args())
    assert rc != 0 and "job 0" in msg and "ablation" in msg, msg
    assert L.cn_debug_set_ablate(t.b[0].h, 0) == 0
    g = t.group()
    assert t.name(g) == E_ + "_grp"
    t.run(g, 8)
    t.snapshots_equal()
    t.close()
