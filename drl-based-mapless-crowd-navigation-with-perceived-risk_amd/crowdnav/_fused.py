"""What the TD3, DDPG, DQN and SAC agents share on the way to libcrowdnav's fused learners (csrc/crowdnav_td3.hip, crowdnav_ddpg.hip, crowdnav_dqn.hip, crowdnav_sac.hip): the network
pointers, views of the library's device memory, and the owners of a learner handle, of a population's handles and of an evaluator's."""
import ctypes as C

import torch

from . import _abi


def mlp_of(m):
    """The `cn_td3_mlp` of a module with linear1 / linear2 / linear3: device pointers to its nn.Linear storages."""
    ps = [m.linear1.weight, m.linear1.bias, m.linear2.weight, m.linear2.bias, m.linear3.weight, m.linear3.bias]
    assert all(p.is_contiguous() and p.dtype == torch.float32 and p.is_cuda for p in ps)
    return _abi.CnTd3Mlp(*[p.data_ptr() for p in ps])


def _device_view(ptr, shape, dtype, device):
    """A tensor aliasing device memory owned by libcrowdnav (alive as long as its handle)."""
    ts = {torch.float32: "<f4", torch.int32: "<i4", torch.int64: "<i8"}[dtype]
    n = 1
    for x in shape:
        n *= int(x)

    class _Arr:
        __cuda_array_interface__ = {"shape": (n,), "typestr": ts, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_Arr(), device=device).reshape(tuple(shape))


class _StateBlob:
    """cn_<...>_state_size / _save / _load of a handle (include/crowdnav.h): the learner's whole state as one blob, out and in by one
    launch each.  The host class gives `_state_fn(what)` (the library function), `h`, `device`, `_check`."""

    def state_size(self):
        """Bytes of this handle's state blob; the first call builds the launch's job table (it synchronises)."""
        n = int(self._state_fn("size")(self.h))
        if n == 0:
            self._check("state_size", -1)
        return n

    def _state_buffers(self):
        n = self.state_size()
        if getattr(self, "_state_dev", None) is None or self._state_dev.numel() != n:
            self._state_dev = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._state_host = torch.empty(n, dtype=torch.uint8).pin_memory()
        return self._state_dev, self._state_host

    def save_state(self, wait=True):
        """One launch into the handle's device buffer, then one asynchronous copy to its pinned host buffer, both on torch's current
        stream: a consistent picture at this point of the stream.  Returns the pinned uint8 tensor, which the next save_state
        overwrites; wait=False leaves the waiting (for the stream) to the caller."""
        dev, host = self._state_buffers()
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._check("state_save", self._state_fn("save")(self.h, C.c_void_p(dev.data_ptr()), dev.numel(), st))
        host.copy_(dev, non_blocking=True)
        if wait:
            torch.cuda.current_stream(self.device).synchronize()
        return host

    def load_state(self, blob):
        """The state of a save_state blob (uint8 tensor or array-like of state_size() bytes) into this handle: one small synchronous
        read of header and directory, then one launch on torch's current stream.  A blob of another shape is refused and nothing
        is written."""
        dev, _ = self._state_buffers()
        b = torch.as_tensor(blob).reshape(-1)
        if b.dtype != torch.uint8:
            raise ValueError("a state blob is uint8")
        if b.numel() == dev.numel():
            dev.copy_(b)
            src, n = dev, dev.numel()
        else:                                      # the library words the refusal
            src, n = b.to(self.device).contiguous(), b.numel()
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._check("state_load", self._state_fn("load")(self.h, C.c_void_p(src.data_ptr()), n, st))


class FusedLearner(_StateBlob):
    """Owns one learner handle of libcrowdnav: family = "td3", "ddpg" or "dqn" names cn_<family>_create / _update / _destroy /
    _loss_dev / _batch_dev.  An error raises CrowdNavError("<function>: <cn_td3_last_error>")."""

    def __init__(self, family, cfg, device, dev_index, loss_shape=(), replay_sample="with"):
        mode = _abi.replay_sample_mode(replay_sample)
        self._L = L = _abi.lib()
        self.family, self.cfg, self.device = family, cfg, device
        self.h = C.c_void_p()
        self._check("create", self._fn("create")(C.byref(cfg), dev_index, C.byref(self.h)))
        self._loss = _device_view(self._fn("loss_dev")(self.h), loss_shape, torch.float32, device)
        self._keep, self._update = None, self._fn("update")
        self.replay_sample = "with"               # a fresh handle's mode
        if mode != _abi.CN_SAMPLE_WITH_REPLACEMENT:
            self.set_replay_sample(replay_sample)

    def _fn(self, what):
        return getattr(self._L, "cn_%s_%s" % (self.family, what))

    def _state_fn(self, what):
        if self.family != "td3":
            raise _abi.CrowdNavError("cn_%s_state_%s: only the TD3 learners' state can be saved and loaded" % (self.family, what))
        return self._fn("state_" + what)

    def _check(self, what, rc):
        if rc != 0:
            raise _abi.CrowdNavError("cn_%s_%s: %s" % (self.family, what, self._L.cn_td3_last_error().decode()))

    def update(self, *args, batch=None, keep=None):
        """cn_<family>_update(handle, *args, batch, torch's current stream): enqueue-only.  batch: the ctypes batch struct or None
        (= sample the replay); keep: the tensors it points into, held until the next explicit batch because the launches are
        asynchronous.  Returns the loss where the kernels left it as a fresh tensor per call, the same contract as the PyTorch
        learners (no host synchronisation: one small device-to-device copy on the update's stream).  The view of the handle's own
        loss is overwritten by the next update and dies with the handle, so it is not handed out."""
        if batch is not None:
            self._keep = (batch, keep)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._check("update", self._update(self.h, *args, C.byref(batch) if batch is not None else None, st))
        return self._loss.clone()

    def set_replay_sample(self, replay_sample):
        """cn_<family>_set_replay_sample: "with" (replacement, the default) or "without" (distinct rows, as the reference's
        random.sample) for the updates enqueued from now on; a captured update keeps the mode it was captured with."""
        self._check("set_replay_sample", self._fn("set_replay_sample")(self.h, _abi.replay_sample_mode(replay_sample)))
        self.replay_sample = replay_sample

    def batch_dev(self, what, shape, dtype=torch.float32):
        """A view of what the last update gathered or computed (cn_<family>_batch_dev), valid until the next update."""
        return _device_view(self._fn("batch_dev")(self.h, int(what)), shape, dtype, self.device)

    def __del__(self):
        try:
            if self.h:
                self._fn("destroy")(self.h)
                self.h = None
        except Exception:
            pass


class FusedPopulation(_StateBlob):
    """Owns one cn_td3_pop handle: P TD3 learners updated by the launches of one (include/crowdnav.h, cn_td3_pop_create).  cfgs: the
    members' CnTd3Config, in member order.  The sibling of FusedLearner for the population calls; errors raise the same way."""

    def __init__(self, cfgs, device, dev_index, replay_sample="with", replay_source="own"):
        mode = _abi.replay_sample_mode(replay_sample)
        source = _abi.replay_source(replay_source)
        self._L = L = _abi.lib()
        self.device, self.P = device, len(cfgs)
        self.cfgs = (_abi.CnTd3Config * self.P)(*cfgs)
        self.h = C.c_void_p()
        self._check("create", L.cn_td3_pop_create(self.cfgs, self.P, dev_index, C.byref(self.h)))
        self._loss = _device_view(L.cn_td3_pop_loss_dev(self.h), (self.P,), torch.float32, device)
        self.replay_sample = "with"
        if mode != _abi.CN_SAMPLE_WITH_REPLACEMENT:
            self.set_replay_sample(replay_sample)
        self.replay_source = "own"
        if source != _abi.CN_REPLAY_OWN:
            self.set_replay_source(replay_source)

    def _check(self, what, rc):
        if rc != 0:
            raise _abi.CrowdNavError("cn_td3_pop_%s: %s" % (what, self._L.cn_td3_last_error().decode()))

    def _state_fn(self, what):
        return getattr(self._L, "cn_td3_pop_state_" + what)

    def update(self, do_actor):
        """cn_td3_pop_update on torch's current stream: enqueue-only.  Returns the P losses as a fresh tensor (one small
        device-to-device copy on that stream; the handle's own buffer is overwritten by the next update)."""
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._check("update", self._L.cn_td3_pop_update(self.h, int(do_actor), st))
        return self._loss.clone()

    def set_replay_sample(self, replay_sample):
        """cn_td3_pop_set_replay_sample: "with" | "without", for all members, for the updates enqueued from now on."""
        self._check("set_replay_sample", self._L.cn_td3_pop_set_replay_sample(self.h, _abi.replay_sample_mode(replay_sample)))
        self.replay_sample = replay_sample

    def set_replay_source(self, replay_source):
        """cn_td3_pop_set_replay_source: "own" (every member samples its own ring, the default) | "shared" (every member samples
        the union of all members' rings), for the updates enqueued from now on; a captured update keeps its source."""
        self._check("set_replay_source", self._L.cn_td3_pop_set_replay_source(self.h, _abi.replay_source(replay_source)))
        self.replay_source = replay_source

    def batch_src(self, member, batch):
        """An int64 view [batch, 2] of {ring, row} of `member`'s rows in the last shared update (cn_td3_pop_batch_src_dev), valid
        until the next one."""
        ptr = self._L.cn_td3_pop_batch_src_dev(self.h, int(member))
        if not ptr:
            raise _abi.CrowdNavError("cn_td3_pop_batch_src_dev: member %r out of range, or no shared update yet" % (member,))
        return _device_view(ptr, (int(batch), 2), torch.int64, self.device)

    def batch_dev(self, member, what, shape, dtype=torch.float32):
        """A view of what the last update gathered for `member` (cn_td3_pop_batch_dev), valid until the next update."""
        ptr = self._L.cn_td3_pop_batch_dev(self.h, int(member), int(what))
        if not ptr:
            raise _abi.CrowdNavError("cn_td3_pop_batch_dev: member %r / what %r out of range" % (member, what))
        return _device_view(ptr, shape, dtype, self.device)

    def pbt_bind(self, cfg, logs=None, keep=None):
        """cn_td3_pop_pbt_bind: cfg a CnTd3PbtConfig, logs the members' CnEpisodeLog in member order or None; keep: what the logs
        point into.  Synchronises (it uploads the state); binding again starts over."""
        arr = (_abi.CnEpisodeLog * self.P)(*logs) if logs is not None else None
        self._check("pbt_bind", self._L.cn_td3_pop_pbt_bind(self.h, C.byref(cfg), arr))
        self._pbt_keep = (cfg, arr, keep)
        nbytes = C.sizeof(_abi.CnTd3PbtState)
        ptr = self._L.cn_td3_pop_pbt_state_dev(self.h)

        class _Arr:
            __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
        self._pbt_state = torch.as_tensor(_Arr(), device=self.device)
        self._pbt_host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    def exploit(self, fitness=None):
        """cn_td3_pop_exploit on torch's current stream: two launches, enqueue-only.  fitness: float32 [P] on the device, or None = from
        the bound logs."""
        if fitness is not None and not (fitness.dtype == torch.float32 and fitness.is_cuda and fitness.is_contiguous() and fitness.numel() == self.P):
            raise ValueError("fitness must be a contiguous float32 tensor of %d values on %s" % (self.P, self.device))
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._pbt_fitness = fitness                # alive until the next call: the launches are asynchronous
        self._check("exploit", self._L.cn_td3_pop_exploit(self.h, None if fitness is None else C.c_void_p(fitness.data_ptr()), st))

    def pbt_state(self):
        """One device-to-host copy of cn_td3_pbt_state (it waits for the stream) -> a CnTd3PbtState."""
        if getattr(self, "_pbt_state", None) is None:
            raise _abi.CrowdNavError("cn_td3_pop_pbt_state_dev: no cn_td3_pop_pbt_bind yet")
        self._pbt_host.copy_(self._pbt_state)
        return _abi.CnTd3PbtState.from_buffer_copy(self._pbt_host.numpy().tobytes())

    def __del__(self):
        try:
            if self.h:
                self._L.cn_td3_pop_destroy(self.h)
                self.h = None
        except Exception:
            pass


class FusedPopulationActor:
    """Owns one cn_actor_pop handle: P actors run by one launch and re-packed by one launch (include/crowdnav.h,
    cn_actor_pop_create).  members: the CnActorPopMember of every member, in member order; keep: whatever their pointers point into
    (the handle holds them for its lifetime).  Errors raise CrowdNavError("<function>: <cn_last_error>")."""

    def __init__(self, members, obs_dim, device, dev_index, keep=None):
        self._L = L = _abi.lib()
        self.device, self.P, self.obs_dim, self._keep = device, len(members), int(obs_dim), keep
        self.members = (_abi.CnActorPopMember * self.P)(*members)
        self._counters = (C.c_uint64 * self.P)()
        self.h = C.c_void_p()
        self._check("create", L.cn_actor_pop_create(self.members, self.P, self.obs_dim, dev_index, C.byref(self.h)))

    def _check(self, what, rc):
        if rc != 0:
            raise _abi.CrowdNavError("cn_actor_pop_%s: %s" % (what, self._L.cn_last_error().decode()))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def pack(self):
        """cn_actor_pop_pack on torch's current stream: every member's packed weights from its nn.Linear storages, one launch."""
        self._check("pack", self._L.cn_actor_pop_pack(self.h, self._stream()))

    def forward(self, counters, add_noise=True):
        """cn_actor_pop_forward on torch's current stream: one launch; counters[p] keys member p's exploration noise."""
        c = self._counters
        for p, v in enumerate(counters):
            c[p] = v
        self._check("forward", self._L.cn_actor_pop_forward(self.h, c, int(bool(add_noise)), self._stream()))

    def weights(self, member):
        """The CnActorWeights of `member` (cn_actor_pop_weights): the handle's packed buffers, the member's biases and w3."""
        w = _abi.CnActorWeights()
        self._check("weights", self._L.cn_actor_pop_weights(self.h, int(member), C.byref(w)))
        return w

    def packed(self, member):
        """Views (w1p [Dp, 256], w2p [256, 256]) of the handle's packed buffers of `member`, alive as long as the handle."""
        w = self.weights(member)
        return (_device_view(w.w1p, (w.obs_dim_padded, 256), torch.float32, self.device),
                _device_view(w.w2p, (256, 256), torch.float32, self.device))

    def __del__(self):
        try:
            if self.h:
                self._L.cn_actor_pop_destroy(self.h)
                self.h = None
        except Exception:
            pass


class FusedPopulationRecorder:
    """Owns one cn_pop_record handle: every member's replay write and episode log as two launches (include/crowdnav.h,
    cn_pop_record_create).  members: the CnPopRecordMember of every member, in member order; keep: whatever their pointers point into
    (the handle holds them for its lifetime).  Errors raise CrowdNavError("<function>: <cn_last_error>")."""
    _prefix = "cn_pop_record"

    def __init__(self, members, obs_dim, device, dev_index, keep=None):
        self._L = L = _abi.lib()
        self.device, self.P, self.obs_dim, self._keep = device, len(members), int(obs_dim), keep
        self.members = (_abi.CnPopRecordMember * self.P)(*members)
        self.h = C.c_void_p()
        self._check("_create", L.cn_pop_record_create(self.members, self.P, self.obs_dim, dev_index, C.byref(self.h)))

    def _fn(self, what):
        return getattr(self._L, self._prefix + what)

    def _check(self, what, rc):
        if rc != 0:
            raise _abi.CrowdNavError("%s%s: %s" % (self._prefix, what, self._L.cn_last_error().decode()))

    def _rows(self, member):
        return int(self.members[int(member)].n)

    def record(self, launch):
        """cn_pop_record on torch's current stream: at most two launches; `launch` is the index the finished episodes' rows carry."""
        self._check("", self._fn("")(self.h, float(launch), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def resetting(self, member):
        """A uint8 view [n_member] of the handle's flags of `member` (cn_pop_record_resetting), alive as long as the handle: row i's
        next record is its environment's reset launch, not a transition."""
        ptr = self._fn("_resetting")(self.h, int(member))
        if not ptr:
            raise _abi.CrowdNavError("%s_resetting: %s" % (self._prefix, self._L.cn_last_error().decode()))
        n = self._rows(member)
        if n == 0:
            return torch.zeros(0, dtype=torch.uint8, device=self.device)

        class _Arr:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(_Arr(), device=self.device)

    def __del__(self):
        try:
            if self.h:
                self._fn("_destroy")(self.h)
                self.h = None
        except Exception:
            pass


class FusedNStepRecorder(FusedPopulationRecorder):
    """Owns one cn_nstep_record handle: FusedPopulationRecorder's job with n-step rows (include/crowdnav.h, cn_nstep_record_create).
    members: the CnNstepMember of every member (its CnPopRecordMember and its one-step gamma), in member order; n_step: the window,
    one for all.  record(launch) is cn_nstep_record, resetting(member) the handle's flags; pending(member) its pending store."""
    _prefix = "cn_nstep_record"
    PENDING = ("s", "a", "ret", "count", "clock")

    def __init__(self, members, n_step, obs_dim, device, dev_index, keep=None):
        self._L = L = _abi.lib()
        self.device, self.P, self.n_step, self.obs_dim, self._keep = device, len(members), int(n_step), int(obs_dim), keep
        self.members = (_abi.CnNstepMember * self.P)(*members)
        self.h = C.c_void_p()
        self._check("_create", L.cn_nstep_record_create(self.members, self.P, self.n_step, self.obs_dim, dev_index, C.byref(self.h)))

    def _rows(self, member):
        return int(self.members[int(member)].rec.n)

    def pending(self, member):
        """Views (s [n, W, obs_dim], a [n, W, 2], ret [n, W] float32; count [n], clock [n] int32) of `member`'s pending store
        (cn_nstep_record_pending), alive as long as the handle; with resetting(member) they are the handle's whole state."""
        pd = _abi.CnNstepPending()
        self._check("_pending", self._L.cn_nstep_record_pending(self.h, int(member), C.byref(pd)))
        n, W, D = int(pd.n), int(pd.n_step), int(pd.obs_dim)
        shapes = (((n, W, D), torch.float32), ((n, W, 2), torch.float32), ((n, W), torch.float32), ((n,), torch.int32), ((n,), torch.int32))
        if n == 0:
            return tuple(torch.zeros(sh, dtype=dt, device=self.device) for sh, dt in shapes)
        return tuple(_device_view(getattr(pd, k), sh, dt, self.device) for k, (sh, dt) in zip(self.PENDING, shapes))


class FusedEvaluator:
    """Owns one cn_eval handle: the evaluation bookkeeping of J jobs as one launch per step (include/crowdnav.h, cn_eval_create).
    jobs: the CnEvalJob of every job, in job order; keep: whatever their pointers point into (the handle holds them for its lifetime).
    Errors raise CrowdNavError("<function>: <cn_last_error>")."""

    def __init__(self, jobs, n_groups, device, dev_index, keep=None):
        self._L = L = _abi.lib()
        self.device, self.J, self.G, self._keep = device, len(jobs), int(n_groups), keep
        self.jobs = (_abi.CnEvalJob * self.J)(*jobs)
        self.h = C.c_void_p()
        self._check("create", L.cn_eval_create(self.jobs, self.J, self.G, dev_index, C.byref(self.h)))
        nbytes = C.sizeof(_abi.CnEvalState)
        ptr = L.cn_eval_state_dev(self.h)

        class _Arr:
            __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
        self._state = torch.as_tensor(_Arr(), device=device)
        self._host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.remaining_dev = _device_view(ptr + _abi.CnEvalState.remaining.offset, (_abi.CN_EVAL_MAX,), torch.int32, device)[:self.J]
        self.summary_dev = _device_view(ptr + _abi.CnEvalState.summary.offset, (_abi.CN_EVAL_MAX, 8), torch.float32, device)[:self.J]
        self.fitness_dev = _device_view(ptr + _abi.CnEvalState.fitness.offset, (_abi.CN_EVAL_MAX,), torch.float32, device)[:self.G]

    def _check(self, what, rc):
        if rc != 0:
            raise _abi.CrowdNavError("cn_eval_%s: %s" % (what, self._L.cn_last_error().decode()))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self):
        """cn_eval_reset on torch's current stream: one launch; every job's counts, sums and log start over."""
        self._check("reset", self._L.cn_eval_reset(self.h, self._stream()))

    def record(self, launch):
        """cn_eval_record on torch's current stream: one launch; `launch` is the index the counted episodes' rows carry."""
        self._check("record", self._L.cn_eval_record(self.h, float(launch), self._stream()))

    def finish(self, metric, fitness=None):
        """cn_eval_finish on torch's current stream: one launch; metric CN_EVAL_SUCCESS_RATE | CN_EVAL_MEAN_RETURN; fitness: float32
        [n_groups] on the device that also receives the groups' fitness, or None."""
        if fitness is not None and not (fitness.dtype == torch.float32 and fitness.is_cuda and fitness.is_contiguous() and fitness.numel() == self.G):
            raise ValueError("fitness must be a contiguous float32 tensor of %d values on %s" % (self.G, self.device))
        self._fitness = fitness                    # alive until the next call: the launch is asynchronous
        self._check("finish", self._L.cn_eval_finish(self.h, int(metric), None if fitness is None else C.c_void_p(fitness.data_ptr()), self._stream()))

    def state(self):
        """One device-to-host copy of cn_eval_state (it waits for the stream) -> a CnEvalState."""
        self._host.copy_(self._state)
        return _abi.CnEvalState.from_buffer_copy(self._host.numpy().tobytes())

    def __del__(self):
        try:
            if self.h:
                self._L.cn_eval_destroy(self.h)
                self.h = None
        except Exception:
            pass
