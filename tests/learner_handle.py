"""TEST INFRASTRUCTURE.  The raw learner handle of the GPU tests, stated once: cn_<family>_create / _update / _batch_dev / _loss_dev
/ _set_replay_sample / _destroy called through ctypes on crowdnav._abi's structs, and the few helpers every such test needs.
Deliberately not built on crowdnav._fused: these tests hold the library independently of the product's Python glue."""
import ctypes as C

import torch


def lib():
    from crowdnav import _abi
    return _abi, _abi.lib()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def alias(ptr, shape, typestr="<f4"):
    """The device memory at `ptr` as a tensor of `shape` (() for a scalar): a view, not a copy."""
    n = 1
    for x in shape:
        n *= int(x)

    class _Arr:
        __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_Arr(), device="cuda").reshape(tuple(shape))


def err():
    return lib()[1].cn_td3_last_error().decode()


def mlp_struct(p, names, struct="CnTd3Mlp"):
    """The struct of pointers to p's tensors `names` (CnSacActor for SAC's eight)."""
    return getattr(lib()[0], struct)(*[p[k].data_ptr() for k in names])


def ring_fields(ring):
    """A config's replay_* fields from a ring {s, a, r, s2, d, size: device tensors}; none for None."""
    if ring is None:
        return {}
    return dict(replay_s=ring["s"].data_ptr(), replay_a=ring["a"].data_ptr(), replay_r=ring["r"].data_ptr(), replay_s2=ring["s2"].data_ptr(),
                replay_d=ring["d"].data_ptr(), replay_size_dev=ring["size"].data_ptr())


def batch_struct(batch, struct="CnTd3Batch"):
    """The batch struct of an explicit batch (a tuple of device tensors, None for a null field), holding on to the tensors; None
    for None."""
    if batch is None:
        return None
    st = getattr(lib()[0], struct)(*[None if x is None else x.data_ptr() for x in batch])
    st.tensors = batch
    return st


class LearnerHandle:
    """One cn_<family> handle made from the config struct `cfg`; `keep`: whatever cfg points at."""

    def __init__(self, family, cfg, keep=None):
        self.L, self.family, self.cfg, self.keep, self.h = lib()[1], family, cfg, keep, C.c_void_p()
        rc = self._f("create")(C.byref(cfg), 0, C.byref(self.h))
        assert rc == 0, self.L.cn_td3_last_error()

    def _f(self, name):
        return getattr(self.L, "cn_%s_%s" % (self.family, name))

    def update(self, *lead, batch=None, sync=True):
        """lead: TD3's do_actor; batch: a batch struct (batch_struct) or None for the replay path."""
        self.batch = batch
        rc = self._f("update")(self.h, *lead, None if batch is None else C.byref(batch), stream())
        assert rc == 0, self.L.cn_td3_last_error()
        if sync:
            torch.cuda.synchronize()

    def batch_dev(self, what, shape, typestr="<f4"):
        """A copy of the buffer cn_<family>_batch_dev names `what`."""
        p = self._f("batch_dev")(self.h, what)
        assert p, (self.family, what)
        torch.cuda.synchronize()
        return alias(p, shape, typestr).clone()

    def loss(self, shape=()):
        torch.cuda.synchronize()
        return alias(self._f("loss_dev")(self.h), shape).clone()

    def set_replay_sample(self, mode):
        return self._f("set_replay_sample")(self.h, mode)

    def close(self):
        if self.h:
            self._f("destroy")(self.h)
            self.h = None
