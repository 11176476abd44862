"""The two libraries a test of a device-pointer entry point runs on (parametrize over BACKENDS).  Both: .library() and .gpu, .kw (the
constructor keywords of the side's plain geometry) on the class; on an instance .ptr(array) -> device pointer of a copy it keeps
alive, .alloc(nbytes) -> (keep-alive, pointer, read-back) of a poisoned array.  torch is imported inside Gpu's methods only."""
import numpy as np
import pytest

GENERIC = dict(jit="off", envs_per_workgroup=4, threads_per_workgroup=64)   # the generic kernel on 4-env workgroups
POISON, GUARD = 0xA5, 64


def emu_library():
    """the host-thread build of the product sources (tests/emu), built on first use"""
    from engine_backend import build_emu
    return build_emu()


class Host:
    """"device" arrays of the host-thread build: numpy arrays"""
    gpu = False
    kw = GENERIC
    library = staticmethod(emu_library)

    def __init__(self):
        self.keep = []

    def ptr(self, a):
        if a is None:
            return 0
        a = np.ascontiguousarray(a)
        self.keep.append(a)
        return a.ctypes.data

    @staticmethod
    def alloc(nbytes):
        raw = np.full(nbytes + 16, POISON, np.uint8)
        off = (-raw.ctypes.data) % 16
        return raw, raw.ctypes.data + off, lambda: raw[off:off + nbytes].copy()


class Gpu:
    """device arrays of the real library: torch tensors, complete before an engine on a stream of its own reads or writes them"""
    gpu = True
    kw = {}
    library = staticmethod(lambda: None)

    def __init__(self):
        self.keep = []

    def ptr(self, a):
        import torch

        if a is None:
            return 0
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
        torch.cuda.synchronize()
        self.keep.append(t)
        return t.data_ptr()

    @staticmethod
    def alloc(nbytes):
        import torch

        t = torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert t.data_ptr() % 16 == 0
        return t, t.data_ptr(), lambda: t.cpu().numpy()


BACKENDS = [pytest.param(Host, id="emulated"), pytest.param(Gpu, id="gpu", marks=pytest.mark.gpu)]
