"""Fenced buffers for the GPU tests (tests/test_fences_gpu.py, tests/test_call_order_gpu.py).

An output handed to the library is one uint8 allocation `[front guard | payload | slack | back
guard]`: the guards are GUARD bytes of a position-dependent pattern (no constant store can
reproduce it), the payload starts on a 256-B boundary (every alignment rule of
include/sd_hip_cas.h holds) and the back guard starts at the byte after the payload, or after
the `slack` bytes an entry point documents as writable past it.  `check()` compares the guards
with the pattern and names the first changed offset.  DevFence lives in device memory, HostFence
in numpy memory (the host outputs of the blocking entry points, through the raw ABI).

An input is fenced the same way (DevInput), but its guards hold a typed, adversarial value
instead of the pattern — a key that occurs in the payload, a valid index, 2^40 for a size — so
a kernel that reads past its input computes something wrong instead of something lucky; after
the call the whole allocation must equal its snapshot: the library wrote nothing into it.

GUARD = 4,096 B is one u32 store by every thread of the widest workgroup of the library
(1,024 threads): a choice, not a measurement."""
import numpy as np

GUARD = 4096
_TORCH = {"uint8": "uint8", "int8": "uint8", "uint32": "int32", "int32": "int32",
          "uint64": "int64", "int64": "int64"}


def pattern(nbytes: int, salt: int = 0) -> np.ndarray:
    i = np.arange(nbytes, dtype=np.uint64)
    return ((i * np.uint64(197) + np.uint64(31 + salt)) ^ (i >> np.uint64(8)) ^ np.uint64(0x5C)).astype(np.uint8)


class DevFence:
    """A fenced device output of `count` elements of numpy dtype `dtype`.  `.t` is the payload as
    a contiguous torch tensor (u32 / u64 as int32 / int64, bit for bit), `.host()` its numpy
    copy in `dtype`.  fill: the payload's initial bytes (a uint8 value), so an unwritten
    element shows; slack: bytes after the payload that the callee may write."""

    def __init__(self, dtype, count: int, fill: int = 0xC3, slack: int = 0, salt: int = 0):
        import torch
        self.dtype = np.dtype(dtype)
        self.count = int(count)
        self.nbytes = self.count * self.dtype.itemsize
        self.slack = int(slack)
        total = GUARD + self.nbytes + self.slack + GUARD
        self.buf = torch.from_numpy(pattern(total, salt)).cuda()
        assert self.buf.data_ptr() % 256 == 0
        self.ref = self.buf.clone()
        self.lo, self.hi = GUARD, GUARD + self.nbytes
        self.buf[self.lo:self.hi + self.slack] = fill
        self.t = self.buf[self.lo:self.hi].view(getattr(torch, _TORCH[self.dtype.name]))
        assert self.t.is_contiguous() and self.t.data_ptr() % 256 == 0

    @property
    def ptr(self) -> int:
        return int(self.t.data_ptr())

    def host(self) -> np.ndarray:
        return self.buf[self.lo:self.hi].cpu().numpy().view(self.dtype)

    def check(self, what: str = "output") -> None:
        ne = self.buf != self.ref  # on the device
        ne[self.lo:self.hi + self.slack] = False
        if bool(ne.any()):
            at = int(ne.nonzero()[0])
            where = f"{self.lo - at} B before the payload" if at < self.lo else \
                f"{at - self.hi} B past the payload's end"
            raise AssertionError(f"{what}: guard changed {where} ({int(ne.sum())} bytes in all; "
                                 f"{self.count} x {self.dtype.name})")


class HostFence:
    """The same over numpy memory: `.a` is the payload (dtype, count), `.ptr` its address."""

    def __init__(self, dtype, count: int, fill: int = 0xC3, salt: int = 0):
        self.dtype = np.dtype(dtype)
        self.count = int(count)
        self.nbytes = self.count * self.dtype.itemsize
        raw = np.empty(GUARD + 256 + self.nbytes + GUARD, dtype=np.uint8)
        self.lo = GUARD + (-(raw.ctypes.data + GUARD)) % 256
        self.hi = self.lo + self.nbytes
        raw[:] = pattern(len(raw), salt)
        self.ref = raw.copy()
        raw[self.lo:self.hi] = fill
        self.buf = raw
        self.a = raw[self.lo:self.hi].view(self.dtype)

    @property
    def ptr(self) -> int:
        return int(self.a.ctypes.data) if self.nbytes else int(self.buf.ctypes.data) + self.lo

    def check(self, what: str = "host output") -> None:
        ne = self.buf != self.ref
        ne[self.lo:self.hi] = False
        if ne.any():
            at = int(np.flatnonzero(ne)[0])
            where = f"{self.lo - at} B before the payload" if at < self.lo else \
                f"{at - self.hi} B past the payload's end"
            raise AssertionError(f"{what}: guard changed {where} ({int(ne.sum())} bytes in all; "
                                 f"{self.count} x {self.dtype.name})")


class DevInput:
    """A fenced device input: `values` (numpy) between two guards of GUARD bytes holding
    `guard` (a value of the same dtype), then `slack` bytes of `guard` too (the readable
    round-up some entry points document).  `.t` is the payload; `unchanged()` compares the whole
    allocation with its snapshot."""

    def __init__(self, values: np.ndarray, guard, slack: int = 0):
        import torch
        v = np.ascontiguousarray(values)
        self.dtype = v.dtype
        g = GUARD // v.dtype.itemsize
        s = -(-int(slack) // v.dtype.itemsize)
        whole = np.concatenate([np.full(g, guard, dtype=v.dtype), v.reshape(-1),
                                np.full(s + g, guard, dtype=v.dtype)])
        self.buf = torch.from_numpy(whole.view(np.uint8)).cuda()
        assert self.buf.data_ptr() % 256 == 0
        self.snap = self.buf.clone()
        self.t = self.buf[GUARD:GUARD + v.nbytes].view(getattr(torch, _TORCH[v.dtype.name]))

    @property
    def ptr(self) -> int:
        return int(self.t.data_ptr())

    def unchanged(self, what: str = "input") -> None:
        import torch
        if not torch.equal(self.buf, self.snap):
            at = int((self.buf != self.snap).nonzero()[0]) - GUARD
            raise AssertionError(f"{what}: the library wrote into a const input, first at payload byte {at}")


class HostInput:
    """DevInput over numpy memory (the const host arrays of the blocking entry points)."""

    def __init__(self, values: np.ndarray, guard):
        v = np.ascontiguousarray(values)
        g = GUARD // v.dtype.itemsize
        self.buf = np.concatenate([np.full(g, guard, dtype=v.dtype), v.reshape(-1),
                                   np.full(g, guard, dtype=v.dtype)])
        self.snap = self.buf.copy()
        self.a = self.buf[g:g + v.size]

    @property
    def ptr(self) -> int:
        return int(self.a.ctypes.data) if self.a.size else int(self.buf.ctypes.data) + GUARD

    def unchanged(self, what: str = "host input") -> None:
        if not (self.buf.view(np.uint8) == self.snap.view(np.uint8)).all():
            raise AssertionError(f"{what}: the library wrote into a const host input")


def check_all(*fences) -> None:
    """check() / unchanged() of every fence given (None entries skipped)."""
    for k, f in enumerate(fences):
        if f is None:
            continue
        if isinstance(f, (DevInput, HostInput)):
            f.unchanged(f"input #{k}")
        else:
            f.check(f"output #{k}")
