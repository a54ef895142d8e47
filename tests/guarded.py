"""Guarded, poisoned device buffers for the buffer-contract tests (tests/test_gpu_buffer_contract.py).

A plain helper module: `from tests import guarded`.  An Arena hands out tensors that sit between two guard bands and start out
as poison, and a GuardedTorch stands in for the `torch` name of mscnn_amd.hipapi so that every buffer a wrapper allocates comes
from the arena:

    arena = guarded.Arena("cuda")
    monkeypatch.setattr(hipapi, "torch", guarded.GuardedTorch(torch, arena))
    x = arena.input(x_np, np.nan)
    y = hipapi.relu(x)
    torch.cuda.synchronize()
    arena.check()

Layout of one allocation (byte offsets from a 512-byte boundary):

    [ front guard: GUARD_BYTES (+ lead) ][ payload ][ rear guard: GUARD_BYTES ]

The rear guard starts at the first byte after the payload, without rounding.  `lead` is 0 except for offset_view(), which moves the
payload's base off the 512-byte boundary; the bytes it skips belong to the front guard.
"""
import numpy as np
import torch as _torch

GUARD_BYTES = 65536          # a multiple of 512: the payload keeps the alignment torch would have given it
POISON = 0xFF                # NaN as fp32 / fp16 / fp64, -1 as int32, 255 as uint8
ALIGN = 512

_NP_OF = {_torch.float32: np.float32, _torch.float64: np.float64, _torch.float16: np.float16, _torch.int32: np.int32,
          _torch.int64: np.int64, _torch.uint8: np.uint8, _torch.int8: np.int8, _torch.int16: np.int16, _torch.bool: np.bool_}


class GuardError(AssertionError):
    pass


class _Record:
    """One allocation: raw = the whole uint8 buffer, [front0, pay0) front guard, [pay0, pay1) payload, [pay1, rear1) rear guard."""

    def __init__(self, name, raw, front0, pay0, pay1, rear1, pattern, tensor, snapshot):
        self.name, self.raw, self.front0, self.pay0, self.pay1, self.rear1 = name, raw, front0, pay0, pay1, rear1
        self.pattern = pattern        # bytes of one guard element; the guards hold it end to end
        self.tensor = tensor          # the payload as the caller sees it
        self.snapshot = snapshot      # input(): the uploaded payload bytes (numpy uint8), else None

    @property
    def is_input(self):
        return self.snapshot is not None


class Arena:
    def __init__(self, device):
        self.device = _torch.device(device)
        self.records = []
        self._expected = {}

    # ---- allocation
    def _carve(self, nbytes, lead, pattern, name):
        """A raw buffer with the payload `lead` bytes past a 512-byte boundary; guards filled with `pattern` end to end."""
        assert GUARD_BYTES % len(pattern) == 0 and lead % len(pattern) == 0 and nbytes % len(pattern) == 0, (nbytes, lead, pattern)
        raw = _torch.empty(ALIGN + GUARD_BYTES + lead + nbytes + GUARD_BYTES, dtype=_torch.uint8, device=self.device)
        front0 = (-raw.data_ptr()) % ALIGN
        pay0 = front0 + GUARD_BYTES + lead
        pay1 = pay0 + nbytes
        rear1 = pay1 + GUARD_BYTES
        raw[front0:pay0] = self._pattern(pattern, pay0 - front0)
        raw[pay1:rear1] = self._pattern(pattern, GUARD_BYTES)
        rec = _Record(name or f"alloc#{len(self.records)}", raw, front0, pay0, pay1, rear1, pattern, None, None)
        self.records.append(rec)
        return rec

    def _pattern(self, pattern, length):
        """`length` bytes of `pattern` repeated, on the arena's device (cached: check() compares the guards with it)."""
        key = (pattern, length)
        if key not in self._expected:
            reps = np.frombuffer(pattern * (length // len(pattern)), dtype=np.uint8).copy()
            self._expected[key] = _torch.from_numpy(reps).to(self.device)
        return self._expected[key]

    @staticmethod
    def _shape(shape):
        if isinstance(shape, (int, np.integer)):
            return (int(shape),)
        return tuple(int(s) for s in shape)

    def _view(self, rec, shape, dtype):
        return rec.raw[rec.pay0:rec.pay1].view(dtype).view(shape)

    def alloc(self, shape, dtype=_torch.float32, fill=None, name=None, _lead=0):
        """A contiguous tensor between guards of 0xFF bytes.  fill None: the payload is 0xFF bytes too; otherwise that value."""
        shape = self._shape(shape)
        itemsize = _torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        rec = self._carve(nbytes, _lead, bytes([POISON]), name)
        rec.raw[rec.pay0:rec.pay1] = POISON
        rec.tensor = self._view(rec, shape, dtype)
        if fill is not None:
            rec.tensor.fill_(fill)
        return rec.tensor

    def input(self, np_array, guard_value, name=None, _lead=0):
        """Upload np_array between guards that hold guard_value in the array's dtype; check() also proves it was not written."""
        a = np.ascontiguousarray(np_array)
        pattern = np.array([guard_value], dtype=a.dtype).tobytes()
        rec = self._carve(a.nbytes, _lead, pattern, name or f"input#{len(self.records)}")
        rec.snapshot = np.frombuffer(a.tobytes(), dtype=np.uint8).copy()
        if a.nbytes:
            rec.raw[rec.pay0:rec.pay1] = _torch.from_numpy(rec.snapshot.copy()).to(self.device)
        dtype = next(t for t, n in _NP_OF.items() if np.dtype(n) == a.dtype)
        rec.tensor = self._view(rec, a.shape, dtype)
        return rec.tensor

    def record(self, t):
        """The allocation whose payload starts where t starts."""
        for rec in self.records:
            if rec.tensor is not None and rec.tensor.data_ptr() == t.data_ptr() and rec.pay1 > rec.pay0:
                return rec
        raise KeyError("tensor is not the start of a guarded allocation")

    def offset_view(self, t, elems):
        """A copy of the guarded tensor t in an allocation of its own whose base lies `elems` elements past a 512-byte boundary,
        guards right up against both ends.  It inherits t's kind: an input() stays an input with the same guard value."""
        rec = self.record(t)
        lead = elems * t.element_size()
        if rec.is_input:
            host = rec.snapshot.view(_NP_OF[t.dtype]).reshape(tuple(t.shape))
            guard = np.frombuffer(rec.pattern, dtype=_NP_OF[t.dtype])[0]
            v = self.input(host, guard, name=rec.name + f"+{elems}", _lead=lead)
        else:
            v = self.alloc(tuple(t.shape), t.dtype, name=rec.name + f"+{elems}", _lead=lead)
            v.copy_(t)
        assert v.data_ptr() % ALIGN == lead % ALIGN
        return v

    # ---- the check
    def check(self):
        """Every guard byte unchanged, every input() payload byte-identical to its upload."""
        for rec in self.records:
            for side, lo, hi in (("front", rec.front0, rec.pay0), ("rear", rec.pay1, rec.rear1)):
                got = rec.raw[lo:hi]
                want = self._pattern(rec.pattern, hi - lo)
                if not _torch.equal(got, want):
                    first = int(_torch.nonzero(got != want)[0, 0])
                    where = f"{hi - lo - first} bytes before the payload" if side == "front" else f"{first} bytes past its end"
                    raise GuardError(f"{rec.name} {tuple(rec.tensor.shape)} {rec.tensor.dtype}: {side} guard overwritten, first at guard byte "
                                     f"{first} ({where})")
            if rec.is_input:
                got = rec.raw[rec.pay0:rec.pay1].cpu().numpy()
                if not np.array_equal(got, rec.snapshot):
                    first = int(np.nonzero(got != rec.snapshot)[0][0])
                    raise GuardError(f"{rec.name} {tuple(rec.tensor.shape)} {rec.tensor.dtype}: input payload written, first at byte {first}")


def scribble(t, byte):
    """Every byte of the contiguous tensor t = byte (garbage a workspace may hold between two calls)."""
    t.view(-1).view(_torch.uint8).fill_(byte)


def all_poison(t):
    """True where the contiguous tensor t still holds nothing but the 0xFF bytes it was born with."""
    return bool((t.reshape(-1).view(_torch.uint8) == POISON).all())


class GuardedTorch:
    """`torch` with empty / empty_like / zeros / full on a device other than the CPU served by an Arena; everything else is torch's."""

    def __init__(self, real_torch, arena):
        self._torch = real_torch
        self._arena = arena

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def _on_device(self, device):
        return device is not None and self._torch.device(device).type != "cpu"

    @staticmethod
    def _size(size):
        return size[0] if len(size) == 1 and not isinstance(size[0], (int, np.integer)) else size

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._on_device(device):
            return self._torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._arena.alloc(self._size(size), dtype or self._torch.get_default_dtype())

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._on_device(device):
            return self._torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._arena.alloc(self._size(size), dtype or self._torch.get_default_dtype(), fill=0)

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._on_device(device):
            return self._torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = self._torch.get_default_dtype() if isinstance(fill_value, float) else self._torch.int64
        return self._arena.alloc(size, dtype, fill=fill_value)

    def empty_like(self, t, dtype=None, device=None, **kw):
        device = t.device if device is None else device
        if not self._on_device(device):
            return self._torch.empty_like(t, dtype=dtype, device=device, **kw)
        return self._arena.alloc(tuple(t.shape), dtype or t.dtype)
