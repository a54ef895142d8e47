"""tests/guarded.py has to detect what it claims before the GPU tests may lean on it: on CPU tensors, every kind of stray write is
reported, a payload filled end to end is not, and the torch shim forwards everything it does not serve itself."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import guarded  # noqa: E402


@pytest.fixture
def arena():
    return guarded.Arena("cpu")


def _raw(arena, t):
    return arena.record(t)


def test_layout_and_poison(arena):
    t = arena.alloc((3, 5), torch.float32)
    rec = _raw(arena, t)
    assert guarded.GUARD_BYTES == 65536 and guarded.GUARD_BYTES % 512 == 0
    assert t.data_ptr() % 512 == 0 and t.is_contiguous() and t.shape == (3, 5) and t.dtype == torch.float32
    assert rec.pay0 - rec.front0 == guarded.GUARD_BYTES and rec.rear1 - rec.pay1 == guarded.GUARD_BYTES
    assert rec.pay1 - rec.pay0 == 60                               # the rear guard starts at the first byte after the payload
    assert bool((rec.raw[rec.front0:rec.rear1] == 0xFF).all())
    assert bool(torch.isnan(t).all()) and guarded.all_poison(t)
    assert bool(torch.isnan(arena.alloc(4, torch.float16)).all()) and bool(torch.isnan(arena.alloc(4, torch.float64)).all())
    assert arena.alloc(4, torch.int32).tolist() == [-1] * 4 and arena.alloc(3, torch.uint8).tolist() == [255] * 3
    z = arena.alloc((2, 2), torch.int32, fill=0)
    assert z.tolist() == [[0, 0], [0, 0]]
    assert arena.alloc(3, torch.float32, fill=2.5).tolist() == [2.5] * 3
    arena.check()


def test_write_one_element_past_the_payload(arena):
    t = arena.alloc(7, torch.float32)
    rec = _raw(arena, t)
    rec.raw[rec.pay1:rec.pay1 + 4] = torch.tensor([0, 0, 128, 63], dtype=torch.uint8)       # 1.0f
    with pytest.raises(guarded.GuardError, match=r"rear guard.*guard byte 0 "):
        arena.check()


def test_write_one_element_before_the_payload(arena):
    arena.alloc(9, torch.float32, name="bystander")
    t = arena.alloc(7, torch.float32, name="victim")
    rec = _raw(arena, t)
    rec.raw[rec.pay0 - 4:rec.pay0] = 0
    with pytest.raises(guarded.GuardError, match=r"victim.*front guard.*4 bytes before the payload"):
        arena.check()


def test_write_at_the_last_guard_byte(arena):
    t = arena.alloc(5, torch.uint8)
    rec = _raw(arena, t)
    rec.raw[rec.rear1 - 4:rec.rear1] = 0
    with pytest.raises(guarded.GuardError, match=rf"rear guard.*guard byte {guarded.GUARD_BYTES - 4} "):
        arena.check()
    rec.raw[rec.rear1 - 4:rec.rear1] = 0xFF
    arena.check()
    rec.raw[rec.front0] = 1                                         # ... and the first one
    with pytest.raises(guarded.GuardError, match=r"front guard.*guard byte 0 "):
        arena.check()


def test_write_into_an_input_payload(arena):
    x = arena.input(np.arange(12, dtype=np.float32).reshape(3, 4), np.nan)
    assert x.tolist() == np.arange(12, dtype=np.float32).reshape(3, 4).tolist()
    arena.check()
    x[1, 2] = -6.0
    with pytest.raises(guarded.GuardError, match=r"input payload written, first at byte 2[4-7]$"):      # element 6
        arena.check()


def test_a_canonical_nan_in_a_guard_is_not_the_poison(arena):
    t = arena.alloc(4, torch.float32)
    rec = _raw(arena, t)
    rec.raw[rec.pay1:rec.pay1 + 4] = torch.from_numpy(np.array([0x7FC00000], dtype=np.uint32).view(np.uint8).copy())
    assert bool(torch.isnan(rec.raw[rec.pay1:rec.pay1 + 4].view(torch.float32)).all())
    with pytest.raises(guarded.GuardError, match="rear guard"):
        arena.check()
    # ... nor an input's NaN guard: the same value must come back byte for byte
    arena2 = guarded.Arena("cpu")
    x = arena2.input(np.ones(4, np.float32), np.nan)
    r2 = arena2.record(x)
    want = np.array([np.nan], np.float32).view(np.uint8)
    other = want.copy(); other[0] ^= 1                              # another NaN
    r2.raw[r2.pay0 - 4:r2.pay0] = torch.from_numpy(other)
    with pytest.raises(guarded.GuardError, match="front guard"):
        arena2.check()


def test_a_full_payload_is_silent(arena):
    for dtype, shape in ((torch.float32, (3, 5)), (torch.uint8, (7,)), (torch.float64, (2, 1, 3)), (torch.int32, (1,)), (torch.float16, (9,))):
        arena.alloc(shape, dtype).fill_(3)
    x = arena.input(np.full((5, 3), 7, np.uint8), 255)
    y = arena.input(np.linspace(-1, 1, 11).astype(np.float32), np.inf)
    ry = arena.record(y)
    assert bool(torch.isinf(ry.raw[ry.pay1:ry.rear1].view(torch.float32)).all()) and bool(torch.isinf(ry.raw[ry.front0:ry.pay0].view(torch.float32)).all())
    rx = arena.record(x)
    assert bool((rx.raw[rx.front0:rx.pay0] == 255).all())
    arena.check()
    t = arena.alloc(6, torch.float32)
    guarded.scribble(t, 0x5A)
    assert not guarded.all_poison(t)
    arena.check()


@pytest.mark.parametrize("elems", [1, 2, 3, 5])
def test_offset_view_base(arena, elems):
    t = arena.alloc((4, 6), torch.float32, fill=1.5)
    v = arena.offset_view(t, elems)
    assert v.data_ptr() % 512 == 4 * elems and v.data_ptr() % 16 == (4 * elems) % 16
    assert v.shape == t.shape and v.is_contiguous() and torch.equal(v, t)
    rec = arena.record(v)
    assert rec.pay0 - rec.front0 == guarded.GUARD_BYTES + 4 * elems and not rec.is_input
    rec.raw[rec.pay0 - 1] = 0                                       # the bytes the view skipped are guard
    with pytest.raises(guarded.GuardError, match="front guard"):
        arena.check()
    rec.raw[rec.pay0 - 1] = 0xFF
    x = arena.input(np.arange(8, dtype=np.float32), np.inf)
    xv = arena.offset_view(x, elems)
    rx = arena.record(xv)
    assert xv.data_ptr() % 16 == (4 * elems) % 16 and xv.tolist() == x.tolist() and rx.is_input
    assert bool(torch.isinf(rx.raw[rx.front0:rx.pay0].view(torch.float32)).all())
    arena.check()
    xv[0] = 9
    with pytest.raises(guarded.GuardError, match="input payload written"):
        arena.check()


def test_guarded_torch_forwards(arena):
    gt = guarded.GuardedTorch(torch, arena)
    assert gt.float32 is torch.float32 and gt.from_numpy is torch.from_numpy and gt.cuda is torch.cuda and gt.uint8 is torch.uint8
    assert gt.Tensor is torch.Tensor and gt.device("cpu") == torch.device("cpu")
    n0 = len(arena.records)
    c = gt.empty((2, 2), dtype=torch.float32, device="cpu")        # the CPU stays torch's own
    assert len(arena.records) == n0 and c.shape == (2, 2)
    assert gt.zeros(3).tolist() == [0, 0, 0] and gt.full((2,), 4).tolist() == [4, 4] and gt.empty_like(c).shape == (2, 2)
    assert len(arena.records) == n0


def test_guarded_torch_allocations(arena):
    gt = guarded.GuardedTorch(torch, arena)
    e = gt.empty((3, 5), dtype=torch.float32, device="cuda")        # any device but the CPU goes to the arena (here a CPU arena)
    assert e.shape == (3, 5) and e.dtype == torch.float32 and e.is_contiguous() and guarded.all_poison(e)
    assert arena.record(e).tensor is e
    assert gt.empty(7, dtype=torch.uint8, device=torch.device("cuda")).shape == (7,)
    assert gt.empty(2, 3, device="cuda").shape == (2, 3)
    z = gt.zeros((2, 3), dtype=torch.float64, device="cuda")
    assert z.dtype == torch.float64 and z.tolist() == [[0.0] * 3] * 2
    f = gt.full((4,), -7, dtype=torch.int32, device="cuda")
    assert f.tolist() == [-7] * 4
    like = gt.empty_like(z.to("meta").to(torch.float32))            # a tensor that lives on another device
    assert like.shape == (2, 3) and like.dtype == torch.float32 and guarded.all_poison(like)
    assert len(arena.records) == 6
    arena.check()
    e.view(-1)[14] = 1.0                                             # its last element: fine
    arena.check()
