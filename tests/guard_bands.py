"""Guard bands for kernel tests: operands and outputs as views in the middle of one larger, poisoned allocation (no tests in this module).

The library works on plain pointers + leading dimensions, in place on slices of fused buffers.  A store past the logical rectangle lands in somebody else's
memory, a load of the padding may leak into the result; neither shows when every operand is contiguous and exactly sized.  Here

  * ``banded(..., kind="in")`` surrounds the caller's data with NaN (a leak turns the result non-finite, whatever it is multiplied with);
  * ``banded(..., kind="out")`` fills the whole allocation with seeded random words (a kernel may well write zeros), ``snapshot`` keeps a copy and
    ``assert_outside_unchanged`` compares every bit outside the view afterwards, reporting the first changed (row, col) relative to the view.

The margins (MARGIN_ROWS rows of ``ld`` before and after the view, MARGIN_FLAT elements around a flat slice) are larger than any tile of the library, so even a
kernel that wrote a whole ragged tile would stay inside the allocation: a wrong kernel fails the comparison, it cannot fault.
"""
import math

import torch

MARGIN_ROWS = 520      # > the tallest tile (256 rows) and any 16-row workgroup rounding, twice over
MARGIN_FLAT = 8192     # elements before and after a flat slice

_INT_OF_SIZE = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _as_int(t):
    """The same memory through an integer dtype of the same width: NaN compares equal to itself, -0.0 differs from 0.0."""
    return t if not t.dtype.is_floating_point else t.view(_INT_OF_SIZE[t.element_size()])


def _fill(backing, kind, seed):
    if kind == "in":
        if backing.dtype.is_floating_point:
            backing.fill_(float("nan"))      # bf16 0x7FC0, f32 0x7FC00000
        else:
            backing.zero_()                  # 8-bit and integer data carry no poison
    elif kind == "out":
        it = _INT_OF_SIZE[backing.element_size()]
        bits = min(8 * backing.element_size(), 63) - 1
        g = torch.Generator().manual_seed(seed)
        words = torch.randint(-(1 << bits), 1 << bits, (backing.numel(),), generator=g, dtype=torch.int64).to(it)
        _as_int(backing).copy_(words.to(backing.device))
    else:
        raise ValueError(kind)


def banded(shape, ld, dtype, device, kind, data=None, seed=0, align=16):
    """(view, backing): a [rows, width] view with row stride ``ld`` -- or a [tokens, heads, D] view with token stride ``ld`` and packed heads -- in the middle of one
    1-D allocation: MARGIN_ROWS rows of ``ld`` before the first and after the last logical row, ``ld - width`` pad elements to the right of every row, the view's
    first element ``align`` bytes aligned.  kind "in": everything outside the logical rectangle is NaN; kind "out": the whole allocation holds seeded random words.
    ``data`` (same shape) is copied into the view; kind "in" requires it."""
    shape = tuple(int(s) for s in shape)
    assert len(shape) in (2, 3)
    rows, width = shape[0], int(math.prod(shape[1:]))
    ld = int(ld)
    assert ld >= width > 0 and rows > 0
    esz = torch.empty((), dtype=dtype).element_size()
    q = max(1, align // esz)
    off = (MARGIN_ROWS * ld + q - 1) // q * q
    backing = torch.empty(off + (rows + MARGIN_ROWS) * ld, dtype=dtype, device=device)
    assert backing.data_ptr() % align == 0
    _fill(backing, kind, seed)
    strides = (ld, 1) if len(shape) == 2 else (ld, shape[2], 1)
    view = backing.as_strided(shape, strides, off)
    assert view.data_ptr() % align == 0
    if data is not None:
        assert tuple(data.shape) == shape, (tuple(data.shape), shape)
        view.copy_(data.to(device=device, dtype=dtype))
    else:
        assert kind == "out", "an input view needs its data"
    return view, backing


def banded_flat(n, dtype, device, kind, data=None, seed=0, align=16):
    """(view, backing) for flat and per-row statistic outputs (and their inputs): a length-``n`` slice of a longer 1-D allocation, MARGIN_FLAT elements guarding
    each end, the slice ``align`` bytes aligned."""
    n = int(n)
    backing = torch.empty(n + 2 * MARGIN_FLAT, dtype=dtype, device=device)
    assert backing.data_ptr() % align == 0 and (MARGIN_FLAT * backing.element_size()) % align == 0
    _fill(backing, kind, seed)
    view = backing[MARGIN_FLAT:MARGIN_FLAT + n]
    if data is not None:
        assert data.numel() == n
        view.copy_(data.reshape(-1).to(device=device, dtype=dtype))
    else:
        assert kind == "out", "an input slice needs its data"
    return view, backing


def snapshot(backing):
    return backing.clone()


def inside(view):
    """The logical rectangle as a contiguous tensor of its own."""
    return view.clone(memory_format=torch.contiguous_format)


def assert_outside_unchanged(backing, view, snap, what=""):
    """Every element of ``backing`` outside ``view`` still holds the bits of ``snap``.  On failure: the first changed (row, col) relative to the view (row < 0: before
    the view, row >= rows: after it, col >= width: the pad to the right of a row; for a flat slice the index relative to its first element)."""
    assert backing.dim() == 1 and snap.shape == backing.shape and snap.dtype == backing.dtype
    off = view.storage_offset() - backing.storage_offset()
    changed = _as_int(backing) != _as_int(snap)
    changed.as_strided(tuple(view.shape), tuple(view.stride()), off).fill_(False)
    if not bool(changed.any()):
        return
    n = int(changed.sum())
    i = int(changed.nonzero()[0, 0])
    if view.dim() == 1:
        where = f"index {i - off} of a slice of {view.shape[0]}"
    else:
        ld = view.stride(0)
        row = (i - off) // ld      # floor: elements before the view get negative rows
        col = (i - off) - row * ld
        where = f"(row {row}, col {col}) of a [{view.shape[0]}, {int(math.prod(view.shape[1:]))}] view with ld {ld}"
    raise AssertionError(f"{what}: {n} element(s) changed outside the view, the first at {where}".lstrip(": "))


def assert_finite_where(out, ref, what=""):
    """``out`` is finite wherever ``ref`` is: NaN padding that reaches a result shows here, however small its weight."""
    out, ref = out.float().cpu(), ref.float().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    bad = ~torch.isfinite(out) & torch.isfinite(ref)
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} non-finite result(s) where the reference is finite, the first at {idx}".lstrip(": "))
