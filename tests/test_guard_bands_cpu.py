"""The guard-band helper (tests/guard_bands.py) catches what it claims: fake "kernels" written in torch on the CPU, each wrong in exactly one way, must trip
assert_outside_unchanged or the finiteness check -- with the right coordinates -- and a correct fake must pass.  These fakes ARE the subtly wrong kernels the GPU
file (tests/test_guard_bands_gpu.py) would fail on; nothing is broken on purpose on the device."""
import pytest
import torch

from tests import guard_bands as G

CPU = torch.device("cpu")
M, W, LD = 13, 24, 32


def _flip_one(backing, index):
    """Change one element of the allocation (flip its lowest bit through the integer view)."""
    G._as_int(backing)[index] ^= 1


def _operands(dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(3)
    a = torch.randn(M, W, generator=g).to(dtype)
    b = torch.randn(M, W, generator=g).to(dtype)
    av, _ = G.banded((M, W), LD, dtype, CPU, "in", data=a)
    bv, _ = G.banded((M, W), LD + 8, dtype, CPU, "in", data=b)
    out, backing = G.banded((M, W), LD, dtype, CPU, "out", seed=7)
    return a, b, av, bv, out, backing


def _offset(view, backing):
    return view.storage_offset() - backing.storage_offset()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.int64, torch.uint8])
def test_layout_of_a_banded_view(dtype):
    v, backing = G.banded((M, W), LD, dtype, CPU, "out", seed=1)
    off = _offset(v, backing)
    assert v.shape == (M, W) and v.stride() == (LD, 1) and v.data_ptr() % 16 == 0
    assert off >= G.MARGIN_ROWS * LD and backing.numel() - off - M * LD >= (G.MARGIN_ROWS - 1) * LD
    assert torch.unique(G._as_int(backing)).numel() > 8          # random words, not a constant
    v3, b3 = G.banded((5, 3, 8), 40, dtype, CPU, "out", seed=2)
    assert v3.shape == (5, 3, 8) and v3.stride() == (40, 8, 1)
    f, bf = G.banded_flat(299, dtype, CPU, "out", seed=3)
    assert f.shape == (299,) and _offset(f, bf) == G.MARGIN_FLAT and bf.numel() == 299 + 2 * G.MARGIN_FLAT and f.data_ptr() % 16 == 0


def test_input_poison_is_nan_outside_and_data_inside():
    a, _, av, _, _, _ = _operands()
    assert torch.equal(G.inside(av), a)
    base = av.as_strided((M, LD), (LD, 1), av.storage_offset())
    assert bool(torch.isnan(base[:, W:]).all())                                   # the right pad
    assert bool(torch.isnan(av.as_strided((1, LD), (LD, 1), av.storage_offset() - LD)).all())   # the row before
    assert bool(torch.isnan(av.as_strided((1, LD), (LD, 1), av.storage_offset() + M * LD)).all())   # row M
    bits = base[:, W:].view(torch.int16)
    assert bool((bits == 0x7FC0).all())
    x32, _ = G.banded((M, W), LD, torch.float32, CPU, "in", data=a.float())
    assert bool(torch.isnan(x32.as_strided((M, LD), (LD, 1), x32.storage_offset())[:, W:]).all())
    i8, b8 = G.banded((M, W), LD, torch.uint8, CPU, "in", data=torch.ones(M, W, dtype=torch.uint8))
    assert int(b8.sum()) == M * W                                                  # 8-bit data: no poison


def test_correct_fake_passes():
    a, b, av, bv, out, backing = _operands()
    snap = G.snapshot(backing)
    out.copy_((av.float() + bv.float()).to(torch.bfloat16))                        # reads and writes the logical rectangle only
    G.assert_outside_unchanged(backing, out, snap)
    ref = a.float() + b.float()
    G.assert_finite_where(out, ref)
    assert torch.equal(G.inside(out), ref.to(torch.bfloat16)) and G.inside(out).is_contiguous()
    assert G.inside(out).data_ptr() != out.data_ptr()


@pytest.mark.parametrize("name,row,col", [("right pad", 2, W), ("last pad column", M - 1, LD - 1), ("row M", M, 1), ("row before the view", -1, 3),
                                          ("far before", -G.MARGIN_ROWS, 0)])
def test_one_element_outside_the_view_is_caught_with_its_coordinates(name, row, col):
    _, _, av, bv, out, backing = _operands()
    snap = G.snapshot(backing)
    out.copy_((av.float() + bv.float()).to(torch.bfloat16))
    _flip_one(backing, _offset(out, backing) + row * LD + col)                     # the faulty store
    with pytest.raises(AssertionError, match=rf"1 element\(s\) changed outside the view, the first at \(row {row}, col {col}\)"):
        G.assert_outside_unchanged(backing, out, snap, name)


def test_last_element_of_the_backing_buffer_is_caught():
    _, _, av, bv, out, backing = _operands()
    snap = G.snapshot(backing)
    out.copy_((av.float() + bv.float()).to(torch.bfloat16))
    _flip_one(backing, backing.numel() - 1)
    rel = backing.numel() - 1 - _offset(out, backing)
    with pytest.raises(AssertionError, match=rf"\(row {rel // LD}, col {rel % LD}\)"):
        G.assert_outside_unchanged(backing, out, snap)
    assert rel // LD >= M + G.MARGIN_ROWS - 1 and rel % LD == LD - 1


def test_first_of_several_changes_is_reported_and_counted():
    _, _, _, _, out, backing = _operands()
    snap = G.snapshot(backing)
    off = _offset(out, backing)
    for r, c in ((4, W + 2), (1, W + 5), (M + 2, 0)):
        _flip_one(backing, off + r * LD + c)
    with pytest.raises(AssertionError, match=rf"3 element\(s\) changed outside the view, the first at \(row 1, col {W + 5}\)"):
        G.assert_outside_unchanged(backing, out, snap)


def test_rewriting_the_same_value_does_not_trip():
    _, _, av, bv, out, backing = _operands()
    snap = G.snapshot(backing)
    out.copy_((av.float() + bv.float()).to(torch.bfloat16))
    pad = out.as_strided((M, LD - W), (LD, 1), out.storage_offset() + W)
    pad.copy_(pad.clone())                                                         # a store of what was already there: the bits do not change
    i = _offset(out, backing) + M * LD
    backing[i] = backing[i].clone()
    G.assert_outside_unchanged(backing, out, snap)


def test_nan_words_in_the_random_fill_compare_equal_to_themselves():
    out, backing = G.banded((M, W), LD, torch.float32, CPU, "out", seed=5)
    backing[3] = float("nan")
    backing[_offset(out, backing) + W] = float("nan")
    snap = G.snapshot(backing)
    G.assert_outside_unchanged(backing, out, snap)
    backing[3] = -0.0
    snap = G.snapshot(backing)
    backing[3] = 0.0                                                               # -0.0 -> 0.0 is a change of bits
    with pytest.raises(AssertionError, match="changed outside the view"):
        G.assert_outside_unchanged(backing, out, snap)


def test_a_result_that_sums_one_pad_column_comes_out_non_finite():
    a, _, av, _, _, _ = _operands()
    ref = a.float().sum(1)
    good = av.float().sum(1)
    G.assert_finite_where(good, ref)
    wide = av.as_strided((M, W + 1), (LD, 1), av.storage_offset())                  # the faulty load: one column of padding
    leaked = (wide.float() * torch.cat([torch.ones(W), torch.zeros(1)])).sum(1)     # "masked" by a multiplication with zero
    assert not bool(torch.isfinite(leaked).any())
    with pytest.raises(AssertionError, match=r"13 non-finite result\(s\) where the reference is finite, the first at \(0,\)"):
        G.assert_finite_where(leaked, ref)
    rows = av.as_strided((M + 1, W), (LD, 1), av.storage_offset())                  # ... and one row past the last
    with pytest.raises(AssertionError, match="non-finite"):
        G.assert_finite_where(rows.float().sum(0), a.float().sum(0))


def test_a_three_dimensional_view_guards_the_pad_behind_the_packed_heads():
    T, H, D, st = 6, 3, 8, 40
    out, backing = G.banded((T, H, D), st, torch.bfloat16, CPU, "out", seed=9)
    snap = G.snapshot(backing)
    out.copy_(torch.ones(T, H, D, dtype=torch.bfloat16))
    G.assert_outside_unchanged(backing, out, snap)
    _flip_one(backing, _offset(out, backing) + 2 * st + H * D)
    with pytest.raises(AssertionError, match=rf"\(row 2, col {H * D}\) of a \[6, 24\] view with ld 40"):
        G.assert_outside_unchanged(backing, out, snap)


@pytest.mark.parametrize("where,rel", [("tail", 299), ("head", -1), ("end of the buffer", 299 + G.MARGIN_FLAT - 1)])
def test_flat_slice_guards_both_ends(where, rel):
    out, backing = G.banded_flat(299, torch.float32, CPU, "out", seed=4)
    snap = G.snapshot(backing)
    out.copy_(torch.arange(299, dtype=torch.float32))
    G.assert_outside_unchanged(backing, out, snap)
    _flip_one(backing, G.MARGIN_FLAT + rel)
    with pytest.raises(AssertionError, match=rf"the first at index {rel} of a slice of 299"):
        G.assert_outside_unchanged(backing, out, snap, where)


def test_in_place_view_keeps_the_other_heads():
    """An in-place op on heads [h0, h0 + nh) of a fused buffer: the view handed to assert_outside_unchanged is the slice of heads that may change."""
    T, H, D, st = 5, 6, 8, 56
    data = torch.randn(T, H, D).to(torch.bfloat16)
    x, backing = G.banded((T, H, D), st, torch.bfloat16, CPU, "out", data=data, seed=11)
    snap = G.snapshot(backing)
    mine = x[:, 2:4]
    mine.mul_(2)
    G.assert_outside_unchanged(backing, mine, snap)
    x[1, 4, 0] = 7.0                                                               # a head it was not given
    with pytest.raises(AssertionError, match="changed outside the view"):
        G.assert_outside_unchanged(backing, mine, snap)
