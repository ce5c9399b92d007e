"""GPU: J&F scoring on the device (csrc/maskmetrics.hip through rga3.hip.ops.mask_jf_counts and rga3.utils.metrics) against the reference's own results
(tests/golden/jf_cases.npz).  The arithmetic is integer, so every comparison is exact: the six counts are equal and F / J are == the reference's floats."""
import numpy as np
import pytest

from tests import jf_cases

pytestmark = pytest.mark.gpu


def dev_masks(c, dev):
    import torch

    return tuple(None if m is None else torch.from_numpy(m).to(dev) for m in (c.ann, c.seg, c.void))


def check_case(c, dev, convert=lambda t: t):
    """Counts through the op, J / F through the public function, both on `convert`ed device tensors."""
    from rga3.hip import ops
    from rga3.utils import metrics

    ann, seg, void = (None if m is None else convert(m) for m in dev_masks(c, dev))
    counts = ops.mask_jf_counts(ann, seg, void, radius=c.radius).cpu().numpy()
    print(c.name, c.shape, "r", c.radius, "counts", counts.tolist())
    assert counts.dtype == np.int64 and np.array_equal(counts, c.counts), (c.name, counts.tolist(), c.counts.tolist())
    J, F = metrics.mask_jf(ann, seg, void, bound_th=c.bound_th)
    if len(c.shape) == 2:
        assert isinstance(J, float) and isinstance(F, float)
    else:
        assert J.dtype == F.dtype == np.float64 and J.shape == F.shape == (c.shape[0],)
    assert np.array_equal(np.asarray(F), c.F) and np.array_equal(np.asarray(J), c.J), (c.name, F, c.F, J, c.J)
    assert np.array_equal(np.asarray(metrics.db_eval_boundary(ann, seg, void, bound_th=c.bound_th)), c.F)


@pytest.mark.parametrize("name", jf_cases.names())
def test_counts_and_scores_equal_the_reference(dev, name):
    """Every fixture case: word edges (widths 1..129 x heights 1..37), the disk at offsets on / past the circle for r = 1..64, frame borders, degenerate masks,
    void pixels, the default threshold."""
    check_case(jf_cases.case(name), dev)


def test_identical_masks_score_one_and_distant_masks_zero(dev):
    from rga3.utils import metrics

    c = jf_cases.case("degenerate")
    ann, seg, _ = dev_masks(c, dev)
    J, F = metrics.mask_jf(ann, seg, bound_th=c.bound_th)
    assert F[5] == 1.0 and J[5] == 1.0      # identical blobs
    assert F[6] == 0.0 and J[6] == 0.0      # disjoint, farther apart than the radius
    assert F[0] == 1.0 and J[0] == 1.0      # empty vs empty: the reference's conventions
    assert F[3] == 1.0 and J[3] == 1.0      # full vs full: a full mask has no boundary


def test_frames_do_not_see_each_other(dev):
    """The blob of the middle frame touches the top and bottom rows and sits between two checkerboards (every pixel a boundary pixel): its counts are those of
    the same frame scored alone."""
    from rga3.hip import ops

    c, alone = jf_cases.case("frames3"), jf_cases.case("frames3_middle_alone")
    ann, seg, _ = dev_masks(c, dev)
    both = ops.mask_jf_counts(ann, seg, radius=c.radius).cpu().numpy()
    mid = ops.mask_jf_counts(ann[1], seg[1], radius=c.radius).cpu().numpy()
    assert mid.shape == (1, 6) and np.array_equal(both[1], mid[0]) and np.array_equal(mid, alone.counts)
    no_wrap = jf_cases.case("row_end_no_wrap")
    a, s, _ = dev_masks(no_wrap, dev)
    got = ops.mask_jf_counts(a, s, radius=no_wrap.radius).cpu().numpy()[0]
    assert got[0] > 0 and got[1] > 0 and got[2] == 0 and got[3] == 0, got   # the last column of a row is not next to column 0 of the row below


@pytest.mark.parametrize("name", ["edge_37x129", "void", "frames3_middle_alone"])
def test_dtypes_and_layouts(dev, name):
    """uint8 masks with values {0, 1, 255} and non-contiguous views score as the bool masks do."""
    import torch

    c = jf_cases.case(name)

    def u8(t):
        v = t.to(torch.uint8)
        v[..., ::2] *= 255
        return v

    def strided(t):   # every other column of a twice-as-wide tensor
        wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
        wide[..., ::2] = t
        v = wide[..., ::2]
        assert not v.is_contiguous()
        return v

    check_case(c, dev, u8)
    check_case(c, dev, strided)
    check_case(c, dev, lambda t: strided(u8(t)).transpose(-1, -2).contiguous().transpose(-1, -2))   # column-major


def test_numpy_masks_are_uploaded(dev):
    from rga3.utils import metrics

    c = jf_cases.case("default_97x131")
    J, F = metrics.mask_jf(c.ann.astype(np.uint8) * 255, c.seg, bound_th=c.bound_th)
    assert np.array_equal(F, c.F) and np.array_equal(J, c.J)
    assert c.bound_th == 0.008 and jf_cases.case("default_270x480").radius == 5


def test_j_and_f_accumulator(dev):
    """Two sequences: J / F / J&F as evaluation/mevis_val_u/eval_mevis.py forms them from the reference's per-frame values."""
    from rga3.utils.metrics import JAndF

    seqs = [jf_cases.case("default_97x131"), jf_cases.case("frames3")]
    acc = JAndF()
    for c in seqs:
        ann, seg, _ = dev_masks(c, dev)
        acc.update(seg, ann, bound_th=c.bound_th)
    j, f = [c.J.mean() for c in seqs], [c.F.mean() for c in seqs]
    want = {"J": np.mean(j), "F": np.mean(f), "J&F": (np.mean(j) + np.mean(f)) / 2}
    assert acc.compute() == want, (acc.compute(), want)
    other = JAndF()
    other.load_sums(acc.sums())
    assert other.compute() == want


def test_rejected_input_leaves_the_op_usable(dev):
    import torch

    from rga3.hip import lib, ops

    c = jf_cases.case("edge_3x65")
    ann, seg, _ = dev_masks(c, dev)
    for bad in (lambda: ops.mask_jf_counts(ann, seg, radius=0), lambda: ops.mask_jf_counts(ann, seg, radius=65),
                lambda: ops.mask_jf_counts(ann, seg[:, :-1], radius=2), lambda: ops.mask_jf_counts(ann[:-1], seg, radius=2),
                lambda: ops.mask_jf_counts(ann.float(), seg.float(), radius=2), lambda: ops.mask_jf_counts(ann, seg, seg.float(), radius=2),
                lambda: ops.mask_jf_counts(ann[:0], seg[:0], radius=2)):
        with pytest.raises(lib.Rga3Error):
            bad()
    torch.cuda.synchronize()
    check_case(c, dev)
