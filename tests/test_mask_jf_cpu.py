"""CPU: the J&F fixture (tests/golden/jf_cases.npz) is pinned against a brute-force restatement that shares nothing with its generator's dilation stand-ins,
and the device-only entry points refuse host input loudly."""
import numpy as np
import pytest

from tests import jf_cases

SMALL = [n for n in jf_cases.names() if np.prod(jf_cases.case(n).shape[-2:]) <= 13000]


def boundary(m):
    """b = (m^E) | (m^S) | (m^SE), neighbours zero filled; last row m^E only, last column m^S only, bottom-right pixel 0."""
    h, w = m.shape
    p = np.zeros((h + 1, w + 1), bool)
    p[:h, :w] = m
    e, s, se = p[:h, 1:], p[1:, :w], p[1:, 1:]
    b = (m ^ e) | (m ^ s) | (m ^ se)
    b[-1, :] = m[-1, :] ^ e[-1, :]
    b[:, -1] = m[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def matched(b, other, r):
    """How many pixels of b have a pixel of `other` with dx^2 + dy^2 <= r^2."""
    p, q = np.argwhere(b).astype(np.int64), np.argwhere(other).astype(np.int64)
    if len(p) == 0 or len(q) == 0:
        return 0
    n = 0
    for i in range(0, len(p), 512):
        d = p[i:i + 512, None, :] - q[None, :, :]
        n += int(((d ** 2).sum(-1) <= r * r).any(1).sum())
    return n


def test_small_cases_cover_every_group():
    assert {n.split("_")[0] for n in SMALL} >= {"edge", "disk", "blob", "frames3", "row", "degenerate", "void", "default"}, SMALL


@pytest.mark.parametrize("name", SMALL)
def test_fixture_counts_equal_brute_force(name):
    c = jf_cases.case(name)
    h, w = c.shape[-2:]
    void = np.zeros(c.shape, bool) if c.void is None else c.void
    got = []
    for a, s, v in zip(c.ann.reshape(-1, h, w), c.seg.reshape(-1, h, w), void.reshape(-1, h, w)):
        a, s = a & ~v, s & ~v
        bs, ba = boundary(s), boundary(a)
        got.append([bs.sum(), ba.sum(), matched(bs, ba, c.radius), matched(ba, bs, c.radius), (s & a).sum(), (s | a).sum()])
    assert np.array_equal(np.asarray(got, np.int64), c.counts), (got, c.counts.tolist())


def test_fixture_radius_and_scores_follow_from_counts():
    """radius = bound_th or ceil(bound_th * diagonal); the stored F / J are the reference's expressions on the stored counts (rga3.utils.metrics restates them)."""
    from rga3.utils import metrics

    for name in jf_cases.names():
        c = jf_cases.case(name)
        assert metrics._jf_radius(c.bound_th, *c.shape[-2:]) == c.radius, name
        f = [metrics._f_from_counts(*(int(v) for v in row[:4])) for row in c.counts]
        j = [1.0 if row[5] == 0 else row[4] / row[5] for row in c.counts]
        assert np.array_equal(np.asarray(f, np.float64), np.atleast_1d(c.F)) and np.array_equal(np.asarray(j, np.float64), np.atleast_1d(c.J)), name


def test_cpu_tensors_are_rejected_loudly():
    import torch

    from rga3.hip import lib, ops

    m = torch.zeros(2, 8, 8, dtype=torch.bool)
    with pytest.raises(lib.Rga3Error):
        ops.mask_jf_counts(m, m, radius=2)


def test_non_integer_pixel_radius_is_a_value_error():
    from rga3.utils import metrics

    m = np.zeros((8, 8), bool)
    with pytest.raises(ValueError):
        metrics.mask_jf(m, m, bound_th=2.5)
    with pytest.raises(ValueError):
        metrics.db_eval_boundary(m, m, bound_th=1.5)


def test_library_rejects_bad_arguments_without_a_device():
    """The argument checks come before anything touches a device: radius 0 / 65, null pointers, an empty shape and a short workspace return the library's negative
    code with the message set, and the workspace query matches the two packed boundary maps."""
    from rga3.hip import lib

    L = lib.load()
    assert L.rga3_mask_jf_ws_bytes(3, 5, 65) == 2 * 3 * 5 * 2 * 8 and L.rga3_mask_jf_ws_bytes(1, 1, 64) == 16
    for shape in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (65536, 4, 4)):
        assert L.rga3_mask_jf_ws_bytes(*shape) < 0
        assert "mask_jf" in lib.last_error()
    ok = dict(seg=8, ann=8, vd=0, counts=8, ws=8, ws_bytes=1 << 20, frames=2, h=4, w=4, radius=3)   # non-null dummies: every call below must fail before a launch
    for bad in (dict(radius=0), dict(radius=65), dict(seg=0), dict(ann=0), dict(counts=0), dict(ws=0), dict(frames=0), dict(h=0), dict(w=0), dict(ws_bytes=63), dict(ws=4)):
        a = dict(ok, **bad)
        rc = L.rga3_mask_jf_counts(a["seg"], a["ann"], a["vd"], a["counts"], a["ws"], a["ws_bytes"], a["frames"], a["h"], a["w"], a["radius"], None)
        assert rc < 0 and "mask_jf_counts" in lib.last_error(), (bad, rc, lib.last_error())
