"""CPU: the host halves of STOM's device route (rga3/model/STOM.py; kernels in csrc/stom.hip) against the numpy path they restate -- Pillow's compositing in integers,
the span table of the closing's structuring element, the half-width table of the circle, the gather form of the overlay shift -- and the argument refusals of the
device route, all of which are raised before any launch and so are reachable without a GPU.  Every comparison is equality."""
import numpy as np
import pytest
import torch

from rga3.hip.lib import Rga3Error
from rga3.model import STOM as ST


def test_pil_over_equals_pillow_for_every_triple():
    """alpha_composite over an opaque base, then convert("RGB"): all 256^3 (base, overlay, alpha) triples, one 256 x 256 image per alpha."""
    from PIL import Image

    base, over = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    b3 = np.ascontiguousarray(np.stack([base, base, base], -1))
    for a in range(256):
        ov = np.ascontiguousarray(np.stack([over, over, over, np.full_like(over, a)], -1))
        want = np.array(Image.alpha_composite(Image.fromarray(b3, "RGB").convert("RGBA"), Image.fromarray(ov, "RGBA")).convert("RGB"))
        got = ST.pil_over(base, over, np.uint8(a))
        assert np.array_equal(got, want[..., 0]) and np.array_equal(got, want[..., 2]), a
    rng = np.random.default_rng(0)
    f = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    o = rng.integers(0, 256, (9, 13, 4), dtype=np.uint8)
    o[::2, ::3, 3] = 0
    assert np.array_equal(ST.composite_int(f, o), ST.composite(f, o))


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 10, 32, 72])
def test_span_table_rebuilds_the_ellipse(k):
    sp = ST.ellipse_spans(k)
    ker = ST.ellipse_kernel(k)
    assert sp.dtype == np.uint8 and sp.shape == (max(k, 1), 2)
    again = np.zeros_like(ker)
    for i, (lo, hi) in enumerate(sp):
        again[i, lo:hi + 1] = 1
    assert np.array_equal(again, ker)
    anchor = k // 2
    assert (sp[:, 0] <= anchor).all() and (sp[:, 1] >= anchor).all()      # every span holds the anchor column: what the word kernel assumes
    assert ST.ellipse_spans(k) is not sp and np.array_equal(ST.ellipse_spans(k), sp)


def circle_from_table(shape_hw, cx, cy, r):
    hw = ST.circle_half_widths(r).astype(np.int64)
    y, x = np.mgrid[0:shape_hw[0], 0:shape_hw[1]]
    ady, adx = np.abs(y - cy), np.abs(x - cx)
    return ((ady <= r) & (adx <= hw[np.minimum(ady, r)])).astype(np.uint8) * 255


@pytest.mark.parametrize("r", [0, 1, 2, 3, 7, 24, 54])
def test_half_width_table_rebuilds_the_circle(r):
    hw = ST.circle_half_widths(r)
    assert hw.dtype == np.uint8 and hw.shape == (r + 1,) and hw[0] == r and (hw <= r).all()
    h, w = 2 * r + 9, 2 * r + 14
    centres = [(w // 2, h // 2), (0, h // 2), (w - 1, h // 2), (w // 2, 0), (w // 2, h - 1), (0, 0), (w - 1, h - 1), (r // 2, h - 1 - r // 2), (w - 1 - r // 3, r // 3)]
    for cx, cy in centres:
        assert np.array_equal(circle_from_table((h, w), cx, cy, r), ST.filled_circle((h, w), cx, cy, r)), (cx, cy)


def overlay(h, w, seed, density=0.5):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    src[rng.random((h, w)) > density, 3] = 0
    return src


FLOWS = [(0.0, 0.0), (-0.5, -0.5), (-0.25, 0.75), (0.75, -0.25), (-0.999, 0.0), (0.0, -0.999), (-1.0, -1.0), (-1.5, -2.5), (3.25, 2.875), (-3.625, 4.5),
         (-7.125, -0.125), (18.5, 0.0), (0.0, 40.0), (-31.0, -5.0), (-30.5, -21.5), (30.5, 21.5), (1e-30, -1e-30), (1e12, 0.0), (0.0, -1e15),
         (float(np.float32(-2.3)), float(np.float32(1.7)))]


@pytest.mark.parametrize("dx,dy", FLOWS)
def test_gather_rule_equals_the_scatter(dx, dy):
    """Fractional negative flows collide at the left / top border ((-1, 1) truncates to 0: the larger source wins), positive ones do not; whole-frame shifts
    leave nothing.  Dense and sparse overlays, so that the winner of a collision is sometimes transparent."""
    for seed, density in ((1, 1.0), (2, 0.5), (3, 0.1)):
        src = overlay(22, 31, seed, density)
        want = ST.shift_overlay(src, (22, 31), dx, dy)
        assert np.array_equal(ST.shift_overlay_gather(src, (22, 31), dx, dy), want), (dx, dy, seed)
    if abs(dx) >= 31 or abs(dy) >= 22:
        assert not want.any()


def test_gather_collision_takes_the_larger_source():
    src = np.zeros((4, 5, 4), np.uint8)
    src[0, 0] = (10, 0, 0, 255)
    src[0, 1] = (20, 0, 0, 255)
    src[1, 0] = (30, 0, 0, 255)
    src[1, 1] = (40, 0, 0, 255)
    got = ST.shift_overlay_gather(src, (4, 5), -0.5, -0.5)      # all four land on (0, 0)
    assert got[0, 0, 0] == 40 and np.count_nonzero(got[..., 3]) == 1
    assert np.array_equal(got, ST.shift_overlay(src, (4, 5), -0.5, -0.5))
    src[1, 1, 3] = 0                                            # a transparent pixel is no writer
    assert ST.shift_overlay_gather(src, (4, 5), -0.5, -0.5)[0, 0, 0] == 30


def good_args(T=3, H=30, W=40, N=8):
    return dict(frames=torch.zeros((T, H, W, 3), dtype=torch.uint8), src_frame_vip=torch.zeros((H, W, 4), dtype=torch.uint8), vip_frame_idx=0,
                tracks=torch.zeros((1, T, N, 2)), visibility=torch.ones((1, T, N), dtype=torch.bool))


def refused(shape, why, **change):
    a = good_args()
    a.update(change)
    with pytest.raises(Rga3Error, match=why):
        ST.STOM().propagate_in_video(a["frames"], a["src_frame_vip"], a["vip_frame_idx"], shape=shape, tracks=a["tracks"], visibility=a["visibility"])


@pytest.mark.parametrize("shape", ["rectangle", "mask"])
def test_device_route_refuses_bad_arguments(shape):
    """Each refusal for its own reason: the device check comes last, so the message tells which check fired."""
    g = good_args()
    refused(shape, "no CPU fallback")                                                                 # everything right but on the CPU
    refused(shape, "no CPU fallback", src_frame_vip=np.zeros((30, 40, 4), np.uint8))                  # a numpy overlay is fine, CPU frames are not
    refused(shape, "frames are uint8", frames=g["frames"].float())
    refused(shape, "frames are uint8", frames=g["frames"].to(torch.int8))
    refused(shape, "frames are uint8", frames=g["frames"][..., :2])
    refused(shape, "frames must be contiguous", frames=torch.zeros((3, 30, 80, 3), dtype=torch.uint8)[:, :, ::2])
    refused(shape, "frames must be contiguous", frames=torch.zeros((3, 40, 30, 3), dtype=torch.uint8).transpose(1, 2))
    refused(shape, "overlay", src_frame_vip=g["src_frame_vip"].to(torch.int32))
    refused(shape, "overlay", src_frame_vip=np.zeros((30, 40, 4), np.float32))
    refused(shape, "overlay", src_frame_vip=torch.zeros((30, 41, 4), dtype=torch.uint8))
    refused(shape, "overlay", src_frame_vip=torch.zeros((30, 40, 8), dtype=torch.uint8)[..., ::2])
    refused(shape, "tracks are float32", tracks=g["tracks"].double())
    refused(shape, "tracks are float32", tracks=g["tracks"].half())
    refused(shape, "tracks are float32", tracks=g["tracks"].numpy())
    refused(shape, "tracks are float32", tracks=torch.zeros((1, 4, 8, 2)))
    refused(shape, "visibility is bool", visibility=g["visibility"].to(torch.uint8))
    refused(shape, "visibility is bool", visibility=g["visibility"].float())
    refused(shape, "visibility is bool", visibility=torch.ones((1, 3, 7), dtype=torch.bool))
    refused(shape, "tracks and visibility must be contiguous", tracks=torch.zeros((1, 3, 8, 4))[..., ::2])
    refused(shape, "vip_frame_idx", vip_frame_idx=3)
    refused(shape, "vip_frame_idx", vip_frame_idx=-1)
    n = ST.MAX_POINTS + 1
    refused(shape, "tracked points", tracks=torch.zeros((1, 3, n, 2)), visibility=torch.ones((1, 3, n), dtype=torch.bool))


def test_limits_are_refused_for_their_own_reason():
    """N over the limit and k over the limit are refused as such (not merely because the tensors are on the CPU), and the library refuses them too."""
    from rga3.hip import lib

    assert ST.MAX_POINTS == 16384 and ST.MAX_KERNEL == 128
    n = ST.MAX_POINTS + 1
    with pytest.raises(Rga3Error, match="tracked points"):
        ST.STOM().propagate_in_video(torch.zeros((3, 30, 40, 3), dtype=torch.uint8), torch.zeros((30, 40, 4), dtype=torch.uint8), 0, tracks=torch.zeros((1, 3, n, 2)),
                                     visibility=torch.ones((1, 3, n), dtype=torch.bool))
    side = 15 * (ST.MAX_KERNEL + 1)       # min(H, W) // 15 = 129
    big = dict(frames=torch.zeros((2, side, side + 1, 3), dtype=torch.uint8), src_frame_vip=torch.zeros((side, side + 1, 4), dtype=torch.uint8))
    with pytest.raises(Rga3Error, match="closing kernel of 129"):
        ST.STOM().propagate_in_video(big["frames"], big["src_frame_vip"], 0, shape="mask", tracks=torch.zeros((1, 2, 8, 2)), visibility=torch.ones((1, 2, 8), dtype=torch.bool))
    with pytest.raises(Rga3Error, match="no CPU fallback"):     # the flow route has no closing: the same frames get as far as the device check
        ST.STOM().propagate_in_video(big["frames"], big["src_frame_vip"], 0, tracks=torch.zeros((1, 2, 8, 2)), visibility=torch.ones((1, 2, 8), dtype=torch.bool))

    L = lib.load()
    assert L.rga3_stom_ws_bytes(3, 5, 65) == (1 + 4 * 3 + 2 * 3 * 5 * 2) * 8
    for bad in ((0, 5, 5), (3, 0, 5), (3, 5, 0), (65536, 5, 5), (1, 1 << 16, 1 << 15)):
        assert L.rga3_stom_ws_bytes(*bad) < 0 and "stom_ws_bytes" in lib.last_error()
    # host-side refusals of the entry points come before any device call: dummy non-null pointers are never dereferenced
    buf = np.zeros(512, np.uint8)
    p = buf.ctypes.data
    assert L.rga3_stom_flow(p, p, p, 3, ST.MAX_POINTS + 1, 0, None) < 0 and "points" in lib.last_error()
    assert L.rga3_stom_flow(p, p, p, 3, 8, 3, None) < 0 and "vip_frame_idx" in lib.last_error()
    assert L.rga3_stom_shift_composite(p, p, p, p, 3, 5, 5, 0, None) < 0 and "in-place" in lib.last_error()
    assert L.rga3_stom_mask_composite(p, p, p, p, p + 8, p + 16, 1 << 20, 3, 5, 5, 8, 0, p, ST.MAX_KERNEL + 1, p, 0, None) < 0 and "structuring element" in lib.last_error()
    assert L.rga3_stom_mask_composite(p, p, p, p, p + 8, p + 16, 8, 3, 5, 5, 8, 0, p, 0, p, 0, None) < 0 and "workspace" in lib.last_error()
