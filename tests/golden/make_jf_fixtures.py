"""Generates tests/golden/jf_cases.npz: J&F scoring cases for rga3.utils.metrics.mask_jf / rga3.hip.ops.mask_jf_counts, scored by the REFERENCE's own
/root/reference/evaluation/revos/metrics.py (db_eval_iou, db_eval_boundary, f_measure, _seg2bmap), imported and run unmodified.

That module needs two calls from libraries this container does not have; they are RESTATED here and are therefore NOT pinned by the reference:
  * cv2.dilate(src, kernel)        -> scipy.ndimage.binary_dilation(src, structure=kernel) (centred anchor, nothing outside the image: OpenCV's default border for
                                      a dilation), as uint8;
  * skimage.morphology.disk(r)     -> X^2 + Y^2 <= r^2 over arange(-r, r + 1), as uint8.
tests/test_mask_jf_cpu.py pins the stored counts against a brute-force nearest-boundary count that shares nothing with either stand-in.

Per case `name`: name.ann / name.seg / name.void (np.packbits of the bool masks; void may be absent), name.shape ([T, h, w] or [h, w]), name.bound_th, name.radius,
name.counts (int64 [T, 6] = n_fg, n_gt, fg_match, gt_match, inter, union -- the boundary counts through the reference's _seg2bmap and the same dilation, mirroring
f_measure:117-133; inter / union with the expressions of db_eval_iou:66-67), name.F (the reference's db_eval_boundary), name.J (its db_eval_iou).
No program text of the reference is stored.
    python tests/golden/make_jf_fixtures.py"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))


def _disk(radius):
    r = int(radius)
    L = np.arange(-r, r + 1)
    X, Y = np.meshgrid(L, L)
    return (X ** 2 + Y ** 2 <= r ** 2).astype(np.uint8)


def _dilate(src, kernel):
    return scipy.ndimage.binary_dilation(src.astype(bool), structure=kernel.astype(bool)).astype(np.uint8)


sys.modules.setdefault("cv2", types.SimpleNamespace(dilate=_dilate))
_morph = types.SimpleNamespace(disk=_disk)
sys.modules.setdefault("skimage", types.SimpleNamespace(morphology=_morph))
sys.modules.setdefault("skimage.morphology", _morph)
_spec = importlib.util.spec_from_file_location("reference_revos_metrics", "/root/reference/evaluation/revos/metrics.py")
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)  # the reference

OUT = {}
NAMES = []


def add(name, ann, seg, void=None, bound_th=0.008):
    ann, seg = np.asarray(ann, bool), np.asarray(seg, bool)
    void = None if void is None else np.asarray(void, bool)
    assert ann.shape == seg.shape and ann.ndim in (2, 3) and name not in NAMES
    h, w = ann.shape[-2:]
    radius = bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((h, w)))
    counts = []
    for a, s, v in zip(ann.reshape(-1, h, w), seg.reshape(-1, h, w), np.zeros((ann.size // (h * w), h, w), bool) if void is None else void.reshape(-1, h, w)):
        fg_b, gt_b = M._seg2bmap(s * np.logical_not(v)), M._seg2bmap(a * np.logical_not(v))
        fg_dil, gt_dil = _dilate(fg_b.astype(np.uint8), _disk(radius)), _dilate(gt_b.astype(np.uint8), _disk(radius))
        counts.append([np.sum(fg_b), np.sum(gt_b), np.sum(fg_b * gt_dil), np.sum(gt_b * fg_dil), np.sum((s & a) & np.logical_not(v)), np.sum((s | a) & np.logical_not(v))])
    with np.errstate(divide="ignore", invalid="ignore"):
        F = M.db_eval_boundary(ann, seg, void, bound_th=bound_th)
        J = M.db_eval_iou(ann, seg, void)
    NAMES.append(name)
    OUT[name + ".ann"], OUT[name + ".seg"] = np.packbits(ann), np.packbits(seg)
    if void is not None:
        OUT[name + ".void"] = np.packbits(void)
    OUT[name + ".shape"] = np.asarray(ann.shape, np.int64)
    OUT[name + ".bound_th"] = np.float64(bound_th)
    OUT[name + ".radius"] = np.int64(radius)
    OUT[name + ".counts"] = np.asarray(counts, np.int64)
    OUT[name + ".F"] = np.asarray(F, np.float64)
    OUT[name + ".J"] = np.asarray(J, np.float64)


def blob(h, w, cy, cx, ry, rx, phase=0.0):
    """A wobbly ellipse, centre / radii in pixels."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ang = np.arctan2(y - cy, x - cx)
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < (1.0 + 0.2 * np.sin(3 * ang + phase)) ** 2


rng = np.random.default_rng(20240607)

# ---- word edges: rows of 1, 2 words (with and without padding bits) and 3 words; 1 to 37 rows (more than one 8-row strip); dense noise, boundary pixels on columns 63 / 64
for i, (h, w) in enumerate((h, w) for w in (1, 2, 63, 64, 65, 127, 129) for h in (1, 2, 3, 37)):
    ann, seg = rng.random((h, w)) < 0.4, rng.random((h, w)) < 0.4
    if w > 64:
        ann[::2, 63], ann[1::2, 63], ann[::2, 64], ann[1::2, 64] = True, False, False, True
        seg[:, 62:64], seg[:, 64:66] = False, True
    add(f"edge_{h}x{w}", ann, seg, bound_th=(1, 2, 5)[i % 3])

# ---- disk exactness: one-pixel masks (2x2 boundary blocks) at offsets on and just past the circle
H, W, Y0, X0 = 80, 150, 5, 5


def pixel_pairs(offsets):
    ann, seg = np.zeros((len(offsets), H, W), bool), np.zeros((len(offsets), H, W), bool)
    for t, (dy, dx) in enumerate(offsets):
        ann[t, Y0, X0] = True
        seg[t, Y0 + dy, X0 + dx] = True
    return ann, seg


add("disk_r5", *pixel_pairs([(3, 4), (0, 5), (5, 1), (4, 4)]), bound_th=5)
for r in (1, 2, 8, 18, 36, 64):
    dy = max(1, round(0.6 * r))
    kx = int(np.floor(np.sqrt(r * r - dy * dy)))
    add(f"disk_r{r}", *pixel_pairs([(r, 0), (0, r), (r + 1, 0), (0, r + 1), (r + 2, 0), (0, r + 2), (dy, kx), (dy, kx + 1), (dy + 1, kx + 1), (dy + 1, kx + 2)]), bound_th=r)
for r in (36, 64):   # a dilation wider than the blobs' distance to every border
    add(f"blob_r{r}", blob(H, W, 30, 40, 18, 25)[None], blob(H, W, 45, 100, 20, 30, 1.0)[None], bound_th=r)

# ---- frame borders and isolation
h, w = 24, 70
yy, xx = np.mgrid[0:h, 0:w]
checker, checker2 = (yy + xx) % 2 == 0, ((yy // 2) + (xx // 2)) % 2 == 0
tall_a, tall_s = blob(h, w, 11, 30, 16, 12), blob(h, w, 13, 36, 15, 10, 2.0)
assert tall_a[0].any() and tall_a[-1].any() and tall_s[0].any() and tall_s[-1].any()
add("frames3", np.stack([checker, tall_a, checker2]), np.stack([checker2, tall_s, checker]), bound_th=3)
add("frames3_middle_alone", tall_a, tall_s, bound_th=3)
ann, seg = np.zeros((20, 70), bool), np.zeros((20, 70), bool)
ann[5:9, 69], seg[6:10, 0] = True, True   # adjacent in memory (end of a row / start of the next), 69 columns apart
add("row_end_no_wrap", ann, seg, bound_th=2)

# ---- degenerate masks
h, w = 33, 70
E, Fu, B = np.zeros((h, w), bool), np.ones((h, w), bool), blob(h, w, 15, 20, 8, 10)
far = blob(h, w, 17, 55, 7, 8, 1.0)
assert not (B & far).any()
add("degenerate", np.stack([E, E, B, Fu, Fu, B, B, B]), np.stack([E, B, E, Fu, B, B, far, Fu]), bound_th=2)

# ---- void pixels: a band through both masks; a frame that is all void
h, w = 40, 90
a, s = blob(h, w, 20, 40, 12, 25), blob(h, w, 22, 48, 12, 22, 1.5)
band = np.zeros((h, w), bool)
band[:, 38:52] = True
add("void", np.stack([a, a]), np.stack([s, s]), np.stack([band, np.ones((h, w), bool)]), bound_th=3)

# ---- the default threshold (a fraction of the diagonal)
h, w = 97, 131
add("default_97x131", np.stack([blob(h, w, 40 + 3 * t, 60 + 4 * t, 25, 35, 0.3 * t) for t in range(3)]),
    np.stack([blob(h, w, 43 + 2 * t, 57 + 5 * t, 23, 37, 1.0 + 0.4 * t) for t in range(3)]))
h, w = 270, 480
add("default_270x480", blob(h, w, 130, 230, 80, 120)[None], blob(h, w, 138, 240, 76, 128, 0.8)[None])
assert int(OUT["default_270x480.radius"]) == 5

OUT["names"] = np.asarray(NAMES)
path = os.path.join(HERE, "jf_cases.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:   # np.savez_compressed's layout with a fixed timestamp: the file regenerates byte for byte
    for k, v in OUT.items():
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
        info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        z.writestr(info, buf.getvalue())
print(len(NAMES), "cases,", os.path.getsize(path), "bytes")
