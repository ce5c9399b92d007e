"""STOM — Spatio-Temporal Overlay Module, the numpy half (reference model/STOM.py:72-207).

The point tracker the reference delegates to (CoTracker3, third-party, not installed, weights absent) is a "next" row
(SURVEY.md 8(f).4): callers pass tracks in.  What is restated here is the reference's own arithmetic: median/MAD
filtering of the flow magnitudes, mean flow, integer-pixel shift of the RGBA visual prompt and alpha compositing
(shapes other than masks, :102-160), and for mask-shaped prompts the tracked-point raster -> morphological closing ->
centroid -> filled circle of :163-207.  The reference calls OpenCV for the last four (cv2.getStructuringElement / morphologyEx /
moments / circle); cv2 is not in this image, so those are restated from OpenCV 4.x's published algorithms (imgproc morph.cpp,
drawing.cpp) -- parity with the installed cv2 of a reference deployment is unpinned, the structuring elements are checked against
OpenCV's documented 3x3 / 5x5 ellipses.

The same stage runs on the device (csrc/stom.hip through rga3.hip.ops.stom_*) when ``propagate_in_video`` is given the clip as a CUDA uint8 tensor: flow filter,
overlay shift, closing, centroid, circle and compositing in HIP, every per-frame decision kept in device memory, the result equal to this numpy path byte for byte.
The helpers the kernels are built from -- Pillow's compositing in integers (``pil_over``), the span table of the structuring element (``ellipse_spans``), the
half-width table of the circle (``circle_half_widths``) and the gather form of the shift (``shift_overlay_gather``) -- are restated here and pinned against the
numpy path on the CPU.
"""
from __future__ import annotations

import functools

import numpy as np

MAX_POINTS = 16384   # device route: tracked points per frame (the reference's grid_size = 100 gives at most 10^4)
MAX_KERNEL = 128     # device route: side of the closing's structuring element, min(h, w) // 15


def mean_flow(vip_track: np.ndarray, tgt_track: np.ndarray, visibility: np.ndarray):
    """reference STOM.py:102-130 -> (dx, dy) or None when the frame is left untouched."""
    vis = visibility.astype(bool)
    flows = tgt_track[vis] - vip_track[vis]
    if len(flows) == 0:
        return None
    mag = np.linalg.norm(flows, axis=1)
    med = np.median(mag)
    thr = 3 * np.median(np.abs(mag - med))
    keep = (mag >= med - thr) & (mag <= med + thr)
    f = flows[keep]
    if len(f) < visibility.shape[0] // 2:
        return None
    dx, dy = np.mean(f[:, 0]), np.mean(f[:, 1])
    if np.isnan(dx) or np.isnan(dy):
        return None
    return float(dx), float(dy)


def shift_overlay(src_rgba: np.ndarray, shape_hw, dx: float, dy: float) -> np.ndarray:
    """reference STOM.py:145-156: move every pixel with alpha > 0 by (int(x+dx), int(y+dy)) (truncation toward zero)."""
    out = np.zeros_like(src_rgba)
    ys, xs = np.nonzero(src_rgba[:, :, 3] > 0)
    nx = np.trunc(xs + dx).astype(np.int64)
    ny = np.trunc(ys + dy).astype(np.int64)
    ok = (nx >= 0) & (nx < shape_hw[1]) & (ny >= 0) & (ny < shape_hw[0])
    out[ny[ok], nx[ok]] = src_rgba[ys[ok], xs[ok]]
    return out


def ellipse_kernel(k: int) -> np.ndarray:
    """cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k)) (OpenCV morph.cpp): row i spans c - dx .. c + dx with
    dx = round(c * sqrt((r^2 - (i - r)^2) / r^2)), r = c = k // 2."""
    if k <= 1:
        return np.ones((max(k, 1), max(k, 1)), np.uint8)
    r = c = k // 2
    out = np.zeros((k, k), np.uint8)
    for i in range(k):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) / float(r * r))))
            out[i, max(c - dx, 0): min(c + dx + 1, k)] = 1
    return out


def _morph(img: np.ndarray, kernel: np.ndarray, dilate: bool) -> np.ndarray:
    """cv2.dilate / cv2.erode with the anchor at the kernel centre and the default border (outside pixels never win):
    dst(y, x) = max / min over kernel elements (i, j) != 0 of src(y + i - ay, x + j - ax)."""
    h, w = img.shape
    ay, ax = kernel.shape[0] // 2, kernel.shape[1] // 2
    out = np.zeros_like(img) if dilate else np.full_like(img, 255)
    for i, j in np.argwhere(kernel > 0):
        dy, dx = i - ay, j - ax
        ys0, ys1 = max(0, -dy), min(h, h - dy)        # destination rows whose source row y + dy is inside
        xs0, xs1 = max(0, -dx), min(w, w - dx)
        if ys0 >= ys1 or xs0 >= xs1:
            continue
        src = img[ys0 + dy: ys1 + dy, xs0 + dx: xs1 + dx]
        dst = out[ys0:ys1, xs0:xs1]
        np.maximum(dst, src, out=dst) if dilate else np.minimum(dst, src, out=dst)
    return out


def morph_close(mask: np.ndarray, k: int) -> np.ndarray:
    """cv2.morphologyEx(mask, cv2.MORPH_CLOSE, ellipse(k)): dilation, then erosion, same kernel and anchor."""
    ker = ellipse_kernel(k)
    return _morph(_morph(mask, ker, True), ker, False)


def filled_circle(shape_hw, cx: int, cy: int, radius: int) -> np.ndarray:
    """cv2.circle(img, (cx, cy), radius, 255, -1) on a zero uint8 image (OpenCV drawing.cpp Circle(): midpoint algorithm, horizontal spans)."""
    h, w = shape_hw
    img = np.zeros((h, w), np.uint8)

    def hline(y, x0, x1):
        if 0 <= y < h:
            x0, x1 = max(x0, 0), min(x1, w - 1)
            if x0 <= x1:
                img[y, x0:x1 + 1] = 255

    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        hline(cy - dy, cx - dx, cx + dx)
        hline(cy + dy, cx - dx, cx + dx)
        hline(cy - dx, cx - dy, cx + dy)
        hline(cy + dx, cx - dy, cx + dy)
        dy += 1
        err += plus
        plus += 2
        m = -1 if err > 0 else 0          # (err <= 0) - 1
        err -= minus & m
        dx += m
        minus -= m & 2
    return img


def warp_point(src_rgba: np.ndarray, tgt_rgb: np.ndarray, tracks: np.ndarray, visibility: np.ndarray):
    """reference STOM.py:163-207 (mask-shaped prompts): the visible tracked points are rasterised, closed with an elliptical kernel of min(h, w) // 15,
    and a filled circle of radius min(h, w) // 20 in the prompt's colour (alpha clamped to [96, 148]) is drawn at the centroid of the closed mask.
    Returns the composited RGB frame (the frame itself when fewer than half of the points are visible)."""
    vis = visibility.astype(bool)
    if vis.sum() < len(tracks) // 2:
        return tgt_rgb
    on = src_rgba[:, :, 3] > 0
    colour = src_rgba[on][0].copy() if on.any() else np.zeros(4, np.uint8)
    colour[3] = max(min(int(colour[3]), 148), 96)
    h, w = src_rgba.shape[:2]
    mask = np.zeros((h, w), np.uint8)
    for pt, v in zip(tracks, vis):
        if v:
            x, y = int(pt[1]), int(pt[0])          # the reference's naming: x is the ROW, y the column
            if 0 <= x < h and 0 <= y < w:
                mask[x, y] = 255
    closed = morph_close(mask, min(h, w) // 15)
    overlay = np.zeros_like(src_rgba)
    m00 = float(closed.astype(np.float64).sum())
    if m00 != 0:
        ys, xs = np.nonzero(closed)
        wgt = closed[ys, xs].astype(np.float64)
        cx, cy = int((xs * wgt).sum() / m00), int((ys * wgt).sum() / m00)
        overlay[filled_circle((h, w), cx, cy, min(h, w) // 20) > 0] = colour
    return composite(tgt_rgb, overlay)


def composite(tgt_rgb: np.ndarray, overlay_rgba: np.ndarray) -> np.ndarray:
    from PIL import Image

    base = Image.fromarray(tgt_rgb, "RGB").convert("RGBA")
    return np.array(Image.alpha_composite(base, Image.fromarray(overlay_rgba, "RGBA")).convert("RGB"))


def pil_over(base, over, alpha) -> np.ndarray:
    """Pillow's ``alpha_composite(dst, src)`` over an OPAQUE dst followed by ``convert("RGB")``, one channel, in Pillow's integer arithmetic (libImaging
    AlphaComposite.c): ``base`` / ``over`` / ``alpha`` are broadcastable uint8 arrays (dst channel, src channel, src alpha).  With dst alpha 255:
        blend = 255 * (255 - a);  outa255 = a * 255 + blend;  coef1 = a * 255 * 255 * 2^7 // outa255;  coef2 = 255 * 2^7 - coef1   (7 precision bits)
        out = SHIFTFORDIV255(over * coef1 + base * coef2 + (0x80 << 7)) >> 7,   SHIFTFORDIV255(t) = ((t >> 8) + t) >> 8
    and a == 0 copies dst.  ``convert("RGB")`` drops the (opaque) alpha.  csrc/stom.hip mirrors this function."""
    d, s, a = (np.asarray(v).astype(np.uint32) for v in (base, over, alpha))
    blend = 255 * (255 - a)
    outa255 = a * 255 + blend
    coef1 = a * 255 * 255 * 128 // outa255
    coef2 = 255 * 128 - coef1
    t = s * coef1 + d * coef2 + (0x80 << 7)
    out = (((t >> 8) + t) >> 8) >> 7
    return np.where(a == 0, d, out).astype(np.uint8)


def composite_int(tgt_rgb: np.ndarray, overlay_rgba: np.ndarray) -> np.ndarray:
    """``composite`` without Pillow: ``pil_over`` on the three colour channels."""
    return pil_over(tgt_rgb, overlay_rgba[..., :3], overlay_rgba[..., 3:4])


@functools.lru_cache(maxsize=None)
def _ellipse_spans(k: int) -> bytes:
    ker = ellipse_kernel(k)
    spans = np.zeros((ker.shape[0], 2), np.uint8)
    for i, row in enumerate(ker):
        on = np.nonzero(row)[0]
        if len(on) == 0 or len(on) != on[-1] - on[0] + 1:
            raise ValueError(f"ellipse_kernel({k}) row {i} is not one span")
        spans[i] = on[0], on[-1]
    return spans.tobytes()


def ellipse_spans(k: int) -> np.ndarray:
    """uint8 [max(k, 1), 2]: first and last set column of every row of ``ellipse_kernel(k)`` (each row is one span).  Derived from the kernel itself, cached per k;
    the anchor of ``_morph`` is (k // 2, k // 2)."""
    return np.frombuffer(_ellipse_spans(int(k)), np.uint8).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _circle_half_widths(radius: int) -> bytes:
    side = 2 * radius + 1
    img = filled_circle((side, side), radius, radius, radius) > 0
    hw = np.zeros(radius + 1, np.uint8)
    for d in range(radius + 1):
        on = np.nonzero(img[radius + d])[0]
        if len(on) == 0 or len(on) != on[-1] - on[0] + 1 or on[0] + on[-1] != 2 * radius or not np.array_equal(img[radius + d], img[radius - d]):
            raise ValueError(f"filled_circle(radius {radius}) row {d} is not one symmetric span")
        hw[d] = on[-1] - radius
    return hw.tobytes()


def circle_half_widths(radius: int) -> np.ndarray:
    """uint8 [radius + 1]: ``filled_circle`` of this radius covers |x - cx| <= hw[|y - cy|] on the rows |y - cy| <= radius.  Derived from ``filled_circle`` on a
    (2 radius + 1)^2 canvas, cached per radius (radius 0 is the single centre pixel)."""
    return np.frombuffer(_circle_half_widths(int(radius)), np.uint8)


def shift_overlay_gather(src_rgba: np.ndarray, shape_hw, dx: float, dy: float) -> np.ndarray:
    """``shift_overlay`` as a gather, the rule of the device kernel: ``shift_overlay`` scatters in row-major order and the last writer wins, so destination
    (ny, nx) takes the lexicographically largest source (y, x) with alpha > 0, trunc(x + dx) == nx and trunc(y + dy) == ny (fp64, as there).  Truncation toward zero
    maps (-1, 1) onto 0, so two rows or columns can collide at the border; the candidates are ny - trunc(dy) + {1, 0, -1} and the same in x."""
    h, w = shape_hw
    sh, sw = src_rgba.shape[:2]
    out = np.zeros_like(src_rgba)
    if not (abs(dx) < 1e9 and abs(dy) < 1e9):
        return out
    ny, nx = np.mgrid[0:h, 0:w]
    done = np.zeros((h, w), bool)
    for oy in (1, 0, -1):
        y = ny - int(np.trunc(dy)) + oy
        ok_y = (y >= 0) & (y < sh) & (np.trunc(y + dy) == ny)
        for ox in (1, 0, -1):
            x = nx - int(np.trunc(dx)) + ox
            ok = ok_y & (x >= 0) & (x < sw) & (np.trunc(x + dx) == nx) & ~done
            yy, xx = y[ok], x[ok]
            hit = src_rgba[yy, xx, 3] > 0
            out[ny[ok][hit], nx[ok][hit]] = src_rgba[yy[hit], xx[hit]]
            done[ny[ok][hit], nx[ok][hit]] = True
    return out


def _check_device_args(frames, src_frame_vip, vip_frame_idx, shape, tracks, visibility):
    """Argument checks of the device route, all before any launch.  The device check comes last so that every other refusal is reachable without a GPU."""
    import torch

    from rga3.hip.lib import Rga3Error

    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or frames.shape[0] == 0:
        raise Rga3Error(f"STOM device route: frames are uint8 [T, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise Rga3Error("STOM device route: frames must be contiguous")
    T, H, W, _ = frames.shape
    ov = src_frame_vip
    if isinstance(ov, np.ndarray):
        if ov.dtype != np.uint8 or ov.shape != (H, W, 4):
            raise Rga3Error(f"STOM device route: the overlay is uint8 [{H}, {W}, 4], got {ov.dtype} {ov.shape}")
    elif not hasattr(ov, "is_cuda") or ov.dtype != torch.uint8 or tuple(ov.shape) != (H, W, 4) or not ov.is_contiguous():
        raise Rga3Error(f"STOM device route: the overlay is a contiguous uint8 [{H}, {W}, 4] tensor or numpy array")
    if not hasattr(tracks, "is_cuda") or tracks.dtype != torch.float32 or tracks.dim() != 4 or tracks.shape[0] != 1 or tracks.shape[1] != T or tracks.shape[3] != 2:
        raise Rga3Error(f"STOM device route: tracks are float32 [1, {T}, N, 2], got {getattr(tracks, 'dtype', type(tracks))} {tuple(getattr(tracks, 'shape', ()))}")
    N = tracks.shape[2]
    if not hasattr(visibility, "is_cuda") or visibility.dtype != torch.bool or tuple(visibility.shape) != (1, T, N):
        raise Rga3Error(f"STOM device route: visibility is bool [1, {T}, {N}], got {getattr(visibility, 'dtype', type(visibility))} {tuple(getattr(visibility, 'shape', ()))}")
    if not tracks.is_contiguous() or not visibility.is_contiguous():
        raise Rga3Error("STOM device route: tracks and visibility must be contiguous")
    if not 1 <= N <= MAX_POINTS:
        raise Rga3Error(f"STOM device route: {N} tracked points per frame (1..{MAX_POINTS})")
    if int(vip_frame_idx) != vip_frame_idx or not 0 <= vip_frame_idx < T:
        raise Rga3Error(f"STOM device route: vip_frame_idx {vip_frame_idx} outside [0, {T})")
    if shape in ("mask", "mask contour") and min(H, W) // 15 > MAX_KERNEL:
        raise Rga3Error(f"STOM device route: {H} x {W} frames need a closing kernel of {min(H, W) // 15} (at most {MAX_KERNEL})")
    for t in (frames, ov, tracks, visibility):
        if hasattr(t, "is_cuda") and (not t.is_cuda or t.device != frames.device):
            raise Rga3Error("STOM device route: frames, overlay, tracks and visibility live on one GPU (no CPU fallback on the product path)")


class STOM:
    def __init__(self, tracker=None):
        self.tracker = tracker  # callable(frames, src_vip, idx) -> (tracks [1,T,N,2], visibility [1,T,N]); CoTracker3 is not vendored

    def propagate_in_video(self, frames, src_frame_vip, vip_frame_idx, shape="rectangle", tracks=None, visibility=None):
        """frames: list of HxWx3 uint8; src_frame_vip: HxWx4 uint8 overlay -> list of HxWx3 uint8 (numpy, on the host).

        Device route: ``frames`` a CUDA uint8 tensor [T, H, W, 3] (contiguous), ``src_frame_vip`` uint8 [H, W, 4] (a CUDA tensor is used as is, a numpy array is
        uploaded once), ``tracks`` float32 [1, T, N, 2] and ``visibility`` bool [1, T, N] on the same GPU (or the tracker's return) -> CUDA uint8 [T, H, W, 3], equal to
        the numpy route byte for byte and ready for ``sam_preprocess_frames`` / ``qwen_preprocess_video``.  Nothing is read back and nothing synchronises: whether a
        frame is touched, its flow and its centroid stay in device memory.  Limits: N <= 16384, and for mask shapes min(H, W) // 15 <= 128.  Finite tracks are a
        precondition (a frame with a non-finite flow magnitude is left untouched).  Where the reference swallows every exception of the mask branch and keeps the
        frame, the device route raises ``Rga3Error`` for bad arguments BEFORE the loop, i.e. before any launch; there is no CPU fallback."""
        if hasattr(frames, "is_cuda"):
            return self._propagate_on_device(frames, src_frame_vip, vip_frame_idx, shape, tracks, visibility)
        if tracks is None:
            if self.tracker is None:
                raise RuntimeError("STOM needs point tracks: no tracker is bundled (CoTracker3 is a third-party dependency of the reference)")
            tracks, visibility = self.tracker(frames, src_frame_vip, vip_frame_idx)
        out = []
        vip_track = tracks[0, vip_frame_idx]
        for i, f in enumerate(frames):
            if i == vip_frame_idx:
                out.append(composite(f, src_frame_vip))
                continue
            if shape in ("mask", "mask contour"):
                try:
                    out.append(warp_point(src_frame_vip, f, tracks[0, i], visibility[0, i]))
                except Exception:      # the reference swallows every failure of this branch and keeps the frame (:95-101)
                    out.append(f)
                continue
            fl = mean_flow(vip_track, tracks[0, i], visibility[0, i])
            out.append(f if fl is None else composite(f, shift_overlay(src_frame_vip, f.shape[:2], fl[0], fl[1])))
        return out

    def _propagate_on_device(self, frames, src_frame_vip, vip_frame_idx, shape, tracks, visibility):
        import torch

        from rga3.hip import ops

        if tracks is None:
            if self.tracker is None:
                raise RuntimeError("STOM needs point tracks: no tracker is bundled (CoTracker3 is a third-party dependency of the reference)")
            tracks, visibility = self.tracker(frames, src_frame_vip, vip_frame_idx)
        _check_device_args(frames, src_frame_vip, vip_frame_idx, shape, tracks, visibility)
        ov = src_frame_vip
        if isinstance(ov, np.ndarray):     # one upload, from pinned memory: the copy is ordered on the stream and nothing waits for it
            ov = torch.from_numpy(np.ascontiguousarray(ov)).pin_memory().to(frames.device, non_blocking=True)
        H, W = frames.shape[1:3]
        if shape in ("mask", "mask contour"):
            k, radius = min(H, W) // 15, min(H, W) // 20
            return ops.stom_mask_composite(frames, ov, tracks[0], visibility[0], int(vip_frame_idx), ellipse_spans(k), k, circle_half_widths(radius), radius)
        records = ops.stom_flow(tracks[0], visibility[0], int(vip_frame_idx))
        return ops.stom_shift_composite(frames, ov, records, int(vip_frame_idx))
