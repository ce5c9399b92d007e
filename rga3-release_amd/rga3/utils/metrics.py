"""Mask metrics of the reference's validation / evaluation harness, vectorised.

 * intersection_and_union  — utils/utils.py:140-152 (histc over K classes, ignore_index copied into the prediction)
 * giou_ciou               — train_joint.py:615-641 (gIoU = mean per-frame IoU with empty-target = 1; cIoU = sum I / sum U)
 * db_eval_iou             — evaluation/mevis_val_u/metrics.py:6-37 (the "mask IoU" of the parity metric)

J&F, the score of every video benchmark the reference reports (MeViS, Ref-YouTube-VOS, Ref-DAVIS, ReVOS, ReasonVOS), computed on the device the masks are on:

 * mask_jf                 — region similarity J and boundary F-measure per frame from the six integer counts of rga3.hip.ops.mask_jf_counts (HIP, csrc/maskmetrics.hip)
                             and the reference's own float64 expressions (evaluation/revos/metrics.py:69-73, 136-153): equal to its floats, with one device -> host
                             read per call and no OpenCV / scikit-image.  Needs the HIP library and a GPU; there is no CPU path.
 * db_eval_boundary        — evaluation/revos/metrics.py:77-91 (name and return convention), on mask_jf
 * JAndF                   — evaluation/mevis_val_u/eval_mevis.py:48-49, 89-91 (per-sequence mean J / mean F, then their means and J&F)
"""
from __future__ import annotations

import numpy as np
import torch


def intersection_and_union(output: torch.Tensor, target: torch.Tensor, K: int, ignore_index: int = 255):
    assert output.dim() in (1, 2, 3) and output.shape == target.shape
    o = output.reshape(-1).clone()
    t = target.reshape(-1)
    o[t == ignore_index] = ignore_index
    inter = o[o == t]
    cnt = lambda v: torch.bincount(v[(v >= 0) & (v < K)].long(), minlength=K).float()
    ai, ao, at = cnt(inter), cnt(o), cnt(t)
    return ai, ao + at - ai, at


class GIoUCIoU:
    """Accumulator reproducing train_joint.py:586-648 for one rank (call all_reduce_sums across ranks if distributed)."""

    def __init__(self):
        self.inter = np.zeros(2)
        self.union = np.zeros(2)
        self.acc = np.zeros(2)
        self.count = 0

    def update(self, pred_masks: torch.Tensor, gt_masks: torch.Tensor):
        """pred/gt [T, h, w] (bool or int)."""
        inter, union, acc = torch.zeros(2), torch.zeros(2), torch.zeros(2)
        for m, o in zip(gt_masks.int(), pred_masks.int()):
            i, u, _ = intersection_and_union(o.contiguous().clone(), m.contiguous(), 2, ignore_index=255)
            i, u = i.cpu(), u.cpu()
            inter += i
            union += u
            a = i / (u + 1e-5)
            a[u == 0] += 1.0  # no-object target
            acc += a
        n = gt_masks.shape[0]
        self.inter += inter.numpy()
        self.union += union.numpy()
        self.acc += acc.numpy() / n * n
        self.count += n

    def sums(self):
        return np.concatenate([self.inter, self.union, self.acc, [self.count]])

    def load_sums(self, s):
        self.inter, self.union, self.acc, self.count = s[0:2], s[2:4], s[4:6], float(s[6])

    def compute(self):
        iou_class = self.inter / (self.union + 1e-10)
        return float(self.acc[1] / max(self.count, 1e-5)), float(iou_class[1])  # (giou, ciou)


def db_eval_iou(annotation: np.ndarray, segmentation: np.ndarray, void_pixels=None):
    assert annotation.shape == segmentation.shape
    a, s = annotation.astype(bool), segmentation.astype(bool)
    v = np.zeros_like(s) if void_pixels is None else void_pixels.astype(bool)
    inters = np.sum((s & a) & ~v, axis=(-2, -1))
    union = np.sum((s | a) & ~v, axis=(-2, -1))
    with np.errstate(divide="ignore", invalid="ignore"):
        j = inters / union
    if np.ndim(j) == 0:
        return 1 if np.isclose(union, 0) else j
    j[np.isclose(union, 0)] = 1
    return j


def _jf_radius(bound_th, h: int, w: int) -> int:
    """evaluation/revos/metrics.py:114 (bound_pix); a disk needs a whole radius."""
    if bound_th >= 1:
        if int(bound_th) != bound_th:
            raise ValueError(f"bound_th {bound_th}: a pixel radius (>= 1) is an integer")
        return int(bound_th)
    return int(np.ceil(bound_th * np.linalg.norm((h, w))))


def _jf_device(x):
    if x is None or isinstance(x, torch.Tensor):
        return x
    if not torch.cuda.is_available():
        from rga3.hip.lib import Rga3Error

        raise Rga3Error("mask_jf scores on the device and found no GPU (no CPU fallback on the product path)")
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _f_from_counts(n_fg: int, n_gt: int, fg_match: int, gt_match: int):
    """evaluation/revos/metrics.py:136-153 on the counts."""
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1, 0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0, 1
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1, 1
    else:
        precision, recall = fg_match / float(n_fg), gt_match / float(n_gt)
    return 0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)


def mask_jf(annotation, segmentation, void_pixels=None, bound_th=0.008):
    """(J, F) per frame of ground-truth / predicted masks [T, h, w] (float64 arrays of length T) or [h, w] (python floats): the reference's db_eval_iou and
    db_eval_boundary.  bool or uint8 masks; torch device tensors are scored where they are, numpy arrays are uploaded to the current device.
    bound_th as in the reference: a pixel radius if >= 1, else a fraction of the frame diagonal (rounded up)."""
    assert annotation.shape == segmentation.shape and (void_pixels is None or void_pixels.shape == annotation.shape)
    if len(annotation.shape) not in (2, 3):
        raise ValueError(f"mask_jf does not support tensors with {len(annotation.shape)} dimensions")
    radius = _jf_radius(bound_th, int(annotation.shape[-2]), int(annotation.shape[-1]))
    from rga3.hip import ops

    counts = ops.mask_jf_counts(_jf_device(annotation), _jf_device(segmentation), _jf_device(void_pixels), radius=radius).cpu().numpy()
    f = np.array([_f_from_counts(*(int(v) for v in row[:4])) for row in counts], dtype=np.float64)
    inters, union = counts[:, 4], counts[:, 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        j = inters / union
    j[np.isclose(union, 0)] = 1
    if len(annotation.shape) == 2:
        return float(j[0]), float(f[0])
    return j, f


def db_eval_boundary(annotation, segmentation, void_pixels=None, bound_th=0.008):
    return mask_jf(annotation, segmentation, void_pixels, bound_th)[1]


class JAndF:
    """Accumulator reproducing evaluation/mevis_val_u/eval_mevis.py:48-49, 86-91 for one rank (add sums() across ranks and load_sums() the total if distributed):
    one (mean J, mean F) per sequence, then the mean over sequences.  The sequence means are added in update() order."""

    def __init__(self):
        self.j = 0.0
        self.f = 0.0
        self.count = 0

    def update(self, pred_masks, gt_masks, void_pixels=None, bound_th=0.008):
        """pred/gt [T, h, w] (bool or uint8): one sequence of one expression / object."""
        j, f = mask_jf(gt_masks, pred_masks, void_pixels, bound_th)
        self.j += float(np.mean(j))
        self.f += float(np.mean(f))
        self.count += 1

    def sums(self):
        return np.array([self.j, self.f, self.count], dtype=np.float64)

    def load_sums(self, s):
        self.j, self.f, self.count = float(s[0]), float(s[1]), int(s[2])

    def compute(self):
        n = max(self.count, 1)
        j, f = self.j / n, self.f / n
        return {"J": j, "F": f, "J&F": (j + f) / 2}
