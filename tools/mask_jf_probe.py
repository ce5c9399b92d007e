#!/usr/bin/env python3
"""Device time of J&F scoring (rga3.hip.ops.mask_jf_counts, csrc/maskmetrics.hip) for T = 16 bool masks at 480x854 and 1080x1920 with the reference's default
radius (8 / 18 px): 3 warm-up calls, then 20 calls each between its own pair of events; prints one JSON line per shape with the median / minimum call time and the
algorithmic traffic (2 T h w mask bytes read + the packed boundary workspace written once and read at least once).  A recorded figure, not a gate: the parent has no
device path and the reference's host path (OpenCV) is not available here, so no speed-up is claimed.
python3 tools/mask_jf_probe.py"""
import json
import math
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rga3-release_amd"))
from rga3.hip import lib, ops  # noqa: E402


def blobs(T, h, w, dev, shift):
    """One drifting ellipse per frame (an object mask: thin boundary, like evaluate()'s output)."""
    y, x = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    t = torch.arange(T, device=dev, dtype=torch.float32)[:, None, None]
    cy, cx = 0.5 * h + 0.01 * h * t + shift, 0.45 * w + 0.012 * w * t + shift
    return ((y - cy) / (0.28 * h)) ** 2 + ((x - cx) / (0.22 * w)) ** 2 < 1.0


def main():
    signal.alarm(240)   # a hung device call ends the probe instead of holding the machine
    dev = torch.device("cuda:0")
    for h, w in ((480, 854), (1080, 1920)):
        T, radius = 16, math.ceil(0.008 * math.hypot(h, w))
        ann, seg = blobs(T, h, w, dev, 0.0), blobs(T, h, w, dev, 0.6 * radius)
        for _ in range(3):
            counts = ops.mask_jf_counts(ann, seg, radius=radius)
        torch.cuda.synchronize()
        times = []
        for _ in range(20):
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            counts = ops.mask_jf_counts(ann, seg, radius=radius)
            en.record()
            en.synchronize()
            times.append(st.elapsed_time(en) * 1e3)
        times.sort()
        c = counts.cpu()
        assert (c[:, 2] <= c[:, 0]).all() and (c[:, 3] <= c[:, 1]).all() and (c[:, 4] <= c[:, 5]).all() and int(c[:, 0].min()) > 0
        ws = int(lib.load().rga3_mask_jf_ws_bytes(T, h, w))
        print(json.dumps({"probe": "mask_jf_counts", "T": T, "h": h, "w": w, "radius": radius, "median_us": round(times[10], 1), "min_us": round(times[0], 1),
                          "mask_bytes_read": 2 * T * h * w, "workspace_bytes": ws, "boundary_pixels_per_frame": float(c[:, :2].float().mean())}), flush=True)


if __name__ == "__main__":
    main()
