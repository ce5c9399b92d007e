#!/usr/bin/env python3
"""Device time of STOM's device route (rga3.model.STOM.STOM.propagate_in_video on CUDA tensors, csrc/stom.hip) next to the numpy route on this machine's host:
T = 16 frames at 480x854 with N = 4096 and N = 10000 tracked points for the flow route (shape "rectangle") and the mask route (shape "mask"), and the mask route at
1080x1920.  Device: 3 warm-up calls, then 20 calls each between its own pair of events, median / minimum.  Host: one timed call of the numpy route on the first
`host_frames` frames of the same clip (the closing of a 1080x1920 frame takes seconds there), reported per frame.  Prints one JSON line per configuration.  A recorded
figure, not a gate; the device result of the timed clip is compared with the numpy result of its first frames.
python3 tools/stom_probe.py"""
import json
import os
import signal
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rga3-release_amd"))
from rga3.model import STOM as ST  # noqa: E402


def clip(T, h, w, n, seed):
    """Random frames, an elliptical translucent prompt, points inside it drifting on a 1/8-pixel lattice with jitter and a few far outliers."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (T, h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    inside = ((y - 0.45 * h) / (0.2 * h)) ** 2 + ((x - 0.4 * w) / (0.15 * w)) ** 2 < 1.0
    ov = np.zeros((h, w, 4), np.uint8)
    ov[inside] = (255, 40, 40, 128)
    ys, xs = np.nonzero(inside)
    pick = rng.integers(0, len(ys), n)
    vip = np.stack([xs[pick], ys[pick]], 1).astype(np.float32)
    tracks = np.zeros((1, T, n, 2), np.float32)
    for t in range(T):
        jitter = rng.integers(-8, 9, (n, 2)) / 8.0
        tracks[0, t] = vip + np.array([1.5 * t, 0.75 * t], np.float32) + (jitter if t else 0)
        far = rng.permutation(n)[:n // 50]
        if t:
            tracks[0, t, far] += np.array([60.0, -35.0], np.float32)
    vis = rng.random((1, T, n)) < 0.9
    return frames, ov, tracks, vis


def main():
    signal.alarm(420)   # a hung device call ends the probe instead of holding the machine
    dev = torch.device("cuda:0")
    stom = ST.STOM()
    configs = [("rectangle", 480, 854, 4096, 16), ("rectangle", 480, 854, 10000, 16), ("mask", 480, 854, 4096, 4), ("mask", 480, 854, 10000, 4), ("mask", 1080, 1920, 4096, 2)]
    for shape, h, w, n, host_frames in configs:
        T = 16
        frames, ov, tracks, vis = clip(T, h, w, n, seed=h + n)
        d = [torch.from_numpy(a).to(dev) for a in (frames, ov, tracks, vis)]
        for _ in range(3):
            out = stom.propagate_in_video(d[0], d[1], 0, shape=shape, tracks=d[2], visibility=d[3])
        torch.cuda.synchronize()
        times = []
        for _ in range(20):
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            out = stom.propagate_in_video(d[0], d[1], 0, shape=shape, tracks=d[2], visibility=d[3])
            en.record()
            en.synchronize()
            times.append(st.elapsed_time(en) * 1e3)
        times.sort()
        t0 = time.perf_counter()
        host = stom.propagate_in_video(list(frames[:host_frames]), ov, 0, shape=shape, tracks=tracks[:, :host_frames], visibility=vis[:, :host_frames])
        host_s = time.perf_counter() - t0
        got = out[:host_frames].cpu().numpy()
        touched = sum(bool((a != b).any()) for a, b in zip(host, frames[:host_frames]))
        print(json.dumps({"probe": "stom", "shape": shape, "T": T, "h": h, "w": w, "N": n, "device_median_us": round(times[10], 1), "device_min_us": round(times[0], 1),
                          "device_us_per_frame": round(times[10] / T, 1), "host_frames": host_frames, "host_ms_per_frame": round(host_s * 1e3 / host_frames, 2),
                          "host_frames_touched": touched, "equal_to_host": bool(np.array_equal(got, np.stack(host)))}), flush=True)


if __name__ == "__main__":
    main()
