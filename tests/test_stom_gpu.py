"""GPU: STOM's device route (csrc/stom.hip through rga3.model.STOM.STOM.propagate_in_video on CUDA tensors) against the numpy route of the same module, which
tests/test_harness_cpu.py pins.  The arithmetic is integer or single-operation IEEE, so every comparison is byte equality.  Flows lie on a 1/8-pixel lattice, so the
fp32 mean of the kept flows is exact in any summation order.  Each case's numpy result is computed once and shared."""
import functools

import numpy as np
import pytest

from rga3.model import STOM as ST

pytestmark = pytest.mark.gpu

# (H, W): 60 x 90 k = 4 (even kernel), W crosses one word; 45 x 130 three words, the last ragged; 150 x 200 k = 10, r = 7; 12 x 40 k = 0, radius 0; 64 x 64 one full
# word; 480 x 854 k = 32, r = 24, spans cross words (one frame pair)
SIZES = [(60, 90), (45, 130), (150, 200), (12, 40), (64, 64), (480, 854)]


def lattice(rng, lo, hi, size):
    return (rng.integers(int(lo * 8), int(hi * 8) + 1, size) / 8.0).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- flow scenarios
# each: (vip points [N, 2], rng, H, W) -> (points of the frame [N, 2] f32, visibility [N] bool, "apply" | "skip")
def _uniform(dx, dy, visible=None):
    def make(vip, rng, H, W):
        n = len(vip)
        vis = np.ones(n, bool)
        if visible is not None:
            vis[:] = False
            vis[rng.permutation(n)[:visible(n)]] = True
        want = "apply" if vis.sum() >= max(n // 2, 1) else "skip"
        return vip + np.array([dx(W) if callable(dx) else dx, dy], np.float32), vis, want
    return make


def _outliers(vip, rng, H, W):
    """a fifth of the points moves as a far cluster: the MAD filter must drop it"""
    n = len(vip)
    pts = vip + np.array([5.25, -1.125], np.float32) + lattice(rng, -1, 1, (n, 2))
    far = rng.permutation(n)[:n // 5]
    pts[far] += np.array([150.0, 90.0], np.float32)
    return pts, np.ones(n, bool), "apply"


def _spread(vip, rng, H, W):
    n = len(vip)
    vis = rng.random(n) < 0.8
    vis[:n // 2 + 1] = True
    return vip + np.array([-2.375, 3.5], np.float32) + lattice(rng, -1.5, 1.5, (n, 2)), vis, "apply"


def _mad_zero(vip, rng, H, W):
    """two thirds share one flow exactly, so the MAD is 0 and only they survive"""
    n = len(vip)
    pts = vip + np.array([1.5, 2.0], np.float32)
    odd = rng.permutation(n)[:n // 3]
    pts[odd] += lattice(rng, 2, 9, (len(odd), 2))
    return pts, np.ones(n, bool), "apply"


def _kept(delta):
    """N // 2 + 2 points are visible; all share one flow (MAD 0) but 2 - delta far ones, which the filter drops: exactly N // 2 + delta are kept"""
    def make(vip, rng, H, W):
        n = len(vip)
        order = rng.permutation(n)
        vis = np.zeros(n, bool)
        vis[order[:n // 2 + 2]] = True
        pts = vip + np.array([-1.75, 4.125], np.float32)
        pts[order[:2 - delta]] += np.array([33.0, -20.5], np.float32)
        return pts, vis, "apply" if delta >= 0 else "skip"
    return make


FLOW_GROUPS = [
    [_uniform(-3.625, -2.5), _outliers, _uniform(0.0, 0.0, visible=lambda n: 0), _uniform(2.0, 7.5, visible=lambda n: n // 2)],
    [_uniform(1.25, -0.875, visible=lambda n: n // 2 - 1), _uniform(lambda W: W + 5.5, 0.0), _uniform(-0.5, -0.75), _spread],
    [_mad_zero, _uniform(0.375, 0.875), _kept(0), _kept(-1)],
]


# ---------------------------------------------------------------------------------------------------------------- mask scenarios
# each: (N, rng, H, W) -> (points [N, 2] f32 as (column, row), visibility [N] bool)
def _cluster(n, rng, H, W):
    return (np.array([W * 0.5, H * 0.5]) + rng.normal(0, min(H, W) / 6, (n, 2))).astype(np.float32), np.ones(n, bool)


def _half(delta):
    def make(n, rng, H, W):
        pts, vis = _cluster(n, rng, H, W)
        vis[:] = False
        vis[rng.permutation(n)[:max(n // 2 + delta, 0)]] = True
        return pts, vis
    return make


def _borders(n, rng, H, W):
    """points at -0.5, on the last row / column, just outside, far outside, and a cloud along every border"""
    edge = [(-0.5, -0.5), (W - 1, H - 1), (W - 0.5, H - 0.5), (-0.5, H - 1), (W - 1, -0.5), (-1.0, 3), (3, -1.0), (W, 2), (2, H), (W + 10.25, H + 0.25), (-3.5, -7),
            (0, H // 2), (W - 1, H // 2), (W // 2, 0), (W // 2, H - 1)]
    pts = np.array([edge[i % len(edge)] for i in range(n)], np.float32)
    extra = slice(len(edge), n)
    m = max(n - len(edge), 0)
    if m:
        side = rng.integers(0, 4, m)
        along = rng.random(m)
        x = np.where(side == 0, 0.25, np.where(side == 1, W - 0.75, along * W))
        y = np.where(side == 2, 0.5, np.where(side == 3, H - 0.25, along * H))
        pts[extra] = np.stack([x, y], 1).astype(np.float32)
    return pts, np.ones(n, bool)


def _two_clusters(n, rng, H, W):
    a = np.array([W * 0.2, H * 0.25]) + rng.normal(0, 1.5, (n // 2, 2))
    b = np.array([W * 0.8, H * 0.7]) + rng.normal(0, 1.5, (n - n // 2, 2))
    return np.concatenate([a, b]).astype(np.float32), np.ones(n, bool)


def _all_outside(n, rng, H, W):
    return (np.array([W + 4.0, -6.0]) + rng.random((n, 2))).astype(np.float32), np.ones(n, bool)


MASK_GROUPS = [[_cluster, _half(0), _half(-1), _borders], [_borders, _two_clusters, _all_outside, _cluster]]
OVERLAYS = ["mid", "low", "high", "clear"]      # alpha of the first set pixel inside [96, 148], below, above; nothing set


class Case:
    pass


def _frames(rng, T, H, W):
    return rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def flow_case(i):
    H, W = SIZES[i]
    big = (H, W) == (480, 854)
    rng = np.random.default_rng(100 + i)
    c = Case()
    c.name, c.shape = f"flow_{H}x{W}", "rectangle"
    c.T = 2 if big else 5
    c.N = [24, 25, 40, 13, 33, 64][i]
    c.vip = [0, 2, 1, 4, 0, 1][i] % c.T
    vip_pts = np.stack([lattice(rng, 0, W - 1, c.N), lattice(rng, 0, H - 1, c.N)], 1)
    scen = [_outliers] if big else FLOW_GROUPS[i % 3]
    c.tracks = np.zeros((1, c.T, c.N, 2), np.float32)
    c.vis = np.ones((1, c.T, c.N), bool)
    c.tracks[0, c.vip] = vip_pts
    c.want = {}
    for t, make in zip([t for t in range(c.T) if t != c.vip], scen):
        c.tracks[0, t], c.vis[0, t], c.want[t] = make(vip_pts, rng, H, W)
    c.frames = _frames(rng, c.T, H, W)
    ov = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)        # dense in the top-left quarter (border collisions), a sparse band elsewhere, holes everywhere
    ov[H // 2:, :, 3] = 0
    ov[:, W // 2:, 3] = 0
    ov[H // 2:H // 2 + 3, W // 3:, 3] = 77
    ov[rng.random((H, W)) < 0.3, 3] = 0
    c.overlay = ov
    c.flows = {t: ST.mean_flow(vip_pts, c.tracks[0, t], c.vis[0, t]) for t in c.want}
    for t, w in c.want.items():       # the scenario reaches the branch it is named for
        assert (c.flows[t] is not None) == (w == "apply"), (c.name, t, w, c.flows[t])
    c.expected = np.stack(ST.STOM().propagate_in_video(list(c.frames), c.overlay, c.vip, tracks=c.tracks, visibility=c.vis))
    return c


@functools.lru_cache(maxsize=None)
def mask_case(i, overlay=None):
    H, W = SIZES[i]
    big = (H, W) == (480, 854)
    rng = np.random.default_rng(200 + i)
    c = Case()
    kind = overlay or OVERLAYS[i % 4]
    c.name, c.shape = f"mask_{H}x{W}_{kind}", "mask" if i % 2 == 0 else "mask contour"
    c.T = 2 if big else 5
    c.N = [30, 41, 64, 17, 36, 300][i]
    c.vip = [2, 0, 3, 1, 4, 0][i] % c.T
    scen = [_borders] if big else MASK_GROUPS[i % 2]
    c.tracks = np.zeros((1, c.T, c.N, 2), np.float32)
    c.vis = np.ones((1, c.T, c.N), bool)
    c.tracks[0, c.vip], _ = _cluster(c.N, rng, H, W)
    for t, make in zip([t for t in range(c.T) if t != c.vip], scen):
        c.tracks[0, t], c.vis[0, t] = make(c.N, rng, H, W)
    c.frames = _frames(rng, c.T, H, W)
    ov = np.zeros((H, W, 4), np.uint8)
    if kind != "clear":
        ov[H // 4:H // 2 + 1, W // 3:W // 2 + 1] = rng.integers(1, 256, 4, dtype=np.uint8)
        ov[H // 4:H // 2 + 1, W // 3:W // 2 + 1, 3] = {"mid": 120, "low": 50, "high": 200}[kind]
        ov[H // 4, W // 3, :3] = (250, 3, 129)                 # the first set pixel has its own colour: a later pixel's colour would show
        ov[H // 2, W // 2] = (9, 9, 9, 255)
    c.overlay = ov
    c.expected = np.stack(ST.STOM().propagate_in_video(list(c.frames), c.overlay, c.vip, shape=c.shape, tracks=c.tracks, visibility=c.vis))
    return c


CASES = [("flow", i) for i in range(len(SIZES))] + [("mask", i) for i in range(len(SIZES))] + [("mask", 0, k) for k in OVERLAYS[1:]] + [("mask", 2, "clear")]


def get_case(key):
    return flow_case(key[1]) if key[0] == "flow" else mask_case(*key[1:])


def on_device(c, dev, numpy_overlay=False):
    import torch

    up = lambda a: torch.from_numpy(a).to(dev)
    return up(c.frames), (c.overlay if numpy_overlay else up(c.overlay)), up(c.tracks), up(c.vis)


def run(c, dev, **kw):
    frames, ov, tracks, vis = on_device(c, dev, **kw)
    return ST.STOM().propagate_in_video(frames, ov, c.vip, shape=c.shape, tracks=tracks, visibility=vis)


def describe(c, got):
    diff = np.argwhere((got != c.expected).any(-1))
    return f"{c.name}: {len(diff)} pixels differ, first (t, y, x) {diff[:5].tolist()}; frames touched by numpy {[bool((e != f).any()) for e, f in zip(c.expected, c.frames)]}"


@pytest.mark.parametrize("key", CASES, ids=lambda k: "-".join(map(str, k)))
def test_device_route_equals_the_numpy_route(dev, key):
    import torch

    c = get_case(key)
    out = run(c, dev)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == c.frames.shape and out.is_contiguous()
    got = out.cpu().numpy()
    print(describe(c, got))
    assert np.array_equal(got, c.expected), describe(c, got)
    again = run(c, dev, numpy_overlay=True)       # second run, overlay uploaded from numpy this time: bit-identical
    assert torch.equal(again, out)


def test_every_branch_is_reached():
    """What the cases are for, checked on the numpy side: frames that are shifted, frames that are kept, the vip frame, circles drawn and not drawn."""
    seen = set()
    for i in range(len(SIZES)):
        c = flow_case(i)
        for t, fl in c.flows.items():
            seen.add("flow applied" if fl is not None else "flow skipped")
            if fl is not None and not (c.expected[t] != c.frames[t]).any():
                seen.add("shift left the frame")
            if fl is not None and (fl[0] < 0 and fl[0] != int(fl[0])) and (fl[1] < 0 and fl[1] != int(fl[1])):
                seen.add("negative fractional flow")
        assert (c.expected[c.vip] != c.frames[c.vip]).any()
        m = mask_case(i)
        for t in range(m.T):
            if t != m.vip:
                seen.add("circle drawn" if (m.expected[t] != m.frames[t]).any() else "frame kept")
    assert seen == {"flow applied", "flow skipped", "shift left the frame", "negative fractional flow", "circle drawn", "frame kept"}, seen
    kept = {t for t in range(5) if t != flow_case(0).vip and flow_case(0).flows[t] is None}
    assert len(kept) == 1      # group 0: only the frame without a visible point is skipped; the one with exactly N // 2 kept is applied
    assert sum(fl is None for fl in flow_case(1).flows.values()) == 1      # group 1: only N // 2 - 1 visible is skipped
    assert sum(fl is None for fl in flow_case(2).flows.values()) == 1      # group 2: N // 2 kept by the filter is applied, N // 2 - 1 is skipped


@pytest.mark.parametrize("i", range(len(SIZES)))
def test_flow_records_equal_mean_flow(dev, i):
    """The per-frame record {apply, dx, dy, kept} against mean_flow: the decision, and the fp32 bits of the mean."""
    import torch

    from rga3.hip import ops

    c = flow_case(i)
    rec = ops.stom_flow(torch.from_numpy(c.tracks[0]).to(dev), torch.from_numpy(c.vis[0]).to(dev), c.vip).cpu().numpy()
    assert rec.dtype == np.int32 and rec.shape == (c.T, 4) and not rec[c.vip].any()
    for t, fl in c.flows.items():
        dx, dy = rec[t, 1:3].view(np.float32)
        print(c.name, t, "numpy", fl, "device", int(rec[t, 0]), float(dx), float(dy), "kept", int(rec[t, 3]))
        assert bool(rec[t, 0]) == (fl is not None), (c.name, t, fl, rec[t])
        if fl is not None:
            assert np.float32(fl[0]).tobytes() == dx.tobytes() and np.float32(fl[1]).tobytes() == dy.tobytes(), (c.name, t, fl, dx, dy)


def test_many_points_sort_in_lds(dev):
    """N = 10 000 (the reference's grid) and the limit 16 384: the multi-pass sort, odd / even medians of many values."""
    import torch

    from rga3.hip import ops

    rng = np.random.default_rng(7)
    for n in (10000, 16384, 4097):
        vip = np.stack([lattice(rng, 0, 853, n), lattice(rng, 0, 479, n)], 1)
        tracks = np.stack([vip, vip + np.array([3.5, -1.25], np.float32) + lattice(rng, -2, 2, (n, 2)), vip + lattice(rng, -40, 40, (n, 2))])
        vis = rng.random((3, n)) < 0.9
        rec = ops.stom_flow(torch.from_numpy(tracks).to(dev), torch.from_numpy(vis).to(dev), 0).cpu().numpy()
        for t in (1, 2):
            fl = ST.mean_flow(vip, tracks[t], vis[t])
            print(n, t, fl, rec[t].tolist())
            assert bool(rec[t, 0]) == (fl is not None)
            if fl is not None:
                assert np.array_equal(rec[t, 1:3].view(np.float32), np.array(fl, np.float32))
        assert rec[1, 0] == 1


@pytest.mark.parametrize("key", [("flow", 0), ("flow", 1), ("mask", 0), ("mask", 1), ("mask", 3)], ids=lambda k: "-".join(map(str, k)))
def test_no_synchronising_call(dev, key):
    """The whole call under set_sync_debug_mode("error"), with a device overlay and with a numpy overlay (one upload from pinned memory)."""
    import torch

    c = get_case(key)
    args = [on_device(c, dev), on_device(c, dev, numpy_overlay=True)]
    run(c, dev, numpy_overlay=True)      # a first call has sized the workspace; the calls below are the steady state of a clip loop
    torch.cuda.synchronize()
    outs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for frames, ov, tracks, vis in args:
            outs.append(ST.STOM().propagate_in_video(frames, ov, c.vip, shape=c.shape, tracks=tracks, visibility=vis))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for out in outs:
        assert np.array_equal(out.cpu().numpy(), c.expected)


@pytest.mark.parametrize("key", [("flow", 0), ("mask", 0)], ids=lambda k: "-".join(map(str, k)))
def test_result_feeds_the_preprocessors(dev, key):
    import torch

    from rga3.utils.preproc import sam_preprocess_frames

    c = get_case(key)
    got = sam_preprocess_frames(run(c, dev))
    want = sam_preprocess_frames(torch.from_numpy(c.expected).to(dev))
    assert got.shape == (c.T, 3, 1024, 1024) and torch.equal(got, want)


def test_device_refusals_on_the_gpu(dev):
    import torch

    from rga3.hip.lib import Rga3Error

    c = flow_case(0)
    frames, ov, tracks, vis = on_device(c, dev)
    s = ST.STOM()
    for bad in (lambda: s.propagate_in_video(frames, ov, c.vip, tracks=tracks.cpu(), visibility=vis),
                lambda: s.propagate_in_video(frames, ov.cpu(), c.vip, tracks=tracks, visibility=vis),
                lambda: s.propagate_in_video(frames, ov, c.T, tracks=tracks, visibility=vis),
                lambda: s.propagate_in_video(frames.permute(0, 2, 1, 3), ov, c.vip, tracks=tracks, visibility=vis),
                lambda: s.propagate_in_video(frames, ov, c.vip, tracks=tracks, visibility=vis.to(torch.uint8))):
        with pytest.raises(Rga3Error):
            bad()
    with pytest.raises(RuntimeError):
        s.propagate_in_video(frames, ov, c.vip)      # no tracker, no tracks
    out = ST.STOM(tracker=lambda f, o, i: (tracks, vis)).propagate_in_video(frames, ov, c.vip)      # the tracker's return is taken as it is
    assert np.array_equal(out.cpu().numpy(), c.expected)
