"""Scratch that kernels receive by pointer (stream-K slabs / flags, TN ticket words, the attention kernels' partial sums, the STOM masks): who owns it, and the one
procedure that captures a step into a hipGraph.  Imports nothing from ops or the models: ops.py and every model file import this module."""
import contextlib
import weakref

import torch

from .derived import versions

NAMES = ("gemm", "tn", "memattn", "stom", "decattn")
_by_stream = {}               # (device index, stream handle) -> the Scratch of the eager launches on that stream, kept for the life of the process
_by_token = {}                # workspace_scope(token) -> its Scratch, kept for the life of the process
_owned = weakref.WeakSet()    # every Scratch that was entered as a scope: the health checks reach its GEMM workspaces through here, its owner alone keeps it alive
_current = [None]             # the Scratch of the innermost workspace_scope


class Scratch:
    """The named buffers of one owner, on one device.  Once entered as a scope it never releases a buffer it has handed out (a captured graph points at it): a buffer
    that take() outgrows moves to `retired` and is freed with the Scratch, i.e. when the owner drops it together with the graphs captured inside it."""
    gemm = tn = memattn = stom = decattn = retired = None     # retired: [(name, tensor)] once entered as a scope; None: a grown buffer releases its predecessor

    def take(self, name, count, dtype, device, zero=False):
        """The buffer `name` of at least `count` elements: the existing one if it is large enough, else a new one (zero-filled once if `zero`)."""
        t = getattr(self, name)
        if t is None or t.numel() < count:
            if t is not None and self.retired is not None:
                self.retired.append((name, t))
            t = (torch.zeros if zero else torch.empty)(count, dtype=dtype, device=device)
            setattr(self, name, t)
        return t

    def held(self):     # [(name, tensor)] of every buffer this Scratch keeps alive, the retired ones included
        return [(n, getattr(self, n)) for n in NAMES if getattr(self, n) is not None] + list(self.retired or ())


def of(device) -> Scratch:
    """The Scratch of a launch on `device` now: the scope's, else the one of (device, current stream).  Runs on every launch: one key, one lookup."""
    if _current[0] is not None:
        return _current[0]
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    return _by_stream.get(key) or _by_stream.setdefault(key, Scratch())


def gemm_buffers():
    """Every live GEMM workspace of this process: the streams' and the owner-held ones, retired ones included (what the stream-K health checks walk)."""
    return [t for s in list(_by_stream.values()) + list(_owned) for n, t in s.held() if n == "gemm"]


@contextlib.contextmanager
def workspace_scope(scratch):
    """``with ops.workspace_scope(scratch): ...`` -- every scratch buffer handed to a kernel inside the block comes from `scratch`, a Scratch, not from the Scratch of
    (device, current stream).  A captured hipGraph bakes the POINTERS it saw and is replayed on whatever stream is current, so the scratch of a capture must belong
    to the graph's owner, not to a stream handle: torch.cuda.Stream() hands out a pool of 32 round-robin, and a later eager launch on a stream that happens to BE a
    capture stream would share that graph's scratch while the graph replays elsewhere.  The owner keeps the Scratch beside the graphs captured inside it, replays
    them one after the other and drops them together: only that frees the buffers.  A hashable token in place of a Scratch names one kept for the life of the process."""
    s = scratch if isinstance(scratch, Scratch) else _by_token.setdefault(scratch, Scratch())
    _owned.add(s)
    s.retired = [] if s.retired is None else s.retired
    old, _current[0] = _current[0], s
    try:
        yield s
    finally:
        _current[0] = old


def capture_step(body, scratch, *, stream=None, pool=None, between=lambda: None):
    """Capture body() into a hipGraph whose scratch is `scratch` -> (graph, what the captured body() returned); `stream` / `pool` are torch.cuda.graph's.  body() first
    runs for real on a side stream (`stream`, else a fresh one), so that tuner picks, workspaces and lazily built tables exist before the capture, and between() undoes
    what that run must not leave behind.  Capturing executes nothing: the caller replays."""
    cur, side = torch.cuda.current_stream(), stream if stream is not None else torch.cuda.Stream()
    side.wait_stream(cur)
    with workspace_scope(scratch):
        with torch.cuda.stream(side):
            body()
        cur.wait_stream(side)
        between()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=pool, stream=stream):
            return graph, body()


def drop_if_weights_changed(cache: dict, module):
    """The graphs kept in `cache` read the weights of `module` (and the operands derived from them) through their pointers: if a parameter was updated in place or
    replaced since cache["sig"] was taken, clear the cache -- the graphs and, with them, the Scratch objects they point into -- and store the new signature."""
    sig = versions(*module.parameters())
    if cache.get("sig") != sig:
        if len(cache) > 1 and torch.cuda.is_initialized():     # a dropped graph's replay may still run on a stream nothing here waits on, and the re-capture's warm-up
            torch.cuda.synchronize()                            # allocates before torch.cuda.graph's own device sync: finish it before its scratch is freed (slow path only)
        cache.clear()
        cache["sig"] = sig
