"""rga3.hip.scratch on CPU tensors: reuse and growth of a Scratch, what a scope keeps alive, scopes and tokens, what the health checks enumerate, and the
weights-changed rule of the captured-graph caches."""
import gc
import weakref

import pytest
import torch
import torch.nn as nn

from rga3.hip import scratch as S
from rga3.hip.scratch import Scratch, drop_if_weights_changed, workspace_scope

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def registry_as_found():
    streams, tokens = dict(S._by_stream), dict(S._by_token)
    yield
    for d, was in ((S._by_stream, streams), (S._by_token, tokens)):
        d.clear()
        d.update(was)
    assert S._current[0] is None


def scoped():
    with workspace_scope(Scratch()) as s:
        pass
    return s


@pytest.mark.parametrize("owner", [Scratch, scoped])
def test_take_reuses_what_fits_and_grows_otherwise(owner):
    s = owner()
    a = s.take("memattn", 64, torch.float32, CPU)
    assert a.dtype == torch.float32 and a.numel() == 64 and a.device == CPU
    assert s.take("memattn", 64, torch.float32, CPU) is a and s.take("memattn", 3, torch.float32, CPU) is a
    b = s.take("memattn", 65, torch.float32, CPU)
    assert b is not a and b.numel() == 65 and b.data_ptr() != a.data_ptr()
    assert s.take("memattn", 64, torch.float32, CPU) is b                      # the larger buffer serves the smaller request from now on
    assert s.take("stom", 16, torch.uint8, CPU) is not b and s.stom.dtype == torch.uint8     # names are independent
    assert s.memattn is b


def test_zero_buffers_come_back_zero_filled():
    s = Scratch()
    junk = [torch.full((4096,), 255, dtype=torch.uint8) for _ in range(8)]      # dirty the allocator's free lists first
    del junk
    g = s.take("gemm", 4096, torch.uint8, CPU, zero=True)
    t = s.take("tn", 256, torch.int32, CPU, zero=True)
    assert g.numel() == 4096 and not g.any() and t.numel() == 256 and not t.any()
    g[:8] = 1
    assert s.take("gemm", 4096, torch.uint8, CPU, zero=True) is g and int(g.sum()) == 8      # zeroed once, at allocation


def test_a_scope_never_releases_what_it_handed_out():
    s = scoped()
    first = s.take("memattn", 64, torch.float32, CPU)
    ptr, ref = first.data_ptr(), weakref.ref(first)
    second = s.take("memattn", 4096, torch.float32, CPU)
    assert second is not first and any(n == "memattn" and t is first for n, t in s.held())
    del first
    gc.collect()
    assert ref() is not None and ref().data_ptr() == ptr, "a buffer a captured graph may point at was released while its owner lives"
    assert {t.data_ptr() for _, t in s.held()} == {ptr, second.data_ptr()}
    del s
    gc.collect()
    assert ref() is None                                                        # dropping the owner frees everything it holds


def test_a_streams_scratch_releases_the_outgrown_buffer():
    s = Scratch()
    ref = weakref.ref(s.take("decattn", 64, torch.float32, CPU))
    s.take("decattn", 4096, torch.float32, CPU)
    gc.collect()
    assert ref() is None and len(s.held()) == 1


def test_two_owners_never_share_storage():
    a, b = scoped(), scoped()
    for name, dtype in (("gemm", torch.uint8), ("tn", torch.int32), ("memattn", torch.float32), ("stom", torch.uint8), ("decattn", torch.float32)):
        ta, tb = a.take(name, 128, dtype, CPU, zero=name in ("gemm", "tn")), b.take(name, 128, dtype, CPU, zero=name in ("gemm", "tn"))
        assert ta is not tb and ta.untyped_storage().data_ptr() != tb.untyped_storage().data_ptr()
    assert not {t.data_ptr() for _, t in a.held()} & {t.data_ptr() for _, t in b.held()}


def test_nested_scopes_restore_the_outer_one():
    a, b = Scratch(), Scratch()
    assert S._current[0] is None
    with workspace_scope(a) as got:
        assert got is a and S._current[0] is a
        with workspace_scope(b):
            assert S._current[0] is b
        assert S._current[0] is a
        with pytest.raises(RuntimeError, match="inside"):
            with workspace_scope(b):
                raise RuntimeError("inside")
        assert S._current[0] is a
    assert S._current[0] is None
    with pytest.raises(RuntimeError, match="outer"):
        with workspace_scope(a):
            raise RuntimeError("outer")
    assert S._current[0] is None


def test_a_token_names_one_scratch():
    with workspace_scope(("my-graphs", 3)) as s1:
        assert isinstance(s1, Scratch) and S._current[0] is s1
        t = s1.take("tn", 256, torch.int32, CPU, zero=True)
    with workspace_scope(("my-graphs", 3)) as s2, workspace_scope(("my-graphs", 4)) as s3:
        assert s2 is s1 and s3 is not s1 and s2.take("tn", 256, torch.int32, CPU, zero=True) is t
    assert s1.retired is not None                                               # a token's Scratch is a scope like any other: it retires, it does not release


def test_health_checks_enumerate_stream_and_owner_held_workspaces():
    before = {t.data_ptr() for t in S.gemm_buffers()}
    stream = S._by_stream.setdefault((0, 0x7E57), Scratch())                     # what of() keeps for eager launches on (device 0, that stream handle)
    ws = stream.take("gemm", 4096, torch.uint8, CPU, zero=True)
    stream.take("memattn", 64, torch.float32, CPU)
    owner = scoped()
    old = owner.take("gemm", 4096, torch.uint8, CPU, zero=True)
    new = owner.take("gemm", 8192, torch.uint8, CPU, zero=True)                 # (the real workspace has one size; a retired one must still be reached)
    owner.take("tn", 256, torch.int32, CPU, zero=True)
    unused = Scratch()                                                          # never entered: nobody's scope, not enumerated
    unused.take("gemm", 4096, torch.uint8, CPU, zero=True)
    assert owner in S._owned and unused not in S._owned
    assert {t.data_ptr() for t in S.gemm_buffers()} - before == {ws.data_ptr(), old.data_ptr(), new.data_ptr()}
    del owner
    gc.collect()
    assert {t.data_ptr() for t in S.gemm_buffers()} - before == {ws.data_ptr()}


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = nn.Linear(3, 2), nn.Linear(2, 2)


def test_weights_changed_rule():
    m, cache = Net(), {}
    drop_if_weights_changed(cache, m)
    assert set(cache) == {"sig"}
    cache["graph"], cache["scratch"] = object(), Scratch()
    drop_if_weights_changed(cache, m)
    drop_if_weights_changed(cache, m)
    assert set(cache) == {"sig", "graph", "scratch"}                            # nothing was updated: nothing is dropped
    ref = weakref.ref(cache["scratch"])
    with torch.no_grad():
        m.b.bias.mul_(1.0)                                                      # same values, one version counter bumped
    drop_if_weights_changed(cache, m)
    gc.collect()
    assert set(cache) == {"sig"} and ref() is None                              # the graphs go, and their scratch with them
    cache["graph"] = object()
    drop_if_weights_changed(cache, m)
    assert "graph" in cache                                                     # a second call without an update keeps it
    m.a.weight.data = m.a.weight.data.clone()                                   # a replaced tensor counts like an update
    drop_if_weights_changed(cache, m)
    assert set(cache) == {"sig"}
