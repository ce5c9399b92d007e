"""rga3.hip.derived on CPU tensors with plain-torch builders: when an entry is kept, when it is rebuilt, where it lives."""
import copy
import gc
import weakref

import pytest
import torch
import torch.nn as nn

from rga3.hip import derived as D
from rga3.hip.derived import derived, versions


class Owner(nn.Module):
    def __init__(self, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.arange(6.0).view(2, 3))
        self.bias = nn.Parameter(torch.ones(2)) if bias else None
        self.calls = 0

    def doubled(self, extra=()):
        def build():
            self.calls += 1
            self.grad_seen = torch.is_grad_enabled()
            return self.weight.detach() * 2 + (0 if self.bias is None else self.bias.detach()[:, None])
        return derived(self, "doubled", self.weight, self.bias, build=build, extra=extra)


@pytest.fixture(autouse=True)
def empty_shared_store():
    D._shared.clear()
    yield
    D._shared.clear()


def test_versions_is_pointer_counter_dtype_of_every_tensor_given():
    a, b = torch.zeros(3), torch.zeros(2, dtype=torch.float64)
    assert versions(a, None, b) == ((a.data_ptr(), a._version, torch.float32), (b.data_ptr(), b._version, torch.float64))
    assert versions() == () and versions(None) == ()


def test_hit_returns_the_same_object_without_building():
    m = Owner()
    v = m.doubled()
    assert m.calls == 1 and torch.equal(v, m.weight.detach() * 2 + 1)
    assert m.doubled() is v and m.doubled() is v and m.calls == 1


def test_in_place_update_rebuilds():
    m = Owner()
    v = m.doubled()
    with torch.no_grad():
        m.weight.add_(1)
    v2 = m.doubled()
    assert m.calls == 2 and v2 is not v and torch.equal(v2, m.weight.detach() * 2 + 1)
    assert m.doubled() is v2 and m.calls == 2


def test_repointed_data_rebuilds():
    m = Owner()
    m.doubled()
    other = torch.full((2, 3), 7.0)
    m.weight.data = other
    assert torch.equal(m.doubled(), other * 2 + 1) and m.calls == 2
    m.bias.data = torch.zeros(2)          # a bias counts like a weight
    assert torch.equal(m.doubled(), other * 2) and m.calls == 3


def test_dtype_change_rebuilds():
    w = torch.zeros(4, dtype=torch.float32)
    o = nn.Module()
    calls = []
    get = lambda t: derived(o, "v", t, build=lambda: calls.append(1) or t.clone())
    get(w)
    get(w)
    assert len(calls) == 1
    same_bytes = w.view(torch.int32)      # same address, same version counter, other dtype
    assert same_bytes.data_ptr() == w.data_ptr() and same_bytes._version == w._version
    assert get(same_bytes).dtype == torch.int32 and len(calls) == 2


def test_bias_appearing_rebuilds():
    m = Owner(bias=False)
    v = m.doubled()
    assert torch.equal(v, m.weight.detach() * 2)
    m.bias = nn.Parameter(torch.ones(2))
    assert torch.equal(m.doubled(), m.weight.detach() * 2 + 1) and m.calls == 2


def test_extra_is_compared_and_a_new_extra_replaces_the_entry():
    m = Owner()
    a = m.doubled(extra=(4, 4))
    assert m.doubled(extra=(4, 4)) is a and m.calls == 1
    b = m.doubled(extra=(8, 4))
    assert b is not a and m.calls == 2
    assert list(m.__dict__["_wt_cache"]) == ["doubled"]            # one entry per name: (8, 4) took the place of (4, 4)
    assert m.doubled(extra=(4, 4)) is not a and m.calls == 3
    assert m.doubled() is not None and m.calls == 4                # no extra is one more value of extra


def test_two_names_on_one_owner_are_independent():
    o = nn.Module()
    w1, w2 = torch.ones(2), torch.ones(2)
    n = {"a": 0, "b": 0}

    def get(name, w):
        def build():
            n[name] += 1
            return w + 1
        return derived(o, name, w, build=build)
    a, b = get("a", w1), get("b", w2)
    w1.add_(1)
    assert get("b", w2) is b and get("a", w1) is not a and n == {"a": 2, "b": 1}
    assert set(o.__dict__["_wt_cache"]) == {"a", "b"}


def test_build_runs_without_grad_and_may_return_any_object():
    m = Owner()
    with torch.enable_grad():
        v = m.doubled()
    assert m.grad_seen is False and not v.requires_grad
    o = nn.Module()
    w = torch.ones(2, requires_grad=True)
    d = derived(o, "packs", w, build=lambda: {"w2": w * 2, "n": 3})
    assert d["n"] == 3 and not d["w2"].requires_grad and derived(o, "packs", w, build=dict) is d


def test_deepcopy_owns_its_entries():
    m = Owner()
    v = m.doubled()
    c = copy.deepcopy(m)
    with torch.no_grad():
        c.weight.mul_(3)
    vc = c.doubled()
    assert torch.equal(vc, c.weight.detach() * 2 + 1) and not torch.equal(vc, v)
    assert m.doubled() is v and m.calls == 1
    assert c.__dict__["_wt_cache"] is not m.__dict__["_wt_cache"]


def test_owner_layout_is_versions_then_value():
    m = Owner()
    v = m.doubled()
    assert m.__dict__["_wt_cache"]["doubled"] == (versions(m.weight, m.bias), v)
    e = m.doubled(extra=5)
    entry = m.__dict__["_wt_cache"]["doubled"]
    assert entry[0] == versions(m.weight, m.bias) and entry[1] is e
    assert "_wt_cache" not in m.state_dict() and "_wt_cache" not in dict(m.named_buffers())


def test_shared_store_keeps_its_sources_alive():
    w = torch.ones(3)
    ref = weakref.ref(w)
    v = derived(None, "neg", w, build=lambda: -w)
    assert derived(None, "neg", w, build=lambda: 1 / 0) is v
    del w
    gc.collect()
    assert ref() is not None, "a source of a live entry was freed: its address could be handed to another tensor"
    D._shared.clear()
    gc.collect()
    assert ref() is None


def test_shared_store_misses_like_an_owner_does():
    w = torch.ones(3)
    calls = []
    get = lambda extra=(): derived(None, "neg", w, build=lambda: calls.append(torch.is_grad_enabled()) or -w, extra=extra)
    a = get()
    w.add_(1)
    b = get()
    assert b is not a and torch.equal(b, -w) and get() is b
    assert get(extra=2) is not b and get(extra=2) is get(extra=2)
    assert derived(None, "other", w, build=lambda: w * 1) is not b
    assert calls == [False, False, False]


def test_shared_store_never_exceeds_64_entries():
    ws = [torch.ones(1) for _ in range(200)]
    for w in ws:
        derived(None, "neg", w, build=lambda: -w)
        assert len(D._shared) <= 64
    assert derived(None, "neg", ws[-1], build=lambda: 1 / 0) is not None      # the newest entry survives a clear


def test_put_stores_what_derived_then_serves():
    m = Owner()
    v = torch.full((2, 3), 9.0)
    D.put(m, "doubled", (m.weight, m.bias), v)                      # a value built elsewhere, e.g. this owner's slice of a build over many owners
    assert m.__dict__["_wt_cache"]["doubled"] == (versions(m.weight, m.bias), v)
    assert m.doubled() is v and m.calls == 0 and D.held(m, "doubled") is v and D.held(m, "doubled", (m.weight, m.bias)) is v
    with torch.no_grad():
        m.weight.add_(1)
    assert D.held(m, "doubled") is v and D.held(m, "doubled", (m.weight, m.bias)) is None      # kept, but no longer current
    assert torch.equal(m.doubled(), m.weight.detach() * 2 + 1) and m.calls == 1
    D.put(m, "doubled", (m.weight, m.bias), v, extra=5)
    assert m.__dict__["_wt_cache"]["doubled"][2:] == (5,) and list(m.__dict__["_wt_cache"]) == ["doubled"]
    assert m.doubled(extra=5) is v and m.calls == 1 and D.held(m, "doubled", (m.weight, m.bias), 5) is v
    assert D.held(m, "doubled", (m.weight, m.bias)) is None and D.held(m, "doubled", (m.weight, m.bias), 6) is None
    assert m.doubled(extra=6) is not v and m.calls == 2
    assert D.held(nn.Module(), "doubled") is None
