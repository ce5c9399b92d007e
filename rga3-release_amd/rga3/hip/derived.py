"""Operands that are a function of the weights alone (packed, concatenated, folded, re-laid-out copies): built once, rebuilt when a source tensor changes.

Imports nothing from ops or the models: ops.py and every model file import this module.
"""
from __future__ import annotations

import torch

_SHARED_MAX = 64
_shared = {}   # owner=None: (name, versions, extra) -> (value, the source tensors)


def versions(*tensors):
    """What a derived operand is compared against: (address, version counter, dtype) of every source that is not None."""
    return tuple((t.data_ptr(), t._version, t.dtype) for t in tensors if t is not None)


def derived(owner, name, *srcs, build, extra=()):
    """build() of the source tensors `srcs`, kept until one of them (or `extra`, a hashable for values that also depend on a call argument) changes.

    owner: the module the value belongs to.  Its entry is owner.__dict__["_wt_cache"][name] = (versions, value[, extra]): one entry per name, a rebuilt or
    re-argumented value replaces the old one.  owner=None, for callers with no module in reach, selects a process-wide store of at most 64 entries (cleared whole
    when full).  build() runs under no_grad and may return any object."""
    ver = versions(*srcs)
    if owner is None:
        key = (name, ver, extra)
        hit = _shared.get(key)
        if hit is None:
            with torch.no_grad():
                value = build()
            if len(_shared) >= _SHARED_MAX:
                _shared.clear()
            # the entry keeps its sources alive: the address of a freed tensor can be handed to another one at version 0, which this key could not tell apart
            hit = _shared[key] = (value, srcs)
        return hit[0]
    cache = owner.__dict__.setdefault("_wt_cache", {})
    tail = () if extra == () else (extra,)
    hit = cache.get(name)
    if hit is None or hit[0] != ver or hit[2:] != tail:
        with torch.no_grad():
            hit = cache[name] = (ver, build()) + tail
    return hit[1]


def put(owner, name, srcs, value, extra=()):
    """Make `value` owner's entry `name` for the sources `srcs`, as derived() would have stored it: for values that are built for many owners at once (one stacked
    build, every owner given its slice), which derived() then serves until a source or `extra` changes."""
    owner.__dict__.setdefault("_wt_cache", {})[name] = (versions(*srcs), value) + (() if extra == () else (extra,))


def held(owner, name, srcs=None, extra=()):
    """The value of owner's entry `name`, None if there is none; with `srcs`, None also if derived(owner, name, *srcs, extra=extra) would rebuild it."""
    hit = owner.__dict__.get("_wt_cache", {}).get(name)
    if hit is None or (srcs is not None and (hit[0] != versions(*srcs) or hit[2:] != (() if extra == () else (extra,)))):
        return None
    return hit[1]
