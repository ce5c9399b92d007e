"""Loader for tests/golden/jf_cases.npz (J&F scoring cases scored by the reference's own metrics.py; generator: tests/golden/make_jf_fixtures.py)."""
import functools
import os
from types import SimpleNamespace

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jf_cases.npz")
COUNT_NAMES = ("n_fg", "n_gt", "fg_match", "gt_match", "inter", "union")


@functools.lru_cache(maxsize=None)
def gold():
    with np.load(PATH) as g:
        return {k: g[k] for k in g.files}


def names():
    return [str(n) for n in gold()["names"]]


def case(name: str) -> SimpleNamespace:
    """ann / seg / void: bool arrays of the stored shape ([T, h, w] or [h, w]; void None if the case has none); counts int64 [T, 6]; F / J as the reference
    returned them (arrays of length T, 0-d for 2-D masks)."""
    g = gold()
    shape = tuple(int(v) for v in g[name + ".shape"])
    unpack = lambda k: np.unpackbits(g[k])[: int(np.prod(shape))].reshape(shape).astype(bool)
    return SimpleNamespace(name=name, shape=shape, ann=unpack(name + ".ann"), seg=unpack(name + ".seg"), void=unpack(name + ".void") if name + ".void" in g else None,
                           bound_th=float(g[name + ".bound_th"]), radius=int(g[name + ".radius"]), counts=g[name + ".counts"], F=g[name + ".F"], J=g[name + ".J"])
