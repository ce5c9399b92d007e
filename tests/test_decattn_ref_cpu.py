"""CPU: the float64 reference of ops.decode_attn (tests/decattn_ref.py) against torch.softmax and the oracle's rotate-half, and the three new entry points in the
header, the ctypes table and the built library."""
import ctypes
import os

import pytest
import torch

from oracle import qwen25vl as Q
from tests import decattn_ref as R
from tests.qwen_tiny import oracle_cfg
from tests.test_abi import header_decls

NEW = ("rga3_decode_attn", "rga3_decode_attn_ws_floats", "rga3_decode_attn_slice_keys")


def test_new_entry_points_in_header_table_and_library():
    from rga3.hip import lib

    decls = header_decls()
    for name in NEW:
        assert name in decls, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == len(decls[name]), name
    assert "rga3_decode_attn_ws_floats" in lib._INT64_RESULTS
    assert os.path.exists(lib.LIB_PATH), "build the extension first (__graft_entry__.build())"
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(so, name), name
    L = lib.load()
    ks = L.rga3_decode_attn_slice_keys()
    assert ks >= 16 and ks & (ks - 1) == 0
    # host-only query: B * Hq * ceil(cap / KS) partials of D + 2 floats
    assert L.rga3_decode_attn_ws_floats(3, 4 * ks + 1, 28, 128) == 3 * 28 * 5 * 130
    assert L.rga3_decode_attn_ws_floats(0, 64, 28, 128) < 0 and L.rga3_decode_attn_ws_floats(1, 0, 28, 128) < 0


@pytest.mark.parametrize("B,Hq,Hkv,D,cap", [(3, 6, 2, 16, 9), (2, 7, 1, 32, 5), (1, 4, 4, 16, 3)])
def test_reference_equals_torch_softmax(B, Hq, Hkv, D, cap):
    """cos = 1, sin = 0 (no rotation): the reference is softmax attention over the stored rows and the new one; rows at and beyond lens[b] are ignored."""
    c = R.random_case(B, Hq, Hkv, D, cap, seed=B * 100 + D)
    cos, sin = torch.ones(B, D), torch.zeros(B, D)
    lens = [min(b * 3, cap - 1) for b in range(B)]
    c["k_cache"][0, lens[0]:] = float("nan")
    ref = R.decode_attn_ref(c["qkv"], cos, sin, c["k_cache"], c["v_cache"], lens, Hq, Hkv, 0.3)
    G = Hq // Hkv
    for b in range(B):
        n = lens[b]
        K = torch.cat((c["k_cache"][b, :n], c["qkv"][b, Hq:Hq + Hkv][None])).double()
        V = torch.cat((c["v_cache"][b, :n], c["qkv"][b, Hq + Hkv:][None])).double()
        for hq in range(Hq):
            p = torch.softmax((K[:, hq // G] @ c["qkv"][b, hq].double()) * 0.3, 0)
            want = p @ V[:, hq // G]
            assert torch.allclose(ref["out"][b, hq], want, rtol=1e-12, atol=1e-13), (b, hq)
    assert torch.equal(ref["v_row"], c["qkv"][:, Hq + Hkv:])
    assert torch.equal(ref["k_exact"], c["qkv"][:, Hq:Hq + Hkv].double())


def test_full_sequence_is_nan_in_the_reference():
    c = R.random_case(2, 2, 1, 16, 4, seed=3)
    ref = R.decode_attn_ref(c["qkv"], c["cos"], c["sin"], c["k_cache"], c["v_cache"], [4, 1], 2, 1, 0.25)
    assert torch.isnan(ref["out"][0]).all() and torch.isfinite(ref["out"][1]).all()


def test_rotation_equals_the_oracle_on_the_tiny_models_tables():
    """rotate_ref and mrope_tables against oracle.qwen25vl (rotate_half, mrope_cos_sin) at the tiny model's head shape (D = 16, sections (2, 3, 3))."""
    cfg = oracle_cfg()
    D = cfg.text.hidden_size // cfg.text.num_attention_heads
    g = torch.Generator().manual_seed(1)
    B = 5
    pos3 = torch.randint(0, 5001, (3, B), generator=g)
    cos_o, sin_o = Q.mrope_cos_sin(pos3[:, :, None], cfg)           # [B, 1, D]
    cos, sin = R.mrope_tables(pos3, D, theta=cfg.text.rope_theta)
    assert torch.equal(cos, cos_o[:, 0]) and torch.equal(sin, sin_o[:, 0])
    x = torch.randn((B, 8, D), generator=g).to(torch.bfloat16)
    want = x.double() * cos.double()[:, None] + Q.rotate_half(x.double()) * sin.double()[:, None]
    got, mag = R.rotate_ref(x, cos, sin)
    assert torch.allclose(got, want, rtol=1e-14, atol=1e-15)
    assert (mag >= got.abs() - 1e-12).all()
    assert (R.rotation_bound(got, mag) >= 2.0 ** -8 * got.abs()).all()
