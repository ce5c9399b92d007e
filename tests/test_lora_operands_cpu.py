"""The operands derived from LoRA factors (rga3.model.qwen_train: sA, A^T, (sB)^T per projection, the W2 / Wn block matrices per attention module) on CPU
tensors -- their builds are plain torch ops: who owns them, when they are rebuilt, and which buffers a rebuild writes."""
import gc
import weakref

import pytest
import torch

from rga3.model import qwen_train as QT
from rga3.model.qwen2_5_vl import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration
from tests.qwen_tiny import product_cfg_kwargs

R, HQ, HK, D = 32, 8, 2, 16          # LoRA rank; query heads, key / value heads, head size of the model below
NQ, NALL = HQ * D, (HQ + 2 * HK) * D


def build(seed):
    kw = dict(product_cfg_kwargs(), vocab_size=320, hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2)
    kw["vision_config"] = dict(kw["vision_config"], depth=1, fullatt_block_indexes=[0])
    m = Qwen2_5_VLForConditionalGeneration(Qwen2_5_VLConfig(**kw))
    assert len(QT.add_lora(m, r=R, alpha=64)) == 6
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "lora_" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return m.to(torch.bfloat16)


def factors(lin):
    return lin.lora_A["default"].weight.detach(), lin.lora_B["default"].weight.detach()


def check_projection(lin):
    """_lora_ops(lin) against its definition, exactly: the scaling is applied in bf16 to the bf16 factor, as the build does."""
    A, B = factors(lin)
    sA, At, Bts = QT._lora_ops(lin)
    assert torch.equal(sA, A * lin.scaling) and torch.equal(At, A.t()) and torch.equal(Bts, (B * lin.scaling).t())


def check_attention(at):
    """_lora_cat_ops(at) against its definition, exactly: W2 = [B_q 0; 0 0; 0 B_v], Wn = [(s B_q)^T 0 0; 0 0 (s B_v)^T]."""
    Bq, Bv = factors(at.q_proj)[1], factors(at.v_proj)[1]
    W2, Wn = QT._lora_cat_ops(at)
    want2 = torch.zeros(NALL, 2 * R, dtype=Bq.dtype)
    want2[:NQ, :R], want2[NQ + HK * D:, R:] = Bq, Bv
    wantn = torch.zeros(2 * R, NALL, dtype=Bq.dtype)
    wantn[:R, :NQ], wantn[R:, NQ + HK * D:] = (Bq * at.q_proj.scaling).t(), (Bv * at.v_proj.scaling).t()
    assert torch.equal(W2, want2) and torch.equal(Wn, wantn)


def check_model(m):
    for layer in m.model.layers:
        at = layer.self_attn
        check_projection(at.q_proj)
        check_projection(at.v_proj)
        check_attention(at)


def test_operands_die_with_the_model():
    m = build(1)
    QT.lora_refresh(m.model.layers)
    at = m.model.layers[1].self_attn
    refs = [weakref.ref(t) for t in QT._lora_ops(at.q_proj) + QT._lora_cat_ops(at)]
    assert len(refs) == 5 and all(r() is not None for r in refs)
    del m, at
    gc.collect()
    assert [r() is None for r in refs] == [True] * 5


def test_no_module_level_tensor_containers():
    for name in ("_lora_cache", "_lora_cat", "_lora_cat_store"):
        assert not hasattr(QT, name), name
    holders = [n for n, v in vars(QT).items() if isinstance(v, (dict, list, tuple, set))
               and any(isinstance(x, torch.Tensor) for x in (v.values() if isinstance(v, dict) else v))]
    assert holders == []


def test_entries_are_in_the_owner_layout_of_derived():
    from rga3.hip.derived import versions

    m = build(1)
    QT.lora_refresh(m.model.layers)
    at = m.model.layers[2].self_attn
    q = at.q_proj
    ver, val, extra = q.__dict__["_wt_cache"]["lora"]
    assert ver == versions(q.lora_A["default"].weight, q.lora_B["default"].weight) and extra == 2.0
    assert all(a is b for a, b in zip(val, QT._lora_ops(q)))                       # derived() serves what lora_refresh stored
    ver, val, extra = at.__dict__["_wt_cache"]["lora_cat"]
    assert ver == versions(q.lora_B["default"].weight, at.v_proj.lora_B["default"].weight) and extra == (2.0, 2.0)
    assert all(a is b for a, b in zip(val, QT._lora_cat_ops(at)))
    assert not any("_wt_cache" in k for k in m.state_dict())


@pytest.mark.parametrize("refresh", [True, False], ids=["all-modules build", "per-module fallback"])
def test_in_place_copy_into_lora_b_is_followed(refresh):
    m = build(1)
    QT.lora_refresh(m.model.layers)
    check_model(m)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for layer in m.model.layers:
            for lin in (layer.self_attn.q_proj, layer.self_attn.v_proj):
                B = lin.lora_B["default"].weight
                B.copy_((torch.randn(B.shape, generator=g) * 0.2).to(B.dtype))         # same storage, version + 1: what the optimizer does
    if refresh:
        QT.lora_refresh(m.model.layers)
    check_model(m)


def test_a_changed_scaling_is_followed():
    m = build(1)
    QT.lora_refresh(m.model.layers)
    at = m.model.layers[1].self_attn           # a middle layer: lora_refresh probes the first and the last, the per-module lookups must notice
    old = QT._lora_ops(at.q_proj)[2].clone()
    at.q_proj.scaling = 3.0
    at.v_proj.scaling = 0.5
    QT.lora_refresh(m.model.layers)
    check_model(m)
    assert not torch.equal(QT._lora_ops(at.q_proj)[2], old)
    assert len({QT._lora_cat_ops(layer.self_attn)[0].data_ptr() for layer in m.model.layers}) == 3


def test_a_model_built_after_another_was_dropped_gets_its_own_operands():
    for i in range(10):
        m = build(100 + i)                     # other factors every time: an entry left by a dead model at a reused id or address would show
        QT.lora_refresh(m.model.layers)
        check_model(m)
        del m
        gc.collect()


def test_the_stacked_base_is_reused_and_layers_never_share_a_block_matrix():
    m = build(1)
    QT.lora_refresh(m.model.layers)
    ptrs = [tuple(t.data_ptr() for t in QT._lora_cat_ops(layer.self_attn)) for layer in m.model.layers]
    assert len({p[0] for p in ptrs}) == 3 and len({p[1] for p in ptrs}) == 3
    with torch.no_grad():
        for layer in m.model.layers:
            B = layer.self_attn.q_proj.lora_B["default"].weight
            B.copy_(B * 2)
    QT.lora_refresh(m.model.layers)
    assert [tuple(t.data_ptr() for t in QT._lora_cat_ops(layer.self_attn)) for layer in m.model.layers] == ptrs      # rewritten in place: no allocation per step
    check_model(m)
    # per-module fallback (per-layer scaling: the all-modules build refuses): every layer gets a buffer of its own, and keeps it over the next update
    for li, layer in enumerate(m.model.layers):
        layer.self_attn.q_proj.scaling = 2.5 + 0.5 * li
    QT.lora_refresh(m.model.layers)
    check_model(m)
    own = [QT._lora_cat_ops(layer.self_attn)[0].data_ptr() for layer in m.model.layers]
    assert len(set(own)) == 3
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.v_proj.lora_B["default"].weight.add_(1)
    check_model(m)
    assert [QT._lora_cat_ops(layer.self_attn)[0].data_ptr() for layer in m.model.layers] == own
