"""CPU: the next-token selector's reference (tests/select_ref.py) against the installed transformers' own logits processors and against HF's penalised greedy
generate() on the tiny model (tests/golden/qwen_tiny_generate.npz); how generate() resolves its sampling arguments against a generation config; the
generation_config.json round trip; the four new symbols in header, ctypes table and library."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import select_ref as R
from tests.test_abi import header_decls

GEN_GOLD = os.path.join(os.path.dirname(__file__), "golden", "qwen_tiny_generate.npz")


def bf16_grid_logits(B, V, seed, std=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * std).to(torch.bfloat16).float()


def seen_table(B, V, seed, frac=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, V, generator=g) < frac).to(torch.uint8)


def well_separated_inputs(B, V, penalty, temperature, top_k, top_p):
    """(logits, seen, the f32 reference's rows) of the first seed at which no row ties across the k-th place and no tail sum lies within 1e-4 of the top-p threshold:
    conditions on the inputs alone, under which HF's rule and the reference's have one answer."""
    for seed in range(100):
        logits, seen = bf16_grid_logits(B, V, seed=1000 * seed + V), seen_table(B, V, seed=1000 * seed + V + 1)
        refs = R.select(logits, seen, penalty, temperature, top_k, top_p)
        if all((len(r["order"]) == V or r["scores"][r["order"][-1]] > r["scores"].sort(descending=True).values[len(r["order"])]) and (top_p == 1 or r["margin_p"] > 1e-4) for r in refs):
            return logits, seen, refs
    raise AssertionError("no well separated inputs in 100 seeds")


# ------------------------------------------------------------------------------------------------ 1. HF's processors
@pytest.mark.parametrize("V", [64, 320, 4099])
@pytest.mark.parametrize("top_k,top_p,temperature,penalty", [(50, 0.9, 0.7, 1.05), (8, 0.5, 1.3, 1.3), (64, 1.0, 1.0, 2.0), (1, 0.9, 0.7, 1.05), (20, 0.99, 0.1, 1.0)])
def test_reference_equals_hf_processors(V, top_k, top_p, temperature, penalty):
    """RepetitionPenalty -> Temperature -> TopK -> TopP of the installed transformers on f32 tensors: the tokens they leave finite are the reference's kept set and
    their scores there are the reference's, bit for bit.  The inputs have no tie across the k-th place and no tail sum within 1e-4 of the top-p threshold (HF
    normalises before it sums, the reference compares unnormalised sums with a scaled threshold: the two round differently)."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    B = 3
    logits, seen, refs = well_separated_inputs(B, V, penalty, temperature, top_k, top_p)
    ids = [seen[b].nonzero()[:, 0] for b in range(B)]
    n = max(len(i) for i in ids)
    input_ids = torch.stack([torch.cat([i, i[:1].expand(n - len(i))]) for i in ids])      # rows padded with a repeat: HF gathers duplicates too
    x = logits.clone()
    x = lp.RepetitionPenaltyLogitsProcessor(penalty=penalty)(input_ids, x)
    x = lp.TemperatureLogitsWarper(temperature)(input_ids, x)
    assert torch.equal(x, R.scores(logits, seen, penalty, temperature))
    x = lp.TopKLogitsWarper(top_k=top_k)(input_ids, x)
    if top_p < 1:
        x = lp.TopPLogitsWarper(top_p=top_p)(input_ids, x)
    for b, r in enumerate(refs):
        s = r["scores"]
        kept = torch.isfinite(x[b]).nonzero()[:, 0]
        assert torch.equal(kept, r["kept"].sort().values), (b, kept, r["kept"])
        assert torch.equal(x[b][kept], s[kept])
        assert r["token"] == int(s.argmax())


def test_reference_orders_ties_zeros_and_infinities():
    x = torch.tensor([1.0, -0.0, 0.0, 1.0, float("-inf"), -2.0])
    r = R.select_row(x, top_k=6, u=0.0)
    assert r["order"].tolist() == [0, 3, 1, 2, 5, 4] and r["token"] == 0
    assert R.select_row(torch.full((5,), float("-inf")).index_fill(0, torch.tensor([3]), -7.0), top_k=3, top_p=0.5, u=0.999)["token"] == 3
    seen = torch.tensor([1, 0, 0, 0, 0, 0], dtype=torch.uint8)
    assert R.select_row(x, seen, penalty=1.5)["token"] == 3                      # 1.0 / 1.5 loses to the unseen 1.0
    assert R.select_row(-x.abs() - 1, seen, penalty=1.5)["token"] == 1           # -2 * 1.5 loses to -1
    for dt in (torch.float32, torch.float64):
        toks, mu, mp = R.draws(x, torch.tensor([0.0, 0.3, 0.6, 0.99]), top_k=4, dtype=dt)
        assert toks.tolist() == [R.select_row(x, top_k=4, u=u, dtype=dt)["token"] for u in (0.0, 0.3, 0.6, 0.99)]


# ------------------------------------------------------------------------------------------------ 2. HF's penalised generate()
def test_reference_reproduces_hf_penalised_generate():
    g = np.load(GEN_GOLD, allow_pickle=False)
    p = float(g["penalty"])
    ids, S0 = torch.from_numpy(g["ids"]), g["input_ids"].shape[1]
    assert p in (1.05, 1.3, 2.0) and not np.array_equal(g["ids"], g["plain_ids"]) and ids.shape[1] == S0 + 8
    V = g["logits"].shape[-1]
    for t in range(8):
        seen = torch.zeros(1, V, dtype=torch.uint8).scatter_(1, ids[:, :S0 + t], 1)
        r = R.select(torch.from_numpy(g["logits"][:, t]), seen, penalty=p)[0]
        assert r["token"] == int(ids[0, S0 + t]), t
        assert np.array_equal(r["scores"].numpy().view(np.int32), g["scores"][0, t].view(np.int32)), t


# ------------------------------------------------------------------------------------------------ 3. argument resolution
def _cfg():
    from rga3.model.qwen2_5_vl import Qwen2_5_VLConfig

    return Qwen2_5_VLConfig(vocab_size=320, eos_token_id=319, pad_token_id=None)


QWEN_GC = dict(do_sample=True, temperature=0.1, top_k=1, top_p=0.001, repetition_penalty=1.05, eos_token_id=[151645, 151643], pad_token_id=151643, bos_token_id=151643)


def test_resolution_without_a_generation_config():
    from rga3.model.qwen2_5_vl import resolve_generation as res

    c = _cfg()
    assert res(None, c) == dict(max_new_tokens=128, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, eos_token_id=[319],
                                pad_token_id=None, route="default")
    for name, off in (("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("repetition_penalty", 1.0), ("do_sample", False)):
        assert res(None, c, **{name: None})[name] == off
    assert res(None, c, eos_token_id=None)["eos_token_id"] == [319] and res(None, c, eos_token_id=[7, 3])["eos_token_id"] == [3, 7]
    assert res(None, c, do_sample=True)["route"] == "default" and res(None, c, do_sample=True, temperature=0.5, top_p=1.0, top_k=None)["route"] == "default"
    assert res(None, c, repetition_penalty=1.3)["route"] == "select" and res(None, c, repetition_penalty=1.3, top_k=500, top_p=0.2)["route"] == "select"
    assert res(None, c, do_sample=True, top_k=64, top_p=0.9)["route"] == "select" and res(None, c, do_sample=True, repetition_penalty=0.9)["route"] == "penalize"
    assert res(None, c, max_new_tokens=3)["max_new_tokens"] == 3
    for bad in (dict(do_sample=True, top_p=0.9), dict(do_sample=True, top_k=65), dict(do_sample=True, top_p=0.9, top_k=0), dict(do_sample=True, top_k=100, repetition_penalty=1.1)):
        with pytest.raises(NotImplementedError, match="64"):
            res(None, c, **bad)
    for bad in (dict(repetition_penalty=0.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(do_sample=True, top_k=5, temperature=0.0)):
        with pytest.raises(ValueError):
            res(None, c, **bad)


def test_resolution_with_a_generation_config():
    from rga3.model.qwen2_5_vl import GenerationConfig, resolve_generation as res

    c, gc = _cfg(), GenerationConfig(**QWEN_GC)
    r = res(gc, c)
    assert r == dict(max_new_tokens=128, do_sample=True, temperature=0.1, top_k=1, top_p=0.001, repetition_penalty=1.05, eos_token_id=[151643, 151645],
                     pad_token_id=151643, route="select")
    # the reference's evaluation call (inference_videorefer.py:186-193): sampling off, the warpers off -- the penalty of the config stays
    r = res(gc, c, do_sample=False, temperature=None, top_p=None, top_k=None, max_new_tokens=1024)
    assert r == dict(max_new_tokens=1024, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.05, eos_token_id=[151643, 151645],
                     pad_token_id=151643, route="select")
    assert res(gc, c, repetition_penalty=None, do_sample=False)["route"] == "default"
    assert res(gc, c, repetition_penalty=1.0, top_k=None, top_p=None)["route"] == "default"          # plain sampling at the config's temperature
    assert res(gc, c, repetition_penalty=1.0, top_k=None, top_p=None)["temperature"] == 0.1
    assert res(gc, c, top_k=None, top_p=None)["route"] == "penalize"
    assert res(gc, c, top_k=50, top_p=0.9, temperature=0.7)["top_k"] == 50 and res(gc, c, eos_token_id=5)["eos_token_id"] == [5]
    with pytest.raises(NotImplementedError):
        res(gc, c, top_k=None)                                                                         # the config's top_p 0.001 without a top-k
    part = GenerationConfig(repetition_penalty=1.2, max_new_tokens=40)
    r = res(part, c)
    assert (r["repetition_penalty"], r["max_new_tokens"], r["do_sample"], r["top_k"], r["eos_token_id"], r["route"]) == (1.2, 40, False, 0, [319], "select")


# ------------------------------------------------------------------------------------------------ 4. generation_config.json
def test_generation_config_round_trip(tmp_path):
    from rga3.model.qwen2_5_vl import GenerationConfig
    from rga3.model.qwen_2_5_vl_sam2 import UniGRConfig, UniGRModel
    from tests.test_checkpoint_cpu import TINY

    m = UniGRModel(UniGRConfig(**TINY))
    assert m.generation_config is None
    m.save_pretrained(str(tmp_path / "plain"))
    assert "generation_config.json" not in os.listdir(tmp_path / "plain")
    assert UniGRModel.from_pretrained(str(tmp_path / "plain"), config=m.config).generation_config is None
    m.generation_config = GenerationConfig(**QWEN_GC)
    m.save_pretrained(str(tmp_path / "gc"))
    assert json.load(open(tmp_path / "gc" / "generation_config.json")) == QWEN_GC            # unknown keys (bos_token_id) are kept
    m2 = UniGRModel.from_pretrained(str(tmp_path / "gc"), config=m.config)
    assert m2.generation_config == m.generation_config and m2.generation_config.repetition_penalty == 1.05 and m2.generation_config.eos_token_id == [151645, 151643]
    for k in GenerationConfig.FIELDS:
        assert hasattr(m2.generation_config, k)


# ------------------------------------------------------------------------------------------------ 5. symbols
def test_selector_symbols_in_header_table_and_library():
    from rga3.hip import lib

    decls = header_decls()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ("rga3_mark_tokens", "rga3_penalize_logits", "rga3_select_ws_bytes", "rga3_select_token"):
        assert name in decls and name in lib.SIGNATURES and hasattr(so, name), name
    L = lib.load()
    assert L.rga3_select_ws_bytes(8, 152064) > 0 and L.rga3_select_ws_bytes(0, 5) < 0 and L.rga3_select_ws_bytes(1, 0) < 0
