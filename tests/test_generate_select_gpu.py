"""GPU: generate() with a repetition penalty, top-k / top-p sampling, a seed and a generation config, on the tiny model of tests/qwen_tiny.py.

HF's penalised greedy run (tests/golden/qwen_tiny_generate.npz) is the outside reference; everything else replays generate()'s own output token by token through
the KV cache and picks with tests/select_ref.py on the host (exact for greedy; under the reference's decision margins for draws)."""
import os

import numpy as np
import pytest
import torch

from oracle.detweights import det_tensor
from tests import select_ref as R
from tests.qwen_tiny import gold
from tests.test_generate_batch_gpu import _count_ops, _left_padded, _reset, fresh_model

pytestmark = pytest.mark.gpu

GEN_GOLD = os.path.join(os.path.dirname(__file__), "golden", "qwen_tiny_generate.npz")


@pytest.fixture(scope="module")
def model(dev):
    """The snapped model (prefill and e4m3 decode evaluate the same function); every test leaves it at ("bf16", "varlen") without a generation config."""
    return fresh_model(dev, snap=True)


class _count_select(_count_ops):
    NAMES = ("select_token", "mark_tokens_", "penalize_logits")


def _step_logits(model, dev, full, S0, am=None, **vision):
    """[steps, B, V] logits (on the device, as the LM head leaves them) of a prefill on full[:, :S0] and teacher-forced single-token steps through the KV cache:
    row t decides token full[:, S0 + t].  am: the prompt's attention mask (left padded)."""
    from rga3.model.qwen2_5_vl import KVCache

    c = model.config
    B = full.shape[0]
    full = full.to(dev)
    am = torch.ones((B, S0), dtype=torch.long, device=dev) if am is None else am.to(dev)
    cache = KVCache(c.num_hidden_layers, B, full.shape[1] + 1, c.num_key_value_heads, c.head_dim, dev, torch.bfloat16)
    with torch.no_grad():
        rows = [model(input_ids=full[:, :S0], attention_mask=am, past_key_values=cache, **vision).logits[:, -1]]
        for t in range(S0, full.shape[1] - 1):
            am = torch.cat([am, torch.ones((B, 1), dtype=am.dtype, device=dev)], 1)
            rows.append(model(input_ids=full[:, t:t + 1].contiguous(), attention_mask=am, past_key_values=cache).logits[:, -1])
    return torch.stack(rows)


def _seen_before(full, upto, V):
    ids = full[:, :upto].cpu()
    return torch.zeros((full.shape[0], V), dtype=torch.uint8).scatter_(1, ids, 1)


def _assert_greedy_replay(model, dev, out, S0, penalty, am=None):
    """Every new token of `out` is the float32 reference's greedy choice on the logits the model gives for the tokens before it, with every earlier id marked."""
    lg = _step_logits(model, dev, out, S0, am).float().cpu()
    for t in range(lg.shape[0]):
        seen = _seen_before(out, S0 + t, lg.shape[-1]) if penalty != 1.0 else None
        want = [r["token"] for r in R.select(lg[t], seen, penalty)]
        assert out[:, S0 + t].tolist() == want, t


# ------------------------------------------------------------------------------------------------ 1. HF
def test_hf_parity_of_the_penalised_greedy_run(dev):
    from rga3.hip import ops

    g, G = np.load(GEN_GOLD, allow_pickle=False), gold()
    p = float(g["penalty"])
    ids, S0 = torch.from_numpy(g["ids"]), g["input_ids"].shape[1]
    assert np.array_equal(g["input_ids"], G["gen_input_ids"])
    vision = dict(pixel_values_videos=det_tensor("pixel_values_full0", (192, 1176), 1.0, seed=5).to(torch.bfloat16).to(dev), video_grid_thw=torch.tensor([[2, 8, 12]]),
                  second_per_grid_ts=torch.tensor([1.0]))
    m = fresh_model(dev, snap=False)
    lg = _step_logits(m, dev, ids, S0, **vision)                                  # [8, 1, V] product logits, teacher-forced on HF's ids
    V = lg.shape[-1]
    top2 = torch.from_numpy(g["scores"][0]).topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 0.05 * float(np.abs(g["logits"]).max())
    assert bool(decided[0]), "the first step must be decided"
    got = []
    for t in range(lg.shape[0]):
        seen = ops.mark_tokens_(torch.zeros((1, V), dtype=torch.uint8, device=dev), ids[:, :S0 + t].to(dev))
        got.append(int(ops.select_token(lg[t], seen, p)[0]))
    got, want = torch.tensor(got), ids[0, S0:]
    print(f"HF parity, penalty {p}: {int(decided.sum())} of {len(decided)} steps decided; product {got.tolist()} HF {want.tolist()}")
    assert torch.equal(got[decided], want[decided])
    with torch.no_grad():
        first = m.generate(input_ids=ids[:, :S0].to(dev), repetition_penalty=p, max_new_tokens=1, **vision)
        assert first.shape == (1, S0 + 1) and int(first[0, S0]) == int(want[0])
        n = int((~decided).nonzero()[0]) if not bool(decided.all()) else len(decided)      # the free run follows HF up to the first undecided step
        run = m.generate(input_ids=ids[:, :S0].to(dev), repetition_penalty=p, max_new_tokens=8, eos_token_id=-1, **vision)
        assert torch.equal(run[0, S0:S0 + n].cpu(), want[:n])
        plain = m.generate(input_ids=ids[:, :S0].to(dev), max_new_tokens=8, eos_token_id=-1, **vision)
        assert not torch.equal(plain, run)                                                    # the argument is not ignored


# ------------------------------------------------------------------------------------------------ 2. the loop by hand
def test_penalised_generate_equals_the_manual_loop(model, dev):
    ids, am = _left_padded((37,), dev, seed=3)
    with torch.no_grad():
        out = model.generate(input_ids=ids, attention_mask=am, repetition_penalty=1.3, max_new_tokens=12, eos_token_id=-1, decode_graph=False)
        plain = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=12, eos_token_id=-1, decode_graph=False)
    assert out.shape == (1, 37 + 12) and not torch.equal(out, plain)
    _assert_greedy_replay(model, dev, out, 37, 1.3)


# ------------------------------------------------------------------------------------------------ 3. graph and eager
@pytest.mark.parametrize("B,route", [(1, "varlen"), (1, "cache"), (2, "cache"), (3, "cache"), (4, "cache")])
def test_graph_equals_eager_with_the_selector_between_replays(B, route, model, dev):
    lens = (21, 33, 27, 30)[:B]
    ids, am = _left_padded(lens, dev, seed=11 + B)
    S, new = max(lens), 24
    gen = lambda **k: model.generate(input_ids=ids, attention_mask=am, max_new_tokens=new, repetition_penalty=1.3, **k)
    try:
        with torch.no_grad():
            model.set_decode_attention(route)
            for kind in ("bf16", "e4m3"):
                model.set_decode_weights(kind)
                with _count_select() as c:
                    eager = gen(eos_token_id=-1, decode_graph=False)
                assert c.n == {"select_token": new, "mark_tokens_": 1, "penalize_logits": 0}
                graph = gen(eos_token_id=-1)
                assert eager.shape == (B, S + new) and torch.equal(eager, graph), kind
                assert any("graph" in st for key, st in model.__dict__["_decode_states"].items() if key[-3:] == (B, route, kind))
                eos = int(eager[0, S + 11])                    # an early new token of sequence 0 as EOS: it arrives between two host checks
                e2, g2 = gen(eos_token_id=eos, decode_graph=False), gen(eos_token_id=eos)
                assert torch.equal(e2, g2), kind
                first = int((eager[0, S:] == eos).nonzero()[0])
                assert torch.equal(e2[0, :S + first + 1], eager[0, :S + first + 1])
                assert bool((e2[0, S + first + 1:] == model.config.pad_token_id).all())
                if B == 1:
                    assert e2.shape[1] == S + first + 1
            s1 = gen(eos_token_id=-1, do_sample=True, top_k=50, top_p=0.9, temperature=0.7, seed=5, decode_graph=False)
            s2 = gen(eos_token_id=-1, do_sample=True, top_k=50, top_p=0.9, temperature=0.7, seed=5)
            assert torch.equal(s1, s2)
    finally:
        _reset(model)


# ------------------------------------------------------------------------------------------------ 4. padding
def test_left_padded_batch_of_three_equals_its_rows_with_the_pad_id_marked(model, dev):
    """HF's penalty gathers all of input_ids, the pad id of a left-padded row included: a row of the batch equals the same padded row run alone (the pad id marked),
    and the unpadded row of the batch equals its unpadded single run."""
    lens, new = (21, 33, 27), 12
    ids, am = _left_padded(lens, dev, seed=5)
    S = max(lens)
    kw = dict(max_new_tokens=new, repetition_penalty=1.3, eos_token_id=-1)
    try:
        model.set_decode_attention("cache")
        model.set_decode_weights("e4m3")
        with torch.no_grad():
            batch = model.generate(input_ids=ids, attention_mask=am, **kw)
            for i, n in enumerate(lens):
                one = model.generate(input_ids=ids[i:i + 1], attention_mask=am[i:i + 1], decode_graph=False, **kw)
                assert torch.equal(batch[i], one[0]), i
            bare = model.generate(input_ids=ids[1:2, S - 33:], decode_graph=False, **kw)
            assert torch.equal(batch[1, S:], bare[0, 33:])
        _assert_greedy_replay(model, dev, batch, S, 1.3, am)        # ... and every row follows the reference with ALL of its input ids marked
    finally:
        _reset(model)


# ------------------------------------------------------------------------------------------------ 5. seeds
def test_seeded_sampling_is_reproducible_and_follows_the_manual_loop(model, dev):
    B, S0, new = 2, 30, 16
    ids, am = _left_padded((S0, S0), dev, seed=17)
    kw = dict(top_k=50, top_p=0.9, temperature=0.7)
    gen = lambda seed: model.generate(input_ids=ids, attention_mask=am, max_new_tokens=new, do_sample=True, seed=seed, eos_token_id=-1, decode_graph=False,
                                      repetition_penalty=1.05, **kw)
    with torch.no_grad():
        a, b, c = gen(7), gen(7), gen(8)
    assert torch.equal(a, b) and not torch.equal(a, c)
    lg = _step_logits(model, dev, a, S0, am).float().cpu()
    rng = torch.Generator(device=dev).manual_seed(7)
    close = 0
    for t in range(new):
        u = torch.rand(B, device=dev, generator=rng).cpu()
        seen = _seen_before(a, S0 + t, lg.shape[-1])
        for i, r in enumerate(R.select(lg[t], seen, 1.05, u=u, dtype=torch.float64, **kw)):
            if min(r["margin_u"], r["margin_p"]) < 1e-5:
                close += 1
            else:
                assert int(a[i, S0 + t]) == r["token"], (t, i)
    print(f"seeded sampling: {close} of {B * new} draws within 1e-5 of a decision of the float64 reference")
    assert close <= 2
    assert len({int(v) for v in a[:, S0:].reshape(-1)}) > 4          # not a greedy run in disguise


# ------------------------------------------------------------------------------------------------ 6. generation config
def test_generation_config_is_used_and_arguments_override_it(model, dev):
    from rga3.model.qwen2_5_vl import GenerationConfig

    ids, am = _left_padded((37,), dev, seed=3)      # the prompt of the manual-loop test: its greedy run repeats itself
    gen = lambda **k: model.generate(input_ids=ids, attention_mask=am, eos_token_id=-1, decode_graph=False, **k)
    try:
        with torch.no_grad():
            plain, pen = gen(max_new_tokens=10), gen(max_new_tokens=10, repetition_penalty=1.3)
            assert not torch.equal(plain, pen)
            gc = GenerationConfig(do_sample=True, temperature=0.1, top_k=1, top_p=0.001, repetition_penalty=1.3, eos_token_id=[318, 319], pad_token_id=0, max_new_tokens=10)
            assert torch.equal(gen(generation_config=gc, do_sample=False, temperature=None, top_p=None, top_k=None), pen)     # the reference's evaluation call
            assert torch.equal(gen(generation_config=gc, seed=1), pen)                # top_k 1: the draw has one candidate
            model.generation_config = gc
            assert torch.equal(gen(do_sample=False, temperature=None, top_p=None, top_k=None), pen)
            assert torch.equal(gen(), pen)
            assert torch.equal(gen(repetition_penalty=None, do_sample=False), plain) and torch.equal(gen(repetition_penalty=1.0, do_sample=False), plain)
            assert gen(max_new_tokens=3).shape[1] == 37 + 3
            stop = int(pen[0, 37 + 4])
            model.generation_config = GenerationConfig(repetition_penalty=1.3, eos_token_id=[stop, 400])
            cut = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=10, decode_graph=False)           # eos from the generation config
            first = int((pen[0, 37:] == stop).nonzero()[0])
            assert torch.equal(cut[0], pen[0, :37 + first + 1])
    finally:
        model.generation_config = None


# ------------------------------------------------------------------------------------------------ 7. the default route
def test_default_route_never_calls_the_selector_and_is_argmax(model, dev):
    ids, am = _left_padded((21, 33), dev, seed=29)
    with torch.no_grad():
        with _count_select() as c:
            out = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=10, eos_token_id=-1, decode_graph=False)
            same = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=10, eos_token_id=-1, decode_graph=False, do_sample=False, temperature=1.0,
                                  top_p=1.0, top_k=None, repetition_penalty=1.0)
            torch.manual_seed(3)
            smp = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=10, eos_token_id=-1, decode_graph=False, do_sample=True, temperature=0.8)
        assert c.n == {"select_token": 0, "mark_tokens_": 0, "penalize_logits": 0}
    assert torch.equal(out, same)
    lg = _step_logits(model, dev, out, 33, am)
    assert torch.equal(lg.float().argmax(-1).T, out[:, 33:])                         # the parent's choice: argmax of the f32 logits
    lg = _step_logits(model, dev, smp, 33, am)
    torch.manual_seed(3)
    for t in range(10):                                                              # ... and softmax + multinomial from the process-wide generator
        assert torch.equal(torch.multinomial(torch.softmax(lg[t].float() / 0.8, -1), 1)[:, 0], smp[:, 33 + t]), t
    with torch.no_grad(), _count_select() as c:
        model.generate(input_ids=ids, attention_mask=am, max_new_tokens=4, eos_token_id=-1, decode_graph=False, do_sample=True, repetition_penalty=1.2)
    assert c.n == {"select_token": 0, "mark_tokens_": 1 + 4, "penalize_logits": 4}    # plain sampling with a penalty: the full-vocabulary route


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_what_the_selector_cannot_do_is_refused(model, dev):
    ids, am = _left_padded((21,), dev, seed=31)
    with pytest.raises(NotImplementedError, match="top_p"):
        model.generate(input_ids=ids, attention_mask=am, max_new_tokens=4, do_sample=True, top_p=0.9)
    with pytest.raises(NotImplementedError, match="top_k"):
        model.generate(input_ids=ids, attention_mask=am, max_new_tokens=4, do_sample=True, top_k=65, top_p=0.9)
