"""GPU: generate() with e4m3 decoder weights (set_decode_weights("e4m3"), ops.gemv_w8) on the tiny model of tests/qwen_tiny.py: the in-place snap against the CPU
reference, teacher-forced decode against the oracle on the snapped parameters, which calls take the new route, graph replay against the eager loop in both
modes, packs that follow in-place weight updates, and a left-padded batch of three."""
import re

import numpy as np
import pytest
import torch

from oracle import qwen25vl as Q
from oracle.detweights import det_tensor
from tests.qwen_tiny import det_params, gold, oracle_cfg, product_cfg_kwargs, rel_l2
from tests.w8_ref import snap_ref

pytestmark = pytest.mark.gpu

PROJ = re.compile(r"model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")


def fresh_model(dev, snap):
    from rga3.model.qwen2_5_vl import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    m = Qwen2_5_VLForConditionalGeneration(Qwen2_5_VLConfig(**product_cfg_kwargs()))
    m.load_state_dict(det_params(gold(), bf16_round=False), strict=True)
    m = m.to(torch.bfloat16).to(dev).eval()
    return m.snap_decoder_weights_to_e4m3_() if snap else m


@pytest.fixture(scope="module")
def model(dev):
    return fresh_model(dev, snap=True)


@pytest.fixture(scope="module")
def snapped_params():
    """The oracle's parameters (bf16-rounded, as the product holds them) with snap_ref applied to the decoder projections."""
    sd = det_params(gold())
    return {k: (snap_ref(v.to(torch.bfloat16)).float() if PROJ.match(k) else v) for k, v in sd.items()}


def _teacher_forced(model, dev, wrap=None):
    """Prefill + teacher-forced single-token steps through the KV cache, as test_kv_cache_decode_parity: ([steps, vocab] logits, S0, the full ids).
    wrap(fn) runs each decode step (not the prefill)."""
    from rga3.model.qwen2_5_vl import KVCache

    g = gold()
    full = torch.from_numpy(g["gen_output_ids"])
    S0 = g["gen_input_ids"].shape[1]
    px = det_tensor("pixel_values_full0", (192, 1176), 1.0, seed=5).to(torch.bfloat16)
    c = model.config
    cache = KVCache(c.num_hidden_layers, 1, full.shape[1] + 1, c.num_key_value_heads, c.head_dim, dev, torch.bfloat16)
    with torch.no_grad():
        out = model(input_ids=full[:, :S0].to(dev), attention_mask=torch.ones(1, S0, dtype=torch.long, device=dev), past_key_values=cache,
                    pixel_values_videos=px.to(dev), video_grid_thw=torch.tensor([[2, 8, 12]]), second_per_grid_ts=torch.tensor([1.0]))
        rows = [out.logits[0, -1].float().cpu()]
        for t in range(S0, full.shape[1] - 1):
            am = torch.ones(1, t + 1, dtype=torch.long, device=dev)
            step = lambda: model(input_ids=full[:, t:t + 1].to(dev), attention_mask=am, past_key_values=cache)
            out = step() if wrap is None else wrap(step)
            rows.append(out.logits[0, -1].float().cpu())
    return torch.stack(rows), S0, full


class _count_w8:
    """Counts ops.gemv_w8 calls made by the model file while active."""

    def __enter__(self):
        import rga3.model.qwen2_5_vl as QM

        self.QM, self.real, self.n = QM, QM.ops.gemv_w8, 0

        def counted(*a, **k):
            self.n += 1
            return self.real(*a, **k)

        QM.ops.gemv_w8 = counted
        return self

    def __exit__(self, *exc):
        self.QM.ops.gemv_w8 = self.real


# ------------------------------------------------------------------------------------------------ 1. snap
def test_snap_equals_reference_and_is_idempotent(dev):
    from rga3.hip import ops

    m = fresh_model(dev, snap=False)
    names = [n for n, _ in m.named_parameters() if PROJ.match(n)]
    assert len(names) == 7 * m.config.num_hidden_layers
    before = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    m.snap_decoder_weights_to_e4m3_()
    after = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    for n in before:
        want = snap_ref(before[n]) if n in names else before[n]
        assert torch.equal(after[n].view(torch.int16), want.view(torch.int16)), n
    m.snap_decoder_weights_to_e4m3_()
    for n, p in m.named_parameters():
        assert torch.equal(p.detach().cpu().view(torch.int16), after[n].view(torch.int16)), n
    for n, p in m.named_parameters():
        if n in names:
            assert torch.equal(ops.dequant_e4m3_rows(*ops.quant_e4m3_rows_pow2(p.detach())).view(torch.int16), p.detach().view(torch.int16)), n


# ------------------------------------------------------------------------------------------------ 2. teacher-forced decode against the oracle
def test_teacher_forced_decode_on_snapped_weights(model, dev, snapped_params):
    """Both routes on the snapped model against oracle.qwen25vl.forward on the same snapped parameters: logits rel-L2 <= 2e-2 (the project's stated bound) and the
    greedy token wherever the oracle's top-1 / top-2 margin exceeds 0.05 max|logit| (test_kv_cache_decode_parity's rule).  The figures are printed."""
    g = gold()
    full = torch.from_numpy(g["gen_output_ids"])
    S0 = g["gen_input_ids"].shape[1]
    px = det_tensor("pixel_values_full0", (192, 1176), 1.0, seed=5).to(torch.bfloat16)
    ref = Q.forward(snapped_params, oracle_cfg(), full, torch.ones_like(full), pixel_values_videos=px.float(), video_grid_thw=np.array([[2, 8, 12]]),
                    second_per_grid_ts=np.array([1.0]))["logits"][0]
    want = ref[S0 - 1: full.shape[1] - 1]
    top2 = want.topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 0.05 * want.abs().max()
    errs = {}
    try:
        for kind in ("bf16", "e4m3"):
            model.set_decode_weights(kind)
            assert model.decode_weights == kind
            got = _teacher_forced(model, dev)[0]
            errs[kind] = rel_l2(got, want)
            print(f"teacher-forced decode on snapped weights, {kind}: logits rel-L2 vs oracle {errs[kind]:.3e}")
            # (if the bf16 route missed the bound on these weights the snapped input would be at fault, not the e4m3 route)
            assert errs[kind] < 2e-2, (kind, errs)
            assert torch.equal(got.argmax(-1)[decided], want.argmax(-1)[decided]), kind
    finally:
        model.set_decode_weights("bf16")


# ------------------------------------------------------------------------------------------------ 3. the route ran, and only where asked
def test_route_runs_only_where_asked(model, dev):
    nl = model.config.num_hidden_layers
    never = fresh_model(dev, snap=True)
    base = _teacher_forced(never, dev)[0]
    try:
        with _count_w8() as c:
            off = _teacher_forced(model, dev)[0]
        assert c.n == 0
        model.set_decode_weights("e4m3")
        steps = []

        def wrap(step):
            with _count_w8() as c:
                out = step()
            steps.append(c.n)
            return out

        with _count_w8() as total:
            _teacher_forced(model, dev, wrap)
        assert steps and all(n == 4 * nl for n in steps), steps
        assert total.n == sum(steps)                     # none during prefill
        with _count_w8() as c:
            _teacher_forced(model, dev, lambda step: torch.enable_grad()(step)())
        assert c.n == 0                                  # none under autograd
        model.set_decode_weights("bf16")
        with _count_w8() as c:
            back = _teacher_forced(model, dev)[0]
        assert c.n == 0
        assert torch.equal(off, base) and torch.equal(back, base)
    finally:
        model.set_decode_weights("bf16")


# ------------------------------------------------------------------------------------------------ 4. graph equals eager, and the modes do not mix
def test_graph_equals_eager_and_modes_do_not_mix(model, dev):
    torch.manual_seed(11)
    ids = torch.randint(10, 300, (1, 37), device=dev)
    gen = lambda **k: model.generate(input_ids=ids, max_new_tokens=40, do_sample=False, **k)
    try:
        with torch.no_grad():
            model.set_decode_weights("e4m3")
            with _count_w8() as c:
                a = gen(eos_token_id=-1, decode_graph=False)
            assert c.n == 4 * model.config.num_hidden_layers * 39
            b = gen(eos_token_id=-1)
            assert a.shape == (1, 77) and torch.equal(a, b)
            assert any("graph" in st for key, st in model.__dict__["_decode_states"].items() if key[-1] == "e4m3")       # the captured route ran
            eos = int(a[0, 37 + 11])                     # an early new token as EOS: it arrives between two host checks
            first = int((a[0, 37:] == eos).nonzero()[0])
            c_ = gen(eos_token_id=eos, decode_graph=False)
            d = gen(eos_token_id=eos)
            assert c_.shape[1] == 37 + first + 1 and torch.equal(c_, d) and torch.equal(c_, a[:, :c_.shape[1]])
            outs = []
            for kind in ("bf16", "e4m3", "bf16"):
                model.set_decode_weights(kind)
                eager = gen(eos_token_id=-1, decode_graph=False)
                graph = gen(eos_token_id=-1)
                assert torch.equal(eager, graph), kind
                outs.append(graph)
            assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], a)
    finally:
        model.set_decode_weights("bf16")


# ------------------------------------------------------------------------------------------------ 5. packs follow the weights
def test_packs_follow_in_place_weight_updates(dev):
    m = fresh_model(dev, snap=True).set_decode_weights("e4m3")
    first = _teacher_forced(m, dev)[0]                   # builds the e4m3 packs
    with torch.no_grad():
        m.model.layers[0].self_attn.o_proj.weight.copy_(m.model.layers[1].self_attn.o_proj.weight)
    got = _teacher_forced(m, dev)[0]
    twin = fresh_model(dev, snap=True)
    with torch.no_grad():
        twin.model.layers[0].self_attn.o_proj.weight.copy_(twin.model.layers[1].self_attn.o_proj.weight)
    want = _teacher_forced(twin.set_decode_weights("e4m3"), dev)[0]
    assert torch.equal(got, want) and not torch.equal(got, first)


# ------------------------------------------------------------------------------------------------ 6. batch of three
def test_left_padded_batch_of_three_equals_single_sequences(model, dev):
    torch.manual_seed(5)
    lens, S, new = (21, 33, 27), 33, 12
    ids = torch.zeros((3, S), dtype=torch.long, device=dev)
    am = torch.zeros((3, S), dtype=torch.long, device=dev)
    for i, n in enumerate(lens):
        ids[i, S - n:] = torch.randint(10, 300, (n,), device=dev)
        am[i, S - n:] = 1
    try:
        model.set_decode_weights("e4m3")
        with torch.no_grad():
            with _count_w8() as c:
                batch = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=new, do_sample=False, eos_token_id=-1)
            assert c.n == 4 * model.config.num_hidden_layers * (new - 1)
            for i, n in enumerate(lens):
                one = model.generate(input_ids=ids[i:i + 1, S - n:], max_new_tokens=new, do_sample=False, eos_token_id=-1, decode_graph=False)
                assert torch.equal(batch[i, S:], one[0, n:]), i
    finally:
        model.set_decode_weights("bf16")
