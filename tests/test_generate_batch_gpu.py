"""GPU: generate() with set_decode_attention("cache") (ops.decode_attn on the KV cache where it lies, captured steps for 1 <= B <= 8 sequences) on the tiny model of
tests/qwen_tiny.py: teacher-forced decode against the oracle in both weight modes, which calls take the new route, graph replay against the eager loop for
B = 1 .. 4, a left-padded batch of three against its single runs, reuse of captured graphs, and an eager decode loop without host <-> device syncs."""
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
    """The snapped model (prefill on bf16 kernels and e4m3 decode evaluate the same function); every test leaves it at ("bf16", "varlen")."""
    return fresh_model(dev, snap=True)


@pytest.fixture(scope="module")
def snapped_params():
    sd = det_params(gold())
    return {k: (snap_ref(v.to(torch.bfloat16)).float() if PROJ.match(k) else v) for k, v in sd.items()}


def _reset(m):
    m.set_decode_weights("bf16")
    m.set_decode_attention("varlen")


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


class _count_ops:
    """Counts the calls the model file makes to the named rga3.hip.ops functions while active: .n[name]."""

    NAMES = ("decode_attn", "rope_", "attn_varlen", "attn_varlen_rope")

    def __enter__(self):
        import rga3.model.qwen2_5_vl as QM

        self.QM, self.real, self.n = QM, {k: getattr(QM.ops, k) for k in self.NAMES}, {k: 0 for k in self.NAMES}
        for k in self.NAMES:
            setattr(QM.ops, k, self._counted(k))
        return self

    def _counted(self, k):
        def f(*a, **kw):
            self.n[k] += 1
            return self.real[k](*a, **kw)
        return f

    def __exit__(self, *exc):
        for k in self.NAMES:
            setattr(self.QM.ops, k, self.real[k])


def _left_padded(lens, dev, seed):
    torch.manual_seed(seed)
    S = max(lens)
    ids = torch.zeros((len(lens), S), dtype=torch.long, device=dev)
    am = torch.zeros((len(lens), S), dtype=torch.long, device=dev)
    for i, n in enumerate(lens):
        ids[i, S - n:] = torch.randint(10, 300, (n,), device=dev)
        am[i, S - n:] = 1
    return ids, am


# ------------------------------------------------------------------------------------------------ 1. teacher-forced decode against the oracle
@pytest.mark.parametrize("kind", ["bf16", "e4m3"])
def test_teacher_forced_decode_on_the_cache_route(kind, model, dev, snapped_params):
    """set_decode_attention("cache") against oracle.qwen25vl.forward: logits rel-L2 < 2e-2 and the greedy token wherever the oracle's top-1 / top-2 margin exceeds
    0.05 max|logit| (the rules of test_kv_cache_decode_parity and test_teacher_forced_decode_on_snapped_weights).  bf16: the plain model against the oracle on its
    parameters; e4m3: the snapped model against the oracle on the snapped parameters.  The figures are printed beside the default
    route's; measured on MI355X: bf16 1.23e-2 (varlen 1.31e-2), e4m3 1.20e-2 (varlen 1.37e-2)."""
    g = gold()
    full = torch.from_numpy(g["gen_output_ids"])
    S0 = g["gen_input_ids"].shape[1]
    px = det_tensor("pixel_values_full0", (192, 1176), 1.0, seed=5).to(torch.bfloat16)
    m = model if kind == "e4m3" else fresh_model(dev, snap=False)
    params = snapped_params if kind == "e4m3" else det_params(g)
    ref = Q.forward(params, oracle_cfg(), full, torch.ones_like(full), pixel_values_videos=px.float(), video_grid_thw=np.array([[2, 8, 12]]),
                    second_per_grid_ts=np.array([1.0]))["logits"][0]
    want = ref[S0 - 1: full.shape[1] - 1]
    top2 = want.topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 0.05 * want.abs().max()
    try:
        m.set_decode_weights(kind)
        errs = {}
        for route in ("varlen", "cache"):
            m.set_decode_attention(route)
            assert m.decode_attention == route
            got = _teacher_forced(m, dev)[0]
            errs[route] = rel_l2(got, want)
            print(f"teacher-forced decode, {kind} weights, decode attention {route}: logits rel-L2 vs oracle {errs[route]:.3e}")
            if route == "cache":
                assert errs[route] < 2e-2, errs
                assert torch.equal(got.argmax(-1)[decided], want.argmax(-1)[decided])
    finally:
        _reset(m)


# ------------------------------------------------------------------------------------------------ 2. the route ran, and only where asked
def test_route_runs_only_where_asked(model, dev):
    nl = model.config.num_hidden_layers
    try:
        with _count_ops() as c:
            off = _teacher_forced(model, dev)[0]
        assert c.n["decode_attn"] == 0 and c.n["rope_"] > 0 and c.n["attn_varlen"] > 0
        model.set_decode_attention("cache")
        steps = []

        def wrap(step):
            with _count_ops() as c:
                out = step()
            steps.append(dict(c.n))
            return out

        with _count_ops() as total:
            _teacher_forced(model, dev, wrap)
        assert steps and all(s == {"decode_attn": nl, "rope_": 0, "attn_varlen": 0, "attn_varlen_rope": 0} for s in steps), steps
        assert total.n["decode_attn"] == nl * len(steps)                 # none during prefill
        assert total.n["rope_"] > 0                                      # (the prefill still rotates in place)
        with _count_ops() as c:
            _teacher_forced(model, dev, lambda step: torch.enable_grad()(step)())
        assert c.n["decode_attn"] == 0                                   # none under autograd
        model.set_decode_attention("varlen")
        with _count_ops() as c:
            back = _teacher_forced(model, dev)[0]
        assert c.n["decode_attn"] == 0 and torch.equal(off, back)
    finally:
        _reset(model)


def test_switch_refuses_what_the_kernel_does_not_take(dev):
    from rga3.model.qwen2_5_vl import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    kw = dict(product_cfg_kwargs(), num_hidden_layers=1)
    wide = Qwen2_5_VLForConditionalGeneration(Qwen2_5_VLConfig(**dict(kw, hidden_size=288, num_attention_heads=18, num_key_value_heads=2)))   # G = 9
    with pytest.raises(ValueError, match="set_decode_attention"):
        wide.set_decode_attention("cache")
    odd = Qwen2_5_VLForConditionalGeneration(Qwen2_5_VLConfig(**dict(kw, hidden_size=144, num_attention_heads=6, num_key_value_heads=2)))      # D = 24
    with pytest.raises(ValueError, match="set_decode_attention"):
        odd.set_decode_attention("cache")
    with pytest.raises(ValueError, match="set_decode_attention"):
        odd.set_decode_attention("paged")
    assert odd.decode_attention == "varlen"


# ------------------------------------------------------------------------------------------------ 3. graph equals eager
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_graph_equals_eager(B, model, dev):
    lens = (21, 33, 27, 30)[:B]
    ids, am = _left_padded(lens, dev, seed=11 + B)
    S, new = max(lens), 40
    gen = lambda **k: model.generate(input_ids=ids, attention_mask=am, max_new_tokens=new, do_sample=False, **k)
    try:
        with torch.no_grad():
            model.set_decode_attention("cache")
            for kind in ("bf16", "e4m3"):
                model.set_decode_weights(kind)
                with _count_ops() as c:
                    eager = gen(eos_token_id=-1, decode_graph=False)
                assert c.n["decode_attn"] == model.config.num_hidden_layers * (new - 1)
                graph = gen(eos_token_id=-1)
                assert eager.shape == (B, S + new) and torch.equal(eager, graph), kind
                states = model.__dict__["_decode_states"]
                assert any("graph" in st for key, st in states.items() if key[-3:] == (B, "cache", kind)), list(states)
                if B in (1, 3):
                    eos = int(eager[0, S + 11])             # an early new token of sequence 0 as EOS: it arrives between two host checks
                    e2 = gen(eos_token_id=eos, decode_graph=False)
                    g2 = gen(eos_token_id=eos)
                    assert torch.equal(e2, g2), kind
                    first = int((eager[0, S:] == eos).nonzero()[0])
                    assert torch.equal(e2[0, :S + first + 1], eager[0, :S + first + 1])
                    if B == 1:
                        assert e2.shape[1] == S + first + 1
    finally:
        _reset(model)


def test_modes_do_not_mix(model, dev):
    """varlen -> cache -> varlen on one model, graph replay each time: the third result is the first, and each mode keeps a captured step of its own."""
    ids, am = _left_padded((37,), dev, seed=3)
    gen = lambda: model.generate(input_ids=ids, attention_mask=am, max_new_tokens=40, do_sample=False, eos_token_id=-1)
    try:
        with torch.no_grad():
            outs = []
            for route in ("varlen", "cache", "varlen"):
                model.set_decode_attention(route)
                with _count_ops() as c:
                    model.generate(input_ids=ids, attention_mask=am, max_new_tokens=40, do_sample=False, eos_token_id=-1, decode_graph=False)
                assert (c.n["decode_attn"] > 0) == (route == "cache")
                outs.append(gen())
            assert torch.equal(outs[0], outs[2])
            keys = [key for key, st in model.__dict__["_decode_states"].items() if "graph" in st and key[-1] == "bf16" and key[-3] == 1]
            assert {key[-2] for key in keys} == {"varlen", "cache"}, keys
    finally:
        _reset(model)


# ------------------------------------------------------------------------------------------------ 4. batch of three
def test_left_padded_batch_of_three_equals_single_sequences(model, dev):
    lens, new = (21, 33, 27), 12
    ids, am = _left_padded(lens, dev, seed=5)
    S = max(lens)
    try:
        model.set_decode_attention("cache")
        with torch.no_grad():
            model.set_decode_weights("e4m3")
            with _count_ops() as c:
                batch = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=new, do_sample=False, eos_token_id=-1)
            assert c.n["decode_attn"] == model.config.num_hidden_layers * (new - 1)
            for i, n in enumerate(lens):
                one = model.generate(input_ids=ids[i:i + 1, S - n:], max_new_tokens=new, do_sample=False, eos_token_id=-1, decode_graph=False)
                assert torch.equal(batch[i, S:], one[0, n:]), i
            model.set_decode_weights("bf16")
            eager = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=24, do_sample=False, eos_token_id=-1, decode_graph=False)
            graph = model.generate(input_ids=ids, attention_mask=am, max_new_tokens=24, do_sample=False, eos_token_id=-1)
            assert torch.equal(eager, graph)
    finally:
        _reset(model)


# ------------------------------------------------------------------------------------------------ 5. captured graphs are kept
def test_captured_step_is_reused_and_follows_the_weights(dev):
    import gc

    from rga3.hip import ops, scratch

    m = fresh_model(dev, snap=True).set_decode_attention("cache")
    ids, am = _left_padded((21, 33), dev, seed=9)
    gen = lambda: m.generate(input_ids=ids, attention_mask=am, max_new_tokens=20, do_sample=False, eos_token_id=-1)
    with torch.no_grad():
        a = gen()
        (key, st), = [(k, s) for k, s in m.__dict__["_decode_states"].items() if "graph" in s]
        assert key[-3:-1] == (2, "cache")
        graph, kv = st["graph"], st["kv"]
        b = gen()
        st2 = m.__dict__["_decode_states"][key]
        assert st2 is st and st2["graph"] is graph and st2["kv"] is kv and torch.equal(a, b)
        m.model.layers[0].self_attn.o_proj.weight.mul_(1.0)          # an in-place update (same values): the captured step is dropped and captured again
        c = gen()
        assert m.__dict__["_decode_states"][key]["graph"] is not graph and torch.equal(a, c)
        # every further re-capture drops the scratch of the graph it replaces: no Scratch and no GEMM workspace is left behind (one workspace is what a leak costs)
        one_workspace = ops.gemm_workspace(dev).numel()              # (bytes: a uint8 tensor)
        gc.collect()
        owned, allocated = len(scratch._owned), torch.cuda.memory_allocated()
        for _ in range(3):
            m.model.layers[0].self_attn.o_proj.weight.mul_(1.0)
            c = gen()
            gc.collect()
            grown = torch.cuda.memory_allocated() - allocated
            print(f"re-capture: {len(scratch._owned)} owner-held Scratch (was {owned}), memory_allocated grew by {grown} bytes (one workspace: {one_workspace})")
            assert len(scratch._owned) == owned
            assert grown < one_workspace
            assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ 6. no sync
def test_eager_cache_route_decodes_without_syncs(model, dev):
    """The eager decode loop of generate() under set_decode_attention("cache") holds no host <-> device sync between two host checks: sync debug mode "error" is on from
    the first decode_attn call of the first decode step to the last one of the seventh (every kind of work of a step lies inside: token choice, positions and lengths
    going up, the layers, the LM head).  The first call outside the mode warms allocations and tuner picks up."""
    ids, am = _left_padded((21, 33, 27), dev, seed=13)
    nl = model.config.num_hidden_layers
    gen = lambda: model.generate(input_ids=ids, attention_mask=am, max_new_tokens=8, do_sample=False, eos_token_id=-1, decode_graph=False)
    import rga3.model.qwen2_5_vl as QM

    real, seen = QM.ops.decode_attn, [0]

    def watched(*a, **k):
        seen[0] += 1
        if seen[0] == 1:
            torch.cuda.set_sync_debug_mode("error")
        try:
            return real(*a, **k)
        finally:
            if seen[0] == nl * 7:
                torch.cuda.set_sync_debug_mode("default")

    try:
        model.set_decode_attention("cache")
        with torch.no_grad():
            want = gen()
            QM.ops.decode_attn = watched
            got = gen()
        assert seen[0] == nl * 7 and torch.equal(got, want)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        QM.ops.decode_attn = real
        _reset(model)
