"""GPU: the next-token selector (csrc/select.hip: ops.mark_tokens_, ops.penalize_logits, ops.select_token) against tests/select_ref.py.

Greedy choices and candidate sets are exact against the float32 reference; draws are compared with the float64 reference outside its decision margins.  Every
operand is a view inside a poisoned allocation (tests/guard_bands.py): logits rows are padded with NaN, everything outside the outputs must keep its bits."""
import numpy as np
import pytest
import torch

from tests import select_ref as R
from tests.guard_bands import assert_outside_unchanged, banded, banded_flat, snapshot

pytestmark = pytest.mark.gpu

SLICE = 4096                       # logits per block of the first launch (csrc/select.hip kSlice); test_slice_width_is_what_the_shapes_assume pins it
U_MAX = float(np.nextafter(np.float32(1), np.float32(0)))
QWEN_V = 152064                    # Qwen2.5-VL's vocabulary; 151666 = the tokenizer's 151665 entries + [SEG]
SHAPES = [1, 63, 64, 65, 320, SLICE - 1, SLICE, SLICE + 1, 151666, QWEN_V]


def logits_like_a_decoder(B, V, seed, std=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * std).to(torch.bfloat16).float()


def seen_table(B, V, seed, frac=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, V, generator=g) < frac).to(torch.uint8)


def view2d(shape, ld, dtype, dev, kind, data=None, seed=0):
    """guard_bands.banded for the small shapes; a vocabulary-wide row gets one guard ROW of ``ld`` elements before and after the view (wider than any block's reach)
    and the same pad columns, filled on the device: 520 guard rows of 152 064 elements would cost seconds of host time per call."""
    if shape[1] < 100000:
        return banded(shape, ld, dtype, dev, kind, data=data, seed=seed)
    backing = torch.empty((shape[0] + 2) * ld, dtype=dtype, device=dev)
    if kind == "in":
        backing.fill_(float("nan")) if dtype.is_floating_point else backing.zero_()
    else:
        g = torch.Generator(device=dev).manual_seed(seed)
        backing.view(torch.uint8).copy_(torch.randint(0, 256, (backing.numel() * backing.element_size(),), dtype=torch.uint8, device=dev, generator=g))
    view = backing.as_strided(tuple(shape), (ld, 1), ld)
    if data is not None:
        view.copy_(data.to(device=dev, dtype=dtype))
    return view, backing


class Run:
    """One ops.select_token call on banded operands.  tokens: [B] on the CPU; seen_after: the table as the kernel left it."""

    def __init__(self, dev, logits, dtype=torch.bfloat16, seen=None, u=None, pad=5, **kw):
        from rga3.hip import ops

        B, V = logits.shape
        lg, _ = view2d((B, V), V + pad, dtype, dev, "in", data=logits)
        sv = sb = None
        if seen is not None:
            sv, sb = view2d((B, V), V + 2 * pad + 1, torch.uint8, dev, "out", data=seen, seed=1)
        uv = banded_flat(B, torch.float32, dev, "in", data=u)[0] if u is not None else None
        out, ob = banded_flat(B, torch.int64, dev, "out", seed=2)
        ws, wb = banded_flat(ops.select_ws_bytes(B, V), torch.uint8, dev, "out", seed=3)
        snaps = [snapshot(b) for b in (ob, wb)] + ([snapshot(sb)] if sb is not None else [])
        ops.select_token(lg, sv, u=uv, out=out, ws=ws, **kw)
        self.tokens = out.cpu()
        assert_outside_unchanged(ob, out, snaps[0], "tok_out")
        assert_outside_unchanged(wb, ws, snaps[1], "scratch")
        assert bool(((self.tokens >= 0) & (self.tokens < V)).all()), self.tokens
        if seen is not None:
            assert_outside_unchanged(sb, sv, snaps[2], "seen")
            want = seen.clone()
            want[torch.arange(B), self.tokens] = 1        # exactly the chosen entries are newly set
            assert torch.equal(sv.cpu(), want)


def test_slice_width_is_what_the_shapes_assume(dev):
    from rga3.hip import ops

    one = ops.select_ws_bytes(1, 1)
    assert ops.select_ws_bytes(1, SLICE) == one and ops.select_ws_bytes(1, SLICE + 1) == 2 * one and ops.select_ws_bytes(8, QWEN_V) == 8 * 38 * one


# ------------------------------------------------------------------------------------------------ 1. greedy with penalty: exact
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", SHAPES)
def test_greedy_with_penalty_is_exact(V, dtype, dev):
    B = {1: 8, 63: 3, 64: 1, 65: 8, 320: 3}.get(V, 1 if V in (SLICE, 151666) else (8 if V == QWEN_V else 3))
    logits, seen = logits_like_a_decoder(B, V, seed=V), seen_table(B, V, seed=V + 1, frac=0.5 if V < 100 else 0.1)
    for penalty in (1.05, 2.0):
        want = torch.tensor([r["token"] for r in R.select(logits, seen, penalty)])
        assert torch.equal(Run(dev, logits, dtype, seen, penalty=penalty).tokens, want), penalty
    want = torch.tensor([r["token"] for r in R.select(logits)])
    assert torch.equal(Run(dev, logits, dtype).tokens, want)                       # no table: no penalty
    assert torch.equal(Run(dev, logits, dtype, seen, penalty=1.0).tokens, want)


def test_needle_at_every_position_of_a_slice_and_at_every_edge(dev):
    """One row per needle position: all of slice 1, both sides of every slice edge, index 0 and V - 1 (V = 2 slices + 3: the last slice holds three tokens)."""
    V = 2 * SLICE + 3
    pos = torch.tensor(sorted(set(range(SLICE, 2 * SLICE)) | {0, 1, SLICE - 1, 2 * SLICE, 2 * SLICE + 1, V - 1}))
    logits = torch.full((len(pos), V), -5.0).scatter_(1, pos[:, None], 5.0)
    assert torch.equal(Run(dev, logits).tokens, pos)
    seen = torch.zeros(logits.shape, dtype=torch.uint8).scatter_(1, pos[:, None], 1)
    assert torch.equal(Run(dev, logits, torch.float32, seen, penalty=1.25).tokens, pos)        # 5 / 1.25 still wins; its entry was set already


def test_ties_zeros_infinities_and_penalty_flips(dev):
    V = 2 * SLICE + 3
    rows, seens, want = [], [], []

    def row(fill, entries, seen=(), answer=None):
        x = torch.full((V,), float(fill))
        for i, v in entries.items():
            x[i] = v
        rows.append(x)
        seens.append(torch.zeros(V, dtype=torch.uint8).index_fill_(0, torch.tensor(list(seen), dtype=torch.long), 1))
        want.append(answer)

    row(-3, {7: 2.5, SLICE + 4: 2.5, V - 1: 2.5}, answer=7)                        # equal maxima in three slices: the lowest index
    row(-3, {SLICE - 1: 2.5, SLICE: 2.5}, answer=SLICE - 1)                        # ... on both sides of a slice edge
    row(-3, {SLICE + 9: -0.0, SLICE + 3: 0.0}, answer=SLICE + 3)                   # -0.0 == +0.0
    row(-3, {3: -0.0, 9: 0.0}, answer=3)
    row(float("-inf"), {V - 1: -80.0}, answer=V - 1)                               # everything else suppressed
    row(float("-inf"), {SLICE: 0.5}, seen=(SLICE,), answer=SLICE)
    row(-50, {5: 2.0, 6: 1.9}, seen=(5,), answer=6)                                # 2.0 / 1.3 < 1.9
    row(-50, {5: -1.0, 6: -1.2}, seen=(5,), answer=6)                              # -1.0 * 1.3 < -1.2
    row(-50, {5: 2.0, 6: 1.9}, seen=(), answer=5)                                  # ... and without the mark nothing flips
    logits, seen = torch.stack(rows), torch.stack(seens)
    ref = [r["token"] for r in R.select(logits, seen, 1.3)]
    assert ref == want
    for dtype in (torch.bfloat16, torch.float32):
        assert Run(dev, logits, dtype, seen, penalty=1.3).tokens.tolist() == want


def test_nan_logits_give_a_token_in_range(dev):
    logits = logits_like_a_decoder(4, SLICE + 77, seed=2)
    logits[0, ::3] = float("nan")
    logits[1] = float("nan")
    logits[2, 5] = float("nan")
    logits[3] = float("-inf")
    u = torch.tensor([0.3, 0.9, 0.0, U_MAX])
    Run(dev, logits, torch.float32, seen_table(4, SLICE + 77, 3), u=u, penalty=1.1, temperature=0.7, top_k=50, top_p=0.9)     # Run asserts 0 <= tok < V
    Run(dev, logits, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ 2. candidate set: exact
def _planted(V, where, seed):
    x = logits_like_a_decoder(1, V, seed)[0]
    g = torch.Generator().manual_seed(seed + 1)
    x[where] = (20 + torch.randn(len(where), generator=g)).to(torch.bfloat16).float()
    return x


@pytest.mark.parametrize("name,V,top_k,top_p", [("small", 320, 50, 0.9), ("k-above-V", 63, 64, 0.95), ("two", 65, 2, 1.0), ("spread", QWEN_V, 64, 0.9),
                                                ("one-slice", QWEN_V, 64, 0.9), ("edge", SLICE + 1, 50, 0.9), ("all-kept", 151666, 50, 1.0)])
def test_every_kept_candidate_is_drawn_in_turn(name, V, top_k, top_p, dev):
    """One row, repeated once per candidate place j, with u in the middle of candidate j's share (places past the kept prefix get the largest u): the tokens
    that come back are the reference's kept candidates in order, then its last kept one."""
    if name == "spread":
        x = _planted(V, torch.arange(64) * 2371 + 17, seed=5)                     # the 64 best tokens lie in 37 different slices
    elif name == "one-slice":
        x = _planted(V, 3 * SLICE + torch.arange(64) * 61 + 2, seed=6)            # ... all inside slice 3
    else:
        x = logits_like_a_decoder(1, V, seed=V + top_k)[0]
    seen = seen_table(1, V, seed=V)[0]
    kw = dict(penalty=1.05, temperature=0.7, top_k=top_k, top_p=top_p)
    r = R.select_row(x, seen, **kw)
    K, n = len(r["order"]), len(r["kept"])
    assert K == min(top_k, V) and r["margin_p"] > 1e-5, "the input must not sit on the top-p threshold"
    w = torch.exp(r["scores"][r["order"]][:n].double() - r["scores"][r["order"][0]].double())
    c = torch.cat([torch.zeros(1, dtype=torch.float64), w.cumsum(0)])
    u = torch.full((K,), U_MAX)
    u[:n] = ((c[:-1] + c[1:]) / 2 / c[-1]).float()
    want = torch.cat([r["kept"], r["kept"][-1:].expand(K - n)])
    got = Run(dev, x[None].expand(K, V), torch.bfloat16, seen[None].expand(K, V).clone(), u=u, **kw).tokens
    assert torch.equal(got, want), (n, K)
    assert set(got.tolist()) == set(r["kept"].tolist())
    if name in ("spread", "one-slice"):
        assert n > 8 and {int(t) // SLICE for t in r["order"]} == ({3} if name == "one-slice" else {int(i) // SLICE for i in torch.arange(64) * 2371 + 17})


# ------------------------------------------------------------------------------------------------ 3. draws
@pytest.mark.parametrize("V,dtype", [(320, torch.float32), (QWEN_V, torch.bfloat16)], ids=["320-f32", "152064-bf16"])
def test_4096_draws_against_the_float64_reference(V, dtype, dev):
    """N(0, 3^2) bf16 logits, 10 % of the tokens seen, penalty 1.05, T = 0.7, k = 50, p = 0.9: 8 rows x 512 values of u (0 and the largest float32 below 1 among
    them).  The token is the float64 reference's wherever neither of its margins is under 1e-5; at most 2 % of the draws may be that close."""
    from rga3.hip import ops

    B, N = 8, 512
    kw = dict(penalty=1.05, temperature=0.7, top_k=50, top_p=0.9)
    logits, seen = logits_like_a_decoder(B, V, seed=V + 7), seen_table(B, V, seed=V + 8)
    g = torch.Generator().manual_seed(V)
    u = torch.rand(N, B, generator=g)
    u[0], u[1] = 0.0, U_MAX
    lg = view2d((B, V), V + 3, dtype, dev, "in", data=logits)[0]
    ud, ws = u.to(dev), torch.empty(ops.select_ws_bytes(B, V), dtype=torch.uint8, device=dev)
    got = torch.empty((N, B), dtype=torch.int64, device=dev)
    sd = seen.to(dev)
    for i in range(N):
        ops.select_token(lg, sd.clone(), u=ud[i], out=got[i], ws=ws, **kw)
    got = got.cpu()
    close = wrong = 0
    for b in range(B):
        t64, mu, mp = R.draws(logits[b], u[:, b], seen[b], dtype=torch.float64, **kw)
        t32 = R.draws(logits[b], u[:, b], seen[b], dtype=torch.float32, **kw)[0]
        ok = (mu >= 1e-5) & (mp >= 1e-5)
        close += int((~ok).sum())
        wrong += int((got[:, b] != t64)[ok].sum())
        assert torch.equal(t32[ok], t64[ok])               # the two references agree there: the comparison is well posed
    print(f"V = {V}: {close} of {N * B} draws within 1e-5 of a decision of the float64 reference; {wrong} of the others differ")
    assert close <= 0.02 * N * B, close
    assert wrong == 0, wrong


# ------------------------------------------------------------------------------------------------ 4. seen: mark_tokens_ and penalize_logits
@pytest.mark.parametrize("B,S,V", [(1, 1, 1), (3, 77, 320), (8, 2112, QWEN_V)])
def test_mark_tokens_equals_a_scatter(B, S, V, dev):
    from rga3.hip import ops

    g = torch.Generator().manual_seed(B + S)
    ids = torch.randint(0, V, (B, S), generator=g)
    ids[:, S // 2:] = ids[:, :S - S // 2]                                          # duplicates
    if S > 8:
        ids[0, 1], ids[B - 1, 2], ids[0, 3], ids[B - 1, 4] = -1, V, 1 << 40, -(1 << 40)      # ... and ids outside [0, V): skipped
    before = seen_table(B, V, seed=V + 3, frac=0.01)
    iv = view2d((B, S), S + 3, torch.int64, dev, "in", data=ids)[0]
    sv, sb = view2d((B, V), V + 7, torch.uint8, dev, "out", data=before, seed=4)
    snap = snapshot(sb)
    assert ops.mark_tokens_(sv, iv) is sv
    assert_outside_unchanged(sb, sv, snap, "seen")
    want = before.clone()
    for b in range(B):
        row = ids[b][(ids[b] >= 0) & (ids[b] < V)]
        want[b, row] = 1
    assert torch.equal(sv.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,V", [(1, 1), (3, 65), (8, 151666)])
def test_penalize_logits_is_bit_equal_to_the_torch_expression(B, V, dtype, dev):
    from rga3.hip import ops

    x, seen = logits_like_a_decoder(B, V, seed=V + 11), seen_table(B, V, seed=V + 12, frac=0.3)
    x[0, 0] = float("-inf")
    if V > 4:
        x[0, 1:5] = torch.tensor([0.0, -0.0, float("inf"), 1e-38])
        seen[0, :5] = 1
    lg = view2d((B, V), V + 5, dtype, dev, "in", data=x)[0]
    sv = view2d((B, V), V + 2, torch.uint8, dev, "in", data=seen)[0]
    out, ob = view2d((B, V), V + 9, torch.float32, dev, "out", seed=6)
    snap = snapshot(ob)
    for p in (1.05, 0.8):
        assert ops.penalize_logits(lg, sv, p, out=out) is out
        assert_outside_unchanged(ob, out, snap, "out")
        xf = lg.float().cpu()
        pt = torch.tensor(p, dtype=torch.float32)
        want = torch.where(seen.bool(), torch.where(xf < 0, xf * pt, xf / pt), xf)
        assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)), p
    assert torch.equal(ops.penalize_logits(lg, sv, 1.05).cpu(), R.scores(lg.float().cpu(), seen, 1.05))


# ------------------------------------------------------------------------------------------------ 5. robustness
def test_same_call_same_answer_and_a_batch_equals_its_rows(dev):
    V, B = QWEN_V, 3
    logits, seen = logits_like_a_decoder(B, V, seed=21), seen_table(B, V, seed=22)
    u = torch.tensor([0.11, 0.57, 0.93])
    for kw in (dict(penalty=1.05, temperature=0.7, top_k=50, top_p=0.9, u=u), dict(penalty=1.3)):
        a, b = Run(dev, logits, seen=seen, **kw).tokens, Run(dev, logits, seen=seen, pad=64, **kw).tokens
        assert torch.equal(a, b)
        for i in range(B):
            one = dict(kw, u=u[i:i + 1]) if "u" in kw else kw
            assert torch.equal(Run(dev, logits[i:i + 1], seen=seen[i:i + 1], **one).tokens, a[i:i + 1]), i


def test_the_three_ops_do_not_sync(dev):
    from rga3.hip import ops

    B, V = 3, SLICE + 5
    lg, seen = logits_like_a_decoder(B, V, 1).to(torch.bfloat16).to(dev), torch.zeros((B, V), dtype=torch.uint8, device=dev)
    ids, u = torch.randint(0, V, (B, 9)).to(dev), torch.rand(B).to(dev)
    ws, out = torch.empty(ops.select_ws_bytes(B, V), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.mark_tokens_(seen, ids)
        ops.penalize_logits(lg, seen, 1.05)
        ops.select_token(lg, seen, 1.05, 0.7, 50, 0.9, u, out=out, ws=ws)
        ops.select_token(lg, seen, 1.05)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(seen.sum()) >= 2


def test_refusals(dev):
    from rga3.hip import lib, ops

    B, V = 2, 70
    lg = torch.zeros((B, V), dtype=torch.bfloat16, device=dev)
    seen = torch.zeros((B, V), dtype=torch.uint8, device=dev)
    ids = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    u = torch.zeros(B, device=dev)
    bad = [lambda: ops.select_token(lg.cpu()), lambda: ops.select_token(lg, seen.cpu()), lambda: ops.select_token(lg, u=u.cpu(), top_k=2),
           lambda: ops.mark_tokens_(seen.cpu(), ids), lambda: ops.mark_tokens_(seen, ids.cpu()), lambda: ops.penalize_logits(lg.cpu(), seen, 1.1),
           lambda: ops.penalize_logits(lg, seen.cpu(), 1.1),                                                                  # CPU tensors
           lambda: ops.select_token(lg.half()), lambda: ops.select_token(lg, seen.bool()), lambda: ops.select_token(lg, u=u.double()),
           lambda: ops.select_token(lg, out=torch.zeros(B, dtype=torch.int32, device=dev)), lambda: ops.mark_tokens_(seen, ids.int()),
           lambda: ops.mark_tokens_(seen.int(), ids), lambda: ops.penalize_logits(lg.half(), seen, 1.1), lambda: ops.penalize_logits(lg, seen.int(), 1.1),
           lambda: ops.penalize_logits(lg, seen, 1.1, out=torch.zeros((B, V), dtype=torch.bfloat16, device=dev)),             # dtypes
           lambda: ops.select_token(lg, top_k=0), lambda: ops.select_token(lg, top_k=65), lambda: ops.select_token(lg, top_k=2.0),
           lambda: ops.select_token(lg, top_p=0.0), lambda: ops.select_token(lg, top_p=1.01), lambda: ops.select_token(lg, top_p=-0.5),
           lambda: ops.select_token(lg, temperature=0.0), lambda: ops.select_token(lg, temperature=-1.0),
           lambda: ops.select_token(lg, seen, penalty=0.0), lambda: ops.select_token(lg, seen, penalty=-2.0), lambda: ops.penalize_logits(lg, seen, 0.0),
           lambda: ops.select_token(lg.as_strided((B, V), (V - 1, 1))), lambda: ops.select_token(lg, seen.as_strided((B, V), (V - 1, 1))),
           lambda: ops.select_token(lg[:, ::2]), lambda: ops.penalize_logits(lg.as_strided((B, V), (V - 1, 1)), seen, 1.1),
           lambda: ops.penalize_logits(lg, seen, 1.1, out=torch.zeros(B * V, device=dev).as_strided((B, V), (V - 1, 1))),
           lambda: ops.mark_tokens_(seen.as_strided((B, V), (V - 1, 1)), ids), lambda: ops.mark_tokens_(seen, ids.as_strided((B, 4), (3, 1))),
           lambda: ops.mark_tokens_(seen[:1], ids), lambda: ops.select_token(lg, seen[:, :V - 1]),                            # short strides, shapes
           lambda: ops.select_token(lg, ws=torch.empty(ops.select_ws_bytes(B, V) - 1, dtype=torch.uint8, device=dev)),
           lambda: ops.select_token(lg, ws=torch.empty(ops.select_ws_bytes(B, V), dtype=torch.float32, device=dev)),          # scratch
           lambda: ops.select_ws_bytes(0, V), lambda: ops.select_ws_bytes(B, 0)]
    for i, f in enumerate(bad):
        with pytest.raises(lib.Rga3Error):
            f()
            pytest.fail(f"call {i} was accepted")
    L = lib.load()       # ... and the library refuses the same on its own (the wrappers above never let these through)
    ws = torch.empty(ops.select_ws_bytes(B, V), dtype=torch.uint8, device=dev)
    out = torch.empty(B, dtype=torch.int64, device=dev)
    call = lambda **k: L.rga3_select_token(lg.data_ptr(), 0, seen.data_ptr(), k.get("penalty", 1.0), k.get("temperature", 1.0), k.get("top_k", 1), k.get("top_p", 1.0), 0,
                                           out.data_ptr(), ws.data_ptr(), k.get("ws_bytes", ws.numel()), B, V, k.get("ld", V), V, 0)
    for k in (dict(top_k=0), dict(top_k=65), dict(top_p=0.0), dict(top_p=1.5), dict(temperature=0.0), dict(penalty=0.0), dict(ld=V - 1), dict(ws_bytes=ws.numel() - 8)):
        assert call(**k) == -22, k
    assert L.rga3_penalize_logits(lg.data_ptr(), 0, seen.data_ptr(), ws.data_ptr(), B, V, V, V - 1, V, 1.1, 0) == -22
    assert L.rga3_mark_tokens(ids.data_ptr(), seen.data_ptr(), B, 4, V, 3, V, 0) == -22
    torch.cuda.synchronize()
    assert int(seen.sum()) == 0
