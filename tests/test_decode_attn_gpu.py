"""GPU: ops.decode_attn (csrc/decattn.hip) -- rotation, the two cache appends and attention over the cache where it lies, one call per decode step.

cap = 4 KS, visible key counts n = lens + 1 in {1, 2, KS - 1, KS, KS + 1, 2 KS, 2 KS + 1, 3 KS + 5} (KS = ops.decode_attn_slice_keys()): one key, the slice
boundaries from either side, several slices, a ragged tail.  The exact tests (one key, needle, uniform scores) use operands whose softmax weights are exactly 0 or 1 /
whose sums are small integers, so the expected output is known bit for bit."""
import functools

import pytest
import torch

from tests import decattn_ref as R
from tests.guard_bands import assert_finite_where, assert_outside_unchanged, banded, snapshot
from tests.qwen_tiny import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(7, 1, 128), (28, 4, 128), (16, 2, 128), (6, 2, 16), (8, 1, 64)]


def KS():
    from rga3.hip import ops

    return ops.decode_attn_slice_keys()


def counts():
    ks = KS()
    return [1, 2, ks - 1, ks, ks + 1, 2 * ks, 2 * ks + 1, 3 * ks + 5]


def bits(t):
    return t.contiguous().view(torch.int16)


def call(c, lens, Hq, Hkv, dev, scale=None, **kw):
    """ops.decode_attn on device copies of a case's operands -> (out, k_cache, v_cache, qkv) on the CPU."""
    from rga3.hip import ops

    d = {k: v.to(dev) for k, v in c.items()}
    ld = torch.tensor(list(lens), dtype=torch.int32, device=dev)
    D = c["qkv"].shape[2]
    out = ops.decode_attn(d["qkv"], d["cos"], d["sin"], d["k_cache"], d["v_cache"], ld, Hq, Hkv, D ** -0.5 if scale is None else scale, **kw)
    return out.cpu(), d["k_cache"].cpu(), d["v_cache"].cpu(), d["qkv"].cpu()


@functools.lru_cache(maxsize=None)
def ragged_case(Hq, Hkv, D):
    """One sequence per visible key count, random operands, with its float64 reference (computed once per shape, shared, never modified)."""
    ns = counts()
    c = R.random_case(len(ns), Hq, Hkv, D, 4 * KS(), seed=Hq * 1000 + D)
    lens = [n - 1 for n in ns]
    ref = R.decode_attn_ref(c["qkv"], c["cos"], c["sin"], c["k_cache"], c["v_cache"], lens, Hq, Hkv, D ** -0.5)
    return c, lens, ref


# ------------------------------------------------------------------------------------------------ 1. appended rows, nothing else written
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_appended_rows_and_nothing_else(Hq, Hkv, D, dev):
    from rga3.hip import ops

    c, lens, ref = ragged_case(Hq, Hkv, D)
    B, cap, H = len(lens), 4 * KS(), Hq + 2 * Hkv
    qkv, qkv_b = banded((B, H, D), H * D + 24, torch.bfloat16, dev, "out", data=c["qkv"], seed=1)
    kc3, kc_b = banded((B * cap, Hkv, D), Hkv * D + 8, torch.bfloat16, dev, "out", data=c["k_cache"].reshape(B * cap, Hkv, D), seed=2)
    vc3, vc_b = banded((B * cap, Hkv, D), Hkv * D + 16, torch.bfloat16, dev, "out", data=c["v_cache"].reshape(B * cap, Hkv, D), seed=3)
    out, out_b = banded((B, Hq, D), Hq * D + 8, torch.bfloat16, dev, "out", seed=4)
    kc, vc = kc3.unflatten(0, (B, cap)), vc3.unflatten(0, (B, cap))
    snaps = [snapshot(t) for t in (qkv_b, kc_b, vc_b, out_b)]
    ops.decode_attn(qkv, c["cos"].to(dev), c["sin"].to(dev), kc, vc, torch.tensor(lens, dtype=torch.int32, device=dev), Hq, Hkv, D ** -0.5, out=out)
    for (bk, vw, what), sn in zip(((qkv_b, qkv, "qkv"), (kc_b, kc3, "k_cache"), (vc_b, vc3, "v_cache"), (out_b, out, "out")), snaps):
        assert_outside_unchanged(bk, vw, sn, what)
    assert torch.equal(bits(qkv.cpu()), bits(c["qkv"])), "qkv is read-only"
    k_got, v_got = kc.cpu(), vc.cpu()
    for b, n in enumerate(lens):
        assert torch.equal(bits(v_got[b, n]), bits(ref["v_row"][b])), ("v row", b)
        err = (k_got[b, n].double() - ref["k_exact"][b]).abs()
        bound = R.rotation_bound(ref["k_exact"][b], ref["k_mag"][b])
        assert (err <= bound).all(), ("k row", b, float((err - bound).max()))
        keep = torch.ones(cap, dtype=torch.bool)
        keep[n] = False
        assert torch.equal(bits(k_got[b, keep]), bits(c["k_cache"][b, keep])), ("other k rows", b)
        assert torch.equal(bits(v_got[b, keep]), bits(c["v_cache"][b, keep])), ("other v rows", b)
    assert rel_l2(out.cpu(), ref["out"]) < 1e-2


# ------------------------------------------------------------------------------------------------ 2. one visible key
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_one_visible_key_returns_the_v_row(Hq, Hkv, D, dev):
    c = R.random_case(3, Hq, Hkv, D, 4 * KS(), seed=7)
    out = call(c, [0, 0, 0], Hq, Hkv, dev)[0]
    want = c["qkv"][:, Hq + Hkv:].repeat_interleave(Hq // Hkv, dim=1)
    assert torch.equal(bits(out), bits(want))


# ------------------------------------------------------------------------------------------------ 3. needle
def needle_positions(n):
    ks = KS()
    return list(range(n)) if n <= 2 * ks + 1 else sorted({0, ks - 1, ks, n - 2, n - 1})


@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_needle(Hq, Hkv, D, dev):
    """cos = 1, sin = 0; q = 8 everywhere, every key zero except the needle (8 everywhere): its score 64 sqrt(D) >= 256 leads the others' 0 by more than 150 nats, so
    every other weight is exp(-256 or less) = 0 in f32 and the output is the needle's v row, bit for bit.  One sequence per needle position, one launch per n;
    position n - 1 is the new row itself."""
    cap = 4 * KS()
    for n in counts():
        pos = needle_positions(n)
        B = len(pos)
        base = R.random_case(1, Hq, Hkv, D, cap, seed=n)          # every sequence holds the same random v rows (and NaN keys beyond n): the position tells them apart
        g = torch.Generator().manual_seed(n)
        c = dict(qkv=torch.randn((B, Hq + 2 * Hkv, D), generator=g).to(torch.bfloat16), cos=torch.ones(B, D), sin=torch.zeros(B, D),
                 k_cache=torch.full((B, cap, Hkv, D), float("nan"), dtype=torch.bfloat16), v_cache=base["v_cache"].expand(B, cap, Hkv, D).contiguous())
        c["qkv"][:, :Hq] = 8.0
        c["qkv"][:, Hq:Hq + Hkv] = 0.0
        c["k_cache"][:, :n] = 0.0
        want = torch.empty((B, Hkv, D), dtype=torch.bfloat16)
        for b, p in enumerate(pos):
            if p == n - 1:
                c["qkv"][b, Hq:Hq + Hkv] = 8.0
                want[b] = c["qkv"][b, Hq + Hkv:]
            else:
                c["k_cache"][b, p] = 8.0
                want[b] = c["v_cache"][b, p]
        out = call(c, [n - 1] * B, Hq, Hkv, dev)[0]
        assert torch.equal(bits(out), bits(want.repeat_interleave(Hq // Hkv, dim=1))), n


# ------------------------------------------------------------------------------------------------ 4. uniform scores
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_uniform_scores_give_the_exact_mean(Hq, Hkv, D, dev):
    """q = 0: every visible key weighs the same.  V rows are mean[d] + delta[i] with integer mean[d] in [-64, 64] and integer deltas (+t, -t in pairs, 0 for the odd
    one out) that sum to zero: every partial sum is a small integer (exact in f32 in any order), the column mean is mean[d] exactly, odd n included."""
    ns = counts()
    B, cap = len(ns), 4 * KS()
    c = R.random_case(B, Hq, Hkv, D, cap, seed=11)
    c["qkv"][:, :Hq] = 0.0
    mean = (torch.arange(D) * 37 % 129 - 64).float()
    for b, n in enumerate(ns):
        i = torch.arange(n)
        delta = torch.where(i % 2 == 0, 1.0, -1.0) * (i // 2 % 7 + 1)
        if n % 2:
            delta[n - 1] = 0.0
        assert float(delta.sum()) == 0.0
        rows = (mean[None, None, :] + delta[:, None, None] * (torch.arange(Hkv)[None, :, None] + 1)).expand(n, Hkv, D).to(torch.bfloat16)
        c["v_cache"][b, :n - 1] = rows[:n - 1]
        c["qkv"][b, Hq + Hkv:] = rows[n - 1]
    out = call(c, [n - 1 for n in ns], Hq, Hkv, dev)[0]
    want = mean.to(torch.bfloat16)[None, None, :].expand(B, Hq, D)
    assert torch.equal(bits(out), bits(want))


# ------------------------------------------------------------------------------------------------ 5. poison
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_poison_beyond_the_lengths_and_around_the_inputs(Hq, Hkv, D, dev):
    from rga3.hip import ops

    c, lens, ref = ragged_case(Hq, Hkv, D)
    B, cap, H = len(lens), 4 * KS(), Hq + 2 * Hkv
    clean = call(c, lens, Hq, Hkv, dev)[0]
    kc, vc = c["k_cache"].clone(), c["v_cache"].clone()
    for b, n in enumerate(lens):
        kc[b, n:] = float("nan")      # the row at lens[b] is overwritten by the call, the rest stays poisoned
        vc[b, n:] = float("nan")
    qkv = banded((B, H, D), H * D + 24, torch.bfloat16, dev, "in", data=c["qkv"])[0]
    cos = banded((B, D), D, torch.float32, dev, "in", data=c["cos"])[0]
    sin = banded((B, D), D, torch.float32, dev, "in", data=c["sin"])[0]
    out = ops.decode_attn(qkv, cos, sin, kc.to(dev), vc.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), Hq, Hkv, D ** -0.5).cpu()
    assert_finite_where(out, ref["out"], "poisoned run")
    assert torch.equal(bits(out), bits(clean))
    # other sequences' rows: the same sequence alone, its neighbours all NaN
    for b in (0, B - 1):
        kc2, vc2 = torch.full_like(kc, float("nan")), torch.full_like(vc, float("nan"))
        kc2[b, :lens[b]], vc2[b, :lens[b]] = c["k_cache"][b, :lens[b]], c["v_cache"][b, :lens[b]]
        got = ops.decode_attn(qkv, cos, sin, kc2.to(dev), vc2.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), Hq, Hkv, D ** -0.5).cpu()
        assert torch.equal(bits(got[b]), bits(clean[b])), b


# ------------------------------------------------------------------------------------------------ 6. batch invariance
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_batch_invariance(Hq, Hkv, D, dev):
    ks = KS()
    lens, cap = [0, ks - 1, 2 * ks, 3 * ks + 5], 4 * ks
    c = R.random_case(4, Hq, Hkv, D, cap, seed=21)
    out, k1, v1, _ = call(c, lens, Hq, Hkv, dev)
    again = call(c, lens, Hq, Hkv, dev)
    assert all(torch.equal(bits(a), bits(b_)) for a, b_ in zip((out, k1, v1), again)), "two runs differ"
    for b, n in enumerate(lens):
        one = {k: v[b:b + 1].clone() for k, v in c.items()}
        o1, ka, va, _ = call(one, [n], Hq, Hkv, dev)
        assert torch.equal(bits(o1[0]), bits(out[b])), ("B = 1 differs from the batch", b)
        assert torch.equal(bits(ka[0]), bits(k1[b])) and torch.equal(bits(va[0]), bits(v1[b])), b
        wide = dict(one)
        for name in ("k_cache", "v_cache"):
            wide[name] = torch.cat((one[name], torch.full_like(one[name], float("nan"))), dim=1)
        o2 = call(wide, [n], Hq, Hkv, dev)[0]
        assert torch.equal(bits(o2[0]), bits(out[b])), ("cap doubled differs", b)


# ------------------------------------------------------------------------------------------------ 7. random operands
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_random_operands_against_fp64_and_the_varlen_route(Hq, Hkv, D, dev):
    """Real mRoPE tables at positions up to 5000.  rel-L2 against float64 < 1e-2 (the bound tests/test_kernels_gpu.py holds every attention kernel to) and against
    rope_ + scatter_rows_ + attn_varlen on the same data < 6e-3 (the kernel-to-kernel bound of test_attn_causal32)."""
    from rga3.hip import ops

    c, lens, ref = ragged_case(Hq, Hkv, D)
    B, cap, H = len(lens), 4 * KS(), Hq + 2 * Hkv
    out = call(c, lens, Hq, Hkv, dev)[0]
    e64 = rel_l2(out, ref["out"])
    d = {k: v.to(dev) for k, v in c.items()}
    ops.rope_(d["qkv"], d["cos"], d["sin"], 0, Hq + Hkv)
    rows = d["qkv"].view(B, H * D)
    idx = torch.tensor([b * cap + n for b, n in enumerate(lens)], dtype=torch.int64, device=dev)
    ops.scatter_rows_(d["k_cache"].view(B * cap, Hkv * D), idx, rows[:, Hq * D:(Hq + Hkv) * D])
    ops.scatter_rows_(d["v_cache"].view(B * cap, Hkv * D), idx, rows[:, (Hq + Hkv) * D:])
    kk = torch.cat([d["k_cache"][b, :n + 1] for b, n in enumerate(lens)])
    vv = torch.cat([d["v_cache"][b, :n + 1] for b, n in enumerate(lens)])
    cu_k = torch.tensor([0] + [n + 1 for n in lens], dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)
    cu_q = torch.arange(B + 1, dtype=torch.int32, device=dev)
    old = ops.attn_varlen(d["qkv"][:, :Hq], kk, vv, cu_q, cu_k, 1, D ** -0.5, causal=False, max_k=max(lens) + 1).cpu()
    ekk = rel_l2(out, old)
    print(f"decode_attn Hq={Hq} Hkv={Hkv} D={D}: rel-L2 vs float64 {e64:.3e}, vs rope_ + scatter_rows_ + attn_varlen {ekk:.3e} (that route vs float64 {rel_l2(old, ref['out']):.3e})")
    assert e64 < 1e-2
    assert ekk < 6e-3


# ------------------------------------------------------------------------------------------------ 8. full cache
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_full_cache_writes_nothing_and_returns_nan(Hq, Hkv, D, dev):
    cap = 4 * KS()
    c = R.random_case(2, Hq, Hkv, D, cap, seed=31)
    lens = [cap, 5]
    out, kc, vc, _ = call(c, lens, Hq, Hkv, dev)
    assert torch.isnan(out[0].float()).all()
    assert torch.equal(bits(kc[0]), bits(c["k_cache"][0])) and torch.equal(bits(vc[0]), bits(c["v_cache"][0]))
    ref = R.decode_attn_ref(c["qkv"], c["cos"], c["sin"], c["k_cache"], c["v_cache"], lens, Hq, Hkv, D ** -0.5)
    assert torch.isnan(ref["out"][0]).all()
    assert rel_l2(out[1], ref["out"][1]) < 1e-2
    alone = call({k: v[1:2].clone() for k, v in c.items()}, [5], Hq, Hkv, dev)
    assert torch.equal(bits(alone[0][0]), bits(out[1])) and torch.equal(bits(alone[1][0]), bits(kc[1])) and torch.equal(bits(alone[2][0]), bits(vc[1]))


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_name_the_entry_point(dev):
    from rga3.hip import lib, ops

    def operands(B, Hq, Hkv, D, cap=64):
        z = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=dev)
        return dict(qkv=z(B, Hq + 2 * Hkv, D), cos=torch.ones((B, D), device=dev), sin=torch.zeros((B, D), device=dev), k_cache=z(B, cap, Hkv, D),
                    v_cache=z(B, cap, Hkv, D), lens=torch.zeros(B, dtype=torch.int32, device=dev))

    def run(o, Hq, Hkv, **kw):
        return ops.decode_attn(o["qkv"], o["cos"], o["sin"], o["k_cache"], o["v_cache"], o["lens"], Hq, Hkv, 0.25, **kw)

    run(operands(2, 8, 1, 32), 8, 1)                                       # the operands below are refused for the reason named, not for their construction
    for Hq, Hkv, D in ((9, 1, 32), (4, 2, 24), (4, 2, 256)):
        with pytest.raises(lib.Rga3Error, match="decode_attn"):
            run(operands(2, Hq, Hkv, D), Hq, Hkv)
    o = operands(2, 4, 2, 32)
    short = dict(o, k_cache=o["k_cache"].as_strided((2, 64, 2, 32), (64 * 64, 32, 32, 1)))     # a token stride that does not hold its two heads
    with pytest.raises(lib.Rga3Error, match="decode_attn.*stride"):
        run(short, 4, 2)
    short = dict(o, qkv=o["qkv"].as_strided((2, 8, 32), (8 * 32 - 8, 32, 1)))                  # a row stride shorter than the fused row
    with pytest.raises(lib.Rga3Error, match="decode_attn.*ld_qkv"):
        run(short, 4, 2)
    need = ops.decode_attn_ws_floats(2, 64, 4, 32)
    with pytest.raises(lib.Rga3Error, match="decode_attn.*workspace"):
        run(o, 4, 2, ws=torch.empty(need - 1, dtype=torch.float32, device=dev))
    run(o, 4, 2, ws=torch.empty(need, dtype=torch.float32, device=dev))
    with pytest.raises(lib.Rga3Error, match="decode_attn"):
        run(dict(o, lens=o["lens"].cpu()), 4, 2)
