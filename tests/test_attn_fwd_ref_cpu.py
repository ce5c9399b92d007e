"""CPU: the float64 reference of the attention forward (tests/attn_fwd_ref.py) against the fp32 oracle, against a plain float64 softmax written per segment and
against attn_bwd_ref's o / lse; its bf16 error model pinned on every case of the GPU table; and the checkers of tests/test_attn_fwd_gpu.py on seeded defects, each of
which they must reject while the whole-tensor rel-L2 < 1e-2 of tests/test_kernels_gpu.py::test_attn_varlen lets the small ones pass (the gap those tests close)."""
import pytest
import torch

from oracle import kernels_ref as KR
from tests import attn_bwd_ref as B
from tests import attn_fwd_ref as R

# worst row of the model=True yardstick against the exact result, per case family (measured over the whole table: general 0.0026 .. 0.0048, paired 0.0029 .. 0.0033,
# split 0.0025 .. 0.0036, window 0.0028 .. 0.0045, causal32 0.0028 .. 0.0031, rope 0.0028 .. 0.0031; the largest at D = 8: essentially the final bf16 rounding); the pin is the measured
# maximum times 1.4, the headroom tests/test_attn_bwd_ref_cpu.py leaves (0.0056 -> 0.008)
MODEL_BOUND = {"general": 0.0068, "paired": 0.0047, "split": 0.0050, "window": 0.0063, "causal32": 0.0043, "rope": 0.0044}
MODEL_FLOOR = 0.002


def plain(q, k, v, cq, ck, scale, causal, block=None):
    """softmax(mask(scale q k^T)) v in float64, head by head, with torch.softmax / torch.logsumexp: shares no line with attn_fwd_ref."""
    Tq, Hq, D = q.shape
    G = Hq // k.shape[1]
    o = torch.zeros(Tq, Hq, D, dtype=torch.float64)
    lse = torch.full((Hq, Tq), float("-inf"), dtype=torch.float64)
    for s in range(len(cq) - 1):
        q0, q1, k0, k1 = int(cq[s]), int(cq[s + 1]), int(ck[s]), int(ck[s + 1])
        for h in range(Hq):
            for i in range(q1 - q0):
                js = [j for j in range(k1 - k0) if (not causal or j <= i + (k1 - k0) - (q1 - q0)) and (not block or i // block[0] == j // block[1])]
                if not js:
                    continue
                kk, vv = k[k0:k1, h // G].double()[js], v[k0:k1, h // G].double()[js]
                sc = (kk @ q[q0 + i, h].double()) * scale
                o[q0 + i, h] = torch.softmax(sc, 0) @ vv
                lse[h, q0 + i] = torch.logsumexp(sc, 0)
    return o, lse


SMALL = [([37, 5, 1], [37, 5, 1], 4, 2, 16, True, None), ([9, 6], [20, 11], 3, 3, 8, False, None), ([12], [19], 2, 1, 24, True, None),
         ([7, 3], [4, 3], 2, 1, 8, True, None), ([5, 0, 3, 4], [5, 6, 0, 4], 4, 2, 8, True, None), ([16, 8], [32, 16], 2, 2, 8, False, (4, 8))]


@pytest.mark.parametrize("lq,lk,Hq,Hkv,D,causal,block", SMALL)
def test_reference_against_a_plain_softmax_and_the_fp32_oracle(lq, lk, Hq, Hkv, D, causal, block):
    d = B.make_case(lq, lk, Hq, Hkv, D, seed=sum(lq) + D)
    cq, ck, scale = R.cu(lq), R.cu(lk), D ** -0.5
    ref = R.attn_fwd_ref(d["q"], d["k"], d["v"], cq, ck, scale, causal, block)
    o, lse = plain(d["q"], d["k"], d["v"], cq, ck, scale, causal, block)
    assert torch.equal(torch.isinf(ref.lse), torch.isinf(lse)) and (ref.lse[torch.isinf(lse)] == float("-inf")).all()
    seen = torch.isfinite(lse)
    assert ((ref.lse - lse)[seen].abs() <= 1e-13 * lse[seen].abs().clamp_min(1)).all()
    assert ((ref.o - o).abs() <= 1e-13 * (1 + o.abs())).all()
    assert (ref.o[(~seen).t()] == 0).all()
    if block is None and all(a <= b for a, b in zip(lq, lk)) and all(lk[i] > 0 for i in range(len(lq)) if lq[i]):   # the oracle has no packing and NaN rows without a key
        oo, ol = KR.attn_varlen_ref(d["q"], d["k"], d["v"], cq, ck, scale, causal)
        assert R.rel_l2(oo, ref.o) < 1e-5 and float((ol.double() - ref.lse).abs().max()) < 1e-4


@pytest.mark.parametrize("name", ["513-gqa2-d128", "400x437-d72", "empty-q-segment", "negative-shift", "cross-9x64-d16", "70-noncausal-d32"])
def test_reference_equals_the_backward_reference(name):
    """On the backward table's own operands: attn_bwd_ref's o is bf16(P V) and its lse the f32 rounding, of the same mathematics."""
    c = B.BY_NAME[name]
    d, cq, ck, scale = B.case_operands(c)
    bwd = B.attn_bwd_ref(d["q"], d["k"], d["v"], d["do"], cq, ck, scale, c.causal)
    fwd = R.attn_fwd_ref(d["q"], d["k"], d["v"], cq, ck, scale, c.causal)
    assert torch.equal(torch.isinf(fwd.lse), torch.isinf(bwd.lse))
    seen = torch.isfinite(fwd.lse)
    assert ((fwd.lse - bwd.lse.double())[seen].abs() <= 2.0 ** -24 * (1 + 1e-6) * fwd.lse[seen].abs()).all()      # f32 rounds to nearest
    assert ((fwd.o - bwd.o.double()).abs() <= 2.0 ** -8 * (1 + 1e-5) * fwd.o.abs()).all()                          # bf16: half an ulp <= 2^-8 relative; P = exp(s - f32 lse)
    assert R.rel_l2(R.bf16_of(fwd.o), bwd.o) < 1e-4                                                                # but for rounding ties the same bf16 numbers


def test_model_rounds_p_and_o_only():
    """model=True: lse is the exact one (the row sum is taken from the unrounded exponentials), o is a bf16 number within two roundings of the exact o."""
    for name in ("g64-9x300-d40", "deg-200x136-d64"):
        _, _, _, _, exact, model = R.case_refs(name)
        assert torch.equal(exact.lse, model.lse)
        assert torch.equal(R.bf16_of(model.o), model.o)
        assert 0 < R.rel_l2(model.o, exact.o) < 4e-3


def test_rope_helper():
    """Rotate-half from f32 tables with one rounding: against the oracle's rope_ref (f32), and exact where the rotation is a permutation (cos = 0, sin = 1)."""
    c = R.BY_NAME["rope-w64-qk"]
    cos, sin = R.rope_tables(c.lq, c.D)
    assert cos.dtype == sin.dtype == torch.float32 and tuple(cos.shape) == (sum(c.lq), c.D)
    assert torch.equal(cos * 64, torch.round(cos * 64)) and torch.equal(cos[0], torch.ones(c.D)) and torch.equal(cos[64], torch.ones(c.D))   # positions restart
    x = torch.randn(sum(c.lq), 3, c.D, generator=torch.Generator().manual_seed(3)).to(R.BF)
    assert torch.equal(R.rope_rotate(x, cos, sin), KR.rope_ref(x, cos, sin).to(R.BF))          # exact products: the f32 and the float64 rotation round the same number
    z, one = torch.zeros_like(cos), torch.ones_like(cos)
    assert torch.equal(R.rope_rotate(x, z, one), torch.cat([-x[..., c.D // 2:], x[..., :c.D // 2]], -1))
    d = R.case_refs("rope-w64-q")[0]
    assert torch.equal(d["k"], d["kr"]) and not torch.equal(d["q"], d["qr"])


def test_table_names_every_route():
    """The table is what the GPU tests iterate: every family is there, every case is below the 1 100-key limit, and the split cases split by the entry point's rule."""
    assert {c.family for c in R.CASES} == set(R.FAMILIES)
    assert max(max(c.lk) for c in R.CASES) <= 1100 and max(c.Hq for c in R.CASES) <= 8
    assert R.slice_starts(R.BY_NAME["split-9x1024-d16"]) == [[0, 512]]
    assert R.slice_starts(R.BY_NAME["split-ragged-d64"]) == [[0, 576], [0]]              # the 40-key segment: slice 1 holds no key
    assert R.slice_starts(R.BY_NAME["g64-300"]) == [[]]


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_model_error_stays_where_it_was_measured(name):
    worst = R.model_worst_row(name)
    print(f"{name}: model worst row {worst:.5f}")
    assert MODEL_FLOOR < worst < MODEL_BOUND[R.BY_NAME[name].family], (name, worst)


# ---------------------------------------------------------------------------------------------------------------- seeded defects
def accepts(name, o, lse):
    try:
        R.check_case(name, o, lse, what="seeded")
    except AssertionError as e:
        print("rejected:", e)
        return False
    return True


def splice(name, tokens, h, keys, hk=None, causal=None, q=None):
    """The model's output of case `name` with the rows `tokens` (a global range) of query head h recomputed from the global key range `keys` of kv head hk alone."""
    c = R.BY_NAME[name]
    d, _, _, scale, _, model = R.case_refs(name)
    hk = h // (c.Hq // c.Hkv) if hk is None else hk
    (qa, qb), (ka, kb) = tokens, keys
    qq = d["qr"] if q is None else q
    part = R.attn_fwd_ref(qq[qa:qb, h:h + 1], d["kr"][ka:kb, hk:hk + 1], d["v"][ka:kb, hk:hk + 1], R.cu([qb - qa]), R.cu([kb - ka]), scale,
                          c.causal if causal is None else causal, model=True)
    o, lse = model.o.clone(), model.lse.clone()
    o[qa:qb, h] = part.o[:, 0]
    lse[h, qa:qb] = part.lse[0]
    return o, lse


def defect(which):
    """-> (case name, o, lse) of the model output with one seeded defect."""
    if which == "causal limit + 1 on one 16-row tile of one head":           # rows 496 .. 511 also see key r + 1
        return ("g128-513-d112-causal",) + splice("g128-513-d112-causal", (496, 512), 1, (0, 513))
    if which == "last visible key dropped from row 256 on, one head":        # rows 256 .. 384 of the first segment see keys <= r - 1
        return ("c32-385-1-300",) + splice("c32-385-1-300", (256, 385), 2, (0, 384))
    if which == "last visible key dropped in the single-row last block of [257]":
        return ("c32-257",) + splice("c32-257", (256, 257), 3, (0, 256), causal=False)
    if which == "last 32 keys of a ragged window dropped for one wave":      # segment 1 (100 keys, tokens 256 .. 355), the wave of its rows 16 .. 31
        return ("w64-8-ragged",) + splice("w64-8-ragged", (272, 288), 0, (256, 256 + 68))
    if which == "one query head reads the neighbouring kv head":
        return ("g64-512-gqa3-causal",) + splice("g64-512-gqa3-causal", (0, 512), 3, (0, 512), hk=0)
    if which == "one split slice ignored for one row":                        # row 5 of head 3 without the keys of slice 1 (512 ..)
        return ("split-9x1024-d16",) + splice("split-9x1024-d16", (5, 6), 3, (0, 512))
    if which == "the neighbour token's cos / sin row":
        name = "rope-w64-qk"
        d = R.case_refs(name)[0]
        q = d["qr"].clone()
        q[70:71] = R.rope_rotate(d["q"][70:71], d["cos"][71:72], d["sin"][71:72])
        return (name,) + splice(name, (70, 71), 1, (64, 81), q=q)
    _, _, _, _, _, model = R.case_refs("g128-255-causal")
    o, lse = model.o.clone(), model.lse.clone()
    if which == "lse of one row off by 1e-3":
        lse[1, 200] += 1e-3
    elif which == "one row of o left unwritten":
        o[200, 1] = float("nan")
    else:
        raise KeyError(which)
    return "g128-255-causal", o, lse


DEFECTS = ["causal limit + 1 on one 16-row tile of one head", "last visible key dropped from row 256 on, one head", "last 32 keys of a ragged window dropped for one wave",
           "one query head reads the neighbouring kv head", "one split slice ignored for one row", "the neighbour token's cos / sin row", "lse of one row off by 1e-3",
           "one row of o left unwritten", "last visible key dropped in the single-row last block of [257]"]
SLIPS_PAST_REL_L2 = [DEFECTS[0], DEFECTS[6], DEFECTS[8]]                    # one tile or one row of a few hundred: what the whole-tensor bounds accept


@pytest.mark.parametrize("which", DEFECTS)
def test_checker_rejects_a_seeded_defect(which):
    name, o, lse = defect(which)
    _, _, _, _, exact, model = R.case_refs(name)
    assert accepts(name, model.o, model.lse)
    assert accepts(name, model.o, model.lse.float())                        # and an f32 lse, as the kernels write it: 2^-24 relative is inside the bound
    assert not (torch.equal(o.nan_to_num(7.0), model.o) and torch.equal(lse, model.lse)), "the defect changed nothing"
    assert not accepts(name, o, lse), which
    if which in SLIPS_PAST_REL_L2:
        assert R.rel_l2(o.nan_to_num(0.0), exact.o) < 1e-2 and float((lse - exact.lse).nan_to_num(0.0).abs().max()) < 2e-2, "the old bounds see it too"


def test_checker_names_the_row():
    name, o, lse = defect("one row of o left unwritten")
    with pytest.raises(AssertionError, match=r"token 200 head 1 \(segment 0, row 200, 16-row tile 12\)"):
        R.check_case(name, o, lse)
    _, _, _, _, _, model = R.case_refs("deg-no-keys-d64")
    o = model.o.clone()
    o[110, 2, 5] = 2.0 ** -120                                              # a row without a key must be zero exactly
    with pytest.raises(AssertionError, match=r"not zero at token 110 head 2 \(segment 1, row 10"):
        R.check_case("deg-no-keys-d64", o, model.lse)
    lse = model.lse.clone()
    lse[2, 110] = -1e30                                                     # and its lse -inf, not merely very negative
    with pytest.raises(AssertionError, match="lse"):
        R.check_case("deg-no-keys-d64", model.o, lse)


@pytest.mark.parametrize("name", ["g64-400x437-d48-causal", "w-block4x16", "split-ragged-d64", "c32-385-1-300"])
def test_needle_checker(name):
    """One-hot values: the model of the needle call passes; one masked element of 1e-6 (a P of that size moves a randn row by far less than its allowance), a needle seen
    through the other kv group, and a visible P off by 2 % (2^-7 is 0.8 %, the model's own roundings up to 0.4 %) are each rejected."""
    c = R.BY_NAME[name]
    d, cq, ck, scale, _, _ = R.case_refs(name)
    keys = R.needle_keys(c)
    assert keys == sorted(set(keys)) and 0 <= keys[0] and keys[-1] < sum(c.lk) and len(keys) >= 4
    keys = keys[:c.D]
    v = R.needle_values(c, keys, 1)
    assert float(v.float().sum()) == len(keys)
    want = R.attn_fwd_ref(d["qr"], d["kr"], v, cq, ck, scale, c.causal, c.block).o
    model = R.attn_fwd_ref(d["qr"], d["kr"], v, cq, ck, scale, c.causal, c.block, model=True).o
    G = c.Hq // c.Hkv
    assert (want[:, :G] == 0).all() and (want[:, G:, len(keys):] == 0).all() and (want[:, G:, :len(keys)] > 0).any()
    R.check_needles(name, model, want, cq)
    masked = ((want[:, G:, :len(keys)] == 0).nonzero())
    assert masked.numel(), "every case has needles some row cannot see"
    t, h, n = masked[len(masked) // 2].tolist()
    leak = model.clone()
    leak[t, G + h, n] = 1e-6
    with pytest.raises(AssertionError, match="leaks"):
        R.check_needles(name, leak, want, cq)
    other = model.clone()
    other[:, 0] = model[:, G]
    with pytest.raises(AssertionError, match="leaks"):
        R.check_needles(name, other, want, cq)
    t, h, n = (want == want.max()).nonzero()[0].tolist()
    off = model.clone()
    off[t, h, n] *= 1.02
    with pytest.raises(AssertionError, match="float64 has"):
        R.check_needles(name, off, want, cq)
