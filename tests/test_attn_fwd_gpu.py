"""GPU: ops.attn_varlen / ops.attn_varlen_rope (csrc/attn_fwd.hip: the pipelined kernel, the whole-segment window kernel, split keys + combine; csrc/attn_causal32.hip)
per row against float64 and with an exact mask check, on every dispatch route (the table and the checkers: tests/attn_fwd_ref.py, tested by test_attn_fwd_ref_cpu.py).

a. Every (token, head) row of o of every case within FACTOR = 3 times the worst row of the case's bf16 model (P and o rounded to bf16, as the kernels declare: 0.0025 ..
   0.0048 of the row's norm), + 1 for the rope cases; every lse within a derived f32 bound near 1e-4 (attn_fwd_ref.lse_bound), where tests/test_kernels_gpu.py allows a
   whole-tensor rel-L2 of 1e-2 and 2e-2 on lse; rows without a visible key are o = 0, lse = -inf exactly; outputs are handed in full of NaN.
b. One-hot values: a key a row cannot see -- above the causal diagonal, past the ragged end, in the next segment, in another packed block, behind another kv group, in
   another split slice -- contributes exactly zero, and a visible one its float64 P within 2^-7: with needles at the edges, and on 17 cases with every key in turn.
c. A segment alone gives the same bits as inside its batch (run under the batch's max_q / max_k, so on the same template instance: what is tested is that a
   workgroup's arithmetic does not depend on its neighbours or on the grid).  The split route is left out: its slice count depends on the grid (workgroups of the call).
d. A second call gives the same bits (paired, split + combine, causal32).
e. The parity switches: impl 16 is bit-equal to the default and impl 1 (scalar reads of the same LDS image into the same products) to the transposing reads; impl 1, 2, 4
   and 8 meet the per-row allowance on their table cases in (a).  impl 2 / 4 / 8 choose other tilings of the rows: no bit claim.

Measured on MI355X (each test prints its own; the log of the run is profiles/r11_attn_fwd_rows.log):
  general kernel, unpaired, 28 cases ....................... worst row 0.885 .. 1.091 x model (g128-300x437-d120-causal); lse error <= 0.094 of its bound (g32-70-d8-causal)
  general kernel, paired causal blocks, 5 cases ............ worst row 0.954 .. 1.000 x model (g64-512-gqa3-causal); lse error <= 0.022 of its bound (g64-400x437-d48-causal)
  split keys + combine, 3 cases ............................ worst row 0.961 .. 1.022 x model (split-9x1024-d16); lse error <= 0.061 of its bound (split-9x1024-d16)
  window kernel, 14 cases .................................. worst row 0.923 .. 1.000 x model (w64-4-d8); lse error <= 0.099 of its bound (w64-4-d8)
  attn_causal32_kernel, 5 cases ............................ worst row 0.912 .. 1.047 x model (c32-257); lse error <= 0.006 of its bound (c32-385-1-300)
  rope entry (allowed FACTOR + 1), 11 cases ................ worst row 1.000 .. 1.025 x model (rope-c32-300); lse error <= 0.022 of its bound (rope-g32-causal)
  the other route of a case's impl bit .................... impl 0 on g128-513-impl4 0.968, impl 0 on g64-200-impl2 0.885, impl 0 on w96-8-1-5-impl8 0.923, impl 4 on c32-385-1-300 1.000, impl 2 on w64-8-ragged 0.950
Whole-tensor rel-L2 0.0018 .. 0.0022 throughout.  No masked key leaked anywhere (b: 29 cases at the listed edges, 17 with every key a needle); a segment alone
and a second call gave the same bits on every case of (c) and (d); impl 1 and impl 16 were bit-equal to the default on every case of (e)."""
import ctypes as C
import functools

import pytest
import torch

from tests import attn_fwd_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAMES = [c.name for c in R.CASES]
# (b): one paired general case per DP that has the paired form (64, 128), the causal case of the others, causal32, ragged windows, both packings on both kernels, split,
# rope on each of its three kernels, the GQA group of 3
NEEDLE_CASES = ["g128-513-d112-causal", "g128-513-impl4", "g64-512-gqa3-causal", "g64-400x437-d48-causal", "g64-multi-causal", "g96-200x264-d72-causal",
                "g32-385-causal", "g32-70-d8-causal", "g256-100x133-d136-causal", "g128-130", "c32-257", "c32-385-1-300", "c32-300x437", "c32-300x236",
                "w64-8-ragged", "w64-8-d24-cross", "w96-8-2-5-ragged-d72", "w64-4-d8", "w-block16", "w-block4x16", "g-block16-impl2", "g-block4x16-impl2",
                "split-9x1024-d16", "split-ragged-d64", "rope-w64-qk", "rope-g32-causal", "rope-c32-300", "deg-no-keys-d64", "deg-200x136-d128"]
# (b) with every key a needle: the causal cases of each DP and of causal32, ragged windows, packings, a split and a rope case of each kernel
EVERY_KEY_CASES = ["g128-513-d112-causal", "g64-512-gqa3-causal", "g64-400x437-d48-causal", "g96-200x264-d72-causal", "g32-100x133-d24-causal",
                   "g256-100x133-d136-causal", "c32-257", "c32-385-1-300", "c32-300x236", "w64-8-ragged", "w64-8-d24-cross", "w-block4x16", "g-block16-impl2",
                   "split-ragged-d64", "rope-w64-qk", "rope-g32-causal", "rope-c32-300"]
ALONE_CASES = ["g64-multi-causal", "w64-8-ragged", "w96-8-2-5-ragged-d72", "c32-385-1-300"]
TWICE_CASES = ["g128-513-d112-causal", "g64-512-gqa3-causal", "split-9x1024-d16", "split-64x1024-d256", "split-ragged-d64", "c32-257", "c32-385-1-300"]


def run(dev, c, d, cq, ck, scale, v=None, max_q=None, max_k=None, impl=None, lse=True):
    """One forward call of case c through ops on device copies of the operands d (v: other values; max_q / max_k / impl: other than the case's) -> (o, lse) on the CPU.
    o is handed in full of NaN: a row the kernels do not write stays visible."""
    from rga3.hip import ops

    q, k, vv = (t.to(dev).contiguous() for t in (d["q"], d["k"], d["v"] if v is None else v))
    cqd = cq.to(dev)
    ckd = cqd if c.same_cu else ck.to(dev)
    out = torch.full(q.shape, float("nan"), dtype=BF, device=dev)
    max_q = max(c.lq) if max_q is None else max_q
    if c.rope:
        got = ops.attn_varlen_rope(q, k, vv, cqd, ckd, max_q, scale, d["cos"].to(dev), d["sin"].to(dev), causal=c.causal, rope_k=c.rope == "qk", out=out, return_lse=lse)
    else:
        mk = (max(c.lk) if c.max_k is None else c.max_k) if max_k is None else max_k
        got = ops.attn_varlen(q, k, vv, cqd, ckd, max_q, scale, c.causal, out=out, return_lse=lse, impl=c.impl if impl is None else impl, block=c.block, max_k=mk)
    torch.cuda.synchronize()
    return (got[0].cpu(), got[1].cpu()) if lse else (got.cpu(), None)


def run_c_entry(dev, c, d, cq, ck, scale):
    """The same call through the C entry points with o AND lse handed in full of NaN (ops allocates lse itself); the split workspace as ops sizes it."""
    from rga3.hip import lib

    q, k, v = (t.to(dev).contiguous() for t in (d["q"], d["k"], d["v"]))
    cqd = cq.to(dev)
    ckd = cqd if c.same_cu else ck.to(dev)
    Tq, Hq, D = q.shape
    out = torch.full(q.shape, float("nan"), dtype=BF, device=dev)
    lse = torch.full((Hq, Tq), float("nan"), dtype=F32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    strides = [x for t in (q, k, v, out) for x in (t.stride(0), t.stride(1))]
    if c.rope:
        cos, sin = d["cos"].to(dev), d["sin"].to(dev)
        kc, ks = (cos.data_ptr(), sin.data_ptr()) if c.rope == "qk" else (None, None)
        rc = lib.load().rga3_attn_varlen_fwd_rope(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), cqd.data_ptr(), ckd.data_ptr(), len(c.lq),
                                                  max(c.lq), Tq, Hq, c.Hkv, D, *strides, float(scale), int(c.causal), cos.data_ptr(), sin.data_ptr(), kc, ks, st)
    else:
        ws = torch.empty((8 * Tq * Hq * (D + 1),), dtype=F32, device=dev) if c.family == "split" else None
        bq, bk = c.block or (0, 0)
        rc = lib.load().rga3_attn_varlen_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), cqd.data_ptr(), ckd.data_ptr(), len(c.lq), max(c.lq),
                                             Tq, Hq, c.Hkv, D, *strides, float(scale), int(c.causal), c.impl, ws.data_ptr() if ws is not None else None,
                                             ws.numel() if ws is not None else 0, max(c.lk) if c.max_k is None else c.max_k, bq, bk, st)
    assert rc == 0, (rc, lib.last_error())
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu()


@functools.lru_cache(maxsize=None)
def result(dev, name):
    """(o, lse) of a table case through ops: one call per case and session, shared by the tests that compare against it, never modified."""
    d, cq, ck, scale, _, _ = R.case_refs(name)
    return run(dev, R.BY_NAME[name], d, cq, ck, scale)


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == BF else torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ a. every row against float64
@pytest.mark.parametrize("name", NAMES)
def test_every_row_against_float64(name, dev):
    o, lse = result(dev, name)
    R.check_case(name, o, lse, what=R.BY_NAME[name].family)


@pytest.mark.parametrize("name", NAMES)
def test_c_entry_writes_every_row_of_o_and_lse(name, dev):
    """o and lse pre-filled with NaN: nothing stays unwritten, lse is -inf exactly where the reference has it, and the bits are those of the call through ops."""
    d, cq, ck, scale, exact, _ = R.case_refs(name)
    o, lse = run_c_entry(dev, R.BY_NAME[name], d, cq, ck, scale)
    assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
    assert torch.equal(lse == float("-inf"), torch.isinf(exact.lse)) and torch.isfinite(lse[torch.isfinite(exact.lse)]).all()
    o2, lse2 = result(dev, name)
    assert same_bits(o, o2) and same_bits(lse, lse2)


def test_degenerate_rows_are_exact(dev):
    """What the table's degenerate cases contain, spelled out: rows without a visible key, on the general, window and causal32 kernels."""
    for name, rows in (("deg-no-keys-d64", slice(100, 130)), ("deg-no-keys-d128", slice(100, 130)), ("deg-200x136-d64", slice(0, 64)), ("deg-200x136-d128", slice(0, 64)),
                       ("c32-300x236", slice(0, 64)), ("w64-4-no-keys", slice(40, 70))):
        o, lse = result(dev, name)
        exact = R.case_refs(name)[4]
        assert (exact.lse[:, rows] == float("-inf")).all() and torch.isfinite(exact.lse).sum() == exact.lse.numel() - exact.lse[:, rows].numel()
        assert (o[rows] == 0).all() and (lse[:, rows] == float("-inf")).all(), name
        assert torch.isfinite(lse).sum() == lse.numel() - lse[:, rows].numel(), name


# ------------------------------------------------------------------------------------------------ b. exact mask
@pytest.mark.parametrize("name,every_key", [(n, False) for n in NEEDLE_CASES] + [(n, True) for n in EVERY_KEY_CASES])
def test_a_masked_key_contributes_exactly_nothing(name, every_key, dev):
    """every_key: each key of the call is a needle in turn (ceil(keys / D) calls), so the WHOLE probability matrix of every head is compared with float64, zeros exactly:
    a mask that is off for one row anywhere shows.  Otherwise the needles sit at the edges attn_fwd_ref.needle_keys lists, in ONE kv head per call, so that the query
    heads of the other groups must stay exactly zero."""
    c = R.BY_NAME[name]
    d, cq, ck, scale, _, _ = R.case_refs(name)
    keys = list(range(sum(c.lk))) if every_key else R.needle_keys(c)
    calls = [keys[i:i + c.D] for i in range(0, len(keys), c.D)]
    for n, chunk in enumerate(calls):
        hk = None if every_key else (n + 1) % c.Hkv
        v = R.needle_values(c, chunk, hk)
        want = R.attn_fwd_ref(d["qr"], d["kr"], v, cq, ck, scale, c.causal, c.block).o
        o, _ = run(dev, c, d, cq, ck, scale, v=v, lse=False)
        R.check_needles(f"{name} call {n} (kv head {'all' if hk is None else hk}, keys {chunk[0]} .. {chunk[-1]})", o, want, cq)
    print(f"{name}: {len(keys)} needles in {len(calls)} calls")


# ------------------------------------------------------------------------------------------------ c. a segment does not depend on its neighbours
@pytest.mark.parametrize("name", ALONE_CASES)
def test_a_segment_alone_gives_the_same_bits(name, dev):
    c = R.BY_NAME[name]
    d, cq, ck, scale, _, _ = R.case_refs(name)
    o, lse = result(dev, name)
    for s in range(len(c.lq)):
        qa, qb, ka, kb = int(cq[s]), int(cq[s + 1]), int(ck[s]), int(ck[s + 1])
        one = {"q": d["q"][qa:qb], "k": d["k"][ka:kb], "v": d["v"][ka:kb]}
        o1, lse1 = run(dev, c, one, R.cu([qb - qa]), R.cu([kb - ka]), scale, max_q=max(c.lq), max_k=max(c.lk))
        assert same_bits(o[qa:qb], o1), (name, "segment", s, "o", int((o[qa:qb].view(torch.int16) != o1.view(torch.int16)).sum()), "elements differ")
        assert same_bits(lse[:, qa:qb].contiguous(), lse1), (name, "segment", s, "lse")


# ------------------------------------------------------------------------------------------------ d. same bits on a second call
@pytest.mark.parametrize("name", TWICE_CASES)
def test_second_call_gives_the_same_bits(name, dev):
    """No atomics, fixed order: fresh NaN-filled outputs (and a fresh split workspace) each time."""
    d, cq, ck, scale, _, _ = R.case_refs(name)
    o, lse = result(dev, name)
    o2, lse2 = run(dev, R.BY_NAME[name], d, cq, ck, scale)
    assert same_bits(o, o2) and same_bits(lse, lse2), name


# ------------------------------------------------------------------------------------------------ e. parity switches
def test_impl16_and_impl1_are_bit_equal_to_the_default(dev):
    """impl 16 keeps a sixth output tile whose columns are never stored; impl 1 reads the V fragments element by element from the same LDS image into the same products."""
    for name in ("g96-512-d72", "g96-40x300-d80", "g96-200x264-d72-causal"):     # the three five-tile instances of the table
        c = R.BY_NAME[name]
        d, cq, ck, scale, _, _ = R.case_refs(name)
        o5, lse5 = result(dev, name)
        o6, lse6 = run(dev, c, d, cq, ck, scale, impl=16)
        assert same_bits(o5, o6) and same_bits(lse5, lse6), name
    for name in ("g64-100x150-impl1-causal", "g128-255-causal", "g32-100x133-d24-causal", "g256-70-d192"):
        c = R.BY_NAME[name]
        d, cq, ck, scale, _, _ = R.case_refs(name)
        a = run(dev, c, d, cq, ck, scale, impl=0)
        b = run(dev, c, d, cq, ck, scale, impl=1)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), name


@pytest.mark.parametrize("name,impl", [("g128-513-impl4", 0), ("g64-200-impl2", 0), ("w96-8-1-5-impl8", 0), ("c32-385-1-300", 4), ("w64-8-ragged", 2)])
def test_the_other_route_meets_the_same_allowance(name, impl, dev):
    """The same operands on the route the case's impl bit avoids (or takes): the allowance is the case's own; no bit claim between different tilings."""
    c = R.BY_NAME[name]
    d, cq, ck, scale, _, _ = R.case_refs(name)
    o, lse = run(dev, c, d, cq, ck, scale, impl=impl)
    R.check_case(name, o, lse, what=f"impl {impl}")


# ------------------------------------------------------------------------------------------------ refusals
def test_routes_outside_the_contract_are_refused(dev):
    """The rope entry has no kernel for segments of 65 .. 255 queries, for causal D != 128 rows or for long rows whose keys it would have to rotate; packing is non-causal."""
    from rga3.hip import lib, ops

    c = R.BY_NAME["rope-w64-qk"]
    d, cq, ck, scale, _, _ = R.case_refs(c.name)
    q, k, v, cos, sin = (d[n].to(dev) for n in ("q", "k", "v", "cos", "sin"))
    cud = cq.to(dev)
    for max_q, causal in ((65, False), (255, True), (256, True)):                # D = 64: no long-row form
        with pytest.raises(lib.Rga3Error):
            ops.attn_varlen_rope(q, k, v, cud, cud, max_q, scale, cos, sin, causal=causal, rope_k=True)
    with pytest.raises(lib.Rga3Error):
        ops.attn_varlen(q, k, v, cud, cud, 64, scale, True, block=(16, 16))
    with pytest.raises(lib.Rga3Error):
        ops.attn_varlen(q, k, v, cud, cud, 64, scale, False, block=(16, 12))
    with pytest.raises(lib.Rga3Error):
        ops.attn_varlen(q, k, v, cud, cud, 64, scale, False, impl=32)
    c = R.BY_NAME["rope-c32-300"]
    d, cq, ck, scale, _, _ = R.case_refs(c.name)
    q, k, v, cos, sin = (d[n].to(dev) for n in ("q", "k", "v", "cos", "sin"))
    with pytest.raises(lib.Rga3Error):                                           # long causal rows: keys must arrive rotated
        ops.attn_varlen_rope(q, k, v, cq.to(dev), cq.to(dev), 300, scale, cos, sin, causal=True, rope_k=True)
