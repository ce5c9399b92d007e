"""GPU: the weight-only e4m3 kernels of the decode step (csrc/gemv_w8.hip) -- the power-of-two row quantiser bit for bit against tests/w8_ref.py, the weight
stream against the dequantised weights: every code at every position, bit-identical to the bf16 stream (tile 40) on exactly summable operands, inside derived
bounds of float64 on random ones, inside its views, and refusing what it cannot run."""
import pytest
import torch

from tests import guard_bands as G
from tests.w8_ref import SHAPES, VALID_CODES, dequant_ref, edge_matrix, quant_ref

pytestmark = pytest.mark.gpu

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


@pytest.fixture(scope="module")
def ops():
    from rga3.hip import ops as _ops

    return _ops


# ------------------------------------------------------------------------------------------------ 1. quantiser
def _assert_quant_equals_ref(w_cpu, q, sc):
    codes, scale = quant_ref(w_cpu)
    assert torch.equal(sc.cpu(), scale)
    assert torch.equal(q.cpu(), codes.view(U8))


@pytest.mark.parametrize("rows,K", SHAPES + ((37888, 3584),), ids=lambda v: str(v))
def test_quantiser_bit_for_bit(dev, ops, rows, K):
    """Codes and scales equal quant_ref's: a zero row, amax exactly 448 * 2^k and the next bf16 above it, subnormal codes and their ties, K = 16."""
    w = edge_matrix(rows, K, seed=rows + K)
    q, sc = ops.quant_e4m3_rows_pow2(w.to(dev))
    _assert_quant_equals_ref(w, q, sc)


def test_quantiser_strided_input_and_output(dev, ops):
    w = edge_matrix(96, 176, seed=3)
    back = torch.full((96, 200), float("nan"), dtype=BF, device=dev)
    back[:, :176] = w.to(dev)
    qback = torch.full((96, 208), 0x55, dtype=U8, device=dev)
    sc = torch.empty(96, dtype=F32, device=dev)
    ops.quant_e4m3_rows_pow2(back[:, :176], out=(qback[:, :176], sc))
    _assert_quant_equals_ref(w, qback[:, :176], sc)
    assert bool((qback[:, 176:] == 0x55).all())


def test_quantiser_subnormal_and_huge_rows(dev, ops):
    """Rows of bf16 subnormals (k clamps at -126) and rows near the top of the bf16 range."""
    w = edge_matrix(8, 64, seed=9).float()
    w[4] *= 2.0 ** -130
    w[5] = torch.randn(64) * 2.0 ** -131            # (bf16's smallest subnormal is 2^-133)
    w[6] = torch.randn(64) * 2.0 ** 120
    w = w.to(BF)
    q, sc = ops.quant_e4m3_rows_pow2(w.to(dev))
    _assert_quant_equals_ref(w, q, sc)
    assert sc[5].item() == 2.0 ** -126


# ------------------------------------------------------------------------------------------------ 2. every code, every position
def test_every_code_at_every_position(dev, ops):
    """W [72, 272] cycles through the 254 non-NaN codes, row scales 2^-9 ... 2^-6; one-hot activation rows, four at a time (68 launches, f32 output), read
    the dequantised weight column back exactly: the decode of every code and the (row, k) indexing of every chunk, lane and ragged wave."""
    N, K = 72, 272
    valid = torch.tensor(VALID_CODES, dtype=torch.int64)
    codes = valid[(torch.arange(N * K) * 7 + torch.arange(N * K) // K) % 254].to(U8).view(N, K)
    assert set(codes.flatten().tolist()) == set(VALID_CODES)
    scale = torch.exp2(-9.0 + (torch.arange(N) % 4).float())
    want = dequant_ref(codes.view(torch.float8_e4m3fn), scale)          # [N, K]
    wq, sw = codes.to(dev), scale.to(dev)
    eye = torch.eye(K, dtype=BF, device=dev)
    got = torch.empty((K, N), dtype=F32, device=dev)
    for k0 in range(0, K, 4):
        ops.gemv_w8(eye[k0:k0 + 4], wq, sw, out_dtype=F32, out=got[k0:k0 + 4])
    # compared as numbers: code 0x80 is -0, and a sum that starts at +0 returns +0 for it (as the bf16 stream does); every other value has one bit pattern
    assert torch.equal(got.cpu(), want.t().contiguous()) and bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------ 3. exactly summable operands
EXACT_SHAPES = (("none", 4608, 3584, True, False), ("none", 3584, 3584, False, True), ("swiglu", 37888, 3584, False, False), ("none", 3584, 18944, False, True),
                ("none", 1002, 272, True, False), ("none", 70, 176, True, True), ("swiglu", 96, 176, True, False))
_exact_cache = {}


def _exact_operands(dev, ops, N, K):
    """w = c * 2^-9 with integer c in [-16, 16] and one element per row equal to 448 * 2^-9 (the scale is then exactly 2^-9 and the codes exactly c); activations
    integers in [-4, 4].  sum |x c| <= 4 * (16 K + 448) < 2^24 at K = 18944: every partial sum, in any order, is exact in f32."""
    if (N, K) not in _exact_cache:
        _exact_cache.clear()          # one shape's operands at a time (the widest is 37888 x 3584)
        g = torch.Generator(device=dev).manual_seed(N * 31 + K)
        c = torch.randint(-16, 17, (N, K), generator=g, device=dev, dtype=torch.int32)
        c[torch.arange(N, device=dev), torch.randint(0, K, (N,), generator=g, device=dev)] = 448
        w = (c.float() * 2.0 ** -9).to(BF)
        wq, sw = ops.quant_e4m3_rows_pow2(w)
        assert bool((sw == 2.0 ** -9).all())
        assert torch.equal(wq.view(torch.float8_e4m3fn).float(), c.float())
        a = torch.randint(-4, 5, (4, K), generator=g, device=dev, dtype=torch.int32)
        assert 4 * (16 * K + 448) < 2 ** 24
        _exact_cache[(N, K)] = (c, w, wq, sw, a)
    return _exact_cache[(N, K)]


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("act,N,K,bias,res", EXACT_SHAPES, ids=lambda v: str(v))
def test_exact_operands_bit_identical_to_tile_40(dev, ops, act, N, K, bias, res, M):
    c, w, wq, sw, a32 = _exact_operands(dev, ops, N, K)
    a = a32[:M].to(BF)
    n_out = N // 2 if act == "swiglu" else N
    g = torch.Generator(device=dev).manual_seed(5)
    b = torch.randint(-8, 9, (N,), generator=g, device=dev).to(BF) if bias else None
    r = torch.randn((M, n_out), generator=g, device=dev).to(BF) if res else None
    got = ops.gemv_w8(a, wq, sw, b, r, act=act)
    want = ops.gemm(a, w, b, r, act=act)           # M <= 4: the bf16 weight stream (tile 40)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    if act == "none":
        got32 = ops.gemv_w8(a, wq, sw, b, None, out_dtype=F32)
        want32 = ops.gemm(a, w, b, None, out_dtype=F32)
        assert torch.equal(got32.view(torch.int32), want32.view(torch.int32))
        # integer reference in units of 2^-9 (float64 holds these integers exactly; int64 for the comparison)
        ref = (a32[:M].double() @ c.double().t()).to(torch.int64)
        if bias:
            ref = ref + (b.double() * 512).to(torch.int64)[None, :]
        assert torch.equal((got32.double() * 512).to(torch.int64), ref)


# ------------------------------------------------------------------------------------------------ 4. random operands against float64
@pytest.mark.parametrize("act,N,K,bias,res,M,f32", [("none", 1002, 272, True, False, 3, True), ("none", 70, 176, True, True, 4, False),
                                                    ("swiglu", 96, 176, True, False, 2, False), ("none", 3584, 3584, False, True, 1, False),
                                                    ("swiglu", 256, 3584, False, False, 1, False)], ids=lambda v: str(v))
def test_random_operands_against_float64(dev, ops, act, N, K, bias, res, M, f32):
    """Products are exact in f32, so any summation order of K terms errs by at most K 2^-24 sum|t_k| (t_k = x_k c_k scale).
    f32 output:  |out - ref64| <= K 2^-24 scale sum|x_k c_k| + 2^-23 |ref64|.
    bf16 output: twice the sum term plus 2^-8 |ref64| per bf16 rounding of the epilogue (none: 1, with a residual 2; SwiGLU: gate, up, SiLU, output = 4).
    For that to be a derived bound, the residual here has the sign of the product it is added to (no cancellation: the first rounding's error, relative to the
    product, is then no larger relative to the sum), and the gate pre-activations stay above -5 (asserted), where a relative error of the gate grows by
    |1 + g (1 - sigmoid(g))| < 5 through SiLU: 5 + 1 (up) + 1 (SiLU) + 1 (output) half-ulps = the 4 x 2^-8 the bound allows.
    Measured on an MI355X, rel-L2 against float64 in the order of the cases: 3.9e-8 (f32), 1.7e-3, 3.5e-3, 1.8e-3, 2.7e-3 (bf16: its own rounding); the worst
    error used 0.66 of its bound (0.002 for f32).  The figures are printed.  Run twice, bit-identical."""
    g = torch.Generator().manual_seed(N + K + M)
    w = (torch.randn(N, K, generator=g) * (0.7 / K ** 0.5) * torch.exp2(torch.randint(-3, 1, (N, 1), generator=g).float())).to(BF)
    a = torch.randn(M, K, generator=g).to(BF)
    b = torch.randn(N, generator=g).mul(0.25).to(BF) if bias else None
    codes, scale = quant_ref(w)
    wd = dequant_ref(codes, scale).double()
    prod = a.double() @ wd.t()                                          # [M, N]
    sum_abs = a.double().abs() @ wd.abs().t()                           # scale sum|x_k c_k|
    pre = prod + (b.double()[None, :] if bias else 0)
    sum_term = K * 2.0 ** -24 * sum_abs
    if act == "swiglu":
        blk = pre.view(M, N // 32, 2, 16)
        gate, up = blk[:, :, 0].reshape(M, N // 2), blk[:, :, 1].reshape(M, N // 2)
        assert gate.min().item() > -5
        ref = gate * torch.sigmoid(gate) * up
        sb = sum_term.view(M, N // 32, 2, 16)
        # d(silu(g) up) <= |silu'(g)| |up| dg + |silu(g)| dup, |silu'| <= 1.1
        sum_term = 1.1 * up.abs() * sb[:, :, 0].reshape(M, N // 2) + (gate * torch.sigmoid(gate)).abs() * sb[:, :, 1].reshape(M, N // 2)
        roundings = 4
    else:
        ref, roundings = pre, 1
    r = None
    if res:
        r = (torch.randn(ref.shape, generator=g).abs() * torch.sign(ref).float()).to(BF)
        ref = ref + r.double()
        roundings = 2
    to = lambda t: None if t is None else t.to(dev)
    wq, sw = ops.quant_e4m3_rows_pow2(w.to(dev))
    assert torch.equal(wq.cpu(), codes.view(U8))
    odt = F32 if f32 else BF
    got = ops.gemv_w8(to(a), wq, sw, to(b), to(r), act=act, out_dtype=odt)
    again = ops.gemv_w8(to(a), wq, sw, to(b), to(r), act=act, out_dtype=odt)
    assert torch.equal(got, again)
    err = (got.cpu().double() - ref).abs()
    bound = sum_term + 2.0 ** -23 * ref.abs() if f32 else 2 * sum_term + roundings * 2.0 ** -8 * ref.abs()
    print(f"gemv_w8 {act} N={N} K={K} M={M} {'f32' if f32 else 'bf16'}: rel-L2 vs float64 {(err.norm() / ref.norm()).item():.3e}, "
          f"worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ 5. guard bands
@pytest.mark.parametrize("act,N,K,M,f32", [("none", 70, 176, 3, False), ("swiglu", 96, 176, 4, False), ("none", 1002, 272, 1, True)], ids=lambda v: str(v))
def test_gemv_w8_stays_inside_its_views(dev, ops, act, N, K, M, f32):
    """A, the codes, bias, residual and the output as views inside larger allocations: NaN around the bf16 inputs, e4m3 NaN (0x7F) around the codes, random words
    around the output.  Same bits as the contiguous call, finite, and nothing outside the output view changes."""
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF)
    a = torch.randn(M, K, generator=g).to(BF).to(dev)
    b = torch.randn(N, generator=g).to(BF).to(dev)
    n_out = N // 2 if act == "swiglu" else N
    r = None if f32 else torch.randn(M, n_out, generator=g).to(BF).to(dev)
    wq, sw = ops.quant_e4m3_rows_pow2(w.to(dev))
    odt = F32 if f32 else BF
    want = ops.gemv_w8(a, wq, sw, b, r, act=act, out_dtype=odt)
    av = G.banded(a.shape, K + 8, BF, dev, "in", data=a)[0]
    wv, wback = G.banded(wq.shape, K + 16, U8, dev, "in", data=wq)
    wback.fill_(0x7F)
    wv.copy_(wq)
    bv = G.banded_flat(N, BF, dev, "in", data=b)[0]
    swv = G.banded_flat(N, F32, dev, "in", data=sw)[0]
    rv = None if r is None else G.banded(r.shape, n_out + 8, BF, dev, "in", data=r)[0]
    ov, oback = G.banded((M, n_out), n_out + 8, odt, dev, "out", seed=7)
    snap = G.snapshot(oback)
    ops.gemv_w8(av, wv, swv, bv, rv, act=act, out_dtype=odt, out=ov)
    G.assert_finite_where(ov, want, "gemv_w8")
    assert torch.equal(G.inside(ov), want)
    G.assert_outside_unchanged(oback, ov, snap, "gemv_w8 output")


def test_quantiser_stays_inside_its_views(dev, ops):
    w = edge_matrix(72, 272, seed=4).to(dev)
    wantq, wantsc = ops.quant_e4m3_rows_pow2(w)
    wv = G.banded(w.shape, 272 + 8, BF, dev, "in", data=w)[0]
    qv, qback = G.banded(w.shape, 272 + 16, U8, dev, "out", seed=1)
    sv, sback = G.banded_flat(72, F32, dev, "out", seed=2)
    qsnap, ssnap = G.snapshot(qback), G.snapshot(sback)
    ops.quant_e4m3_rows_pow2(wv, out=(qv, sv))
    assert torch.equal(G.inside(qv), wantq) and torch.equal(sv, wantsc)
    G.assert_outside_unchanged(qback, qv, qsnap, "codes")
    G.assert_outside_unchanged(sback, sv, ssnap, "scales")


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(dev, ops):
    from rga3.hip.lib import Rga3Error

    N, K = 64, 64
    wq = torch.zeros((N, K), dtype=U8, device=dev)
    sw = torch.ones(N, dtype=F32, device=dev)
    a = torch.zeros((4, K), dtype=BF, device=dev)
    ops.gemv_w8(a, wq, sw)                                                       # the accepted form
    with pytest.raises(Rga3Error):                                               # M = 5
        ops.gemv_w8(torch.zeros((5, K), dtype=BF, device=dev), wq, sw)
    with pytest.raises(Rga3Error):                                               # K % 16 != 0
        ops.gemv_w8(torch.zeros((1, 72), dtype=BF, device=dev)[:, :56], torch.zeros((N, 64), dtype=U8, device=dev)[:, :56], sw)
    with pytest.raises(Rga3Error):                                               # a row stride of the codes shorter than a row
        ops.gemv_w8(a, torch.zeros(N * K, dtype=U8, device=dev).as_strided((N, K), (48, 1)), sw)
    with pytest.raises(Rga3Error):                                               # a pointer off its 16 bytes
        ops.gemv_w8(a, torch.zeros(N * K + 16, dtype=U8, device=dev)[8:8 + N * K].view(N, K), sw)
    with pytest.raises(Rga3Error):
        ops.gemv_w8(a, wq, sw, act="gelu")
    with pytest.raises(Rga3Error):                                               # the quantiser's K
        ops.quant_e4m3_rows_pow2(torch.zeros((4, 24), dtype=BF, device=dev))
