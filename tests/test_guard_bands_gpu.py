"""Guard-band tests: every kernel reads and writes only inside the views it is given (tests/guard_bands.py).

The library's contract (include/rga3_hip.h) is plain pointers + sizes + leading dimensions / strides, so that every entry point can work in place on a slice of a
fused buffer.  Each case here places every operand and every output inside a larger poisoned allocation (inputs surrounded by NaN, outputs by seeded random
words) and asserts, with no tolerance of its own:
  1. every bit outside an output (or in/out) view is unchanged;
  2. the result is finite wherever the reference is (NaN padding did not reach it);
  3. the result is bit-identical to the same call -- same explicit tile / impl -- on contiguous, exactly sized copies of the same data;
  4. that contiguous result meets the plain reference and the tolerance the op's existing test states (tests/test_kernels_gpu.py, test_sam2_kernels_gpu.py,
     test_train_gpu.py: the tolerance is quoted next to each check).
Entry points that add with f32 atomics (rga3_colsum_accum, rga3_sumsq_accum, rga3_layernorm_bwd at the atomic widths, rga3_bilinear_bwd with plane_idx) are
outside assertion 3.  Shapes are the smallest at which the edge exists: one ragged tile row and column, one 8-wide K tail, a partial workgroup, n % 8 != 0.
Every view has ld = width + 8; every family also runs at ld = width + 24 (PADS; the e4m3 views, whose strides are multiples of 16 bytes, at + 16 and + 32).  The second half refuses views that cannot hold their rows.

Coverage (entry point of include/rga3_hip.h -> test here; "refuse" = the stride refusal in the test_refuse_* tests):
  rga3_gemm_bf16 ............................. test_gemm_every_tiling_*, _persistent_and_four_wave_*, _wider_pad, _weight_stream_rows, _token_rows, _k_split_tilings,
                                               _ragged_last_tile_row_plan; refuse (ldc, ldr, lda, ldw) + test_gemm_bf16_accepts_the_documented_exemptions
  rga3_gemm_rms_bf16 / _swiglu_pre_bf16 ...... test_gemm_rms_producer_and_consumer / test_gemm_swiglu_pre; refuse
  rga3_layernorm_stats / rga3_gemm_ln_bf16 ... test_layernorm_stats / test_gemm_ln; refuse
  rga3_gemm_lnsum_bf16 / _lnq_bf16 ........... test_gemm_lnsum_and_lnq; refuse          rga3_gemm_cat_bf16 ... test_gemm_cat; refuse (ldc, ldcn)
  rga3_gemm_tn_bf16 / _tn_many / _rows16_many  test_gemm_tn / test_gemm_tn_many / test_gemm_rows16_many; refuse
  rga3_quant_fp8_rows / rga3_gemm_fp8 ........ test_fp8_quant_and_gemm; refuse
  rga3_attn_varlen_fwd / _fwd_rope / _bwd .... test_attn_varlen_fwd / _fwd_rope / _bwd; refuse, test_head_major_layouts_stay_legal
  rga3_attn_fewq / rga3_decimg_rows .......... test_attn_fewq / test_decimg_rows; refuse (both)
  rga3_memattn_cross / rga3_memlayer_rows .... test_memattn_cross_out_and_partials / test_memlayer_rows_three_chains; refuse (both)
  rga3_mlp3_rows / rga3_sam_select_objptr .... test_mlp3_rows_and_sam_select_objptr; refuse (both)
  rga3_rmsnorm_fwd / _bwd, rga3_layernorm_fwd / _bwd ... test_rmsnorm_fwd_with_res_out / test_rmsnorm_bwd / test_layernorm_fwd / test_layernorm_bwd; refuse (fwd)
  rga3_gather_rows / _scatter_rows / _pad_cols test_gather_and_scatter_rows / test_pad_cols; refuse (all three)
  rga3_cross_entropy_rows .................... test_cross_entropy_rows; refuse           rga3_transpose16 / _many ... test_transpose16_and_many; refuse (transpose16)
  rga3_segment_sum_rows / _scatter_add_rows .. test_segment_sum_and_scatter_add_rows; refuse    rga3_colsum ... test_colsum; refuse
  rga3_rope_inplace / rga3_rope_axial_inplace  test_rope_inplace_on_a_head_range / test_rope_axial_inplace_leaves_the_rows_behind_n_rope; refuse
  rga3_silu_mul / _add / _act ................ test_silu_mul_add_and_act_on_a_ragged_length  rga3_swiglu_fwd / _bwd ... test_swiglu_fwd_and_bwd
  rga3_dropout_bf16 / _pair_bf16 ............. test_dropout_and_pair                     rga3_adamw_step / _clip / _clip_rows ... test_adamw_steps
  rga3_sumsq_det, rga3_bce_dice_sums_det / _grad ... test_sumsq_det, test_bce_dice_sums_det_and_grad
  rga3_pixel_shuffle2x / _bwd, rga3_bilinear / _bwd, rga3_mask_product / _bwd ... test_pixel_shuffle2x_and_bwd, test_bilinear_and_bwd, test_mask_product_and_bwd
  rga3_maxpool2x2_win / rga3_add_bcast ....... test_maxpool2x2_win_and_add_bcast; refuse    rga3_im2col ... test_im2col_with_ld_out_and_zero_tail; refuse
  rga3_dwconv7x7 / _conv3x3s2 / _im2col3x3s2 . test_dwconv7x7_conv3x3s2_and_im2col3x3s2
  rga3_colsum_accum / _sumsq_accum / _bilinear_bwd(plane_idx) ... test_entry_points_that_add_with_atomics_stay_inside_their_outputs (atomics: no assertion 3); refuse (colsum_accum)
  rga3_mask_jf_counts, rga3_stom_flow / _shift_composite, rga3_sam_preprocess_u8 / rga3_qwen_patchify_u8 ... the three uint8-pipeline tests (outputs and workspaces)
  rga3_upsample2x_add, rga3_swiglu_{fwd,bwd}_quant_fp8, rga3_hiera_mlp144, rga3_conv3x3s2_ln_gelu, rga3_bce_dice_grad_dev ... test_contiguous_by_contract_entry_points_*
Left out: rga3_hiera_mlp288 (+ _pack), rga3_copy_many, rga3_stom_mask_composite, rga3_bce_dice_sums (the atomic form the wrapper no longer calls): contiguous by
contract, no stride and no ragged vector tail of their own beyond what their existing tests run; the host-only queries (rga3_version, rga3_last_error,
rga3_gemm_tiles, rga3_gemm_ragged_plan, *_ws_floats / *_bytes, rga3_pil_bicubic_coeffs, rga3_qwen_norm_lut, ...) touch no device memory."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import kernels_ref as R
from tests import guard_bands as G

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
EINVAL = -22
PADS = [8, 24]       # every view has ld = width + 8; each family also runs once at ld = width + 24


def _rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _rand(shape, dev, scale=1.0, seed=0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rc(name, *args):
    """The C entry point on data pointers (tensors -> data_ptr(), None -> NULL), current stream appended; returns the code."""
    from rga3.hip import lib

    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    return getattr(lib.load(), name)(*conv, _stream())


def _call(name, *args):
    from rga3.hip import lib

    rc = _rc(name, *args)
    assert rc == 0, (name, rc, lib.last_error())


class Bands:
    """The views of one case: inputs in NaN, outputs in random words, one check for all of them."""

    def __init__(self, dev, pad=8):
        self.dev, self.pad, self.guards, self.seed = dev, pad, [], 1000

    def _ld(self, shape, pad):
        w = 1
        for s in shape[1:]:
            w *= int(s)
        return w + (self.pad if pad is None else pad)

    def inp(self, data, pad=None):
        return G.banded(data.shape, self._ld(data.shape, pad), data.dtype, self.dev, "in", data=data)[0]

    def vec(self, data):
        return G.banded_flat(data.numel(), data.dtype, self.dev, "in", data=data)[0]

    def out(self, shape, dtype=BF, pad=None, data=None, allowed=None):
        self.seed += 1
        v, b = G.banded(shape, self._ld(shape, pad), dtype, self.dev, "out", data=data, seed=self.seed)
        self.guards.append([b, v if allowed is None else allowed(v), None])
        return v

    def flat(self, n, dtype=BF, data=None):
        self.seed += 1
        v, b = G.banded_flat(n, dtype, self.dev, "out", data=data, seed=self.seed)
        self.guards.append([b, v, None])
        return v

    def arm(self):
        torch.cuda.synchronize()
        for g in self.guards:
            g[2] = G.snapshot(g[0])

    def check(self):
        torch.cuda.synchronize()
        for i, (b, v, snap) in enumerate(self.guards):
            G.assert_outside_unchanged(b, v, snap, f"output {i}")


def _same(view, want, ref, what=""):
    """Assertions 2 and 3 for one output."""
    got = G.inside(view)
    want = want.reshape(got.shape)
    G.assert_finite_where(got, ref.reshape(got.shape), what)
    assert torch.equal(got, want), f"{what}: the view and the contiguous call differ in {int((got != want).sum())} element(s)"


# ---------------------------------------------------------------------------------------------------------------- rga3_gemm_bf16

# (tile id, tile rows, tile columns): the rows rga3_gemm_tiles(0) reports (test_tile_table_is_the_librarys pins the copy)
TILES = [(3, 128, 256), (4, 128, 320), (5, 128, 192), (6, 128, 256), (7, 128, 192), (8, 128, 128), (10, 256, 256), (11, 128, 128), (12, 128, 128), (13, 64, 64),
         (14, 64, 64), (20, 256, 256), (21, 256, 256), (22, 256, 256), (23, 256, 192), (25, 256, 256), (26, 256, 256), (27, 256, 256), (28, 256, 256), (31, 192, 256),
         (32, 192, 256), (40, 4, 16), (41, 16, 16)]
SWIGLU_BN = {4: 256, 5: 256, 7: 256}          # the width these run under SwiGLU (kTiles' swiglu_bn)
FORMS = ["none", "gelu", "relu", "swiglu", "f32", "colscale"]


def test_tile_table_is_the_librarys(dev):
    from rga3.hip import lib

    ids, bm, bn = ((C.c_int * 64)() for _ in range(3))
    n = lib.load().rga3_gemm_tiles(0, ids, bm, bn, 64)
    assert [(ids[i], bm[i], bn[i]) for i in range(n)] == TILES


def _gemm_case(dev, tile, M, N, K, form, pad=8, out_pad=None, plain=False, ref_on_device=False):
    """form: none / gelu / relu / swiglu = bias + residual + that activation (tolerance 8e-3: test_gemm_epilogues); f32 = f32 output, bias only (1e-3:
    test_gemm_f32_output_on_the_round5_tilings); colscale = residual + colscale * (a w^T + bias) (8e-3: test_gemm_ktail_and_colscale); plain = no epilogue at all
    (6e-3: test_gemm_plain)."""
    from rga3.hip import ops

    act = form if form in ("gelu", "relu", "swiglu") else "none"
    n_out = N // 2 if act == "swiglu" else N
    odt = F32 if form == "f32" else BF
    a, w = _rand((M, K), dev, seed=1), _rand((N, K), dev, 0.08, seed=2)
    b = None if plain else _rand((N,), dev, 0.5, seed=3)
    r = None if (plain or form == "f32") else _rand((M, n_out), dev, seed=4)
    cs = _rand((n_out,), dev, 0.2, seed=5) if form == "colscale" else None
    want = ops.gemm(a, w, bias=b, residual=r, act=act, out_dtype=odt, tile=tile, colscale=cs)
    B = Bands(dev, pad)
    av, wv = B.inp(a), B.inp(w)
    bv = B.vec(b) if b is not None else None
    rv = B.inp(r) if r is not None else None
    csv = B.vec(cs) if cs is not None else None
    out = B.out((M, n_out), odt, pad=out_pad)
    B.arm()
    ops.gemm(av, wv, bias=bv, residual=rv, act=act, out_dtype=odt, out=out, tile=tile, colscale=csv)
    B.check()
    if ref_on_device:
        ref = R.linear_ref(a, w)
    else:
        ref = R.linear_ref(a.cpu(), w.cpu(), None if b is None else b.cpu(), None, act)
        if cs is not None:
            ref = ref * cs.float().cpu()
        if r is not None:
            ref = ref + r.float().cpu()
    _same(out, want, ref, f"tile {tile} {form}")
    assert _rel_l2(want, ref) < (6e-3 if plain else 1e-3 if form == "f32" else 8e-3), (tile, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tile,bm,bn", [t for t in TILES if t[0] not in (40, 41)])
def test_gemm_every_tiling_ragged_tile_row_column_and_k_tail(dev, tile, bm, bn, form):
    """M = bm + 3, N = bn + 8 (bf16) / bn + 4 (f32) / a multiple of 32 with one ragged 32-block (SwiGLU), K = 72: one ragged tile row, one ragged tile column, one
    8-wide K tail; A, W, residual and C are views, bias and colscale slices of NaN-poisoned vectors."""
    N = bn + 4 if form == "f32" else SWIGLU_BN.get(tile, bn) + 32 if form == "swiglu" else bn + 8
    _gemm_case(dev, tile, bm + 3, N, 72, form)


@pytest.mark.parametrize("tile,bm,bn", [t for t in TILES if t[0] in (21, 22, 26, 27, 28, 31, 32)])
def test_gemm_persistent_and_four_wave_tilings_on_whole_k_tiles(dev, tile, bm, bn):
    """K = 128: the persistent kernels (21 / 22 / 26 / 27 / 31 / 32) and the four-wave kernel (28) run as tile 20 unless K is a multiple of 64."""
    _gemm_case(dev, tile, bm + 3, bn + 8, 128, "gelu")


@pytest.mark.parametrize("tile,bm,bn", [(12, 128, 128), (20, 256, 256)])
def test_gemm_wider_pad(dev, tile, bm, bn):
    _gemm_case(dev, tile, bm + 3, bn + 8, 72, "none", pad=24)


@pytest.mark.parametrize("form", ["none", "gelu", "relu", "swiglu", "f32"])
def test_gemm_weight_stream_rows(dev, form):
    """Tile 40 (M <= 4): M = 3, one ragged 16-column block (SwiGLU: two gate | up blocks of 32)."""
    _gemm_case(dev, 40, 3, {"swiglu": 64, "f32": 16 + 4}.get(form, 16 + 8), 72, form)


@pytest.mark.parametrize("form", ["none", "gelu", "relu"])
def test_gemm_token_rows(dev, form):
    """Tile 41 (M <= 16): M = 13, N = 250 (a last 16-column block of 10), ldc = 256."""
    _gemm_case(dev, 41, 13, 250, 72, form, out_pad=6)


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize("tile,M,N,K,form", [
    (14, 67, 72, 264, "plain"),        # 4 tiles of 64 x 64, nk = 5: S = min(1024 / 4, nk / 2, 32) = 2 slices (launch_split64; plain products only)
    (25, 259, 264, 512, "f32"),        # 4 tiles, nk = 8: S = min(CUs / 4, nk / 4) = 2 slices (launch_splitk; bias allowed, f32 output)
    (22, 259, 264, 1024, "plain"),     # 4 tiles < one round: all four in the stream-K tail, nk = 16: two runs of MIN_SEG = 8 K-tiles per tile (launch_sk)
    (32, 195, 264, 1024, "plain"),     # the same on 192-row tiles
])
def test_gemm_k_split_tilings(dev, tile, M, N, K, form):
    """The K-split / stream-K tilings at the smallest shapes at which the split is still taken (conditions of the launchers quoted above); they fall back to an
    unsplit kernel below these.  That the split IS taken is asserted: the slab area of the workspace is cleared before and holds partial sums afterwards.
    Reproducible, so the view and the contiguous call give the same bits.  The library workspace is not guarded."""
    from rga3.hip import ops

    ws = ops.gemm_workspace(dev)
    ws[4096:].zero_()                      # the partial-sum slabs behind the 4-KiB flag page: scratch that only a K split writes
    _gemm_case(dev, tile, M, N, K, "none" if form == "plain" else form, plain=form == "plain")
    assert bool(ws[4096:].any()), f"tile {tile} left the slabs untouched at {(M, N, K)}: the product no longer takes the K split"
    assert ops.gemm_stream_k_timeouts() == 0


@pytest.mark.parametrize("tile,K", [(27, 128), (26, 1024)])
def test_gemm_ragged_last_tile_row_plan(dev, tile, K):
    """Tiles 27 / 26 take their ragged-row plan only from one full round of tiles on (T >= CUs): M = 259 (a last tile row of 3 rows), N = 127 x 256 + 8; for 26 the
    tail must be split (more runs than tiles).  rga3_gemm_ragged_plan says whether the plan applies on this device."""
    from rga3.hip import lib, ops

    M, N = 259, 127 * 256 + 8
    plan, start = (C.c_int * 8)(), (C.c_uint * 2049)()
    assert lib.load().rga3_gemm_ragged_plan(M, N, K, _cus(dev), int(tile == 26), plan, start) == 0, "no ragged plan on this device: the shape no longer reaches the kernel"
    if tile == 26:
        assert plan[1] > 0 and plan[6] > plan[1], list(plan)
    _gemm_case(dev, tile, M, N, K, "none", plain=True, ref_on_device=True)
    assert ops.gemm_stream_k_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------------- the other NT entry points

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("tile", [12, 20])
def test_gemm_rms_producer_and_consumer(dev, tile, pad):
    """rga3_gemm_rms_bf16 (test_gemm_rmsnorm_folded: sums 1e-5, consumer 1e-2): the producer's row_sumsq_out is a slice of a longer int64 buffer."""
    from rga3.hip import ops

    M, N, K, N2, eps = 131, 136, 72, 72, 1e-6
    a, wo, r = _rand((M, K), dev, seed=1), _rand((N, K), dev, 0.05, seed=2), _rand((M, N), dev, seed=3)
    sums_c = torch.zeros(M, dtype=torch.int64, device=dev)
    x2_c = ops.gemm(a, wo, residual=r, tile=tile, rms_out=sums_c)
    B = Bands(dev, pad)
    x2 = B.out((M, N))
    sums = B.flat(M, torch.int64, data=torch.zeros(M, dtype=torch.int64))
    av, wv, rv = B.inp(a), B.inp(wo), B.inp(r)
    B.arm()
    ops.gemm(av, wv, residual=rv, out=x2, tile=tile, rms_out=sums)
    B.check()
    ref = R.linear_ref(a.cpu(), wo.cpu(), None, r.cpu())
    _same(x2, x2_c, ref, "producer")
    assert torch.equal(sums, sums_c)
    ss = (x2_c.double() ** 2).sum(1)
    assert ((sums_c.double() / 2 ** 20 - ss).abs() / ss).max().item() < 1e-5
    # consumer
    gamma = (1.0 + 0.3 * torch.randn(N, generator=torch.Generator().manual_seed(4))).to(BF).to(dev)
    w2, b2 = _rand((N2, N), dev, 0.05, seed=5), _rand((N2,), dev, seed=6)
    wf = (w2.float() * gamma.float()[None, :]).to(BF).contiguous()
    y_c = ops.gemm(x2_c, wf, b2, tile=tile, rms_in=(sums_c, N, eps))
    B = Bands(dev, pad)
    y = B.out((M, N2))
    xv, wfv, b2v = B.inp(x2_c), B.inp(wf), B.vec(b2)
    sums_in = G.banded_flat(M, torch.int64, dev, "in", data=sums_c)[0]
    B.arm()
    ops.gemm(xv, wfv, b2v, out=y, tile=tile, rms_in=(sums_in, N, eps))
    B.check()
    xf = x2_c.float()
    xn = ((xf * torch.rsqrt((xf ** 2).mean(-1, keepdim=True) + eps)).to(BF).float() * gamma.float()).to(BF).float()
    ref = (xn @ w2.float().t() + b2.float()).cpu()
    _same(y, y_c, ref, "consumer")
    assert _rel_l2(y_c, ref) < 1e-2


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("tile", [12, 21])
def test_gemm_swiglu_pre(dev, tile, pad):
    """rga3_gemm_swiglu_pre_bf16 (test_gemm_swiglu_with_preactivations): C and pre are views (ldpre = N + 8)."""
    from rga3.hip import ops

    M, N, K = 131, 160, 72
    a, w, b = _rand((M, K), dev, seed=1), _rand((N, K), dev, 0.05, seed=2), _rand((N,), dev, 0.3, seed=3)
    act_c, pre_c = ops.gemm_swiglu_pre(a, w, b, tile=tile)
    B = Bands(dev, pad)
    av, wv, bv = B.inp(a), B.inp(w), B.vec(b)
    out, pre = B.out((M, N // 2)), B.out((M, N))
    ws = ops.gemm_workspace(dev)
    B.arm()
    _call("rga3_gemm_swiglu_pre_bf16", av, wv, bv, out, pre, M, N, K, av.stride(0), wv.stride(0), out.stride(0), pre.stride(0), tile, ws, ws.numel())
    B.check()
    _same(pre, pre_c, R.linear_ref(a.cpu(), w.cpu(), b.cpu()), "pre")
    _same(out, act_c, R.linear_ref(a.cpu(), w.cpu(), b.cpu(), None, "swiglu"), "act")
    assert torch.equal(pre_c, ops.gemm(a, w, b, tile=tile))
    ref = ops.swiglu_fwd(pre_c)
    assert _rel_l2(act_c, ref) < 2e-3 and float((act_c.float() - ref.float()).abs().max()) < 0.05


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("dim", [72, 264, 576, 1152, 2304])
def test_layernorm_stats(dev, dim, pad):
    """rga3_layernorm_stats on every kernel of its dispatch (test_gemm_layernorm_folded: allclose 1e-5); stats is a slice of a longer f32 buffer."""
    from rga3.hip import ops

    rows = 37
    x = _rand((rows, dim), dev, 0.7, seed=dim) + 0.5
    st_c = ops.layernorm_stats(x, 1e-6)
    B = Bands(dev, pad)
    xv, st = B.inp(x), B.flat(rows * 2, F32)
    B.arm()
    _call("rga3_layernorm_stats", xv, st, rows, dim, xv.stride(0), 1e-6)
    B.check()
    xf = x.float().cpu()
    ref = torch.stack([xf.mean(1), torch.rsqrt(xf.var(1, unbiased=False) + 1e-6)], 1)
    _same(st, st_c, ref)
    assert torch.allclose(st_c[:, 0].cpu(), ref[:, 0], atol=1e-5, rtol=1e-5) and torch.allclose(st_c[:, 1].cpu(), ref[:, 1], atol=1e-5, rtol=2e-5)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("tile,act", [(12, "gelu"), (20, "none"), (13, "relu")])
def test_gemm_ln(dev, tile, act, pad):
    """rga3_gemm_ln_bf16 (test_gemm_layernorm_folded: 8e-3): colc and the row statistics are slices of NaN-poisoned f32 vectors."""
    from rga3.hip import ops

    bm, bn = {12: (128, 128), 20: (256, 256), 13: (64, 64)}[tile]
    M, N, K = bm + 3, bn + 12, 72
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 0.7 + torch.randn(M, 1, generator=g) * 1.5).to(BF).to(dev)
    w, b = (torch.randn(N, K, generator=g) * 0.05).to(BF).to(dev), (torch.randn(N, generator=g) * 0.2).to(BF).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(K, generator=g)).to(BF).to(dev), (0.1 * torch.randn(K, generator=g)).to(BF).to(dev)
    st = ops.layernorm_stats(x, 1e-6)
    wf, colc, bf = ops.fold_layernorm(w, b, gamma, beta)
    want = ops.gemm_ln(x, st, wf, colc, bf, act=act, tile=tile)
    B = Bands(dev, pad)
    xv, wfv, bfv, colcv, stv = B.inp(x), B.inp(wf), B.vec(bf), B.vec(colc), B.vec(st)
    out = B.out((M, N))
    B.arm()
    _call("rga3_gemm_ln_bf16", xv, wfv, bfv, colcv, stv, out, M, N, K, xv.stride(0), wfv.stride(0), out.stride(0), {"none": 0, "gelu": 1, "relu": 3}[act], tile)
    B.check()
    ref = F.layer_norm(x.float().cpu(), (K,), gamma.float().cpu(), beta.float().cpu(), 1e-6) @ w.float().cpu().t() + b.float().cpu()
    ref = F.gelu(ref) if act == "gelu" else (F.relu(ref) if act == "relu" else ref)
    _same(out, want, ref)
    assert _rel_l2(want, ref) < 8e-3


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("tile", [12, 23])
def test_gemm_lnsum_and_lnq(dev, tile, pad):
    """rga3_gemm_lnsum_bf16 + rga3_gemm_lnq_bf16 (test_layernorm_sums_out_of_the_producer_epilogue: product == plain kernel, sums 2e-5, consumer 8e-3): row_parts is a
    slice of a longer f32 buffer on the way out and a NaN-guarded one on the way in."""
    from rga3.hip import lib, ops

    bm, bn = {12: (128, 128), 23: (256, 192)}[tile]
    M, N, K = bm + 3, bn + 8, 72
    g = torch.Generator().manual_seed(M + N + K)
    a, w = torch.randn(M, K, generator=g).to(BF).to(dev), (torch.randn(N, K, generator=g) * (K ** -0.5)).to(BF).to(dev)
    b = (torch.randn(N, generator=g) * 0.2).to(BF).to(dev)
    res = (torch.randn(M, N, generator=g) * 0.7 + torch.randn(M, 1, generator=g) * 3.0).to(BF).to(dev)
    out_c, parts_c = ops.gemm_lnsum(a, w, b, residual=res, tile=tile)
    ns = int(lib.load().rga3_gemm_lnsum_slices(N, tile))
    assert ns == 2 and tuple(parts_c.shape) == (M, ns, 2)
    B = Bands(dev, pad)
    av, wv, bv, rv = B.inp(a), B.inp(w), B.vec(b), B.inp(res)
    out, parts = B.out((M, N)), B.flat(M * ns * 2, F32)
    B.arm()
    _call("rga3_gemm_lnsum_bf16", av, wv, bv, rv, out, M, N, K, av.stride(0), wv.stride(0), out.stride(0), rv.stride(0), tile, parts)
    B.check()
    ref = R.linear_ref(a.cpu(), w.cpu(), b.cpu(), res.cpu())
    _same(out, out_c, ref, "product")
    of = out_c.double().cpu()
    sums_ref = torch.stack([of.sum(1), (of * of).sum(1)], 1)
    _same(parts.view(M, ns, 2).sum(1), parts_c.sum(1), sums_ref, "partial sums")
    assert torch.equal(parts.view(M, ns, 2), parts_c)
    assert torch.equal(out_c, ops.gemm(a, w, b, residual=res, tile=tile))
    s1, s2 = parts_c[:, :, 0].double().sum(1).cpu(), parts_c[:, :, 1].double().sum(1).cpu()
    assert float((s1 - of.sum(1)).abs().max()) <= 2e-5 * float(of.abs().sum(1).max())
    assert float((s2 - (of * of).sum(1)).abs().max()) <= 2e-5 * float((of * of).sum(1).max())
    # consumer on the sums
    N2 = 72
    w2, b2 = (torch.randn(N2, N, generator=g) * 0.05).to(BF).to(dev), (torch.randn(N2, generator=g) * 0.2).to(BF).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(N, generator=g)).to(BF).to(dev), (0.1 * torch.randn(N, generator=g)).to(BF).to(dev)
    wf, colc, bf = ops.fold_layernorm(w2, b2, gamma, beta)
    y_c = ops.gemm_ln(out_c, ops.LnSums(parts_c, 1e-6), wf, colc, bf, act="gelu", tile=12)
    B = Bands(dev, pad)
    xv, wfv, bfv, colcv, pv = B.inp(out_c), B.inp(wf), B.vec(bf), B.vec(colc), B.vec(parts_c)
    y = B.out((M, N2))
    B.arm()
    _call("rga3_gemm_lnq_bf16", xv, wfv, bfv, colcv, pv, ns, N, 1e-6, y, M, N2, N, xv.stride(0), wfv.stride(0), y.stride(0), 1, 12)
    B.check()
    ref = F.gelu(F.layer_norm(out_c.float().cpu(), (N,), gamma.float().cpu(), beta.float().cpu(), 1e-6) @ w2.float().cpu().t() + b2.float().cpu())
    _same(y, y_c, ref, "consumer")
    assert _rel_l2(y_c, ref) < 8e-3


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("sides", ["k", "n", "both"])
def test_gemm_cat(dev, sides, pad):
    """rga3_gemm_cat_bf16 with a K side, an N side, and both (test_gemm_concatenated_operands: 6e-3, Cn == plain product): C and Cn are views."""
    from rga3.hip import ops

    tile, M, K, K2, N2 = 12, 131, 64, 64, 72
    N = 136 if sides == "k" else 128            # with an N side N is a multiple of the tile width
    a, w, b = _rand((M, K), dev, seed=1), _rand((N, K), dev, 0.05, seed=2), _rand((N,), dev, 0.3, seed=3)
    a2, w2 = (_rand((M, K2), dev, 0.3, seed=4), _rand((N, K2), dev, 0.05, seed=5)) if sides != "n" else (None, None)
    wn = _rand((N2, K), dev, 0.05, seed=6) if sides != "k" else None
    res_c = ops.gemm_cat(a, w, b, a2=a2, w2=w2, wn=wn, tile=tile)
    c_c, cn_c = res_c if wn is not None else (res_c, None)
    B = Bands(dev, pad)
    av, wv, bv = B.inp(a), B.inp(w), B.vec(b)
    a2v, w2v = (B.inp(a2), B.inp(w2)) if a2 is not None else (None, None)
    wnv = B.inp(wn) if wn is not None else None
    c = B.out((M, N))
    cn = B.out((M, N2)) if wn is not None else None
    B.arm()
    _call("rga3_gemm_cat_bf16", av, wv, bv, c, M, N, K, av.stride(0), wv.stride(0), c.stride(0), a2v, w2v, K2 if a2 is not None else 0,
          a2v.stride(0) if a2 is not None else 0, w2v.stride(0) if a2 is not None else 0, wnv, cn, N2 if wn is not None else 0,
          wnv.stride(0) if wn is not None else 0, cn.stride(0) if wn is not None else 0, tile)
    B.check()
    ref = R.linear_ref(a.cpu(), w.cpu(), b.cpu())
    if a2 is not None:
        ref = ref + a2.float().cpu() @ w2.float().cpu().t()
    _same(c, c_c, ref, "C")
    assert _rel_l2(c_c, ref) < 6e-3
    if wn is not None:
        refn = R.linear_ref(a.cpu(), wn.cpu())
        _same(cn, cn_c, refn, "Cn")
        assert _rel_l2(cn_c, refn) < 6e-3 and torch.equal(cn_c, ops.gemm(a, wn, tile=tile))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("form,K,f32", [("plain", 77, False), ("plain", 77, True), ("workspace", 1024, False), ("counters", 1024, True)])
def test_gemm_tn(dev, form, K, f32, pad):
    """rga3_gemm_tn_bf16 plain, with workspace (K = 1024: nk = 32 K-tiles -> 4 slices) and with counters (test_gemm_tn_weight_gradient_product: 6e-3 / 2e-5 and the
    max-abs bound; test_in_launch_reductions_equal_two_launch_forms)."""
    from rga3.hip import ops

    M, N = 136, 72
    odt = F32 if f32 else BF
    a, b = _rand((K, M), dev, seed=K), _rand((K, N), dev, seed=K + 1)
    want = ops.gemm_tn(a, b, out_dtype=odt, fused_sum=form == "counters")
    B = Bands(dev, pad)
    av, bv = B.inp(a), B.inp(b)
    out = B.out((M, N), odt)
    B.arm()
    ops.gemm_tn(av, bv, out_dtype=odt, out=out, fused_sum=form == "counters")
    B.check()
    ref = a.float().cpu().T @ b.float().cpu()
    _same(out, want, ref)
    assert _rel_l2(want, ref) < (2e-5 if f32 else 6e-3)
    assert float((want.float().cpu() - ref).abs().max()) <= (1e-3 if f32 else 2.0 ** -7) * float(ref.abs().max()) + 1e-4
    if form == "counters":
        assert torch.equal(want, ops.gemm_tn(a, b, out_dtype=odt))


@pytest.mark.parametrize("pad", PADS)
def test_gemm_tn_many(dev, pad):
    """rga3_gemm_tn_many (test_gemm_tn_many_equals_single_products: bit-identical to the single form, 6e-3): every A, B and C a view."""
    from rga3.hip import lib, ops

    shapes = [(1024, 136, 72), (300, 8, 264)]
    pairs = [(_rand((K, M), dev, seed=K), _rand((K, N), dev, seed=K + 1)) for K, M, N in shapes]
    want = ops.gemm_tn_many(pairs)
    B = Bands(dev, pad)
    views = [(B.inp(a), B.inp(b)) for a, b in pairs]
    outs = [B.out((M, N)) for _, M, N in shapes]
    n = len(shapes)
    ptrs, dims, need = (C.c_void_p * (3 * n))(), (C.c_int64 * (7 * n))(), 0
    for i, ((K, M, N), (a, b), o) in enumerate(zip(shapes, views, outs)):
        need += lib.gemm_tn_slices(M, N, K) * M * N
        ptrs[3 * i], ptrs[3 * i + 1], ptrs[3 * i + 2] = a.data_ptr(), b.data_ptr(), o.data_ptr()
        for j, v in enumerate((M, N, K, a.stride(0), b.stride(0), o.stride(0), 0)):
            dims[7 * i + j] = v
    ws = torch.empty(need, dtype=F32, device=dev)
    B.arm()
    _call("rga3_gemm_tn_many", C.cast(ptrs, C.c_void_p), C.cast(dims, C.c_void_p), n, ws, ws.numel() * 4)
    B.check()
    for (a, b), o, wnt in zip(pairs, outs, want):
        ref = a.float().cpu().T @ b.float().cpu()
        _same(o, wnt, ref)
        assert torch.equal(wnt, ops.gemm_tn(a, b)) and _rel_l2(wnt, ref) < 6e-3


@pytest.mark.parametrize("pad", PADS)
def test_gemm_rows16_many(dev, pad):
    """rga3_gemm_rows16_many (test_gemm_token_rows_grouped_with_operand_sum: == tile 41 on the pre-added operand; test_gemm_token_rows: 8e-3)."""
    from rga3.hip import ops

    a, pe, w1, b1, res = _rand((9, 72), dev, seed=1), _rand((9, 72), dev, 0.5, seed=2), _rand((250, 72), dev, 0.05, seed=4), _rand((250,), dev, 0.5, seed=5), _rand((9, 250), dev, seed=9)
    a5, w3 = _rand((5, 136), dev, seed=3), _rand((24, 136), dev, 0.05, seed=8)
    want = ops.gemm_rows16_many([(a, pe, w1, b1, res, "gelu"), (a5, None, w3, None, None, "none")])
    B = Bands(dev, pad)
    av, pev, w1v, b1v, resv, a5v, w3v = B.inp(a), B.inp(pe), B.inp(w1), B.vec(b1), B.inp(res), B.inp(a5), B.inp(w3)
    o1, o2 = B.out((9, 250), pad=6), B.out((5, 24))
    ptrs, dims = (C.c_void_p * 12)(), (C.c_int64 * 18)()
    for j, t in enumerate((av, pev, w1v, b1v, resv, o1, a5v, None, w3v, None, None, o2)):
        ptrs[j] = None if t is None else t.data_ptr()
    for j, v in enumerate((9, 250, 72, 1, av.stride(0), pev.stride(0), w1v.stride(0), o1.stride(0), resv.stride(0),
                           5, 24, 136, 0, a5v.stride(0), 0, w3v.stride(0), o2.stride(0), 0)):
        dims[j] = v
    B.arm()
    _call("rga3_gemm_rows16_many", C.cast(ptrs, C.c_void_p), C.cast(dims, C.c_void_p), 2)
    B.check()
    apre = ops.add(a, pe)
    ref1 = R.linear_ref(apre.cpu(), w1.cpu(), b1.cpu(), res.cpu(), "gelu")
    _same(o1, want[0], ref1)
    _same(o2, want[1], R.linear_ref(a5.cpu(), w3.cpu()))
    assert torch.equal(want[0], ops.gemm(apre, w1, b1, residual=res, act="gelu", tile=41)) and torch.equal(want[1], ops.gemm(a5, w3, tile=41))
    assert _rel_l2(want[0], ref1) < 8e-3


@pytest.mark.parametrize("pad,pad8", [(8, 16), (24, 32)])
def test_fp8_quant_and_gemm(dev, pad, pad8):
    """rga3_quant_fp8_rows + rga3_gemm_fp8 (test_fp8_quant_and_gemm: codes and scales exact, 4e-3): ldx / ldq / lda / ldw / ldc / ldr views; ldq, lda and ldw are in
    bytes and must be multiples of 16, so the e4m3 views run at K + 16 and K + 32 where the bf16 views run at + 8 and + 24; 8-bit operands carry no poison."""
    from rga3.hip import ops

    M, N, K = 259, 264, 128
    a, w = _rand((M, K), dev, seed=21), _rand((N, K), dev, 0.05, seed=22)
    a[3, :] = 0
    a[5, 7] = 40.0
    qa_c, sa_c = ops.quant_fp8_rows(a)
    qw_c, sw_c = ops.quant_fp8_rows(w)
    B = Bands(dev, pad)
    av = B.inp(a)
    qa, sa = B.out((M, K), torch.uint8, pad=pad8), B.flat(M, F32)
    B.arm()
    _call("rga3_quant_fp8_rows", av, qa, sa, M, K, av.stride(0), qa.stride(0))
    B.check()
    ra, rsa = R.quant_fp8_rows_ref(a.cpu())
    assert torch.equal(G.inside(qa), qa_c) and torch.equal(sa, sa_c) and torch.equal(sa_c.cpu(), rsa)
    assert torch.equal(qa_c.cpu().view(torch.float8_e4m3fn).float(), ra.float())
    bias, res = _rand((N,), dev, 0.5, seed=23), _rand((M, N), dev, seed=24)
    want = ops.gemm_fp8(qa_c, sa_c, qw_c, sw_c, bias=bias, residual=res)
    B = Bands(dev, pad)
    qav, qwv = B.inp(qa_c, pad=pad8), B.inp(qw_c, pad=pad8)
    sav, swv, bv, rv = B.vec(sa_c), B.vec(sw_c), B.vec(bias), B.inp(res)
    out = B.out((M, N))
    B.arm()
    _call("rga3_gemm_fp8", qav, qwv, sav, swv, bv, rv, out, M, N, K, qav.stride(0), qwv.stride(0), out.stride(0), rv.stride(0))
    B.check()
    rw, rsw = R.quant_fp8_rows_ref(w.cpu())
    ref = R.gemm_fp8_ref(ra, rsa, rw, rsw, bias.cpu(), res.cpu())
    _same(out, want, ref)
    assert _rel_l2(want, ref) < 4e-3


# ---------------------------------------------------------------------------------------------------------------- attention

def _cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


def _attn_fwd(q, k, v, o, lse, cu_q, cu_k, max_q, scale, causal, impl, split_ws, max_k, block):
    Tq, Hq, D = q.shape
    _call("rga3_attn_varlen_fwd", q, k, v, o, lse, cu_q, cu_k, cu_q.numel() - 1, max_q, Tq, Hq, k.shape[1], D, q.stride(0), q.stride(1), k.stride(0), k.stride(1),
          v.stride(0), v.stride(1), o.stride(0), o.stride(1), float(scale), int(causal), impl, split_ws, split_ws.numel() if split_ws is not None else 0, max_k,
          block[0], block[1])


# (query segments, key segments or None = the same, Hq, Hkv, D, causal, block): the smallest case of each kernel path of ATTN_CASES / CAUSAL32_CASES /
# test_attn_window_kernel / test_attention_block_diagonal_packing
ATTN_GUARD_CASES = [
    ([130], [64], 2, 1, 32, False, None),                   # a single key tile, D = 32 (padded to 64), GQA
    ([5], [133], 2, 2, 64, True, None),                     # causal with Lk > Lq
    ([64, 17, 40], None, 4, 2, 64, False, None),            # windows (max_k <= 256: whole segment in LDS), ragged
    ([257], None, 2, 2, 128, True, None),                   # D = 128 causal from 256 rows on: the paired-block kernel; the last block a single row
    ([9], [4096], 8, 8, 16, False, None),                   # few queries over a long key range: the key split + merge pass
    ([64] * 8, [256] * 8, 8, 8, 72, False, (4, 16)),        # 128 windows of 4 queries x 16 keys, packed sixteen to a segment, block-diagonal visibility
]


@pytest.mark.parametrize("case,impl,pad", [(c, i, 8) for c in ATTN_GUARD_CASES for i in ((0, 1) if c[6] is None else (0,))] +      # impl 1: as test_attn_varlen runs it
                         [(ATTN_GUARD_CASES[2], 0, 24), (ATTN_GUARD_CASES[3], 0, 24)])
def test_attn_varlen_fwd(dev, case, impl, pad):
    """rga3_attn_varlen_fwd (test_attn_varlen: 1e-2, lse 2e-2; block-diagonal: test_attn_window_kernel 8e-3): q, k, v are head slices of one fused buffer that is itself
    a banded view (token stride = all heads x D + 8), o a view with token stride Hq D + 8, lse a slice of a longer f32 buffer."""
    lq, lk, Hq, Hkv, D, causal, block = case
    same = lk is None
    lk = lk or lq
    cu_q, cu_k = _cu(lq), _cu(lk)
    Tq, Tk = int(cu_q[-1]), int(cu_k[-1])
    scale = D ** -0.5
    qd = _rand((Tq, Hq, D), dev, seed=11)
    kvd = _rand((Tk, 2 * Hkv, D), dev, seed=12)
    B = Bands(dev, pad)
    if same:
        fused = B.inp(torch.cat([qd, kvd], 1))
        q, k, v = fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:]
    else:
        q, fused = B.inp(qd), B.inp(kvd)
        k, v = fused[:, :Hkv], fused[:, Hkv:]
    kc, vc = kvd[:, :Hkv].contiguous(), kvd[:, Hkv:].contiguous()
    cq, ck = cu_q.to(dev), cu_k.to(dev)
    split = (lambda: torch.empty(8 * Tq * Hq * (D + 1), dtype=F32, device=dev)) if (max(lk) >= 1024 and not causal) else (lambda: None)
    bl = block or (0, 0)
    o_c, lse_c = torch.empty((Tq, Hq, D), dtype=BF, device=dev), torch.empty((Hq, Tq), dtype=F32, device=dev)
    _attn_fwd(qd, kc, vc, o_c, lse_c, cq, ck, max(lq), scale, causal, impl, split(), max(lk), bl)
    o, lse = B.out((Tq, Hq, D)), B.flat(Hq * Tq, F32)
    B.arm()
    _attn_fwd(q, k, v, o, lse, cq, ck, max(lq), scale, causal, impl, split(), max(lk), bl)
    B.check()
    if block is None:
        ref, lse_ref = R.attn_varlen_ref(qd.cpu(), kc.cpu(), vc.cpu(), cu_q, cu_k, scale, causal)
    else:
        nb = Tq // block[0]
        ref, lse_ref = R.attn_varlen_ref(qd.cpu(), kc.cpu(), vc.cpu(), torch.arange(0, (nb + 1) * block[0], block[0], dtype=torch.int32),
                                         torch.arange(0, (nb + 1) * block[1], block[1], dtype=torch.int32), scale, False)
    _same(o, o_c, ref, "o")
    _same(lse, lse_c, lse_ref, "lse")
    assert _rel_l2(o_c, ref) < (8e-3 if block else 1e-2)
    assert (lse_c.cpu() - lse_ref).abs().max().item() < 2e-2


@pytest.mark.parametrize("pad", PADS)
def test_attn_varlen_fwd_rope(dev, pad):
    """rga3_attn_varlen_fwd_rope at ([64, 17, 40], 4, 2, 64) (test_attn_rope_windows_fused: 1e-2 against rotate-half + exact softmax)."""
    lens, Hq, Hkv, D = [64, 17, 40], 4, 2, 64
    cu = _cu(lens)
    T = int(cu[-1])
    qkv = _rand((T, Hq + 2 * Hkv, D), dev, seed=21)
    pos = torch.cat([torch.arange(n) for n in lens]).float()
    fr = pos[:, None] * (1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D)))[None]
    emb = torch.cat([fr, fr], -1)
    cos, sin = emb.cos().contiguous().to(dev), emb.sin().contiguous().to(dev)
    cud = cu.to(dev)

    def run(q, k, v, o, lse):
        _call("rga3_attn_varlen_fwd_rope", q, k, v, o, lse, cud, cud, len(lens), max(lens), T, Hq, Hkv, D, q.stride(0), q.stride(1), k.stride(0), k.stride(1),
              v.stride(0), v.stride(1), o.stride(0), o.stride(1), D ** -0.5, 0, cos, sin, cos, sin)

    qc, kc, vc = (t.contiguous() for t in (qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]))
    o_c, lse_c = torch.empty((T, Hq, D), dtype=BF, device=dev), torch.empty((Hq, T), dtype=F32, device=dev)
    run(qc, kc, vc, o_c, lse_c)
    B = Bands(dev, pad)
    fused = B.inp(qkv)
    o, lse = B.out((T, Hq, D)), B.flat(Hq * T, F32)
    B.arm()
    run(fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], o, lse)
    B.check()
    qf = qkv.float().cpu()
    rot = lambda x: torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    c, s_ = emb.cos()[:, None], emb.sin()[:, None]
    qr = (qf[:, :Hq] * c + rot(qf[:, :Hq]) * s_).to(BF).float()
    kr = (qf[:, Hq:Hq + Hkv] * c + rot(qf[:, Hq:Hq + Hkv]) * s_).to(BF).float()
    ref, lse_ref = R.attn_varlen_ref(qr, kr, qf[:, Hq + Hkv:], cu, cu, D ** -0.5, False)
    _same(o, o_c, ref, "o")
    _same(lse, lse_c, lse_ref, "lse")
    assert _rel_l2(o_c, ref) < 1e-2


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("Hq,Hkv,D,with_ws", [(2, 2, 64, False), (4, 2, 128, True), (4, 2, 128, False)])
def test_attn_varlen_bwd(dev, Hq, Hkv, D, with_ws, pad):
    """rga3_attn_varlen_bwd on segments [130, 1], causal (test_attention_backward: 2e-2): q, k, v head slices of one fused NaN-guarded buffer, dq, dk, dv head slices
    of one fused gradient buffer, delta_ws a slice of a longer f32 buffer; GQA 4:2 with and without dkv_ws."""
    from rga3.hip import ops

    lens = [130, 1]
    cu = _cu(lens)
    T = int(cu[-1])
    scale = D ** -0.5
    H = Hq + 2 * Hkv
    qkv, do = _rand((T, H, D), dev, seed=1), _rand((T, Hq, D), dev, seed=4)
    qc, kc, vc = (t.contiguous() for t in (qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]))
    cud = cu.to(dev)
    o_c, lse_c = ops.attn_varlen(qc, kc, vc, cud, cud, max(lens), scale, True, return_lse=True)

    def run(q, k, v, o, dout, lse, dq, dk, dv, delta):
        st = (C.c_int64 * 16)(*[s for t in (q, k, v, o, dout, dq, dk, dv) for s in (t.stride(0), t.stride(1))])
        ws = torch.empty(2 * Hq * T * D, dtype=F32, device=dev) if with_ws else None
        _call("rga3_attn_varlen_bwd", q, k, v, o, dout, lse, dq, dk, dv, delta, cud, cud, len(lens), max(lens), max(lens), T, Hq, Hkv, D, C.cast(st, C.c_void_p), scale, 1,
              ws, T)

    dq_c, dk_c, dv_c = (torch.empty_like(t) for t in (qc, kc, vc))
    run(qc, kc, vc, o_c, do, lse_c, dq_c, dk_c, dv_c, torch.empty(Hq * T, dtype=F32, device=dev))
    g_c = torch.cat([dq_c, dk_c, dv_c], 1)
    B = Bands(dev, pad)
    fused, ov, dov, lsev = B.inp(qkv), B.inp(o_c), B.inp(do), B.vec(lse_c)
    grad, delta = B.out((T, H, D)), B.flat(Hq * T, F32)
    B.arm()
    run(fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], ov, dov, lsev, grad[:, :Hq], grad[:, Hq:Hq + Hkv], grad[:, Hq + Hkv:], delta)
    B.check()
    qf, kf, vf = (t.float().cpu().requires_grad_(True) for t in (qc, kc, vc))
    ref, _ = R.attn_varlen_ref(qf, kf, vf, cu, cu, scale, True)
    ref.backward(do.float().cpu())
    gref = torch.cat([qf.grad, kf.grad, vf.grad], 1)
    _same(grad, g_c, gref, "dq | dk | dv")
    for name, got, want in (("dq", g_c[:, :Hq], qf.grad), ("dk", g_c[:, Hq:Hq + Hkv], kf.grad), ("dv", g_c[:, Hq + Hkv:], vf.grad)):
        assert _rel_l2(got, want) < 2e-2, name


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("head_major", [False, True])
def test_attn_fewq(dev, head_major, pad):
    """rga3_attn_fewq with row-major and head-major keys (test_attention_few_queries: 1e-2): q, out and the keys are views; the transposed values are contiguous by
    contract and sit in a NaN-guarded slice."""
    from rga3.hip import ops

    frames, nq, nk, H = 2, 5, 20, 2
    g = torch.Generator().manual_seed(7)
    q = (torch.randn(frames * nq, H * 16, generator=g) * 1.5).to(BF).to(dev)
    k = (torch.randn(frames * nk, H * 16, generator=g) * (0.5 + 1.5 * torch.linspace(0, 1, frames * nk)[:, None])).to(BF).to(dev)
    v = torch.randn(frames * nk, H * 16, generator=g).to(BF).to(dev)
    vb = (torch.randn(H * 16, generator=g) * 0.3).to(BF).to(dev)
    vt = v.view(frames, nk, H * 16).permute(0, 2, 1).reshape(frames * H * 16, nk).contiguous()
    khm = k.view(frames * nk, H, 16).permute(1, 0, 2).contiguous()
    want = ops.attn_fewq(q, khm if head_major else k, vt, nq, nk, H, 0.25, vb, k_head_major=head_major)
    B = Bands(dev, pad)
    qv, vtv, vbv = B.inp(q), B.vec(vt), B.vec(vb)
    if head_major:
        kv = B.inp(khm.view(H * frames * nk, 16))                    # [H][frames * nk][16] with a key stride of 24
        k_st, k_hst = kv.stride(0), frames * nk * kv.stride(0)
    else:
        kv = B.inp(k)
        k_st, k_hst = kv.stride(0), 16
    out = B.out((frames * nq, H * 16))
    B.arm()
    _call("rga3_attn_fewq", qv, qv.stride(0), kv, k_st, k_hst, vtv, vbv, out, out.stride(0), frames, nq, nk, H, 0.25)
    B.check()
    qf_, kf_, vf_ = (t.float().cpu().view(frames, -1, H, 16).permute(0, 2, 1, 3) for t in (q, k, v))
    ref = (torch.softmax(qf_ @ kf_.transpose(-1, -2) * 0.25, dim=-1) @ vf_).permute(0, 2, 1, 3).reshape(frames * nq, H * 16) + vb.float().cpu()
    _same(out, want, ref)
    assert _rel_l2(want, ref) < 1e-2


# ---------------------------------------------------------------------------------------------------------------- row ops

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("dim", [256, 2048])
def test_rmsnorm_fwd_with_res_out(dev, dim, pad):
    """rga3_rmsnorm_fwd at dim 256 (rows kernel) and 2048 (block kernel) with res_out (test_rmsnorm: res exact, 6e-3): x, add, y and res_out share ldx."""
    from rga3.hip import ops

    rows = 7
    x, add = _rand((rows, dim), dev, 2.0, seed=31), _rand((rows, dim), dev, seed=32)
    w = (1 + 0.1 * torch.randn(dim, generator=torch.Generator().manual_seed(3))).to(BF).to(dev)
    y_c, res_c = ops.rmsnorm(x, w, 1e-6, add=add, return_residual=True)
    B = Bands(dev, pad)
    xv, addv, wv = B.inp(x), B.inp(add), B.vec(w)
    y, res = B.out((rows, dim)), B.out((rows, dim))
    B.arm()
    _call("rga3_rmsnorm_fwd", xv, addv, wv, y, res, rows, dim, xv.stride(0), 1e-6)
    B.check()
    s = (x.float() + add.float()).to(BF)
    ref = R.rmsnorm_ref(s.cpu(), w.cpu(), 1e-6)
    _same(res, res_c, s.float(), "res_out")
    _same(y, y_c, ref, "y")
    assert torch.equal(res_c, s) and _rel_l2(y_c, ref) < 6e-3


def test_rmsnorm_bwd(dev):
    """rga3_rmsnorm_bwd (contiguous rows; test_rmsnorm_swiglu_backward_and_transpose: 1e-2): dx guarded at both ends."""
    from rga3.hip import ops

    rows, dim = 37, 256
    x, dy, add = _rand((rows, dim), dev, 2.0, 1), _rand((rows, dim), dev, seed=2), _rand((rows, dim), dev, seed=3)
    w = (1 + 0.1 * torch.randn(dim, generator=torch.Generator().manual_seed(4))).to(BF).to(dev)
    want = ops.rmsnorm_bwd(x, w, dy, 1e-6, add=add)
    B = Bands(dev)
    xv, wv, dyv, addv = B.vec(x), B.vec(w), B.vec(dy), B.vec(add)
    dx = B.flat(rows * dim)
    B.arm()
    _call("rga3_rmsnorm_bwd", xv, wv, dyv, addv, dx, rows, dim, 1e-6)
    B.check()
    xf = x.float().cpu().requires_grad_(True)
    R.rmsnorm_ref(xf, w.cpu(), 1e-6).backward(dy.float().cpu())
    ref = xf.grad + add.float().cpu()
    _same(dx.view(rows, dim), want, ref)
    assert _rel_l2(want, ref) < 1e-2


@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("dim", [12, 144, 264, 576, 2304])
def test_layernorm_fwd(dev, dim, act):
    """rga3_layernorm_fwd on every kernel of its dispatch with ldx = dim + 8 != ldy = dim + 24 (test_layernorm: 6e-3; with GELU test_rope_axial_and_layernorm_gelu /
    test_layernorm_narrow_rows: 8e-3)."""
    from rga3.hip import ops

    rows = 13
    x = _rand((rows, dim), dev, 3.0, seed=33) + 0.5
    w, b = _rand((dim,), dev, seed=34), _rand((dim,), dev, seed=35)
    want = ops.layernorm(x, w, b, 1e-6, act=act)
    B = Bands(dev)
    xv, wv, bv = B.inp(x), B.vec(w), B.vec(b)
    y = B.out((rows, dim), pad=24)
    B.arm()
    _call("rga3_layernorm_fwd", xv, wv, bv, y, rows, dim, xv.stride(0), y.stride(0), 1e-6, int(act == "gelu"))
    B.check()
    ref = R.layernorm_ref(x.cpu(), w.cpu(), b.cpu(), 1e-6)
    if act == "gelu":
        ref = F.gelu(ref.to(BF).float()) if dim <= 16 else F.gelu(ref)
    _same(y, want, ref)
    assert _rel_l2(want, ref) < (8e-3 if act == "gelu" else 6e-3)


@pytest.mark.parametrize("dim", [64, 72])
def test_layernorm_bwd(dev, dim):
    """rga3_layernorm_bwd (contiguous rows; test_layernorm_backward: dx 8e-3, dw / db 5e-3) at a deterministic width (64) and an atomic one (72: dweight / dbias are
    added with f32 atomics, so only dx is compared bit for bit)."""
    from rga3.hip import lib, ops

    rows = 37
    x, dy = _rand((rows, dim), dev, seed=1), _rand((rows, dim), dev, seed=2)
    w = (_rand((dim,), dev, 0.3, seed=3).float() + 1).to(BF)
    dx_c, dw_c, db_c = ops.layernorm_bwd(x, w, dy, 1e-6)
    nws = int(lib.load().rga3_layernorm_bwd_ws_floats(rows, dim))
    assert (nws > 0) == (dim == 64)
    ws = torch.empty(max(nws, 1), dtype=F32, device=dev)
    B = Bands(dev)
    xv, wv, dyv = B.vec(x), B.vec(w), B.vec(dy)
    zero = None if nws else torch.zeros(dim)
    dx, dw, db = B.flat(rows * dim), B.flat(dim, F32, data=zero), B.flat(dim, F32, data=zero)
    B.arm()
    _call("rga3_layernorm_bwd", xv, wv, dyv, dx, dw, db, rows, dim, 1e-6, ws if nws else None, nws)
    B.check()
    xr, wr, br = x.float().cpu().requires_grad_(True), w.float().cpu().requires_grad_(True), torch.zeros(dim, requires_grad=True)
    F.layer_norm(xr, (dim,), wr, br, 1e-6).backward(dy.float().cpu())
    _same(dx.view(rows, dim), dx_c, xr.grad, "dx")
    G.assert_finite_where(dw, wr.grad, "dw")
    G.assert_finite_where(db, br.grad, "db")
    if nws:
        assert torch.equal(dw, dw_c) and torch.equal(db, db_c)
    else:
        assert _rel_l2(dw, wr.grad) < 5e-3 and _rel_l2(db, br.grad) < 5e-3
    assert _rel_l2(dx_c, xr.grad) < 8e-3 and _rel_l2(dw_c, wr.grad) < 5e-3 and _rel_l2(db_c, br.grad) < 5e-3


@pytest.mark.parametrize("pad", PADS)
def test_gather_and_scatter_rows(dev, pad):
    """rga3_gather_rows / rga3_scatter_rows (test_gather_scatter_pad: exact): table, source and outputs are views; rows the scatter's idx does not name keep their bits."""
    table = _rand((40, 64), dev, seed=51)
    idx = torch.randperm(10, generator=torch.Generator().manual_seed(1))[:6]
    ref = table.cpu().view(10, 4, 64)[idx].reshape(24, 64)
    B = Bands(dev, pad)
    tv = B.inp(table)
    out = B.out((24, 64))
    B.arm()
    _call("rga3_gather_rows", tv, idx.to(dev), out, 6, 4, 64, tv.stride(0), out.stride(0))
    B.check()
    _same(out, ref.to(dev), ref.float(), "gather")
    old = _rand((40, 64), dev, seed=52)
    B = Bands(dev, pad)
    src = B.inp(ref.to(dev), pad=24)
    dst = B.out((40, 64), data=old)
    B.arm()
    _call("rga3_scatter_rows", src, idx.to(dev), dst, 6, 4, 64, src.stride(0), dst.stride(0))
    B.check()
    want = old.cpu().view(10, 4, 64).clone()
    want[idx] = ref.view(6, 4, 64)
    assert torch.equal(G.inside(dst).cpu().view(torch.int16), want.view(40, 64).view(torch.int16))      # named rows moved, every other row kept its bits


@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(7, 147, 155, 152), (40, 40, 72, 64), (5, 20, 32, 32)])
def test_pad_cols(dev, rows, cols, ld_src, ld_dst):
    """rga3_pad_cols (test_gather_scatter_pad: exact, zero tail): by contract it writes all ld_dst columns, so the destination is a [rows, ld_dst] block guarded before
    and behind; the source is a view whose rows are not 16-byte aligned (147) or are (40, 20)."""
    x = _rand((rows, cols), dev, seed=cols)
    B = Bands(dev)
    src = B.inp(x, pad=ld_src - cols)
    dst = B.out((rows, ld_dst), pad=0)
    B.arm()
    _call("rga3_pad_cols", src, dst, rows, cols, ld_src, ld_dst)
    B.check()
    got = G.inside(dst)
    assert torch.equal(got[:, :cols], x) and float(got[:, cols:].float().abs().sum()) == 0.0


@pytest.mark.parametrize("V", [5003, 5120])
@pytest.mark.parametrize("dtype", [BF, F32])
def test_cross_entropy_rows(dev, dtype, V):
    """rga3_cross_entropy_rows with dlogits and an ignored row (test_cross_entropy: loss 2e-3, gradient 1e-2): ld = V + 8 (bf16) / V + 4 (f32) keeps the scalar path at
    V = 5003 and the 16-byte path at V = 5120; logits and dlogits are views with that ld, row_loss a slice of a longer f32 buffer."""
    from rga3.hip import ops

    rows, pad = 9, 8 if dtype == BF else 4
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(rows, V, generator=g) * 3).to(dtype).to(dev)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[2] = -100
    loss_c, dl_c = ops.cross_entropy_rows(logits, labels.to(dev), want_grad=True, grad_scale=0.5)
    B = Bands(dev)
    lv = B.inp(logits, pad=pad)
    loss, dl = B.flat(rows, F32), B.out((rows, V), BF, pad=pad)
    B.arm()
    _call("rga3_cross_entropy_rows", lv, 0 if dtype == BF else 1, labels.to(dev), loss, dl, rows, V, lv.stride(0), 0.5)
    B.check()
    ref = R.ce_rows_ref(logits.cpu(), labels)
    lf = logits.float().cpu().requires_grad_(True)
    (F.cross_entropy(lf, labels, ignore_index=-100, reduction="sum") * 0.5).backward()
    _same(loss, loss_c, ref, "row_loss")
    _same(dl, dl_c, lf.grad, "dlogits")
    assert float(loss_c[2]) == 0.0 and float(dl_c[2].float().abs().max()) == 0.0
    assert (loss_c.cpu() - ref).abs().max().item() < 2e-3 and _rel_l2(dl_c, lf.grad) < 1e-2


@pytest.mark.parametrize("pad", PADS)
def test_transpose16_and_many(dev, pad):
    """rga3_transpose16 with ld_in / ld_out views and rga3_transpose16_many on contiguous matrices guarded at both ends (exact:
    test_rmsnorm_swiglu_backward_and_transpose)."""
    m = _rand((130, 77), dev, seed=6)
    B = Bands(dev, pad)
    mv = B.inp(m)
    out = B.out((77, 130))
    B.arm()
    _call("rga3_transpose16", mv, out, 130, 77, mv.stride(0), out.stride(0))
    B.check()
    assert torch.equal(G.inside(out), m.t().contiguous())
    m2 = _rand((5, 200), dev, seed=7)
    B = Bands(dev, pad)
    i1, i2 = B.vec(m), B.vec(m2)
    o1, o2 = B.flat(130 * 77), B.flat(5 * 200)
    ptrs, dims = (C.c_void_p * 4)(i1.data_ptr(), o1.data_ptr(), i2.data_ptr(), o2.data_ptr()), (C.c_int64 * 4)(130, 77, 5, 200)
    B.arm()
    _call("rga3_transpose16_many", C.cast(ptrs, C.c_void_p), C.cast(dims, C.c_void_p), 2)
    B.check()
    assert torch.equal(o1.view(77, 130), m.t()) and torch.equal(o2.view(200, 5), m2.t())


@pytest.mark.parametrize("pad", PADS)
def test_segment_sum_and_scatter_add_rows(dev, pad):
    """rga3_segment_sum_rows (test_segment_sum_and_adamw: 5e-3) and rga3_scatter_add_rows (test_deterministic_sumsq_and_scatter_add_rows: exact, other rows untouched)."""
    from rga3.hip import ops

    x = _rand((20, 64), dev, seed=1)
    rows, off = torch.tensor([3, 5, 5, 0, 19, 7, 7, 7]), torch.tensor([0, 1, 3, 5, 8])
    want = ops.segment_sum_rows(x, rows.to(dev), off.to(dev))
    B = Bands(dev, pad)
    xv = B.inp(x)
    out = B.flat(4 * 64)
    B.arm()
    _call("rga3_segment_sum_rows", xv, rows.to(dev), off.to(dev), out, 4, 64, xv.stride(0))
    B.check()
    ref = torch.stack([x.float().cpu()[rows[off[i]:off[i + 1]]].sum(0) for i in range(4)])
    _same(out.view(4, 64), want, ref)
    assert _rel_l2(want, ref) < 5e-3
    old, src = _rand((20, 64), dev, seed=2), _rand((5, 64), dev, seed=3)
    idx = torch.tensor([17, 2, 9, 0, 19])
    B = Bands(dev, pad)
    sv = B.inp(src, pad=24)
    dst = B.out((20, 64), data=old)
    B.arm()
    _call("rga3_scatter_add_rows", dst, idx.to(dev), sv, 5, 64, dst.stride(0), sv.stride(0), 0.25)
    B.check()
    want = old.clone()
    want[idx.to(dev)] = (old[idx.to(dev)].float() + 0.25 * src.float()).to(BF)
    assert torch.equal(G.inside(dst).view(torch.int16), want.view(torch.int16))


def test_colsum(dev):
    """rga3_colsum at (513, 24) with ld = 40 (test_colsum: 2e-5): the plan depends on rows and cols only, so the view takes the contiguous call's path."""
    from rga3.hip import lib, ops

    rows, cols = 513, 24
    x = _rand((rows, cols), dev, seed=rows + cols)
    want = ops.colsum(x)
    nws = int(lib.load().rga3_colsum_ws_floats(rows, cols))
    ws = torch.empty(nws, dtype=F32, device=dev)
    B = Bands(dev, pad=16)
    xv = B.inp(x)
    out = B.flat(cols, F32)
    B.arm()
    _call("rga3_colsum", xv, out, rows, cols, xv.stride(0), ws, nws, None)
    B.check()
    ref = x.double().sum(0).cpu()
    _same(out, want, ref)
    assert ((want.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item() < 2e-5


# ---------------------------------------------------------------------------------------------------------------- in-place ops

@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("nh", [8, 5])
def test_rope_inplace_on_a_head_range(dev, nh, pad):
    """rga3_rope_inplace on heads [2, 2 + nh) of a fused [T, 11, 64] buffer with a padded token stride, nh divisible by 4 and not (test_rope: 4e-3): every other head,
    and the pad, keep their bits."""
    from rga3.hip import ops

    T, H, D, h0 = 13, 11, 64, 2
    x = _rand((T, H, D), dev, seed=41)
    ang = torch.rand(T, D // 2, generator=torch.Generator().manual_seed(2)) * 6.0
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos().contiguous().to(dev), emb.sin().contiguous().to(dev)
    want = x.clone()
    ops.rope_(want, cos, sin, h0, nh)
    B = Bands(dev, pad)
    xv = B.out((T, H, D), data=x, allowed=lambda v: v[:, h0:h0 + nh])
    B.arm()
    ops.rope_(xv, cos, sin, h0, nh)
    B.check()
    ref = x.float().cpu().clone()
    ref[:, h0:h0 + nh] = R.rope_ref(x[:, h0:h0 + nh].cpu(), cos.cpu(), sin.cpu())
    _same(xv, want, ref)
    assert _rel_l2(want, ref) < 4e-3


@pytest.mark.parametrize("pad", PADS)
def test_rope_axial_inplace_leaves_the_rows_behind_n_rope(dev, pad):
    """rga3_rope_axial_inplace (test_rope_axial_and_layernorm_gelu: 4e-3): rows >= n_rope keep their bits."""
    from oracle import sam2 as S
    from rga3.hip import ops

    nk, Cc, n_rope = 40, 64, 32
    cos, sin = S.compute_axial_cis(Cc, 4, 4)
    cos, sin = cos.contiguous().to(dev), sin.contiguous().to(dev)
    k = _rand((nk, Cc), dev, seed=2)
    want = k.clone()
    ops.rope_axial_(want, cos, sin, n_rope)
    B = Bands(dev, pad)
    kv = B.out((nk, Cc), data=k, allowed=lambda v: v[:n_rope])
    B.arm()
    ops.rope_axial_(kv, cos, sin, n_rope)
    B.check()
    q0 = torch.zeros(1, 1, 16, Cc)
    _, rk = S.apply_rotary_enc(q0, k.float().cpu()[None, None][:, :, :n_rope], cos.cpu(), sin.cpu(), repeat_freqs_k=True)
    ref = torch.cat([rk[0, 0], k.float().cpu()[n_rope:]], 0)
    _same(kv, want, ref)
    assert _rel_l2(want, ref) < 4e-3


# ---------------------------------------------------------------------------------------------------------------- elementwise and flat outputs

N_FLAT = 8 * 37 + 3


def test_silu_mul_add_and_act_on_a_ragged_length(dev):
    """rga3_silu_mul / rga3_add (test_elementwise: 6e-3 / 4e-3) and the three kinds of rga3_act at n = 8 x 37 + 3: the output is a slice of a longer buffer."""
    from rga3.hip import ops

    a, b = _rand((N_FLAT,), dev, 2.0, seed=61), _rand((N_FLAT,), dev, seed=62)
    af, bf = a.float().cpu(), b.float().cpu()
    gp = af.clone().requires_grad_(True)
    F.gelu(gp).backward(bf)
    cases = [("rga3_silu_mul", ops.silu_mul(a, b), F.silu(af) * bf, 6e-3, None), ("rga3_add", ops.add(a, b), af + bf, 4e-3, None),
             # rga3_act has no kernel test of its own: one bf16 rounding of an f32 value is 2^-9 relative per element; 2^-8 leaves as much again for erff / __expf
             ("rga3_act", ops.gelu(a), F.gelu(af), 2.0 ** -8, 0), ("rga3_act", ops.act_bwd(a, b, "gelu"), gp.grad, 2.0 ** -8, 1), ("rga3_act", ops.act_bwd(a, b, "relu"), bf * (af > 0), 2.0 ** -8, 2)]
    for name, want, ref, tol, kind in cases:
        B = Bands(dev)
        av, bv, out = B.vec(a), B.vec(b), B.flat(N_FLAT)
        B.arm()
        if kind is None:
            _call(name, av, bv, out, N_FLAT)
        else:
            _call(name, av, bv if kind else None, out, N_FLAT, kind)
        B.check()
        _same(out, want, ref, f"{name} {kind}")
        assert _rel_l2(want, ref) < tol, (name, kind)


def test_swiglu_fwd_and_bwd(dev):
    """rga3_swiglu_fwd / rga3_swiglu_bwd at T = 19, I = 48 (test_rmsnorm_swiglu_backward_and_transpose: 1e-2)."""
    from rga3.hip import ops

    T, I = 19, 48
    gu, da = _rand((T, 2 * I), dev, seed=4), _rand((T, I), dev, seed=5)
    a_c, dgu_c = ops.swiglu_fwd(gu), ops.swiglu_bwd(gu, da)
    B = Bands(dev)
    guv, dav = B.vec(gu), B.vec(da)
    a, dgu = B.flat(T * I), B.flat(T * 2 * I)
    B.arm()
    _call("rga3_swiglu_fwd", guv, a, T, I)
    _call("rga3_swiglu_bwd", guv, dav, dgu, T, I)
    B.check()
    gf = gu.float().cpu().requires_grad_(True)
    gb = gf.view(T, I // 16, 2, 16)
    y = (F.silu(gb[:, :, 0]) * gb[:, :, 1]).reshape(T, I)
    y.backward(da.float().cpu())
    _same(a.view(T, I), a_c, y.detach(), "fwd")
    _same(dgu.view(T, 2 * I), dgu_c, gf.grad, "bwd")
    assert _rel_l2(a_c, y.detach()) < 1e-2 and _rel_l2(dgu_c, gf.grad) < 1e-2


def test_dropout_and_pair(dev):
    """rga3_dropout_bf16 and the pair form at n = 8 x 37 (test_dropout_kernel_matches_oracle_mask: exact against the oracle's mask)."""
    from rga3.hip import ops

    n, p, seed = 8 * 37, 0.25, 12345
    x, z = _rand((n,), dev, seed=3), _rand((n,), dev, seed=6)
    keep, scale = R.dropout_mask_ref(n, p, seed)
    want = (x.float().cpu() * torch.from_numpy(keep).float() * scale).to(BF)
    B = Bands(dev)
    xv, zv = B.vec(x), B.vec(z)
    y, ya, yb = B.flat(n), B.flat(n), B.flat(n)
    B.arm()
    _call("rga3_dropout_bf16", xv, y, n, p, seed, 0)
    _call("rga3_dropout_pair_bf16", xv, zv, ya, yb, n, p, seed, 0.5, 222, 0)
    B.check()
    assert torch.equal(y.cpu(), want) and torch.equal(ya, ops.dropout(x, p, seed)) and torch.equal(yb, ops.dropout(z, 0.5, 222))


def test_adamw_steps(dev):
    """rga3_adamw_step (n = 8 x 37 + 3), rga3_adamw_step_clip and rga3_adamw_step_clip_rows (test_segment_sum_and_adamw: 1e-5 against torch.optim.AdamW): param,
    master, m and v are slices of longer buffers; inactive rows of the row form keep their bits."""
    from rga3.hip import ops

    for form, n in (("plain", N_FLAT), ("clip", N_FLAT), ("rows", 8 * 40)):
        g = torch.Generator().manual_seed(n)
        p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g).to(BF)
        rows, rl = 8, n // 8
        active = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.uint8)
        if form == "rows":
            gr = (gr.view(rows, rl) * active[:, None]).reshape(-1)
        B = Bands(dev)
        pb, master, m, v = B.flat(n, BF, data=p.to(BF)), B.flat(n, F32, data=p), B.flat(n, F32, data=torch.zeros(n)), B.flat(n, F32, data=torch.zeros(n))
        grv = B.vec(gr.to(dev))
        pc, mc, m1, v1 = p.to(BF).to(dev), p.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        B.arm()
        if form == "plain":
            _call("rga3_adamw_step", pb, master, grv, m, v, n, 1e-2, 0.9, 0.95, 1e-8, 0.0, 1, 1.0)
            ops.adamw_step_(pc, mc, gr.to(dev), m1, v1, 1e-2, 0.9, 0.95, 1e-8, 0.0, 1)
        elif form == "clip":
            _call("rga3_adamw_step_clip", pb, master, grv, m, v, n, 1e-2, 0.9, 0.95, 1e-8, 0.0, 1, None, 0.0)
            ops.adamw_step_clip_(pc, mc, gr.to(dev), m1, v1, 1e-2, 0.9, 0.95, 1e-8, 0.0, 1)
        else:
            _call("rga3_adamw_step_clip_rows", pb, master, grv, m, v, rows, rl, active.to(dev), 1e-2, 0.9, 0.95, 1e-8, 1, None, 0.0)
            ops.adamw_step_clip_rows_(pc.view(rows, rl), mc.view(rows, rl), gr.to(dev).view(rows, rl), m1.view(rows, rl), v1.view(rows, rl), active.to(dev), 1e-2, 0.9, 0.95,
                                      1e-8, 1)
        B.check()
        pr = torch.nn.Parameter(p.clone())
        opt = torch.optim.AdamW([pr], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0)
        pr.grad = gr.float()
        opt.step()
        assert torch.equal(pb, pc) and torch.equal(master, mc) and torch.equal(m, m1) and torch.equal(v, v1), form
        assert bool(torch.isfinite(master).all()) and (master.cpu() - pr.data).abs().max().item() < 1e-5, form
        if form == "rows":
            idle = (active == 0).to(dev)
            assert torch.equal(master.view(rows, rl)[idle], p.to(dev).view(rows, rl)[idle]) and torch.equal(pb.view(rows, rl)[idle], p.to(BF).to(dev).view(rows, rl)[idle])


def test_sumsq_det(dev):
    """rga3_sumsq_det on a ragged length (test_deterministic_sumsq_and_scatter_add_rows: 1e-5 against fp64): partials and out are slices of longer buffers."""
    from rga3.hip import ops

    n = 8 * 1000 + 3
    g = _rand((n,), dev, 0.7, seed=0)
    part_c, acc_c = torch.zeros(2048, dtype=F32, device=dev), torch.full((1,), 123.0, dtype=F32, device=dev)
    ops.sumsq_det_(g, part_c, acc_c, accumulate=False)
    B = Bands(dev)
    gv = B.vec(g)
    part, acc = B.flat(2048, F32, data=torch.zeros(2048)), B.flat(1, F32, data=torch.full((1,), 123.0))
    B.arm()
    _call("rga3_sumsq_det", gv, n, part, 2048, acc, 0)
    B.check()
    ref = float((g.double() ** 2).sum())
    assert torch.equal(acc, acc_c) and abs(float(acc_c) - ref) <= 1e-5 * ref


def test_bce_dice_sums_det_and_grad(dev):
    """rga3_bce_dice_sums_det (test_bce_dice_sums: 1e-4) and rga3_bce_dice_grad at a ragged plane of 23 x 13 pixels: out4, the workspace and dlogits are slices."""
    from rga3.hip import lib, ops

    nm, h, w_ = 3, 23, 13
    hw = h * w_
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(nm, h, w_, generator=g) * 3, (torch.randn(nm, h, w_, generator=g) > 0.2).float()
    xd, td = x.to(dev), t.to(dev)
    nws = int(lib.load().rga3_bce_dice_sums_ws_floats(nm, hw))
    ws_c, out_c = torch.empty(max(nws, 1), dtype=F32, device=dev), torch.empty(nm * 4, dtype=F32, device=dev)
    _call("rga3_bce_dice_sums_det", xd, td, out_c, ws_c, nws, nm, hw)
    grad_c = ops.bce_dice_grad(xd, td, out_c.view(nm, 4), 0.7, 0.3)
    B = Bands(dev)
    xv, tv = B.vec(xd), B.vec(td)
    out4, ws, dl = B.flat(nm * 4, F32), B.flat(max(nws, 1), F32), B.flat(nm * hw, F32)
    B.arm()
    _call("rga3_bce_dice_sums_det", xv, tv, out4, ws, nws, nm, hw)
    _call("rga3_bce_dice_grad", xv, tv, B.vec(out_c), dl, nm, hw, 0.7, 0.3)
    B.check()
    bce = F.binary_cross_entropy_with_logits(x, t, reduction="none").flatten(1).sum(1)
    p = torch.sigmoid(x)
    ref = torch.stack([bce, (p * t).flatten(1).sum(1), p.flatten(1).sum(1), t.flatten(1).sum(1)], 1)
    _same(out4.view(nm, 4), out_c.view(nm, 4), ref, "sums")
    assert ((out_c.view(nm, 4).cpu() - ref).abs() / ref.abs().clamp_min(1)).max().item() < 1e-4
    assert torch.equal(dl.view(nm, h, w_), grad_c) and bool(torch.isfinite(dl).all())


def test_pixel_shuffle2x_and_bwd(dev):
    """rga3_pixel_shuffle2x (+ bias, + add, GELU; test_conv3x3s2_dwconv_pixel_shuffle: 1e-2 with GELU) and its backward on a 3 x 5 map of 8 channels."""
    from rga3.hip import ops

    Fn, H, W, cin, co = 2, 3, 5, 16, 8
    x, wt, b = _rand((Fn * H * W, cin), dev, seed=14), _rand((cin, co, 2, 2), dev, 0.1, seed=15), _rand((co,), dev, 0.1, seed=16)
    add = _rand((Fn * 4 * H * W, co), dev, seed=17)
    gm = ops.gemm(x, wt.permute(2, 3, 1, 0).reshape(-1, cin).contiguous(), tile=12)
    want = ops.pixel_shuffle2x(gm, b, add, Fn, H, W, act="gelu")
    dout = _rand((Fn * 4 * H * W, co), dev, seed=18)
    dg_c = ops.pixel_shuffle2x_bwd(dout, Fn, H, W)
    B = Bands(dev)
    gv, bv, addv, dv = B.vec(gm), B.vec(b), B.vec(add), B.vec(dout)
    out, dg = B.flat(Fn * 4 * H * W * co), B.flat(Fn * H * W * 4 * co)
    B.arm()
    _call("rga3_pixel_shuffle2x", gv, bv, addv, out, Fn, H, W, co, 1)
    _call("rga3_pixel_shuffle2x_bwd", dv, dg, Fn, H, W, co)
    B.check()
    ref = F.conv_transpose2d(x.float().cpu().view(Fn, H, W, cin).permute(0, 3, 1, 2), wt.float().cpu(), b.float().cpu(), stride=2).permute(0, 2, 3, 1).reshape(-1, co)
    ref = F.gelu(ref + add.float().cpu())
    _same(out.view(-1, co), want, ref, "forward")
    assert _rel_l2(want, ref) < 1e-2
    assert torch.equal(dg.view(-1, 4 * co), dg_c)
    assert sorted(dg_c.flatten().tolist()) == sorted(dout.flatten().tolist())           # the backward without bias / add / act is a permutation of dout


def test_bilinear_and_bwd(dev):
    """rga3_bilinear / rga3_bilinear_bwd at (5, 7) -> (50, 9) (test_bilinear: 1e-5 max-abs; test_bilinear_backward_gather: 1e-5): f32 planes guarded at both ends."""
    from rga3.hip import ops

    n, hi, wi, ho, wo = 2, 5, 7, 50, 9
    g = torch.Generator().manual_seed(hi * wo)
    x, dout = torch.randn(n, hi, wi, generator=g), torch.randn(n, ho, wo, generator=g)
    want = ops.bilinear(x.to(dev), (ho, wo))
    din_c = ops.bilinear_bwd(dout.to(dev), (n, hi, wi))
    B = Bands(dev)
    xv, dv = B.vec(x.to(dev)), B.vec(dout.to(dev))
    out, din = B.flat(n * ho * wo, F32), B.flat(n * hi * wi, F32)
    B.arm()
    _call("rga3_bilinear", xv, 1, out, None, n, hi, wi, ho, wo)
    _call("rga3_bilinear_bwd", dv, din, None, n, hi, wi, ho, wo)
    B.check()
    ref = F.interpolate(x[None], size=(ho, wo), mode="bilinear", align_corners=False)[0]
    xin = torch.zeros(n, 1, hi, wi, requires_grad=True)
    F.interpolate(xin, size=(ho, wo), mode="bilinear", align_corners=False).backward(dout[:, None])
    _same(out.view(n, ho, wo), want, ref, "forward")
    _same(din.view(n, hi, wi), din_c, xin.grad[:, 0], "backward")
    assert (want.cpu() - ref).abs().max().item() < 1e-5 and _rel_l2(din_c, xin.grad[:, 0]) < 1e-5


def test_mask_product_and_bwd(dev):
    """rga3_mask_product / rga3_mask_product_bwd at (B, P, C) = (1, 77, 8) (test_mask_product_forward_backward: 1e-5, 4e-3)."""
    from rga3.hip import lib, ops

    Bn, P, Cc = 1, 77, 8
    hyper, up = _rand((Bn, 4, Cc), dev, seed=1), _rand((Bn * P, Cc), dev, 0.5, seed=2)
    dm = torch.randn(Bn, 4, P, generator=torch.Generator().manual_seed(3)).to(dev)
    masks_c = ops.mask_product(hyper, up, P)
    dh_c, du_c = ops.mask_product_bwd(dm, hyper, up, P)
    nws = int(lib.load().rga3_mask_product_bwd_ws_floats(Bn, 4, P, Cc))
    ws = torch.empty(max(nws, 1), dtype=F32, device=dev)
    B = Bands(dev)
    hv, uv, dmv = B.vec(hyper), B.vec(up), B.vec(dm)
    masks, dup, dhy = B.flat(Bn * 4 * P, F32), B.flat(Bn * P * Cc), B.flat(Bn * 4 * Cc)
    B.arm()
    _call("rga3_mask_product", hv, uv, masks, Bn, 4, P, Cc)
    _call("rga3_mask_product_bwd", dmv, hv, uv, dup, dhy, Bn, 4, P, Cc, ws, nws)
    B.check()
    hr, ur = hyper.float().cpu().requires_grad_(True), up.float().cpu().view(Bn, P, Cc).requires_grad_(True)
    ref = torch.einsum("bmc,bpc->bmp", hr, ur)
    ref.backward(dm.cpu())
    _same(masks.view(Bn, 4, P), masks_c, ref.detach(), "masks")
    _same(dup.view(Bn * P, Cc), du_c, ur.grad.view(Bn * P, Cc), "dup")
    _same(dhy.view(Bn, 4, Cc), dh_c, hr.grad, "dhyper")
    assert _rel_l2(masks_c, ref.detach()) < 1e-5 and _rel_l2(du_c, ur.grad.view(Bn * P, Cc)) < 4e-3 and _rel_l2(dh_c, hr.grad) < 4e-3


# ---------------------------------------------------------------------------------------------------------------- SAM2 spatial kernels

def test_maxpool2x2_win_and_add_bcast(dev):
    """rga3_maxpool2x2_win with ldx / ldy and rga3_add_bcast with lda / ldb / ldo views (test_maxpool_win_and_upsample_add: exact / 4e-3)."""
    from rga3.hip import ops

    nwin, w_, Cc = 3, 4, 24
    x = _rand((nwin * w_ * w_, Cc), dev, seed=1)
    want = ops.maxpool2x2_win(x, nwin, w_)
    B = Bands(dev)
    xv = B.inp(x)
    y = B.out((nwin * 4, Cc), pad=24)
    B.arm()
    _call("rga3_maxpool2x2_win", xv, y, nwin, w_, Cc, xv.stride(0), y.stride(0))
    B.check()
    ref = F.max_pool2d(x.float().cpu().view(nwin, w_, w_, Cc).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).reshape(-1, Cc)
    _same(y, want, ref, "maxpool")
    assert torch.equal(want.float().cpu(), ref)
    a, pe = _rand((21 * 2, Cc), dev, seed=2), _rand((21, Cc), dev, seed=4)
    want = ops.add_bcast(a, pe, 0.1)
    B = Bands(dev)
    av, pev = B.inp(a), B.inp(pe, pad=16)
    out = B.out((42, Cc), pad=24)
    B.arm()
    _call("rga3_add_bcast", av, pev, out, 42, 21, Cc, av.stride(0), pev.stride(0), out.stride(0), 0.1)
    B.check()
    ref = a.float().cpu() + 0.1 * pe.float().cpu().repeat(2, 1)
    _same(out, want, ref, "add_bcast")
    assert _rel_l2(want, ref) < 4e-3


def test_im2col_with_ld_out_and_zero_tail(dev):
    """rga3_im2col (test_patch_embed_im2col: the columns are a gather, so exact against F.unfold): by contract columns C ks ks .. ld_out - 1 are zero-filled, so the
    output is a [rows, ld_out] block guarded before and behind; the NCHW image sits in a NaN-guarded slice."""
    Fn, Cc, H, W, ks, stride, pad = 2, 3, 13, 9, 7, 4, 3
    img = _rand((Fn, Cc, H, W), dev, seed=1)
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    cols, ld = Cc * ks * ks, (Cc * ks * ks + 7) // 8 * 8 + 8
    B = Bands(dev)
    iv = B.vec(img)
    out = B.out((Fn * Ho * Wo, ld), pad=0)
    B.arm()
    _call("rga3_im2col", iv, out, Fn, Cc, H, W, ks, stride, pad, ld)
    B.check()
    ref = F.unfold(img.float().cpu(), ks, padding=pad, stride=stride).permute(0, 2, 1).reshape(Fn * Ho * Wo, cols)
    got = G.inside(out).float().cpu()
    assert torch.equal(got[:, :cols], ref) and float(got[:, cols:].abs().sum()) == 0.0


def test_dwconv7x7_conv3x3s2_and_im2col3x3s2(dev):
    """rga3_dwconv7x7 at (2, 7, 9, 72), rga3_conv3x3s2 and rga3_im2col3x3s2 (test_dwconv7x7_tiled / test_conv3x3s2_dwconv_pixel_shuffle: 6e-3): no leading dimensions;
    the maps are guarded before and behind."""
    from rga3.hip import ops

    Fn, H, W, Cc = 2, 7, 9, 72
    x, w, b = _rand((Fn * H * W, Cc), dev, seed=H), _rand((Cc, 1, 7, 7), dev, 0.1, seed=W), _rand((Cc,), dev, 0.1, seed=Cc)
    want = ops.dwconv7x7(x, w, b, Fn, H, W)
    B = Bands(dev)
    xv, wv, bv = B.vec(x), B.vec(w), B.vec(b)
    y = B.flat(Fn * H * W * Cc)
    B.arm()
    _call("rga3_dwconv7x7", xv, wv, bv, y, Fn, H, W, Cc)
    B.check()
    ref = F.conv2d(x.float().cpu().view(Fn, H, W, Cc).permute(0, 3, 1, 2), w.float().cpu(), b.float().cpu(), padding=3, groups=Cc).permute(0, 2, 3, 1).reshape(-1, Cc)
    _same(y.view(-1, Cc), want, ref, "dwconv7x7")
    assert _rel_l2(want, ref) < 6e-3
    Fn, H, W, cin = 2, 6, 10, 4
    x, w, b = _rand((Fn * H * W, cin), dev, seed=cin), _rand((cin * 4, cin, 3, 3), dev, 0.2, seed=cin + 1), _rand((cin * 4,), dev, 0.1, seed=cin + 2)
    want = ops.conv3x3s2(x, w, b, Fn, H, W)
    B = Bands(dev)
    xv, wv, bv = B.vec(x), B.vec(w), B.vec(b)
    y = B.flat(want.numel())
    B.arm()
    _call("rga3_conv3x3s2", xv, 0, wv, bv, y, Fn, H, W, cin, cin * 4, 0.0, 0.0)
    B.check()
    ref = F.conv2d(x.float().cpu().view(Fn, H, W, cin).permute(0, 3, 1, 2), w.float().cpu(), b.float().cpu(), stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, cin * 4)
    _same(y.view(-1, cin * 4), want, ref, "conv3x3s2")
    assert _rel_l2(want, ref) < 6e-3
    cin = 8
    x = _rand((Fn * H * W, cin), dev, seed=9)
    B = Bands(dev)
    xv = B.vec(x)
    cols = B.flat(Fn * (H // 2) * (W // 2) * 9 * cin)
    B.arm()
    _call("rga3_im2col3x3s2", xv, cols, Fn, H, W, cin)
    B.check()
    un = F.unfold(x.float().cpu().view(Fn, H, W, cin).permute(0, 3, 1, 2), 3, padding=1, stride=2)                # [F, c * 9 + k, L], k = kh * 3 + kw
    ref = un.view(Fn, cin, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * cin)                                        # rows (f, oh, ow), columns (kh * 3 + kw) * C + c
    assert torch.equal(cols.view(-1, 9 * cin).float().cpu(), ref)


# ---------------------------------------------------------------------------------------------------------------- SAM2 decoder / memory-attention chains

@pytest.mark.parametrize("pad", PADS)
def test_decimg_rows(dev, pad):
    """rga3_decimg_rows on three frames of 24 pixels, 9 tokens (16-row blocks straddle the frame boundaries; test_decoder_image_side_block_boundary: 1.5e-2 / 2e-2
    against fp32): keys, pe, keys_out, k2 and v2 are views; token-side keys / values and the weights are contiguous by contract and sit in NaN-guarded slices."""
    from rga3.hip import ops

    Bn, hw, nk = 3, 24, 9
    M = Bn * hw
    g = torch.Generator().manual_seed(Bn * 100 + hw + nk)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(BF).to(dev)
    keys, pe = (torch.randn(M, 256, generator=g) * 1.2 + 0.3 * torch.randn(M, 1, generator=g)).to(BF).to(dev), r(hw, 256, sc=0.5)
    kt, vt = r(Bn * nk, 128), r(Bn * nk, 128)
    wq, bq, wo, bo = r(128, 256, sc=0.06), r(128, sc=0.1), r(256, 128, sc=0.09), r(256, sc=0.1)
    gam, bet = (1 + 0.2 * torch.randn(256, generator=g)).to(BF).to(dev), r(256, sc=0.1)
    wk, bk, wv, bv = r(128, 256, sc=0.06), r(128, sc=0.1), r(128, 256, sc=0.06), r(128, sc=0.1)
    out_c, k2_c, v2_c = ops.decimg_rows(keys, pe, kt, vt, nk, (wq, bq), (wo, bo), (gam, bet), 1e-5, (wk, bk), (wv, bv), scale=0.25)
    B = Bands(dev, pad)
    kv_, pev = B.inp(keys), B.inp(pe)
    V = B.vec
    out, k2, v2 = B.out((M, 256)), B.out((M, 128)), B.out((M, 128))
    assert k2.stride(0) == v2.stride(0)
    B.arm()
    _call("rga3_decimg_rows", kv_, kv_.stride(0), pev, pev.stride(0), hw, V(kt), V(vt), nk, V(wq), V(bq), V(wo), V(bo), V(gam), V(bet), 1e-5, V(wk), V(bk), V(wv), V(bv),
          out, out.stride(0), k2, v2, k2.stride(0), 0, 0.25, M)
    B.check()
    f = lambda t: t.float().cpu()
    pe_rows = f(pe).repeat(Bn, 1)
    qf_ = (F.linear(f(keys) + pe_rows, f(wq), f(bq))).view(Bn, hw, 8, 16).permute(0, 2, 1, 3)
    kf_, vf_ = f(kt).view(Bn, nk, 8, 16).permute(0, 2, 1, 3), f(vt).view(Bn, nk, 8, 16).permute(0, 2, 1, 3)
    of_ = torch.softmax(qf_ @ kf_.transpose(-1, -2) * 0.25, dim=-1) @ vf_
    xr = F.layer_norm(F.linear(of_.permute(0, 2, 1, 3).reshape(M, 128), f(wo), f(bo)) + f(keys), (256,), f(gam), f(bet), 1e-5)
    k2r, v2r = F.linear(xr + pe_rows, f(wk), f(bk)), F.linear(xr, f(wv), f(bv))
    _same(out, out_c, xr, "keys'")
    _same(k2, k2_c, k2r, "k2")
    _same(v2, v2_c, v2r, "v2")
    assert _rel_l2(out_c, xr) < 1.5e-2 and _rel_l2(k2_c, k2r) < 2e-2 and _rel_l2(v2_c, v2r) < 2e-2


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("Nq,Nk,nsplit", [(37, 70, 1), (261, 300, 3)])
def test_memattn_cross_out_and_partials(dev, Nq, Nk, nsplit, pad):
    """rga3_memattn_cross with the `out` form and the partials form (test_memattn_cross_low_rank_values: 1e-2): q, k, m and out are views, the workspace -- which IS the
    output of the partials form -- a slice of exactly rga3_memattn_cross_ws_floats() floats guarded at both ends."""
    from rga3.hip import lib, ops

    g = torch.Generator().manual_seed(Nq * 7 + Nk)
    q = torch.randn(Nq, 256, generator=g).to(BF).to(dev)
    k = (torch.randn(Nk, 256, generator=g) * (0.5 + 1.5 * torch.linspace(0, 1, Nk)[:, None])).to(BF).to(dev)
    m = torch.randn(Nk, 64, generator=g).to(BF).to(dev)
    scale = 256 ** -0.5
    want = ops.memattn_cross(q, k, m, scale, nsplit=nsplit)
    po_c, pml_c, ns = ops.memattn_cross(q, k, m, scale, nsplit=nsplit, partials=True)
    po_c, pml_c = po_c.clone(), pml_c.clone()
    n = int(lib.load().rga3_memattn_cross_ws_floats(Nq, nsplit))
    assert ns == nsplit and n >= nsplit * Nq * 66
    B = Bands(dev, pad)
    qv, kv_, mv = B.inp(q), B.inp(k), B.inp(m)
    out, ws, ws2 = B.out((Nq, 64)), B.flat(n, F32), B.flat(n, F32)
    B.arm()
    _call("rga3_memattn_cross", qv, kv_, mv, out, Nq, Nk, qv.stride(0), kv_.stride(0), mv.stride(0), out.stride(0), scale, nsplit, ws)
    _call("rga3_memattn_cross", qv, kv_, mv, None, Nq, Nk, qv.stride(0), kv_.stride(0), mv.stride(0), 0, scale, nsplit, ws2)
    B.check()
    ref = torch.softmax(q.float().cpu() @ k.float().cpu().t() * scale, dim=-1) @ m.float().cpu()
    _same(out, want, ref)
    assert _rel_l2(want, ref) < 1e-2
    assert torch.equal(ws2[:nsplit * Nq * 64], po_c) and torch.equal(ws2[nsplit * Nq * 64:nsplit * Nq * 66], pml_c)
    assert bool(torch.isfinite(ws2[:nsplit * Nq * 66]).all())


@pytest.mark.parametrize("pad", PADS)
def test_memlayer_rows_three_chains(dev, pad):
    """rga3_memlayer_rows for the three chains of test_memory_layer_row_chain at M = 16 x 3 + 5 rows (a partial last 16-row workgroup), nq = 64 (table rows wrap):
    a, res, x_out, t_out and y_out are views, the partial sums of chain 3 a NaN-guarded slice.  Tolerances of that test: fp32 1e-2 (x, y of chain 1) / 1.5e-2 (q of
    chain 2); against the launches replaced 2e-3 (x) / 3e-3 (t)."""
    from rga3.hip import ops

    M, nq = 53, 64
    g = torch.Generator().manual_seed(M + nq)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(BF).to(dev)
    x = (torch.randn(M, 256, generator=g) * 1.2 + 0.4 * torch.randn(M, 1, generator=g)).to(BF).to(dev)
    gam, bet = (1 + 0.2 * torch.randn(256, generator=g)).to(BF).to(dev), r(256, sc=0.1)
    ang = torch.rand(nq, 128, generator=g) * 6.28
    cos, sin = ang.cos().contiguous().to(dev), ang.sin().contiguous().to(dev)
    f = lambda t: t.float().cpu()

    def rope_ref(y, cols):
        y = y.clone()
        t = torch.arange(M) % nq
        for c0 in range(0, cols, 256):
            blk = y[:, c0:c0 + 256].reshape(M, 128, 2)
            c, s_ = cos.cpu()[t], sin.cpu()[t]
            y[:, c0:c0 + 256] = torch.stack([blk[..., 0] * c - blk[..., 1] * s_, blk[..., 0] * s_ + blk[..., 1] * c], -1).reshape(M, 256)
        return y

    def raw(B, a, K1, po, pml, ns, w1, b1, xo, to, w2, b2, N2, yo, rope_cols):
        xv = B.inp(x)
        av = B.inp(a) if a is not None else None
        V = lambda t: None if t is None else B.vec(t)
        args = (av, av.stride(0) if a is not None else 0, K1, V(po), V(pml), ns, V(w1), V(b1), xv, xv.stride(0), xo, xo.stride(0) if xo is not None else 0, V(gam), V(bet), 1e-5,
                to, to.stride(0) if to is not None else 0, V(w2), V(b2), N2, yo, yo.stride(0) if yo is not None else 0, cos if rope_cols else None, sin if rope_cols else None,
                rope_cols, nq if rope_cols else 0, M)
        B.arm()
        _call("rga3_memlayer_rows", *args)
        B.check()

    # (1) norm -> qkv (256 -> 768) -> RoPE on q | k
    wqkv, bqkv = r(768, 256, sc=0.06), r(768, sc=0.1)
    _, _, y_c = ops.memlayer_rows(x, (gam, bet), 1e-5, w2=wqkv, b2=bqkv, rope=(cos, sin), rope_cols=512)
    B = Bands(dev, pad)
    y = B.out((M, 768))
    raw(B, None, 0, None, None, 0, None, None, None, None, wqkv, bqkv, 768, y, 512)
    ref = rope_ref(F.linear(F.layer_norm(f(x), (256,), f(gam), f(bet), 1e-5), f(wqkv), f(bqkv)), 512)
    _same(y, y_c, ref, "chain 1 y")
    assert _rel_l2(y_c, ref) < 1e-2
    # (2) out-projection + residual -> norm -> q projection -> RoPE
    a, wo, bo, wq, bq = r(M, 256), r(256, 256, sc=0.06), r(256, sc=0.1), r(256, 256, sc=0.06), r(256, sc=0.1)
    x2_c, t2_c, q2_c = ops.memlayer_rows(x, (gam, bet), 1e-5, a=a, w1=wo, b1=bo, want_t=True, w2=wq, b2=bq, rope=(cos, sin), rope_cols=256)
    B = Bands(dev, pad)
    x2, t2, q2 = B.out((M, 256)), B.out((M, 256), pad=24), B.out((M, 256))
    raw(B, a, 256, None, None, 0, wo, bo, x2, t2, wq, bq, 256, q2, 256)
    xr = F.linear(f(a), f(wo), f(bo)) + f(x)
    tr = F.layer_norm(xr, (256,), f(gam), f(bet), 1e-5)
    qr = rope_ref(F.linear(tr, f(wq), f(bq)), 256)
    _same(x2, x2_c, xr, "chain 2 x")
    _same(t2, t2_c, tr, "chain 2 t")
    _same(q2, q2_c, qr, "chain 2 y")
    assert _rel_l2(x2_c, xr) < 1e-2 and _rel_l2(q2_c, qr) < 1.5e-2
    assert _rel_l2(t2_c, ops.layernorm(ops.gemm(a, wo, bo, residual=x, tile=12), gam, bet, 1e-5)) < 3e-3
    # (3) merge of the cross-attention slices -> (Wo Wv) + residual -> norm
    Nk, nsplit = 300, 3
    qq, kk, mm = r(M, 256), (torch.randn(Nk, 256, generator=g) * (0.5 + 1.5 * torch.linspace(0, 1, Nk)[:, None])).to(BF).to(dev), r(Nk, 64)
    wov, bov = r(256, 64, sc=0.1), r(256, sc=0.1)
    po, pml, ns = ops.memattn_cross(qq, kk, mm, 256 ** -0.5, nsplit=nsplit, partials=True)
    po, pml = po.clone(), pml.clone()
    x3_c, t3_c, _ = ops.memlayer_rows(x, (gam, bet), 1e-5, partials=(po, pml, ns), w1=wov, b1=bov, want_t=True)
    B = Bands(dev, pad)
    x3, t3 = B.out((M, 256)), B.out((M, 256))
    raw(B, None, 64, po, pml, ns, wov, bov, x3, t3, None, None, 0, None, 0)
    pm = ops.memattn_cross(qq, kk, mm, 256 ** -0.5, nsplit=nsplit)
    x_un = ops.gemm(pm, wov, bov, residual=x, tile=12)
    t_un = ops.layernorm(x_un, gam, bet, 1e-5)
    _same(x3, x3_c, x_un.float(), "chain 3 x")
    _same(t3, t3_c, t_un.float(), "chain 3 t")
    assert _rel_l2(x3_c, x_un) < 2e-3 and _rel_l2(t3_c, t_un) < 3e-3


@pytest.mark.parametrize("pad", PADS)
def test_mlp3_rows_and_sam_select_objptr(dev, pad):
    """rga3_mlp3_rows with frame strides wider than the rows (x: one token row of a [B, nq, C] buffer per frame, y: views with a padded frame stride) and
    rga3_sam_select_objptr (test_fused_decoder_heads_and_selection: 6e-3, indices exact): best, sel and obj_ptr are slices guarded at both ends."""
    from rga3.hip import ops

    Bn, nq, Cc = 5, 9, 256
    g = torch.Generator().manual_seed(5)
    hs = torch.randn(Bn, nq, Cc, generator=g).to(BF)

    def mk(i, h, o):
        return [(torch.randn(a, b, generator=g) * 0.08).to(BF) if k == 0 else (torch.randn(a, generator=g) * 0.1).to(BF) for a, b in ((h, i), (h, h), (o, h)) for k in (0, 1)]

    sets, toks, widths = [mk(Cc, 256, 32), mk(Cc, 64, 4), mk(Cc, 256, 1)], [2, 1, 0], [32, 4, 1]
    hsd = hs.to(dev)
    want = ops.mlp3_rows([(hsd.view(-1)[t * Cc:], nq * Cc, tuple(x.to(dev) for x in w), i == 1) for i, (w, t) in enumerate(zip(sets, toks))], Bn)
    B = Bands(dev, pad)
    hv = B.inp(hsd.view(Bn, nq * Cc))                       # frame stride nq C + 8
    outs = [B.out((Bn, o)) for o in widths]
    n = len(sets)
    ptrs, dims, keep = (C.c_void_p * (8 * n))(), (C.c_int64 * (6 * n))(), []
    for i, (w, t, o) in enumerate(zip(sets, toks, outs)):
        ptrs[8 * i] = hv.data_ptr() + 2 * t * Cc                # token t of frame 0
        held = [B.vec(x.to(dev)) for x in w]
        keep.append(held)                                        # the pointer table does not keep the slices alive
        for j, tt in enumerate(held + [o]):
            ptrs[8 * i + 1 + j] = tt.data_ptr()
        for j, v in enumerate((hv.stride(0), o.stride(0), Cc, w[0].shape[0], w[4].shape[0], int(i == 1))):
            dims[6 * i + j] = v
    B.arm()
    _call("rga3_mlp3_rows", C.cast(ptrs, C.c_void_p), C.cast(dims, C.c_void_p), n, Bn)
    B.check()
    for i, (w, t) in enumerate(zip(sets, toks)):
        x = hs[:, t].float()
        for li in range(3):
            x = F.linear(x, w[2 * li].float(), w[2 * li + 1].float()).to(BF).float()
            if li < 2:
                x = F.relu(x)
        if i == 1:
            x = torch.sigmoid(x)
        _same(outs[i], want[i], x, f"mlp {i}")
        assert _rel_l2(want[i], x) < 6e-3, i
    # selection
    iou = torch.tensor([[0.9, 0.2, 0.7, 0.7], [0.1, 0.5, 0.5, 0.4], [0.3, 0.1, 0.2, 0.6], [0.0, 0.8, 0.1, 0.3], [0.2, 0.25, 0.5, 0.125]]).to(BF).to(dev)
    obj = torch.tensor([[1.5], [-0.5], [0.0], [2.0], [0.25]]).to(BF).to(dev)
    proj = [x.to(dev) for x in mk(Cc, Cc, Cc)]
    no_obj = torch.randn(Cc, generator=g).to(BF).to(dev)
    best_c, sel_c, sel64_c, ptr_c = ops.sam_select_objptr(iou, obj, hsd[:, 2:6], tuple(proj), no_obj)
    B = Bands(dev, pad)
    hv = B.inp(hsd.view(Bn, nq * Cc))
    V = B.vec
    best, sel, ptr = B.flat(2 * Bn, torch.int64), B.flat(Bn, torch.int32), B.flat(Bn * Cc)
    toks_ptr = hv.data_ptr() + 2 * 2 * Cc                     # tokens 2..5 of every frame
    B.arm()
    _call("rga3_sam_select_objptr", V(iou), V(obj), toks_ptr, hv.stride(0), Cc, V(proj[0]), V(proj[1]), V(proj[2]), V(proj[3]), V(proj[4]), V(proj[5]), V(no_obj), best, sel, ptr,
          Bn)
    B.check()
    rbest = torch.argmax(iou[:, 1:].float().cpu(), dim=-1)
    assert torch.equal(best[:Bn], best_c) and torch.equal(best[Bn:], sel64_c) and torch.equal(sel, sel_c) and torch.equal(best_c.cpu(), rbest)
    assert torch.equal(sel_c.cpu().long(), torch.arange(Bn) * 4 + 1 + rbest)
    x = hs[torch.arange(Bn), 3 + rbest].float()
    for li in range(3):
        x = F.linear(x, proj[2 * li].float().cpu(), proj[2 * li + 1].float().cpu()).to(BF).float()
        if li < 2:
            x = F.relu(x)
    ref = torch.where(obj.float().cpu() > 0, x, no_obj.float().cpu()[None])
    _same(ptr.view(Bn, Cc), ptr_c, ref, "obj_ptr")
    assert _rel_l2(ptr_c, ref) < 6e-3


# ---------------------------------------------------------------------------------------------------------------- contiguous uint8 pipelines: outputs and workspaces

def test_mask_jf_counts_output_and_workspace(dev):
    """rga3_mask_jf_counts (contiguous 1-byte masks; test_counts_and_scores_equal_the_reference: the six counts are exact): counts and the bit-packed workspace are
    slices guarded at both ends."""
    from rga3.hip import lib
    from tests import jf_cases

    c = jf_cases.case("frames3")
    ann, seg = (torch.from_numpy(m).to(dev).to(torch.uint8).contiguous() for m in (c.ann, c.seg))
    T, h, w = ann.shape
    nws = int(lib.load().rga3_mask_jf_ws_bytes(T, h, w))
    assert nws > 0
    B = Bands(dev)
    counts, ws = B.flat(T * 6, torch.int64), B.flat(nws, torch.uint8)
    B.arm()
    _call("rga3_mask_jf_counts", B.vec(seg), B.vec(ann), None, counts, ws, nws, T, h, w, int(c.radius))
    B.check()
    assert torch.equal(counts.view(T, 6).cpu(), torch.from_numpy(c.counts))


def test_stom_flow_and_shift_composite_outputs(dev):
    """rga3_stom_flow / rga3_stom_shift_composite (contiguous uint8 frames; tests/test_stom_gpu.py pins them byte for byte against the numpy route): the records and the
    composited clip are slices guarded at both ends, equal to the wrapper's results."""
    from rga3.hip import ops

    rng = torch.Generator().manual_seed(3)
    T, H, W, N = 3, 45, 130, 40
    frames = torch.randint(0, 256, (T, H, W, 3), generator=rng, dtype=torch.uint8).to(dev)
    overlay = torch.randint(0, 256, (H, W, 4), generator=rng, dtype=torch.uint8).to(dev)
    base = torch.randint(8 * 10, 8 * 30, (N, 2), generator=rng).float() / 8.0
    tracks = torch.stack([base, base + torch.tensor([3.5, -2.25]), base + torch.tensor([-6.125, 4.0])]).contiguous().to(dev)
    vis = torch.ones(T, N, dtype=torch.uint8, device=dev)
    rec_c = ops.stom_flow(tracks, vis.bool(), 0)
    out_c = ops.stom_shift_composite(frames, overlay, rec_c, 0)
    B = Bands(dev)
    rec, out = B.flat(T * 4, torch.int32), B.flat(frames.numel(), torch.uint8)
    B.arm()
    _call("rga3_stom_flow", B.vec(tracks), B.vec(vis), rec, T, N, 0)
    _call("rga3_stom_shift_composite", B.vec(frames), B.vec(overlay), rec, out, T, H, W, 0)
    B.check()
    assert torch.equal(rec.view(T, 4), rec_c) and torch.equal(out.view(T, H, W, 3), out_c)
    assert rec_c[:, 0].tolist() == [0, 1, 1]                              # the prompt's own frame is left alone, the two others are shifted
    assert not torch.equal(out_c[1], frames[1])


def test_preprocessing_outputs_and_workspace(dev):
    """rga3_sam_preprocess_u8 (both passes: 37 x 53 -> 64 x 64) and rga3_qwen_patchify_u8 (an odd frame count: the last frame repeats) -- contiguous uint8 pipelines that
    tests/test_preproc_gpu.py pins against Pillow / the HF processor: the row-pass workspace, the resized bytes, the normalised planes and the patch rows are slices
    guarded at both ends, equal to the wrappers' results."""
    from rga3.utils import preproc as P

    g = torch.Generator().manual_seed(11)
    T, H, W, size = 2, 37, 53, 64
    frames = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    bf_c, u8_c = P.sam_preprocess_frames(frames, size=size, return_u8=True)
    (bh, kh), (bv, kv) = P._dev_tables(W, size, dev), P._dev_tables(H, size, dev)
    m3, s3 = (C.c_float * 3)(*P.SAM_MEAN), (C.c_float * 3)(*P.SAM_STD)
    B = Bands(dev)
    tmp, u8, bf = B.flat(T * H * size * 3, torch.uint8), B.flat(T * size * size * 3, torch.uint8), B.flat(T * 3 * size * size)
    B.arm()
    _call("rga3_sam_preprocess_u8", B.vec(frames), T, H, W, size, size, bh, kh, kh.shape[1], bv, kv, kv.shape[1], tmp, u8, bf, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p))
    B.check()
    assert torch.equal(u8.view(T, size, size, 3), u8_c) and torch.equal(bf.view(T, 3, size, size), bf_c) and bool(torch.isfinite(bf.float()).all())
    T, h, w = 3, 56, 84
    frames = torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    for odt in (BF, F32):
        want, grid = P.qwen_preprocess_video(frames, out_dtype=odt)
        assert grid.tolist() == [[2, 4, 6]] and tuple(want.shape) == (48, 1176)
        B = Bands(dev)
        out = B.flat(want.numel(), odt)
        B.arm()
        _call("rga3_qwen_patchify_u8", B.vec(frames), T, h, w, P.qwen_norm_lut(dev), out, int(odt == F32), 14, 2, 2)
        B.check()
        assert torch.equal(out.view(48, 1176), want) and bool(torch.isfinite(out.float()).all())


def test_entry_points_that_add_with_atomics_stay_inside_their_outputs(dev):
    """rga3_colsum_accum, rga3_sumsq_accum and rga3_bilinear_bwd with plane_idx add with f32 atomics: no bit-identity between two calls, but the bits outside the
    outputs stay, the padding does not leak, and the values meet test_colsum (2e-5), test_segment_sum_and_adamw (1e-4), test_bilinear_backward_gather (1e-5)."""
    rows, cols = 513, 20
    x = _rand((rows, cols), dev, seed=rows + cols)
    B = Bands(dev)
    xv = B.inp(x)
    out = B.flat(cols, F32, data=torch.zeros(cols))
    B.arm()
    _call("rga3_colsum_accum", xv, out, rows, cols, xv.stride(0))
    B.check()
    ref = x.double().sum(0).cpu()
    G.assert_finite_where(out, ref)
    assert ((out.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item() < 2e-5
    gq = _rand((N_FLAT,), dev, seed=3)
    B = Bands(dev)
    acc = B.flat(1, F32, data=torch.zeros(1))
    B.arm()
    _call("rga3_sumsq_accum", B.vec(gq), acc, N_FLAT)
    B.check()
    ref = float((gq.double() ** 2).sum())
    assert abs(float(acc) - ref) / ref < 1e-4
    n, hi, wi, ho, wo = 2, 5, 7, 50, 9
    dout = torch.randn(n, ho, wo, generator=torch.Generator().manual_seed(hi * wo))
    xin = torch.zeros(n, 1, hi, wi, requires_grad=True)
    F.interpolate(xin, size=(ho, wo), mode="bilinear", align_corners=False).backward(dout[:, None])
    B = Bands(dev)
    din = B.flat(n * hi * wi, F32, data=torch.zeros(n * hi * wi))
    B.arm()
    _call("rga3_bilinear_bwd", B.vec(dout.to(dev)), din, torch.arange(n, dtype=torch.int32, device=dev), n, hi, wi, ho, wo)
    B.check()
    G.assert_finite_where(din.view(n, hi, wi), xin.grad[:, 0])
    assert _rel_l2(din.view(n, hi, wi), xin.grad[:, 0]) < 1e-5


def test_contiguous_by_contract_entry_points_keep_inside_their_outputs(dev):
    """Entry points without a stride (x, y contiguous by contract) at ragged sizes, outputs guarded at both ends, inputs in NaN-guarded slices, bit-identical to the
    wrappers that the existing tests pin: rga3_upsample2x_add (test_maxpool_win_and_upsample_add), rga3_swiglu_fwd_quant_fp8 / rga3_swiglu_bwd_quant_fp8
    (test_swiglu_quant_fused_equals_unfused), rga3_hiera_mlp144 at a partial last workgroup (test_hiera_stage1_mlp_fused), rga3_conv3x3s2_ln_gelu
    (test_mask_downsampler_narrow_stages_fused), rga3_bce_dice_grad_dev."""
    from rga3.hip import ops

    Fn, H, W, Cc = 2, 6, 10, 24
    a, b = _rand((Fn * H * W, Cc), dev, seed=2), _rand((Fn * H * W // 4, Cc), dev, seed=3)
    want = ops.upsample2x_add(a, b, Fn, H, W)
    B = Bands(dev)
    out = B.flat(want.numel())
    B.arm()
    _call("rga3_upsample2x_add", B.vec(a), B.vec(b), out, Fn, H, W, Cc)
    B.check()
    assert torch.equal(out.view(-1, Cc), want) and bool(torch.isfinite(out.float()).all())

    T, I = 19, 48
    gu, da = _rand((T, 2 * I), dev, 1.5, seed=41), _rand((T, I), dev, 0.7, seed=42)
    (q1, s1), (q3, s3) = ops.swiglu_fwd_quant(gu), ops.swiglu_bwd_quant(gu, da)
    B = Bands(dev)
    qf, sf, qb, sb = B.flat(T * I, torch.uint8), B.flat(T, F32), B.flat(T * 2 * I, torch.uint8), B.flat(T, F32)
    B.arm()
    _call("rga3_swiglu_fwd_quant_fp8", B.vec(gu), qf, sf, T, I)
    _call("rga3_swiglu_bwd_quant_fp8", B.vec(gu), B.vec(da), qb, sb, T, I)
    B.check()
    assert torch.equal(qf.view(T, I), q1) and torch.equal(sf, s1) and torch.equal(qb.view(T, 2 * I), q3) and torch.equal(sb, s3) and bool(torch.isfinite(torch.cat([sf, sb])).all())

    M, Ch = 256 + 17, 144
    g = torch.Generator().manual_seed(M + Ch)
    x = (torch.randn(M, Ch, generator=g) * 1.5).to(BF).to(dev)
    w1, b1 = (torch.randn(4 * Ch, Ch, generator=g) * 0.08).to(BF).to(dev), (torch.randn(4 * Ch, generator=g) * 0.1).to(BF).to(dev)
    w2, b2 = (torch.randn(Ch, 4 * Ch, generator=g) * 0.05).to(BF).to(dev), (torch.randn(Ch, generator=g) * 0.1).to(BF).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(Ch, generator=g)).to(BF).to(dev), (0.1 * torch.randn(Ch, generator=g)).to(BF).to(dev)
    wf, colc, biasf = ops.fold_layernorm(w1, b1, gamma, beta)
    want = ops.hiera_mlp(x, wf, colc, biasf, w2, b2, 1e-6)
    B = Bands(dev)
    y = B.flat(M * Ch)
    B.arm()
    _call("rga3_hiera_mlp144", B.vec(x), B.vec(wf), B.vec(colc), B.vec(biasf), B.vec(w2), B.vec(b2), y, M, 1e-6)
    B.check()
    xf = x.float().cpu()
    ref = xf + F.linear(F.gelu(F.linear(F.layer_norm(xf, (Ch,), gamma.float().cpu(), beta.float().cpu(), 1e-6), w1.float().cpu(), b1.float().cpu())), w2.float().cpu(), b2.float().cpu())
    _same(y.view(M, Ch), want, ref, "hiera_mlp144")
    assert _rel_l2(want, ref) < 1e-2

    S_ = 10
    mask = (torch.randn(1, S_, S_, generator=g) * 4).to(dev)
    cw, cb = _rand((4, 1, 3, 3), dev, 0.3, seed=1), _rand((4,), dev, 0.1, seed=2)
    lw, lb = (1 + 0.2 * torch.randn(4, generator=g)).to(BF).to(dev), _rand((4,), dev, 0.1, seed=3)
    want = ops.conv3x3s2_ln_gelu(mask, cw, cb, lw, lb, 1e-6, 1, S_, S_, 20.0, -10.0)
    B = Bands(dev)
    y = B.flat(want.numel())
    B.arm()
    _call("rga3_conv3x3s2_ln_gelu", B.vec(mask), 1, B.vec(cw), B.vec(cb), B.vec(lw), B.vec(lb), 1e-6, y, 1, S_, S_, 1, 4, 20.0, -10.0)
    B.check()
    assert torch.equal(y.view(want.shape), want) and bool(torch.isfinite(y.float()).all())

    nm, hw = 3, 23 * 13
    lg, tg = torch.randn(nm, hw, generator=g).to(dev) * 3, (torch.randn(nm, hw, generator=g) > 0.2).float().to(dev)
    sums = ops.bce_dice_sums(lg.view(nm, 23, 13), tg.view(nm, 23, 13))
    cbce, cdice = torch.tensor([0.7], device=dev), torch.tensor([0.3], device=dev)
    want = ops.bce_dice_grad(lg, tg, sums, cbce, cdice)
    B = Bands(dev)
    dl = B.flat(nm * hw, F32)
    B.arm()
    _call("rga3_bce_dice_grad_dev", B.vec(lg), B.vec(tg), B.vec(sums), dl, nm, hw, B.vec(cbce), B.vec(cdice))
    B.check()
    assert torch.equal(dl.view(nm, hw), want) and bool(torch.isfinite(dl).all())


# ---------------------------------------------------------------------------------------------------------------- views that cannot hold their rows

def _refused(dev, name, args_of, bad, match):
    """One refusal: `args_of(bad)` builds (guards, arguments with the stride `bad`, the same arguments with the output view's own stride).  With `bad` the entry point
    answers RGA3_EINVAL with a message naming the stride and launches nothing (the backing buffer keeps its snapshot bits); the valid call afterwards still works."""
    from rga3.hip import lib

    B, args_bad, args_ok = args_of(bad)
    B.arm()
    rc = _rc(name, *args_bad)
    assert rc == EINVAL, (name, rc)
    msg = lib.last_error()
    assert match in msg, (name, msg)
    torch.cuda.synchronize()
    for b, v, snap in B.guards:
        assert torch.equal(G._as_int(b), G._as_int(snap)), f"{name}: a refused call wrote to its output"
    _call(name, *args_ok)
    B.check()
    for b, v, snap in B.guards:
        assert not torch.equal(G._as_int(b), G._as_int(snap)), f"{name}: the valid call wrote nothing"


def _nt_operands(dev, M=19, N=24, K=16):
    return _rand((M, K), dev, seed=1), _rand((N, K), dev, 0.1, seed=2), _rand((M, N), dev, seed=3)


@pytest.mark.parametrize("which,match", [("ldc", "ldc"), ("ldr", "ldr"), ("lda", "lda"), ("ldw", "ldw")])
def test_refuse_gemm_bf16(dev, which, match):
    from rga3.hip import ops

    M, N, K = 19, 24, 16
    a, w, r = _nt_operands(dev)
    ws = ops.gemm_workspace(dev)

    def args_of(bad):
        B = Bands(dev)
        out = B.out((M, N))
        ld = {"ldc": out.stride(0), "ldr": N, "lda": K, "ldw": K}
        mk = lambda d: (a, w, None, r, None, out, M, N, K, d["lda"], d["ldw"], d["ldc"], d["ldr"], 0, 0, 12, ws, ws.numel())
        return B, mk(dict(ld, **{which: bad})), mk(ld)

    _refused(dev, "rga3_gemm_bf16", args_of, {"ldc": N - 8, "ldr": N - 8, "lda": K - 8, "ldw": K - 8}[which], match)


def test_gemm_bf16_accepts_the_documented_exemptions(dev):
    """ldr without a residual is not looked at; a single row never uses its stride."""
    from rga3.hip import ops

    M, N, K = 19, 24, 16
    a, w, _ = _nt_operands(dev)
    ws = ops.gemm_workspace(dev)
    out = torch.empty((M, N), dtype=BF, device=dev)
    _call("rga3_gemm_bf16", a, w, None, None, None, out, M, N, K, K, K, N, 0, 0, 0, 12, ws, ws.numel())
    assert torch.equal(out, ops.gemm(a, w, tile=12))
    _call("rga3_gemm_bf16", a, w, None, None, None, out, 1, N, K, 0, K, 0, 0, 0, 0, 12, ws, ws.numel())
    assert torch.equal(out[:1], ops.gemm(a[:1], w, tile=12))


def test_refuse_the_other_nt_gemms(dev):
    """rga3_gemm_rms_bf16, _swiglu_pre (ldc and ldpre), _ln, _lnq, _lnsum, _cat (ldc and ldcn), _fp8: an output stride shorter than the width written."""
    from rga3.hip import ops

    M, N, K = 19, 32, 64
    a, w, _ = _nt_operands(dev, M, N, K)
    ws = ops.gemm_workspace(dev)
    sums = torch.zeros(M, dtype=torch.int64, device=dev)
    colc, stat, parts = torch.zeros(N, dtype=F32, device=dev), torch.ones((M, 2), dtype=F32, device=dev), torch.ones((M, 1, 2), dtype=F32, device=dev)
    bz = torch.zeros(N, dtype=BF, device=dev)
    pre = torch.empty((M, N), dtype=BF, device=dev)
    rp = torch.empty((M, 1, 2), dtype=F32, device=dev)
    wn, cn = _rand((8, K), dev, seed=5), torch.empty((M, 8), dtype=BF, device=dev)
    aq, wq = torch.zeros((M, 128), dtype=torch.uint8, device=dev), torch.zeros((N, 128), dtype=torch.uint8, device=dev)
    sa, sw = torch.ones(M, dtype=F32, device=dev), torch.ones(N, dtype=F32, device=dev)

    def case(name, width, mk, match):
        def args_of(bad):
            B = Bands(dev)
            out = B.out((M, width))
            return B, mk(out, bad), mk(out, out.stride(0))
        _refused(dev, name, args_of, width - 8, match)

    case("rga3_gemm_rms_bf16", N, lambda o, ld: (a, w, None, None, o, M, N, K, K, K, ld, 0, 0, 12, ws, ws.numel(), None, 0, 0.0, sums), "ldc")
    case("rga3_gemm_swiglu_pre_bf16", N // 2, lambda o, ld: (a, w, None, o, pre, M, N, K, K, K, ld, N, 12, ws, ws.numel()), "ldc")
    case("rga3_gemm_swiglu_pre_bf16", N, lambda o, ld: (a, w, None, torch.empty((M, N // 2), dtype=BF, device=dev), o, M, N, K, K, K, N // 2, ld, 12, ws, ws.numel()), "ldpre")
    case("rga3_gemm_ln_bf16", N, lambda o, ld: (a, w, bz, colc, stat, o, M, N, K, K, K, ld, 0, 12), "ldc")
    case("rga3_gemm_lnq_bf16", N, lambda o, ld: (a, w, bz, colc, parts, 1, K, 1e-6, o, M, N, K, K, K, ld, 0, 12), "ldc")
    case("rga3_gemm_lnsum_bf16", N, lambda o, ld: (a, w, None, None, o, M, N, K, K, K, ld, 0, 12, rp), "ldc")
    case("rga3_gemm_cat_bf16", N, lambda o, ld: (a, w, None, o, M, N, K, K, K, ld, a, w, K, K, K, None, None, 0, 0, 0, 13), "ldc")
    w64, c64 = torch.cat([w, w]), torch.empty((M, 64), dtype=BF, device=dev)        # with an N side N is a multiple of the tile width (tile 13: 64)
    case("rga3_gemm_cat_bf16", 8, lambda o, ld: (a, w64, None, c64, M, 64, K, K, K, 64, None, None, 0, 0, 0, wn, o, 8, K, ld, 13), "ldcn")
    case("rga3_gemm_fp8", N, lambda o, ld: (aq, wq, sa, sw, None, None, o, M, N, 128, 128, 128, ld, 0), "ldc")


def test_refuse_tn_and_rows16(dev):
    """rga3_gemm_tn_bf16, rga3_gemm_tn_many, rga3_gemm_rows16_many."""
    K, M, N = 40, 16, 24
    a, b = _rand((K, M), dev, seed=1), _rand((K, N), dev, seed=2)

    def tn(bad):
        B = Bands(dev)
        out = B.out((M, N))
        mk = lambda ld: (a, b, None, out, M, N, K, M, N, ld, 0, None, 0, None)
        return B, mk(bad), mk(out.stride(0))

    _refused(dev, "rga3_gemm_tn_bf16", tn, N - 8, "ldc")
    keep = []

    def tn_many(bad):
        B = Bands(dev)
        out = B.out((M, N))
        ws = torch.empty(M * N, dtype=F32, device=dev)

        def mk(ld):
            ptrs, dims = (C.c_void_p * 3)(a.data_ptr(), b.data_ptr(), out.data_ptr()), (C.c_int64 * 7)(M, N, K, M, N, ld, 0)
            keep.extend([ptrs, dims])
            return (C.cast(ptrs, C.c_void_p), C.cast(dims, C.c_void_p), 1, ws, ws.numel() * 4)
        return B, mk(bad), mk(out.stride(0))

    _refused(dev, "rga3_gemm_tn_many", tn_many, N - 8, "ldc")
    x, w = _rand((9, 16), dev, seed=3), _rand((N, 16), dev, 0.1, seed=4)

    def rows16(bad):
        B = Bands(dev)
        out = B.out((9, N))

        def mk(ld):
            ptrs = (C.c_void_p * 6)(x.data_ptr(), None, w.data_ptr(), None, None, out.data_ptr())
            dims = (C.c_int64 * 9)(9, N, 16, 0, 16, 0, 16, ld, 0)
            keep.extend([ptrs, dims])
            return (C.cast(ptrs, C.c_void_p), C.cast(dims, C.c_void_p), 1)
        return B, mk(bad), mk(out.stride(0))

    _refused(dev, "rga3_gemm_rows16_many", rows16, N - 8, "ldc")


def test_refuse_row_ops(dev):
    """rga3_rmsnorm_fwd, rga3_layernorm_fwd (ldy), rga3_gather_rows, rga3_scatter_rows, rga3_scatter_add_rows, rga3_maxpool2x2_win, rga3_add_bcast, rga3_quant_fp8_rows,
    rga3_rope_axial_inplace, rga3_mlp3_rows; rga3_layernorm_stats / rga3_segment_sum_rows (read strides, no strided output)."""
    rows, dim = 6, 32
    x, w, b = _rand((rows, dim), dev, seed=1), _rand((dim,), dev, seed=2), _rand((dim,), dev, seed=3)
    idx = torch.tensor([4, 1, 3], dtype=torch.int64, device=dev)

    def case(name, shape, mk, match, bad=None, dtype=BF, data=None):
        def args_of(bad_):
            B = Bands(dev)
            out = B.out(shape, dtype, data=data)
            return B, mk(out, bad_), mk(out, out.stride(0))
        _refused(dev, name, args_of, shape[1] - 8 if bad is None else bad, match)

    xw = G.banded((rows, dim), dim + 8, BF, dev, "in", data=x)[0]
    case("rga3_rmsnorm_fwd", (rows, dim), lambda o, ld: (xw if ld == dim + 8 else x, None, w, o, None, rows, dim, ld, 1e-6), "ldx")
    case("rga3_layernorm_fwd", (rows, dim), lambda o, ld: (x, w, b, o, rows, dim, dim, ld, 1e-6, 0), "ldy")
    case("rga3_gather_rows", (3, dim), lambda o, ld: (x, idx, o, 3, 1, dim, dim, ld), "ld_out")
    case("rga3_scatter_rows", (rows, dim), lambda o, ld: (x, idx, o, 3, 1, dim, dim, ld), "ld_out")
    case("rga3_scatter_add_rows", (rows, dim), lambda o, ld: (o, idx, x, 3, dim, ld, dim, 0.5), "ld_dst", data=x)
    case("rga3_maxpool2x2_win", (2, dim), lambda o, ld: (_rand((8, dim), dev, seed=4), o, 2, 2, dim, dim, ld), "ldy")
    case("rga3_add_bcast", (rows, dim), lambda o, ld: (x, x, o, rows, rows, dim, dim, dim, ld, 1.0), "ldo")
    case("rga3_quant_fp8_rows", (rows, dim), lambda o, ld: (x, o, torch.empty(rows, dtype=F32, device=dev), rows, dim, dim, ld), "ldq", dtype=torch.uint8)
    cs = torch.ones((4, dim // 2), dtype=F32, device=dev)
    case("rga3_rope_axial_inplace", (rows, dim), lambda o, ld: (o, cs, cs, rows, 4, dim, ld), "ldx", data=x)
    from rga3.hip import lib
    st = torch.empty((rows, 2), dtype=F32, device=dev)
    assert _rc("rga3_layernorm_stats", x, st, rows, dim, dim - 8, 1e-6) == EINVAL and "ldx" in lib.last_error()
    o4 = torch.empty((1, dim), dtype=BF, device=dev)
    assert _rc("rga3_segment_sum_rows", x, idx, torch.tensor([0, 3], device=dev), o4, 1, dim, dim - 8) == EINVAL and "ldx" in lib.last_error()
    keep = []
    ws_ = [_rand((dim, dim), dev, 0.1, seed=5 + i) for i in range(3)]

    def mlp3(bad):
        B = Bands(dev)
        out = B.out((rows, dim))

        def mk(ld):
            ptrs = (C.c_void_p * 8)(x.data_ptr(), ws_[0].data_ptr(), b.data_ptr(), ws_[1].data_ptr(), b.data_ptr(), ws_[2].data_ptr(), b.data_ptr(), out.data_ptr())
            dims = (C.c_int64 * 6)(dim, ld, dim, dim, dim, 0)
            keep.extend([ptrs, dims])
            return (C.cast(ptrs, C.c_void_p), C.cast(dims, C.c_void_p), 1, rows)
        return B, mk(bad), mk(out.stride(0))

    _refused(dev, "rga3_mlp3_rows", mlp3, dim - 8, "y frame stride")


def test_refuse_the_remaining_strided_entry_points(dev):
    """rga3_pad_cols, rga3_cross_entropy_rows, rga3_transpose16, rga3_im2col, rga3_colsum, rga3_colsum_accum, rga3_decimg_rows, rga3_memattn_cross, rga3_memlayer_rows
    and rga3_sam_select_objptr: each names the short stride."""
    from rga3.hip import lib

    def refuse_only(name, args, match):
        assert _rc(name, *args) == EINVAL and match in lib.last_error(), (name, lib.last_error())

    rows, cols = 6, 24
    x = _rand((rows, cols + 8), dev, seed=1)

    def pad_cols(bad):
        B = Bands(dev)
        dst = B.out((rows, 32), pad=0)
        return B, (x, dst, rows, cols, bad, 32), (x, dst, rows, cols, cols + 8, 32)

    _refused(dev, "rga3_pad_cols", pad_cols, cols - 8, "ld_src")
    refuse_only("rga3_pad_cols", (x, torch.empty((rows, 32), dtype=BF, device=dev), rows, cols, cols + 8, 16), "ld_dst")

    V = 40
    labels = torch.tensor([3, -100, 7, 39, 0, 1], device=dev)

    def ce(bad):
        B = Bands(dev)
        lv, loss, dl = B.inp(_rand((rows, V), dev, seed=2)), B.flat(rows, F32), B.out((rows, V))
        mk = lambda ld: (lv, 0, labels, loss, dl, rows, V, ld, 1.0)
        return B, mk(bad), mk(dl.stride(0))

    _refused(dev, "rga3_cross_entropy_rows", ce, V - 8, "cross_entropy: ld")

    R_, C_ = 10, 24
    m = _rand((R_, C_), dev, seed=3)

    def tr(bad):
        B = Bands(dev)
        out = B.out((C_, R_))
        return B, (m, out, R_, C_, C_, bad), (m, out, R_, C_, C_, out.stride(0))

    _refused(dev, "rga3_transpose16", tr, R_ - 2, "ld_out")
    refuse_only("rga3_transpose16", (m, torch.empty((C_, R_), dtype=BF, device=dev), R_, C_, C_ - 8, R_), "ld_in")

    img = _rand((1, 3, 8, 8), dev, seed=4)                                     # ks 3, stride 2, pad 1: 16 rows of 27 columns

    def im2col(bad):
        B = Bands(dev)
        out = B.out((16, 32), pad=0)
        return B, (img, out, 1, 3, 8, 8, 3, 2, 1, bad), (img, out, 1, 3, 8, 8, 3, 2, 1, 32)

    _refused(dev, "rga3_im2col", im2col, 24, "ld_out")

    xs = _rand((50, 16), dev, seed=5)
    nws = int(lib.load().rga3_colsum_ws_floats(50, 16))
    ws = torch.empty(max(nws, 1), dtype=F32, device=dev)

    def colsum(bad):
        B = Bands(dev)
        out = B.flat(16, F32)
        return B, (xs, out, 50, 16, bad, ws, nws, None), (xs, out, 50, 16, 16, ws, nws, None)

    _refused(dev, "rga3_colsum", colsum, 8, "colsum: ld")

    def colsum_accum(bad):
        B = Bands(dev)
        out = B.flat(16, F32, data=torch.zeros(16))
        return B, (xs, out, 50, 16, bad), (xs, out, 50, 16, 16)

    _refused(dev, "rga3_colsum_accum", colsum_accum, 8, "colsum_accum: ld")

    hw, nk = 16, 1
    r = lambda *sh, sc=1.0, seed=0: _rand(sh, dev, sc, seed=seed)
    keys, pe, kt, vt = r(hw, 256, seed=6), r(hw, 256, sc=0.5, seed=7), r(nk, 128, seed=8), r(nk, 128, seed=9)
    wq, bq, wo, bo, lw, lb = r(128, 256, sc=0.06, seed=10), r(128, sc=0.1, seed=11), r(256, 128, sc=0.09, seed=12), r(256, sc=0.1, seed=13), r(256, seed=14), r(256, sc=0.1, seed=15)
    wk, bk = r(128, 256, sc=0.06, seed=16), r(128, sc=0.1, seed=17)
    dec = lambda out, ld, k2=None, v2=None, kvs=0: (keys, 256, pe, 256, hw, kt, vt, nk, wq, bq, wo, bo, lw, lb, 1e-5, wk if k2 is not None else None,
                                                    bk if k2 is not None else None, wk if k2 is not None else None, bk if k2 is not None else None, out, ld, k2, v2, kvs, 0, 0.25, hw)

    def decimg(bad):
        B = Bands(dev)
        out = B.out((hw, 256))
        return B, dec(out, bad), dec(out, out.stride(0))

    _refused(dev, "rga3_decimg_rows", decimg, 248, "keys_out_stride")
    o_, k2_ = torch.empty((hw, 256), dtype=BF, device=dev), torch.empty((hw, 128), dtype=BF, device=dev)
    refuse_only("rga3_decimg_rows", dec(o_, 256, k2_, torch.empty_like(k2_), 120), "kv_stride")

    Nq, Nk = 20, 40
    q, k, mm = r(Nq, 256, seed=18), r(Nk, 256, seed=19), r(Nk, 64, seed=20)
    wsm = torch.empty(int(lib.load().rga3_memattn_cross_ws_floats(Nq, 1)), dtype=F32, device=dev)

    def memattn(bad):
        B = Bands(dev)
        out = B.out((Nq, 64))
        mk = lambda ld: (q, k, mm, out, Nq, Nk, 256, 256, 64, ld, 256 ** -0.5, 1, wsm)
        return B, mk(bad), mk(out.stride(0))

    _refused(dev, "rga3_memattn_cross", memattn, 56, "out_stride")

    w2, b2 = r(256, 256, sc=0.06, seed=21), r(256, sc=0.1, seed=22)
    ml = lambda y, ld, res_st=256, t=None, t_st=0: (None, 0, 0, None, None, 0, None, None, q, res_st, None, 0, lw, lb, 1e-5, t, t_st, w2, b2, 256, y, ld, None, None, 0, 0, Nq)

    def memlayer(bad):
        B = Bands(dev)
        y = B.out((Nq, 256))
        return B, ml(y, bad), ml(y, y.stride(0))

    _refused(dev, "rga3_memlayer_rows", memlayer, 248, "y_stride")
    y_ = torch.empty((Nq, 256), dtype=BF, device=dev)
    refuse_only("rga3_memlayer_rows", ml(y_, 256, res_st=248), "res_stride")
    refuse_only("rga3_memlayer_rows", ml(y_, 256, t=torch.empty_like(y_), t_st=248), "t_stride")

    Bn, Cc = 3, 32
    iou, obj, toks = r(Bn, 4, seed=23), r(Bn, 1, seed=24), r(Bn, 4, Cc, seed=25)
    pw = [r(Cc, Cc, sc=0.1, seed=26 + i) for i in range(3)]
    pb, no_obj = r(Cc, sc=0.1, seed=30), r(Cc, seed=31)

    def select(bad):
        B = Bands(dev)
        best, sel, ptr = B.flat(2 * Bn, torch.int64), B.flat(Bn, torch.int32), B.flat(Bn * Cc)
        mk = lambda tb: (iou, obj, toks, tb, Cc, pw[0], pb, pw[1], pb, pw[2], pb, no_obj, best, sel, ptr, Bn)
        return B, mk(bad), mk(4 * Cc)

    _refused(dev, "rga3_sam_select_objptr", select, 4 * Cc - 8, "tok_bstride")


def test_refuse_attention_strides(dev):
    """rga3_attn_varlen_fwd / _fwd_rope / _bwd, rga3_rope_inplace and rga3_attn_fewq: a head stride shorter than D, a token stride shorter than the heads it spans."""
    from rga3.hip import lib, ops

    T, H, D = 20, 2, 32
    q, k, v = _rand((T, H, D), dev, seed=1), _rand((T, H, D), dev, seed=2), _rand((T, H, D), dev, seed=3)
    cu = torch.tensor([0, T], dtype=torch.int32, device=dev)
    cos = torch.full((T, D), 0.8, dtype=F32, device=dev)
    sin = torch.full((T, D), 0.6, dtype=F32, device=dev)

    def fwd(o_st, o_sh, o):
        return (q, k, v, o, None, cu, cu, 1, T, T, H, H, D, H * D, D, H * D, D, H * D, D, o_st, o_sh, D ** -0.5, 0, 0, None, 0, T, 0, 0)

    def rope(o_st, o_sh, o):
        return (q, k, v, o, None, cu, cu, 1, T, T, H, H, D, H * D, D, H * D, D, H * D, D, o_st, o_sh, D ** -0.5, 0, cos, sin, None, None)

    for name, mk in (("rga3_attn_varlen_fwd", fwd), ("rga3_attn_varlen_fwd_rope", rope)):
        for bad, match in (((H * D - 8, D), "o token stride"), ((H * D + 8, D - 8), "o head stride")):
            def args_of(bad_):
                B = Bands(dev)
                o = B.out((T, H, D))
                return B, mk(bad_[0], bad_[1], o), mk(o.stride(0), o.stride(1), o)
            _refused(dev, name, args_of, bad, match)
        o = torch.empty((T, H, D), dtype=BF, device=dev)
        args = list(mk(H * D, D, o))
        args[15] = D - 8                                             # k_st below D
        assert _rc(name, *args) == EINVAL and "k token stride" in lib.last_error()
    o, lse = ops.attn_varlen(q, k, v, cu, cu, T, D ** -0.5, False, return_lse=True)
    do = _rand((T, H, D), dev, seed=4)
    delta = torch.empty(H * T, dtype=F32, device=dev)
    keep = []

    def bwd(bad):
        B = Bands(dev)
        g = B.out((T, 3 * H, D))

        def mk(dq_st):
            st = (C.c_int64 * 16)(*([H * D, D] * 5 + [dq_st, D, g.stride(0), D, g.stride(0), D]))
            keep.append(st)
            return (q, k, v, o, do, lse, g[:, :H], g[:, H:2 * H], g[:, 2 * H:], delta, cu, cu, 1, T, T, T, H, H, D, C.cast(st, C.c_void_p), D ** -0.5, 0, None, T)
        return B, mk(bad), mk(g.stride(0))

    _refused(dev, "rga3_attn_varlen_bwd", bwd, H * D - 8, "dq token stride")

    def rope_in(bad):
        B = Bands(dev)
        x = B.out((T, H, D), data=q)
        return B, (x, cos, sin, T, 0, H, D, bad, D), (x, cos, sin, T, 0, H, D, x.stride(0), D)

    _refused(dev, "rga3_rope_inplace", rope_in, H * D - 16, "x token stride")
    assert _rc("rga3_rope_inplace", q, cos, sin, T, 0, H, D, H * D, D - 16) == EINVAL and "x head stride" in lib.last_error()
    frames, nq, nk, Hh = 1, 4, 8, 2
    qq, kk = _rand((nq, Hh * 16), dev, seed=5), _rand((nk, Hh * 16), dev, seed=6)
    vt = _rand((Hh * 16, nk), dev, seed=7)

    def fewq(bad):
        B = Bands(dev)
        out = B.out((nq, Hh * 16))
        mk = lambda ld: (qq, Hh * 16, kk, Hh * 16, 16, vt, None, out, ld, frames, nq, nk, Hh, 0.25)
        return B, mk(bad), mk(out.stride(0))

    _refused(dev, "rga3_attn_fewq", fewq, Hh * 16 - 8, "out_stride")
    out = torch.empty((nq, Hh * 16), dtype=BF, device=dev)
    assert _rc("rga3_attn_fewq", qq, Hh * 16, kk, Hh * 16, 8, vt, None, out, Hh * 16, frames, nq, nk, Hh, 0.25) == EINVAL and "k_head_stride" in lib.last_error()


def test_head_major_layouts_stay_legal(dev):
    """The attention entry points take head-major [heads][tokens][D] operands: the head stride then spans the tokens and the token stride is D."""
    from rga3.hip import ops

    T, H, D = 40, 2, 32
    q, k, v = _rand((T, H, D), dev, seed=1), _rand((T, H, D), dev, seed=2), _rand((T, H, D), dev, seed=3)
    cu = torch.tensor([0, T], dtype=torch.int32, device=dev)
    want = ops.attn_varlen(q, k, v, cu, cu, T, D ** -0.5)
    hm = lambda t: t.permute(1, 0, 2).contiguous().permute(1, 0, 2)      # [T, H, D] values, strides (D, T * D, 1)
    got = ops.attn_varlen(hm(q), hm(k), hm(v), cu, cu, T, D ** -0.5)
    assert torch.equal(got, want)
