"""GPU parity tests of the individual HIP kernels (through the C ABI) against the fp32 oracle ops.

Tolerances: inputs are bf16-exact values, accumulation is fp32; outputs are bf16 => rel-L2 <= 1e-2 and
max-abs scaled by the output magnitude (bf16 kernels vs fp32 oracle rel-L2 <= 2e-2).
"""
import numpy as np
import pytest
import torch

from oracle import kernels_ref as R

pytestmark = pytest.mark.gpu


def _rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _rand(shape, dev, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def test_gemm_identity_asymmetric(dev):
    """A = I with an asymmetric W catches a transposed / mis-mapped C fragment layout."""
    from rga3.hip import ops

    for tile in (3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 20, 21, 22, 23, 26, 27, 28, 31, 32):
        n, k = 256, 256
        a = torch.eye(k, dtype=torch.bfloat16, device=dev)
        w = (torch.arange(n * k, dtype=torch.float32).reshape(n, k) % 251 - 125).to(torch.bfloat16).to(dev)
        out = ops.gemm(a, w, tile=tile)
        assert torch.equal(out.float().cpu(), w.float().cpu().t()), f"tile {tile}"


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (300, 200, 128), (2112, 512, 3584), (8192, 1280, 1280), (64, 3456, 1280),
                                   (17, 24, 64), (1000, 152064 // 16, 192)])
@pytest.mark.parametrize("tile", [-1, 3, 4, 5, 10, 11, 12, 13, 14, 20, 21, 22, 23, 26, 27, 28, 31, 32])
def test_gemm_plain(dev, M, N, K, tile):
    from rga3.hip import ops

    a, w = _rand((M, K), dev, seed=1), _rand((N, K), dev, 0.05, seed=2)
    out = ops.gemm(a, w, tile=tile)
    ref = R.linear_ref(a.cpu(), w.cpu())
    assert _rel_l2(out, ref) < 6e-3


@pytest.mark.parametrize("M,N,K,f32", [(2112, 128, 3584, False), (2112, 128, 512, False), (4160, 128, 3584, False), (100, 8, 1000, True), (333, 264, 2056, False),
                                       (64, 64, 128, False)])
def test_gemm_split64_skinny(dev, M, N, K, f32):
    """Tile 14 (64 x 64 tiles, K cut into grid.y slices, f32 slabs summed in slice order): LoRA's x A^T / dY B shapes, ragged K, f32 and strided outputs;
    equal to the unsplit 64 x 64 tiling up to the f32 re-association, and reproducible."""
    from rga3.hip import ops

    a, w = _rand((M, K), dev, seed=41), _rand((N, K), dev, 0.05, seed=42)
    odt = torch.float32 if f32 else torch.bfloat16
    buf = torch.zeros((M, N + 8), dtype=odt, device=dev)
    out = ops.gemm(a, w, out_dtype=odt, out=buf[:, :N], tile=14)
    again = ops.gemm(a, w, out_dtype=odt, tile=14)
    assert torch.equal(out, again) and float(buf[:, N:].abs().max()) == 0.0
    ref = ops.gemm(a, w, out_dtype=odt, tile=13)
    assert _rel_l2(out, ref.float().cpu()) < (1e-5 if f32 else 3e-3), (M, N, K)
    assert _rel_l2(out, R.linear_ref(a.cpu(), w.cpu())) < 6e-3
    # with a bias the split does not apply: the call runs as the plain 64 x 64 tiling
    bias = _rand((N,), dev, 0.5, seed=43)
    assert torch.equal(ops.gemm(a, w, bias=bias, out_dtype=odt, tile=14), ops.gemm(a, w, bias=bias, out_dtype=odt, tile=13))


@pytest.mark.parametrize("M,N,K,act,tile", [(4096, 1728, 576, "none", -1), (4096, 2304, 576, "gelu", 5), (3000, 432, 144, "none", 13), (2500, 1152, 288, "gelu", 3),
                                            (1000, 576, 576, "none", 20), (700, 48, 16, "none", -1), (513, 260, 72, "relu", 12), (65536, 1728, 576, "none", -1),
                                            (1030, 384, 1152, "none", -1), (37, 192, 576, "none", -1), (16389, 3456, 1152, "none", -1),
                                            (4100, 2304, 576, "gelu", 7), (4100, 1728, 576, "none", 6)])   # round 5: the shared-row statistics kernels (576 / 1152 channels), ragged row counts
def test_gemm_layernorm_folded(dev, M, N, K, act, tile):
    """LayerNorm folded into the consuming product (rga3_layernorm_stats + rga3_gemm_ln_bf16, Hiera norm1 -> qkv / norm2 -> fc1): against fp32 LayerNorm + linear
    (+ GELU) of the same bf16 operands, and against the un-folded kernels (ops.layernorm + ops.gemm); rows with a large common offset exercise the
    mean-times-column-sum cancellation."""
    import torch.nn.functional as F
    from rga3.hip import ops

    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 0.7 + torch.randn(M, 1, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    b = (torch.randn(N, generator=g) * 0.2).to(torch.bfloat16).to(dev)
    gamma = (1 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
    beta = (0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
    st = ops.layernorm_stats(x, 1e-6)
    xf = x.float().cpu()
    assert torch.allclose(st[:, 0].cpu(), xf.mean(1), atol=1e-5, rtol=1e-5)
    assert torch.allclose(st[:, 1].cpu(), torch.rsqrt(xf.var(1, unbiased=False) + 1e-6), atol=1e-5, rtol=2e-5)
    wf, colc, bf = ops.fold_layernorm(w, b, gamma, beta)
    out = ops.gemm_ln(x, st, wf, colc, bf, act=act, tile=tile)
    ref = F.layer_norm(xf, (K,), gamma.float().cpu(), beta.float().cpu(), 1e-6) @ w.float().cpu().t() + b.float().cpu()
    ref = F.gelu(ref) if act == "gelu" else (F.relu(ref) if act == "relu" else ref)
    unf = ops.gemm(ops.layernorm(x, gamma, beta, 1e-6), w, b, act=act)
    assert _rel_l2(out, ref) < 8e-3, (M, N, K, act, tile)
    assert _rel_l2(unf, ref) < 8e-3
    assert _rel_l2(out, unf.float().cpu()) < 8e-3


@pytest.mark.parametrize("M,N,K,tile", [(4096, 576, 576, 5), (4096, 576, 2304, 23), (65536, 576, 2304, -1), (3000, 1152, 4608, 20), (2500, 1152, 1152, 3),
                                        (1000, 144, 144, 13), (513, 264, 72, 12), (37, 192, 576, -1), (16389, 1152, 4608, -1)])
def test_layernorm_sums_out_of_the_producer_epilogue(dev, M, N, K, tile):
    """the residual-writing products of a Hiera block (x = shortcut + proj(attn), x = x + fc2(..); reference model/sam2.py:1085-1117) leave the
    LayerNorm statistics of the rows they write -- rga3_gemm_lnsum_bf16: (sum v, sum v^2) per row and tile column, f32, plain stores -- and the
    LayerNorm-folded consumer reads them (rga3_gemm_lnq_bf16) instead of the (mean, 1 / std) of a stand-alone pass over the rows (rga3_layernorm_stats).
    (1) the product itself is bit-identical to the plain kernel of the same tiling; (2) the partial sums add up to those of the bf16 rows written (f32 accumulation)
    and are bit-reproducible; (3) the consumer on the sums equals the consumer on layernorm_stats to bf16 rounding, and fp32 LayerNorm + linear to the
    tolerance of test_gemm_layernorm_folded; rows with a common offset of several standard deviations exercise E[x^2] - mean^2 (formed in f64)."""
    import torch.nn.functional as F
    from rga3.hip import ops

    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g)).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * (K ** -0.5)).to(torch.bfloat16).to(dev)
    b = (torch.randn(N, generator=g) * 0.2).to(torch.bfloat16).to(dev)
    res = (torch.randn(M, N, generator=g) * 0.7 + torch.randn(M, 1, generator=g) * 3.0).to(torch.bfloat16).to(dev)      # offset rows: |mean| ~ 3 sigma
    out, parts = ops.gemm_lnsum(a, w, b, residual=res, tile=tile)
    plain = ops.gemm(a, w, b, residual=res, tile=tile if tile != -1 else 12)
    if tile != -1:
        assert torch.equal(out, plain)
    else:
        assert _rel_l2(out, plain.float().cpu()) < 1e-2
    assert parts.dim() == 3 and parts.shape[0] == M and parts.shape[2] == 2
    of = out.double().cpu()
    s1, s2 = parts[:, :, 0].double().sum(1).cpu(), parts[:, :, 1].double().sum(1).cpu()     # f32 partials per tile column, summed exactly here
    assert float((s1 - of.sum(1)).abs().max()) <= 2e-5 * float(of.abs().sum(1).max())
    assert float((s2 - (of * of).sum(1)).abs().max()) <= 2e-5 * float((of * of).sum(1).max())
    out_b, parts_b = ops.gemm_lnsum(a, w, b, residual=res, tile=tile)
    assert torch.equal(out, out_b) and torch.equal(parts, parts_b)                  # no atomics: fixed combination order, the same bits
    sums = parts
    # consumer
    N2 = 3 * N if N % 8 == 0 else 64
    w2 = (torch.randn(N2, N, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    b2 = (torch.randn(N2, generator=g) * 0.2).to(torch.bfloat16).to(dev)
    gamma = (1 + 0.2 * torch.randn(N, generator=g)).to(torch.bfloat16).to(dev)
    beta = (0.1 * torch.randn(N, generator=g)).to(torch.bfloat16).to(dev)
    wf, colc, bf = ops.fold_layernorm(w2, b2, gamma, beta)
    for act in ("none", "gelu"):
        y_q = ops.gemm_ln(out, ops.LnSums(sums, 1e-6), wf, colc, bf, act=act)
        y_s = ops.gemm_ln(out, ops.layernorm_stats(out, 1e-6), wf, colc, bf, act=act)
        ref = F.layer_norm(out.float().cpu(), (N,), gamma.float().cpu(), beta.float().cpu(), 1e-6) @ w2.float().cpu().t() + b2.float().cpu()
        ref = F.gelu(ref) if act == "gelu" else ref
        assert _rel_l2(y_q, y_s.float().cpu()) < 3e-3, (M, N, K, act)
        assert _rel_l2(y_q, ref) < 8e-3, (M, N, K, act)


def test_gemm_stream_k_split_shapes(dev):
    """Tiles 22 / 32 (256- / 192-row stream-K) on shapes whose last round is split over K (1, 2 contributors per tile, ragged M): equal to the unsplit result up to
    the f32 re-association of the split tiles, reproducible run to run, and no slab wait ever timed out."""
    from rga3.hip import lib, ops

    for (M, N, K) in [(2112, 3584, 3584), (2112, 4608, 3584), (2000, 5120, 2048), (8192, 1280, 1280), (300, 70000 // 8 * 8, 512)]:
        a, w = _rand((M, K), dev, seed=11), _rand((N, K), dev, 0.05, seed=12)
        ref = ops.gemm(a, w, tile=20)
        for tl in (22, 32):
            o1 = ops.gemm(a, w, tile=tl)
            o2 = ops.gemm(a, w, tile=tl)
            assert torch.equal(o1, o2), (M, N, K, tl)
            assert _rel_l2(o1, ref.float().cpu()) < 1e-3, (M, N, K, tl)
    assert ops.gemm_stream_k_timeouts() == 0


@pytest.mark.parametrize("act", ["none", "gelu", "relu", "swiglu"])
@pytest.mark.parametrize("tile", [3, 4, 5, 10, 11, 12, 13, 20, 21, 22, 23, 26, 27, 28, 31, 32])
def test_gemm_epilogues(dev, act, tile):
    from rga3.hip import ops

    M, N, K = 520, 640, 192
    a, w = _rand((M, K), dev, seed=3), _rand((N, K), dev, 0.08, seed=4)
    bias = _rand((N,), dev, 0.5, seed=5)
    n_out = N // 2 if act == "swiglu" else N
    res = _rand((M, n_out), dev, seed=6)
    out = ops.gemm(a, w, bias=bias, residual=res, act=act, tile=tile)
    ref = R.linear_ref(a.cpu(), w.cpu(), bias.cpu(), res.cpu(), act)
    assert out.shape == (M, n_out)
    assert _rel_l2(out, ref) < 8e-3


@pytest.mark.parametrize("M,N,K,act,res", [(2112, 4736, 3584, "swiglu", False), (2112, 3584, 2368, "none", True), (320, 768, 192, "gelu", False), (4160, 1024, 1024, "none", True),
                                             (257, 512, 64, "relu", True), (2112, 9472, 512, "none", False)])
def test_gemm_ragged_last_tile_row(dev, M, N, K, act, res):
    """Tiles 27 / 26 (persistent 256 x 256 / + stream-K tail; a last tile row of <= 64 rows -- M = 2112 = 8 x 256 + 64, the LLM's M in configs[1] / [2] -- runs a
    quarter-work loop on three 40-KiB LDS stages, two such tiles scheduled as one unit): tile 27 has no K split and walks K in tile 21's order, so it is BIT-identical
    to tile 21 (padded rows and all); tile 26 is equal to rounding and identical run to run; both against the fp32 reference (the products the reference reaches through
    cuBLAS: HF modeling_qwen2_5_vl.py:211-321 gate | up, down via reference model/qwen_2_5_vl_sam2.py:182-200)."""
    from rga3.hip import ops

    a, w = _rand((M, K), dev, seed=61), _rand((N, K), dev, 0.05, seed=62)
    bias = _rand((N,), dev, 0.3, seed=63)
    n_out = N // 2 if act == "swiglu" else N
    r = _rand((M, n_out), dev, seed=64) if res else None
    ref21 = ops.gemm(a, w, bias=bias, residual=r, act=act, tile=21)
    for _ in range(3):
        assert torch.equal(ops.gemm(a, w, bias=bias, residual=r, act=act, tile=27), ref21)
    z = ops.gemm(a, w, bias=bias, residual=r, act=act, tile=26)
    for _ in range(3):
        assert torch.equal(ops.gemm(a, w, bias=bias, residual=r, act=act, tile=26), z)
    ref = R.linear_ref(a.cpu(), w.cpu(), bias.cpu(), r.cpu() if res else None, act)
    assert _rel_l2(z, ref) < 8e-3 and _rel_l2(ref21, ref) < 8e-3
    assert _rel_l2(z[M - 64:], ref[M - 64:]) < 8e-3          # the ragged rows by themselves
    if act == "swiglu":    # the training forward's pre-activation output rides in the same epilogue
        y27, pre27 = ops.gemm_swiglu_pre(a, w, bias, tile=27)
        y21, pre21 = ops.gemm_swiglu_pre(a, w, bias, tile=21)
        assert torch.equal(y27, y21) and torch.equal(pre27, pre21)
    assert ops.gemm_stream_k_timeouts() == 0


@pytest.mark.parametrize("M,N,K,act,res", [(2112, 4736, 3584, "swiglu", False), (520, 3584, 2368, "none", True), (320, 768, 192, "gelu", False), (4160, 1024, 64, "none", True),
                                             (257, 512, 128, "relu", True), (1000, 1000, 200, "none", False)])
def test_gemm_four_wave_tile(dev, M, N, K, act, res):
    """Tile 28 (256 x 256 on four waves: 128 x 128 wave blocks, accumulators in the AGPRs, MFMAs / fragment reads / LDS-DMA pieces in one hand-ordered stream, two
    barriers per K-tile): every element is summed in tile 20's K order, so the outputs are BIT-identical to tile 20 -- one, two, three K-tiles (prologue / tail forms),
    ragged M / N, every epilogue kind; K not a multiple of 64 runs as tile 20.  (The products the reference reaches through cuBLAS: HF modeling_qwen2_5_vl.py:211-321.)"""
    from rga3.hip import ops

    a, w = _rand((M, K), dev, seed=71), _rand((N, K), dev, 0.05, seed=72)
    bias = _rand((N,), dev, 0.3, seed=73)
    n_out = N // 2 if act == "swiglu" else N
    r = _rand((M, n_out), dev, seed=74) if res else None
    ref20 = ops.gemm(a, w, bias=bias, residual=r, act=act, tile=20)
    for _ in range(3):
        assert torch.equal(ops.gemm(a, w, bias=bias, residual=r, act=act, tile=28), ref20)
    ref = R.linear_ref(a.cpu(), w.cpu(), bias.cpu(), r.cpu() if res else None, act)
    assert _rel_l2(ref20, ref) < 8e-3


@pytest.mark.parametrize("M,N,K", [(2112, 1536, 512), (320, 520, 192), (577, 256, 64)])
def test_gemm_f32_output_on_the_round5_tilings(dev, M, N, K):
    """f32 output (bias only) through tiles 26 / 27 (ragged last tile row when M leaves <= 64 rows) and 28 (four waves): the tuner offers them for every product,
    f32-output ones included; equal to tile 20 (bit-identical for 27 / 28: same K order) and to the fp32 reference."""
    from rga3.hip import ops

    a, w, bias = _rand((M, K), dev, seed=91), _rand((N, K), dev, 0.05, seed=92), _rand((N,), dev, 0.3, seed=93)
    ref20 = ops.gemm(a, w, bias=bias, out_dtype=torch.float32, tile=20)
    ref = R.linear_ref(a.cpu(), w.cpu(), bias.cpu())
    assert ref20.dtype == torch.float32 and _rel_l2(ref20, ref) < 1e-3
    for tile in (27, 28):
        assert torch.equal(ops.gemm(a, w, bias=bias, out_dtype=torch.float32, tile=tile), ref20), tile
    z = ops.gemm(a, w, bias=bias, out_dtype=torch.float32, tile=26)
    assert _rel_l2(z, ref) < 1e-3 and torch.equal(z, ops.gemm(a, w, bias=bias, out_dtype=torch.float32, tile=26))


def test_gemm_colscale_and_pre_on_the_round5_tilings(dev):
    """Column scale + residual (ConvNeXt layer scale of the SAM2 memory encoder, reference model/sam2.py:2618-2655) and the SwiGLU pre-activation output through tiles
    27 / 28 on a ragged M: bit-identical to tiles 21 / 20."""
    from rga3.hip import ops

    M, N, K = 2112, 768, 256
    a, w, bias = _rand((M, K), dev, seed=95), _rand((N, K), dev, 0.05, seed=96), _rand((N,), dev, 0.3, seed=97)
    r, cs = _rand((M, N), dev, seed=98), _rand((N,), dev, 0.2, seed=99)
    ref = ops.gemm(a, w, bias=bias, residual=r, act="gelu", colscale=cs, tile=20)
    for tile in (27, 28):
        assert torch.equal(ops.gemm(a, w, bias=bias, residual=r, act="gelu", colscale=cs, tile=tile), ref), tile
    y20, pre20 = ops.gemm_swiglu_pre(a, w, bias, tile=20)
    for tile in (27, 28):
        y, pre = ops.gemm_swiglu_pre(a, w, bias, tile=tile)
        assert torch.equal(y, y20) and torch.equal(pre, pre20), tile


def test_gemm_f32_out_and_kpad(dev):
    from rga3.hip import ops

    M, N, K = 130, 72, 1176  # K not a multiple of 64 -> wrapper pads; N not a multiple of 8 -> scalar tail
    a, w = _rand((M, K), dev, seed=7), _rand((N, K), dev, 0.05, seed=8)
    out = ops.gemm(a, w, out_dtype=torch.float32)
    ref = R.linear_ref(a.cpu(), w.cpu())
    assert out.dtype == torch.float32 and _rel_l2(out, ref) < 1e-3
    out2 = ops.gemm(a, w)
    assert _rel_l2(out2, ref) < 6e-3


def test_gemm_rejects_bad_args(dev):
    from rga3.hip import lib, ops

    a, w = _rand((8, 64), dev), _rand((8, 64), dev)
    with pytest.raises(lib.Rga3Error):
        ops.gemm(a, w, out_dtype=torch.float32, act="gelu")
    with pytest.raises(lib.Rga3Error):
        ops.gemm(a.cpu(), w.cpu())


@pytest.mark.parametrize("tile", [-1, 3, 12, 5, 6, 20, 21, 22, 23, 26, 27, 28, 31, 32])
@pytest.mark.parametrize("shape", [(300, 320, 256), (2112, 1280, 1280)])
def test_gemm_rmsnorm_folded(dev, tile, shape):
    """RMSNorm folded into the products on either side (rga3_gemm_rms_bf16; HF Qwen2RMSNorm modeling_qwen2_5_vl.py:470-486 between o_proj / down_proj and
    q|k|v / gate|up).  Producer: x2 = a W_o^T + r leaves the row sums of squares of the bf16 rows it writes as 2^20 fixed-point integers (integer atomics:
    bit-identical run to run).  Consumer: (x2 (W diag(gamma))^T) / rms + b, plain and with the SwiGLU epilogue, against RMSNorm -> Linear in fp32."""
    from rga3.hip import ops

    M, N, K = shape
    a, wo, r = _rand((M, K), dev, seed=1), _rand((N, K), dev, 0.05, seed=2), _rand((M, N), dev, seed=3)
    sums = torch.zeros(M, dtype=torch.int64, device=dev)
    x2 = ops.gemm(a, wo, residual=r, tile=tile, rms_out=sums)
    assert torch.equal(x2, ops.gemm(a, wo, residual=r, tile=tile))            # the sums ride along: the product itself is unchanged
    ss_ref = (x2.double() ** 2).sum(1)
    assert ((sums.double() / 2 ** 20 - ss_ref).abs() / ss_ref).max().item() < 1e-5
    sums2 = torch.zeros_like(sums)
    ops.gemm(a, wo, residual=r, tile=tile, rms_out=sums2)
    assert torch.equal(sums, sums2)
    # consumer
    gamma = (1.0 + 0.3 * torch.randn(N, generator=torch.Generator().manual_seed(4))).to(torch.bfloat16).to(dev)
    eps = 1e-6
    N2 = 384
    w2, b2 = _rand((N2, N), dev, 0.05, seed=5), _rand((N2,), dev, seed=6)
    wf = (w2.float() * gamma.float()[None, :]).to(torch.bfloat16).contiguous()
    xf = x2.float()
    xn = (xf * torch.rsqrt((xf ** 2).mean(-1, keepdim=True) + eps)).to(torch.bfloat16).float() * gamma.float()     # HF: normalised rows rounded, then * weight
    xn = xn.to(torch.bfloat16).float()
    ref = xn @ w2.float().t() + b2.float()
    y = ops.gemm(x2, wf, b2, tile=tile, rms_in=(sums, N, eps))
    assert _rel_l2(y, ref) < 1e-2, (tile, shape)
    # SwiGLU epilogue on the interleaved gate / up pack (16-row blocks)
    g_w, u_w = w2[:192], w2[192:]
    pack = torch.stack([g_w.view(12, 16, N), u_w.view(12, 16, N)], 1).reshape(N2, N)
    packf = (pack.float() * gamma.float()[None, :]).to(torch.bfloat16).contiguous()
    gt, up = (xn @ g_w.float().t()).to(torch.bfloat16).float(), (xn @ u_w.float().t()).to(torch.bfloat16).float()
    ref_s = torch.nn.functional.silu(gt).to(torch.bfloat16).float() * up
    ys = ops.gemm(x2, packf, None, act="swiglu", tile=tile, rms_in=(sums, N, eps))
    assert _rel_l2(ys, ref_s) < 1.5e-2, (tile, shape)


@pytest.mark.parametrize("S,Hq,Hkv", [(2112, 28, 4), (300, 4, 2), (1000, 7, 1)])
def test_attn_causal32_rope_on_load(dev, S, Hq, Hkv):
    """Decoder prefill with the queries rotated as the causal attention kernel loads them (rga3_attn_varlen_fwd_rope -> attn_causal32_kernel; HF
    apply_multimodal_rotary_pos_emb modeling_qwen2_5_vl.py:557-599) against the stand-alone RoPE pass on q and k followed by the same kernel: the same f32 arithmetic and
    one bf16 rounding either way, so the outputs agree to bf16 rounding of the attention sums."""
    from rga3.hip import ops

    D = 128
    g = torch.Generator().manual_seed(S)
    qkv = torch.randn(S, Hq + 2 * Hkv, D, generator=g).to(torch.bfloat16).to(dev)
    pos = torch.arange(S, dtype=torch.float32)[:, None] * (10000.0 ** (-torch.arange(0, D // 2, dtype=torch.float32) / (D // 2)))[None, :]
    cos, sin = torch.cat([pos.cos(), pos.cos()], 1).contiguous().to(dev), torch.cat([pos.sin(), pos.sin()], 1).contiguous().to(dev)
    cu = torch.tensor([0, S], dtype=torch.int32, device=dev)
    a = qkv.clone()
    ops.rope_(a, cos, sin, 0, Hq + Hkv)
    ref = ops.attn_varlen(a[:, :Hq], a[:, Hq:Hq + Hkv], a[:, Hq + Hkv:], cu, cu, S, D ** -0.5, causal=True)
    b = qkv.clone()
    ops.rope_(b, cos, sin, Hq, Hkv)
    assert torch.equal(b[:, Hq:Hq + Hkv], a[:, Hq:Hq + Hkv]) and torch.equal(b[:, :Hq], qkv[:, :Hq])
    out = ops.attn_varlen_rope(b[:, :Hq], b[:, Hq:Hq + Hkv], b[:, Hq + Hkv:], cu, cu, S, D ** -0.5, cos, sin, causal=True)
    assert float((out.float() - ref.float()).abs().max()) < 2e-2 and _rel_l2(out, ref.float().cpu()) < 2e-3


def test_gemm_tn_many_equals_single_products(dev):
    """rga3_gemm_tn_many: the four LoRA weight-gradient products of a decoder layer (dA_q, dB_q, dA_v, dB_v; autograd of PEFT's lora_A / lora_B, reference
    train_joint.py:193-232) in one launch, bit-identical to rga3_gemm_tn_bf16 on each pair (same K split, same slab order), strided operands included.  K is a token
    count: the small products take K = 1000 (31.25 K-tiles of 32, below the 1024 at which the single form once began to split) and K = 1272 (K % 256 > 224: 39.75 K-tiles,
    5 slices of 8), where a second copy of the slice rule in the wrapper of the single form had drifted from the library's, beside K = 1024 where both agreed."""
    from rga3.hip import ops

    T, H, r = 2112, 3584, 128
    g = torch.Generator().manual_seed(5)
    dqkv = (torch.randn(T, 4608, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    h1, hv = _rand((T, H), dev, seed=6), _rand((T, H), dev, seed=7)
    tq, tv, dtq, dtv = _rand((T, r), dev, seed=8), _rand((T, r), dev, seed=9), _rand((T, r), dev, 0.1, seed=10), _rand((T, r), dev, 0.1, seed=11)
    pairs = [(dtq, h1), (dqkv[:, :3584], tq), (dtv, hv), (dqkv[:, 4096:], tv)]
    outs = ops.gemm_tn_many(pairs)
    for (a, b), o in zip(pairs, outs):
        assert torch.equal(o, ops.gemm_tn(a, b)), (a.shape, b.shape)
        assert _rel_l2(o, a.float().cpu().t() @ b.float().cpu()) < 6e-3
    o2 = ops.gemm_tn_many(pairs[:2], out_dtype=torch.float32)
    assert torch.equal(o2[1], ops.gemm_tn(pairs[1][0], pairs[1][1], out_dtype=torch.float32))
    o3 = ops.gemm_tn_many([(dtq[:, :20], h1)])          # ragged width: falls back to the single form
    assert o3[0].shape == (20, H)
    small = [(_rand((K, M), dev, seed=20 + i), _rand((K, N), dev, seed=30 + i)) for i, (K, M, N) in enumerate([(1000, 128, 128), (1272, 128, 128), (1272, 128, 256), (1024, 128, 128)])]
    for odt, tol in ((torch.bfloat16, 6e-3), (torch.float32, 2e-5)):
        for (a, b), o in zip(small, ops.gemm_tn_many(small, out_dtype=odt)):
            assert torch.equal(o, ops.gemm_tn(a, b, out_dtype=odt)), (a.shape, b.shape, odt)
            assert _rel_l2(o, a.float().cpu().t() @ b.float().cpu()) < tol, (a.shape, b.shape, odt)


def test_tuner_times_the_tilings_the_library_lists(dev, monkeypatch):
    """Which tilings a wrapper's first call times, and in which order (tuner.pick keeps the first of equal times): the literal lists of tests/test_gemm_tiles.py, read
    back from tuner.timings() -- the `extra` tilings of ops.gemm on both sides of their predicates, gemm_lnsum with and without the 256 x 192 tiling (M = 1024 / 1008),
    gemm_cat with an N side at a width only the 64-wide tiling divides.  The winner is passed on and accepted, a second call times nothing, and the result equals the
    tile = 12 one.  Bounds (rel-L2, both sides bf16 roundings of f32 sums that differ in summation order only): gemm 1e-3 as test_gemm_streamk_* against tile 20, 2e-3 for
    token rows (M <= 16) as test_gemm_token_rows against tile 12; gemm_swiglu_pre 1e-4 on the pre-activations as test_gemm_swiglu_with_preactivations, its activations as
    gemm; gemm_lnsum 1e-2 as test_layernorm_sums_out_of_the_producer_epilogue (tuned against 12); gemm_ln and gemm_cat have no tile-against-tile bound there: theirs are
    the main loops of gemm behind another epilogue, hence gemm's 1e-3 (gemm_cat against the two plain products it fuses, as test_gemm_concatenated_operands)."""
    from rga3.hip import ops, tuner

    monkeypatch.setattr(tuner, "_enabled", True)
    monkeypatch.setattr(tuner, "_forced", [None])
    base = [20, 21, 22, 27, 28, 31, 32, 12, 13, 3, 4, 5, 6]
    BF = 0

    def close(got, want, tol):
        got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
        tol = tol if isinstance(tol, tuple) else (tol,) * len(got)
        for g, w, t in zip(got, want, tol):
            assert _rel_l2(g, w.float().cpu()) < t, (t, _rel_l2(g, w.float().cpu()))

    def tuned(key, want, call, ref, tol):
        old = (tuner._cache.pop(key, None), tuner._times.pop(key, None))
        try:
            out = call()
            assert list(tuner.timings()[key]) == want, (key, list(tuner.timings()[key]))
            assert tuner.table()[key] in want
            n, times = len(tuner._times), tuner._times[key]
            call()
            assert len(tuner._times) == n and tuner._times[key] is times and list(times) == want       # nothing re-tuned
            close(out, ref(), tol)
        finally:
            for d, v in zip((tuner._cache, tuner._times), old):
                d.pop(key, None)
                if v is not None:
                    d[key] = v

    a, w = _rand((64, 4096), dev, seed=1), _rand((64, 4096), dev, 0.02, seed=2)
    tuned(tuner.key_of(64, 64, 4096, "none", BF, False, False), base + [25, 14], lambda: ops.gemm(a, w), lambda: ops.gemm(a, w, tile=12), 1e-3)
    a, w = _rand((16, 1024), dev, seed=3), _rand((1024, 1024), dev, 0.03, seed=4)
    tuned(tuner.key_of(16, 1024, 1024, "none", BF, False, False), base + [14, 41], lambda: ops.gemm(a, w), lambda: ops.gemm(a, w, tile=12), 2e-3)

    a, w = _rand((64, 1024), dev, seed=5), _rand((256, 1024), dev, 0.03, seed=6)

    def rms(tile):
        sums = torch.zeros(64, dtype=torch.int64, device=dev)
        out = ops.gemm(a, w, tile=tile, rms_out=sums)
        ss = (out.double() ** 2).sum(1)
        assert ((sums.double() / 2 ** 20 - ss).abs() / ss).max().item() < 1e-5      # the trial launches added nothing to the caller's row sums
        return out
    tuned(tuner.key_of(64, 256, 1024, "none", BF, False, False), base, lambda: rms(-1), lambda: rms(12), 1e-3)

    a, w, b = _rand((256, 256), dev, seed=7), _rand((256, 256), dev, 0.06, seed=8), _rand((256,), dev, 0.3, seed=9)
    tuned(tuner.key_of(256, 256, 256, "swiglu+pre", BF, True, False), base, lambda: ops.gemm_swiglu_pre(a, w, b), lambda: ops.gemm_swiglu_pre(a, w, b, tile=12), (1e-3, 1e-4))

    st = ops.layernorm_stats(a, 1e-6)
    gamma, beta = _rand((256,), dev, 0.2, seed=10) + 1, _rand((256,), dev, 0.1, seed=11)
    wf, colc, bfold = ops.fold_layernorm(w, b, gamma, beta)
    tuned(tuner.key_of(256, 256, 256, "ln+gelu", BF, True, False), [20, 3, 5, 12, 13, 6, 7], lambda: ops.gemm_ln(a, st, wf, colc, bfold, act="gelu"),
          lambda: ops.gemm_ln(a, st, wf, colc, bfold, act="gelu", tile=12), 1e-3)

    w = _rand((576, 64), dev, 0.12, seed=12)

    def lnsum(tile):
        out, parts = ops.gemm_lnsum(a, w, tile=tile)
        of = out.double().cpu()
        assert float((parts[:, :, 0].double().sum(1).cpu() - of.sum(1)).abs().max()) <= 2e-5 * float(of.abs().sum(1).max())      # the partial sums are those of the tiling that ran
        return out
    for M, want in ((1024, [20, 3, 5, 12, 13, 23]), (1008, [20, 3, 5, 12, 13])):      # one key (M in buckets of 256): dropped before each
        a = _rand((M, 64), dev, seed=13)
        tuned(tuner.key_of(M, 576, 64, "lnsum", BF, False, False), want, lambda: lnsum(-1), lambda: lnsum(12), 1e-2)

    dy, wt, wn = _rand((256, 64), dev, seed=14), _rand((576, 64), dev, 0.12, seed=15), _rand((64, 64), dev, 0.12, seed=16)
    tuned(tuner.key_of(256, 576 + 64, 64, "cat", BF, False, False), [13], lambda: ops.gemm_cat(dy, wt, wn=wn), lambda: (ops.gemm(dy, wt, tile=12), ops.gemm(dy, wn, tile=12)), 1e-3)


@pytest.mark.parametrize("tile", [-1, 3, 6, 12, 13])
def test_gemm_concatenated_operands(dev, tile):
    """rga3_gemm_cat_bf16 (LoRA's low-rank products folded into the frozen products; PEFT LoRA layer, reference train_joint.py:193-232): the K side
    [a | a2] [w | w2]^T + bias against fp32 and against the two-launch form; the N side's second output bit-identical to a plain product of the same tiling, the first
    output untouched by it; both sides at once; on a grid of several tiles per CU."""
    from rga3.hip import ops

    T, H, Nq, r2 = 2112, 3584, 4608, 256
    h, tt = _rand((T, H), dev, seed=1), _rand((T, r2), dev, 0.3, seed=2)
    w, w2, b = _rand((Nq, H), dev, 0.03, seed=3), _rand((Nq, r2), dev, 0.05, seed=4), _rand((Nq,), dev, 0.3, seed=5)
    ref = h.float().cpu() @ w.float().cpu().t() + tt.float().cpu() @ w2.float().cpu().t() + b.float().cpu()
    out = ops.gemm_cat(h, w, b, a2=tt, w2=w2, tile=tile)
    assert _rel_l2(out, ref) < 6e-3
    assert torch.equal(out, ops.gemm_cat(h, w, b, a2=tt, w2=w2, tile=tile))
    two = ops.gemm(tt, w2, residual=ops.gemm(h, w, b))                       # the form it replaces (one more bf16 rounding)
    assert _rel_l2(out, two.float().cpu()) < 6e-3
    # N side: dX-type product with 256 extra output columns from a second weight
    dy = _rand((T, Nq), dev, 0.2, seed=6)
    wt, wn = _rand((H, Nq), dev, 0.03, seed=7), _rand((r2, Nq), dev, 0.05, seed=8)
    dx, dt = ops.gemm_cat(dy, wt, wn=wn, tile=tile)
    t_plain = tile if tile != -1 else 12
    assert torch.equal(dx, ops.gemm(dy, wt, tile=t_plain)) and torch.equal(dt, ops.gemm(dy, wn, tile=t_plain))
    # strided second operands (column halves of one buffer) and both sides at once
    buf = _rand((T, 2 * r2), dev, 0.3, seed=9)
    o1, o2 = ops.gemm_cat(h, w[:H], a2=buf[:, r2:], w2=w2[:H], wn=wn[:, :H].contiguous(), tile=tile)
    assert _rel_l2(o1, h.float().cpu() @ w[:H].float().cpu().t() + buf[:, r2:].float().cpu() @ w2[:H].float().cpu().t()) < 6e-3
    assert _rel_l2(o2, h.float().cpu() @ wn[:, :H].float().cpu().t()) < 6e-3


@pytest.mark.parametrize("tile", [-1, 3, 12, 20, 21, 22, 31])
def test_gemm_swiglu_with_preactivations(dev, tile):
    """rga3_gemm_swiglu_pre_bf16: the SwiGLU product that also stores the rounded gate | up pre-activations (training forward of HF Qwen2MLP): the pre-activations are
    bit-identical to the plain product on the same packed weight, the activation output to the SwiGLU product without the second output and (up to the f32 rounding of
    the activation) to swiglu_fwd on the pre-activations; ragged M."""
    from rga3.hip import ops

    M, N, K = 2100, 1024, 512
    a, w, b = _rand((M, K), dev, seed=1), _rand((N, K), dev, 0.05, seed=2), _rand((N,), dev, 0.3, seed=3)
    act, pre = ops.gemm_swiglu_pre(a, w, b, tile=tile)
    t_plain = tile if tile != -1 else 12
    assert torch.equal(pre, ops.gemm(a, w, b, tile=t_plain)) or _rel_l2(pre, ops.gemm(a, w, b, tile=t_plain).float().cpu()) < 1e-4      # stream-K tilings re-associate
    assert torch.equal(act, ops.gemm(a, w, b, act="swiglu", tile=tile)) or tile == -1
    ref = ops.swiglu_fwd(pre)
    assert _rel_l2(act, ref.float().cpu()) < 2e-3 and float((act.float() - ref.float()).abs().max()) < 0.05


def _all_bf16_finite(dev):
    bits = torch.arange(0, 65536, dtype=torch.int32)
    bits = bits[(bits & 0x7f80) != 0x7f80]                       # no Inf / NaN
    return bits.to(torch.int16).view(torch.bfloat16).to(dev)


@pytest.mark.parametrize("tile", [-1, 3, 20, 21])
def test_gemm_epilogue_activation_tables_every_bf16_input(dev, tile):
    """GELU / SiLU of the tile epilogues are table-driven on the bf16-rounded linear output (csrc/act_tables.inc, tools/gen_act_tables.py): every finite bf16 value
    goes through a product that reproduces it exactly (one-hot weights) and must come out as the correctly rounded exact-erf GELU (reference nn.GELU(), model/sam2.py
    MLP :2305-2329) resp. silu(gate) * up with up = 1 (HF Qwen2MLP) -- inside the tabulated range [2^-14, 2^6) bit for bit against float64, outside it within one bf16
    ulp / 1e-25 absolute."""
    from rga3.hip import ops

    t = _all_bf16_finite(dev)
    M = (t.numel() + 255) // 256 * 256
    K = 64
    a = torch.zeros((M, K), dtype=torch.bfloat16, device=dev)
    a[:t.numel(), 0] = t
    td = a[:, 0].double().cpu()
    inside = (td.abs() >= 2.0 ** -14) & (td.abs() < 63.75)      # the last entry (63.75) is 0: it also serves every larger magnitude

    def check(out, ref64, what):
        ref = ref64.to(torch.bfloat16)
        o = out.cpu()
        same = o.view(torch.int16) == ref.view(torch.int16)
        both_zero = (o.float() == 0) & (ref.float() == 0)
        bad_in = (~(same | both_zero)) & inside
        assert int(bad_in.sum()) == 0, (what, tile, td[bad_in][:5], o[bad_in][:5], ref[bad_in][:5])
        err = (o.double() - ref64).abs()
        assert bool((err[~inside] <= 2.0 ** -8 * ref64.abs()[~inside] + 1e-25).all()), (what, tile)

    # GELU: 16 output columns, all the identity
    w = torch.zeros((256, K), dtype=torch.bfloat16, device=dev)
    w[:, 0] = 1
    out = ops.gemm(a, w, act="gelu", tile=tile)
    check(out[:, 3], 0.5 * td * torch.erfc(-td / 2 ** 0.5), "gelu")
    check(out[:, 200], 0.5 * td * torch.erfc(-td / 2 ** 0.5), "gelu")
    # SwiGLU: interleaved 16-row blocks of gate | up; gate = t, up = 1 (a second input column of ones)
    a[:, 1] = 1
    wg = torch.zeros((512, K), dtype=torch.bfloat16, device=dev)
    blocks = wg.view(16, 2, 16, K)
    blocks[:, 0, :, 0] = 1      # gate rows pick t
    blocks[:, 1, :, 1] = 1      # up rows pick 1
    outs = ops.gemm(a, wg, act="swiglu", tile=tile)
    silu = td / (1.0 + torch.exp(-td))
    silu = torch.where(td < -700, torch.zeros_like(td), silu)
    check(outs[:, 5], silu, "silu")
    check(outs[:, 250], silu, "silu")


@pytest.mark.parametrize("tile", [-1, 5, 12, 23])
def test_gemm_epilogues_two_workgroups_per_cu(dev, tile):
    """The epilogue variants on grids of MORE than one workgroup per CU (the 64- / 80-KiB tilings co-reside): a packed-f32 form of the LayerNorm fold lost its product
    term in a few waves only when two workgroups shared a CU -- every epilogue kind is therefore also checked at M = 8192 rows, three runs
    each, bit-identical run to run and against fp32."""
    import torch.nn.functional as F
    from rga3.hip import ops

    M, N, K = 8192, 1152, 320
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(M, K, generator=g) * 0.7 + torch.randn(M, 1, generator=g)).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    b = (torch.randn(N, generator=g) * 0.2).to(torch.bfloat16).to(dev)
    r = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev)
    gamma = (1 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
    beta = (0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
    xf, wf32, bf32 = x.float().cpu(), w.float().cpu(), b.float().cpu()

    def runs(fn, ref, tol, what):
        outs = [fn() for _ in range(3)]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (what, tile)
        assert _rel_l2(outs[0], ref) < tol, (what, tile)

    lin = xf @ wf32.t() + bf32
    runs(lambda: ops.gemm(x, w, b, tile=tile), lin, 6e-3, "bias")
    runs(lambda: ops.gemm(x, w, b, residual=r, tile=tile), lin.to(torch.bfloat16).float() + r.float().cpu(), 6e-3, "bias+residual")
    runs(lambda: ops.gemm(x, w, b, act="gelu", tile=tile), F.gelu(lin.to(torch.bfloat16).float()), 8e-3, "gelu")
    if tile != 5:     # 192-wide tiles hold three n-tiles per wave: no gate / up pairs
        gt, up = lin[:, :N // 2], lin[:, N // 2:]
        pack = torch.stack([w[:N // 2].view(-1, 16, K), w[N // 2:].view(-1, 16, K)], 1).reshape(N, K).contiguous()
        bp = torch.stack([b[:N // 2].view(-1, 16), b[N // 2:].view(-1, 16)], 1).reshape(N).contiguous()
        ref_s = F.silu(gt.to(torch.bfloat16).float()).to(torch.bfloat16).float() * up.to(torch.bfloat16).float()
        runs(lambda: ops.gemm(x, pack, bp, act="swiglu", tile=tile), ref_s, 1e-2, "swiglu")
    # LayerNorm folded in
    st = ops.layernorm_stats(x, 1e-6)
    wfold, colc, bfold = ops.fold_layernorm(w, b, gamma, beta)
    ln = F.layer_norm(xf, (K,), gamma.float().cpu(), beta.float().cpu(), 1e-6) @ wf32.t() + bf32
    if tile != 23:    # rga3_gemm_ln_bf16 has no 256 x 192 form
        runs(lambda: ops.gemm_ln(x, st, wfold, colc, bfold, act="none", tile=tile), ln, 8e-3, "ln")
        runs(lambda: ops.gemm_ln(x, st, wfold, colc, bfold, act="gelu", tile=tile), F.gelu(ln), 8e-3, "ln+gelu")
    # RMSNorm folded in (consumer side) with the producer's sums
    sums = torch.zeros(M, dtype=torch.int64, device=dev)
    x2 = ops.gemm(x, torch.eye(K, dtype=torch.bfloat16, device=dev), tile=tile, rms_out=sums)
    assert torch.equal(x2, x)
    wg = (w.float() * gamma.float()[None, :]).to(torch.bfloat16).contiguous()
    xn = (xf * torch.rsqrt((xf ** 2).mean(-1, keepdim=True) + 1e-6)).to(torch.bfloat16).float() * gamma.float().cpu()
    ref_r = xn.to(torch.bfloat16).float() @ wf32.t() + bf32
    runs(lambda: ops.gemm(x, wg, b, tile=tile, rms_in=(sums, K, 1e-6)), ref_r, 1e-2, "rms")


ATTN_CASES = [
    # (seglens_q, seglens_k, Hq, Hkv, D, causal)
    ([64] * 6, None, 4, 4, 80, False),            # ViT windows
    ([1024, 1024], None, 2, 2, 80, False),        # ViT full-attention segments
    ([300, 77, 1], None, 4, 2, 128, True),        # causal GQA, ragged
    ([2112], None, 7, 1, 128, True),              # LLM shape, one KV head group
    ([256, 256], None, 2, 2, 72, False),          # Hiera window
    ([9], [4096], 8, 8, 16, False),               # two-way decoder token->image
    ([4096], [9], 8, 8, 16, False),               # image->token
    ([9], [9], 8, 8, 32, False),
    ([512], [1500], 1, 1, 256, False),            # memory attention, 1 head x 256
    ([5], [133], 2, 2, 64, True),                 # causal with Lk > Lq (decode-style)
    ([1024], [7000], 1, 1, 256, False),           # memory attention over a grown bank: key range split over workgroups
    ([100, 700], [3000, 1200], 2, 2, 64, False),  # split-KV with ragged segments (second segment shorter than a slice set)
    ([640, 129, 1000], None, 6, 2, 128, True),    # paired causal q-blocks, ragged tails, GQA
    ([4096], None, 8, 8, 72, False),              # Hiera-L global attention at full length
    ([1024, 1024, 700, 300], None, 4, 2, 80, False),   # long ragged segments, GQA, head dim 80
    ([512, 256], None, 2, 2, 96, False),          # head dim 96
    ([600], None, 2, 2, 40, False),               # head dim 40
    ([2048], None, 2, 1, 64, False),              # head dim 64, two query heads on one kv head
    ([200], [457], 3, 3, 64, True),               # ... causal with Lk > Lq, one unpaired block pair
    ([333, 128], None, 2, 2, 96, False),          # ... head dim 96, non-causal, ragged
    ([130], [64], 2, 1, 32, False),               # ... a single key tile, D = 32 (padded to 64)
]


@pytest.mark.parametrize("case", ATTN_CASES)
@pytest.mark.parametrize("impl", [0, 1])
def test_attn_varlen(dev, case, impl):
    from rga3.hip import ops

    lq, lk, Hq, Hkv, D, causal = case
    lk = lk or lq
    cu_q = torch.tensor([0] + list(torch.tensor(lq).cumsum(0)), dtype=torch.int32)
    cu_k = torch.tensor([0] + list(torch.tensor(lk).cumsum(0)), dtype=torch.int32)
    Tq, Tk = int(cu_q[-1]), int(cu_k[-1])
    # q/k/v as slices of one fused buffer when shapes allow (exercises strides)
    q = _rand((Tq, Hq, D), dev, seed=11)
    kv = _rand((Tk, 2, Hkv, D), dev, seed=12)
    k, v = kv[:, 0], kv[:, 1]
    scale = D ** -0.5
    out, lse = ops.attn_varlen(q, k, v, cu_q.to(dev), cu_k.to(dev), max(lq), scale, causal, return_lse=True, impl=impl, max_k=max(lk))
    ref, lse_ref = R.attn_varlen_ref(q.cpu(), k.cpu(), v.cpu(), cu_q, cu_k, scale, causal)
    assert _rel_l2(out, ref) < 1e-2, (case, impl)
    assert (lse.cpu() - lse_ref).abs().max().item() < 2e-2


CAUSAL32_CASES = [
    # (seglens_q, seglens_k, Hq, Hkv): causal, D = 128, longest segment >= 256 rows -> attn_causal32_kernel (32-row waves, key range of the heavy block split over
    # the light block's waves, partial results merged in LDS)
    ([2112], None, 28, 4),                 # the decoder's rows of the bench (17 blocks of 128: 8 pairs + the unpaired middle block; last block 64 rows)
    ([256], None, 2, 1),                   # two blocks: one pair, nothing to split (kH - c = 1)
    ([257], None, 2, 2),                   # three blocks, the last one a single row
    ([385, 1, 700], None, 4, 2),           # ragged segments incl. a one-token segment (grid sized by the longest)
    ([300], [900], 2, 1),                  # Lk > Lq (prefill against a cache): every row sees >= 601 keys
    ([1000], [1037], 3, 3),                # shift not a multiple of the tile
    ([4160], None, 4, 2),                  # config-5 length (33 blocks)
    ([128, 640, 129, 1000, 512], None, 6, 2),
]


@pytest.mark.parametrize("case", CAUSAL32_CASES)
def test_attn_causal32(dev, case):
    """Long causal rows at D = 128 (csrc/attn_causal32.hip; HF modeling_qwen2_5_vl.py:602-700 through flash-attn varlen causal): against the fp32 softmax oracle at
    the stated 1e-2 / 2e-2, against the general kernel it replaces (impl = 4 keeps that one), run-to-run bit-identical."""
    from rga3.hip import ops

    lq, lk, Hq, Hkv = case
    lk = lk or lq
    D = 128
    cu_q = torch.tensor([0] + list(torch.tensor(lq).cumsum(0)), dtype=torch.int32)
    cu_k = torch.tensor([0] + list(torch.tensor(lk).cumsum(0)), dtype=torch.int32)
    Tq, Tk = int(cu_q[-1]), int(cu_k[-1])
    q = _rand((Tq, Hq, D), dev, seed=21)
    kv = _rand((Tk, 2, Hkv, D), dev, seed=22)
    k, v = kv[:, 0], kv[:, 1]
    scale = D ** -0.5
    out, lse = ops.attn_varlen(q, k, v, cu_q.to(dev), cu_k.to(dev), max(lq), scale, True, return_lse=True, max_k=max(lk))
    ref, lse_ref = R.attn_varlen_ref(q.cpu(), k.cpu(), v.cpu(), cu_q, cu_k, scale, True)
    assert _rel_l2(out, ref) < 1e-2, case
    assert (lse.cpu() - lse_ref).abs().max().item() < 2e-2
    old, lse_old = ops.attn_varlen(q, k, v, cu_q.to(dev), cu_k.to(dev), max(lq), scale, True, return_lse=True, max_k=max(lk), impl=4)
    assert _rel_l2(out, old.float().cpu()) < 6e-3 and (lse - lse_old).abs().max().item() < 1e-3
    again, lse2 = ops.attn_varlen(q, k, v, cu_q.to(dev), cu_k.to(dev), max(lq), scale, True, return_lse=True, max_k=max(lk))
    assert torch.equal(out, again) and torch.equal(lse, lse2)


def test_attn_causal32_output_view_alignment(dev):
    """attn_causal32_kernel stores 16-byte row pieces; an output view that is only 8-byte aligned (legal for rga3_attn_varlen_fwd: o & 7 == 0, strides
    multiples of 4) must stay on the general kernel -- same values as that kernel on an aligned output, bit for bit -- and the rope entry, which has no other kernel for
    these rows, must refuse it."""
    from rga3.hip import ops

    S, Hq, Hkv, D = 512, 4, 2, 128
    q, kv = _rand((S, Hq, D), dev, seed=31), _rand((S, 2, Hkv, D), dev, seed=32)
    k, v = kv[:, 0], kv[:, 1]
    cu = torch.tensor([0, S], dtype=torch.int32, device=dev)
    want = ops.attn_varlen(q, k, v, cu, cu, S, D ** -0.5, True, impl=4)                   # general kernel, aligned output
    buf = torch.zeros(S * Hq * D + 8, dtype=torch.bfloat16, device=dev)
    view = buf[4:4 + S * Hq * D].view(S, Hq, D)                                           # 8-byte aligned, not 16
    assert view.data_ptr() % 16 == 8
    got = ops.attn_varlen(q, k, v, cu, cu, S, D ** -0.5, True, out=view)
    assert torch.equal(got, want)
    assert float(buf[:4].float().abs().sum()) == 0.0 and float(buf[-4:].float().abs().sum()) == 0.0
    pos = torch.arange(S, dtype=torch.float32)[:, None] * (10000.0 ** (-torch.arange(0, D // 2, dtype=torch.float32) / (D // 2)))[None, :]
    cos, sin = torch.cat([pos.cos(), pos.cos()], 1).contiguous().to(dev), torch.cat([pos.sin(), pos.sin()], 1).contiguous().to(dev)
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.attn_varlen_rope(q, k, v, cu, cu, S, D ** -0.5, cos, sin, causal=True, out=view)


def test_attn_causal32_rescale_branch(dev):
    """The online-softmax rescale fires only when a later tile raises a row's maximum (cdna_hip_programming.md 5.4 rule 26: a rare data-dependent branch needs an
    input that FORCES it).  Keys far down the row are aligned with their queries and scaled up, so the maximum of most rows jumps in the LAST tiles -- in group A's
    range for some rows, in group B's range (the merged partial) for others."""
    from rga3.hip import ops

    S, Hq, Hkv, D = 1536, 2, 1, 128
    g = torch.Generator().manual_seed(5)
    q = torch.randn(S, Hq, D, generator=g)
    k = torch.randn(S, Hkv, D, generator=g) * 0.3
    v = torch.randn(S, Hkv, D, generator=g)
    for i in range(64, S, 7):            # key i - 3 points along query i of head 0: a late, large score (visible: i - 3 <= i)
        k[i - 3, 0] = q[i, 0] * 1.5
    for i in range(700, S, 5):           # and an early one for other rows, so both key halves of a split row carry a spike somewhere
        k[i // 3, 0] = q[i, 1] * 1.2
    q, k, v = (t.to(torch.bfloat16).to(dev) for t in (q, k, v))
    cu = torch.tensor([0, S], dtype=torch.int32)
    out, lse = ops.attn_varlen(q, k, v, cu.to(dev), cu.to(dev), S, D ** -0.5, True, return_lse=True)
    ref, lse_ref = R.attn_varlen_ref(q.cpu(), k.cpu(), v.cpu(), cu, cu, D ** -0.5, True)
    assert _rel_l2(out, ref) < 1e-2
    assert (out.float().cpu() - ref).abs().max().item() < 6e-2
    assert (lse.cpu() - lse_ref).abs().max().item() < 2e-2


@pytest.mark.parametrize("case", [([64] * 12, 16, 16, 80, False), ([64, 17, 40], 4, 2, 64, False), ([33] * 3, 2, 2, 128, True), ([16] * 5, 2, 1, 32, False)])
@pytest.mark.parametrize("rope_k", [True, False])
def test_attn_rope_windows_fused(dev, case, rope_k):
    """Windowed attention with RoPE applied while q (and k) are loaded (rga3_attn_varlen_fwd_rope) == rope pass over q and k, then attention: same
    values (the rotation is the rope kernel's arithmetic with one bf16 rounding), and against the oracle's rotate-half + exact softmax attention;
    longer segments are rejected."""
    from rga3.hip import lib, ops

    lens, Hq, Hkv, D, causal = case
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    T = int(cu[-1])
    qkv = _rand((T, Hq + 2 * Hkv, D), dev, seed=21)
    pos = torch.cat([torch.arange(n) for n in lens]).float()
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = pos[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    cos, sin = emb.cos().contiguous().to(dev), emb.sin().contiguous().to(dev)
    a = qkv.clone()
    ops.rope_(a, cos, sin, 0, Hq + Hkv)
    ref_o, ref_lse = ops.attn_varlen(a[:, :Hq], a[:, Hq:Hq + Hkv], a[:, Hq + Hkv:], cu.to(dev), cu.to(dev), max(lens), D ** -0.5, causal, return_lse=True)
    b = qkv.clone()
    if not rope_k:
        ops.rope_(b, cos, sin, Hq, Hkv)
    o, lse = ops.attn_varlen_rope(b[:, :Hq], b[:, Hq:Hq + Hkv], b[:, Hq + Hkv:], cu.to(dev), cu.to(dev), max(lens), D ** -0.5, cos, sin, causal, rope_k=rope_k,
                                  return_lse=True)
    assert _rel_l2(o, ref_o) < 2e-3 and (lse - ref_lse).abs().max().item() < 1e-3
    qf = qkv.float().cpu()
    rot = lambda x: torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    c, s_ = emb.cos()[:, None], emb.sin()[:, None]
    qr = (qf[:, :Hq] * c + rot(qf[:, :Hq]) * s_).to(torch.bfloat16).float()
    kr = (qf[:, Hq:Hq + Hkv] * c + rot(qf[:, Hq:Hq + Hkv]) * s_).to(torch.bfloat16).float()
    ro, _ = R.attn_varlen_ref(qr, kr, qf[:, Hq + Hkv:], cu, cu, D ** -0.5, causal)
    assert _rel_l2(o, ro) < 1e-2
    with pytest.raises(lib.Rga3Error):
        ops.attn_varlen_rope(b[:, :Hq], b[:, Hq:Hq + Hkv], b[:, Hq + Hkv:], cu.to(dev), cu.to(dev), 65, D ** -0.5, cos, sin, causal, rope_k=rope_k)


@pytest.mark.parametrize("lq,lk,Hq,Hkv,D,block", [
    ([256] * 6, [256] * 6, 8, 8, 72, None),            # Hiera stage 3: 16 x 16 windows, 8 heads x 72
    ([64] * 20, [64] * 20, 2, 2, 72, None),            # Hiera stage 1 / 4: 8 x 8 windows
    ([64] * 9, [64] * 9, 16, 16, 80, None),            # ViT windows (grad-enabled path: rope applied beforehand)
    ([64] * 5, [256] * 5, 4, 4, 72, None),             # pooled queries against the un-pooled window
    ([256, 100, 7, 200, 129], [256, 100, 7, 200, 129], 3, 3, 64, None),   # ragged segments, partial last key tile, idle waves
    ([130, 64], [190, 33], 4, 2, 32, None),            # GQA, Lq != Lk, D = 32 (padded to 64)
    ([64] * 6, [64] * 6, 4, 4, 72, (16, 16)),          # 16-token windows packed four to a segment, block-diagonal visibility
    ([16] * 6, [64] * 6, 4, 4, 72, (4, 16)),           # 4 pooled queries x 16 keys per packed window
])
def test_attn_window_kernel(dev, lq, lk, Hq, Hkv, D, block):
    """Whole-segment-in-LDS window kernel (taken when max_k <= 256 is passed, non-causal): vs the softmax oracle, vs the pipelined kernel (impl=2 keeps it),
    with q / k / v as slices of one packed qkv buffer (the layout the models hand over) and with the log-sum-exp output."""
    from rga3.hip import ops

    Tq, Tk = sum(lq), sum(lk)
    same = lq == lk
    if same:
        buf = _rand((Tq, Hq + 2 * Hkv, D), dev, 0.8, seed=5)
        q, k, v = buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]
    else:
        q, k, v = _rand((Tq, Hq, D), dev, 0.8, seed=5), _rand((Tk, Hkv, D), dev, 0.8, seed=6), _rand((Tk, Hkv, D), dev, 0.8, seed=7)
    cu_q = torch.tensor([0] + list(np.cumsum(lq)), dtype=torch.int32)
    cu_k = torch.tensor([0] + list(np.cumsum(lk)), dtype=torch.int32)
    scale = D ** -0.5
    out, lse = ops.attn_varlen(q, k, v, cu_q.to(dev), cu_k.to(dev), max(lq), scale, causal=False, return_lse=True, block=block, max_k=max(lk))
    old = ops.attn_varlen(q, k, v, cu_q.to(dev), cu_k.to(dev), max(lq), scale, causal=False, block=block, max_k=max(lk), impl=2)
    assert _rel_l2(out, old.float().cpu()) < 4e-3
    if block is None:
        ref, rlse = R.attn_varlen_ref(q.cpu(), k.cpu(), v.cpu(), cu_q, cu_k, scale, False)
    else:   # block-diagonal visibility = independent windows of (block_q queries, block_k keys)
        bq, bk = block
        nb = Tq // bq
        cq = torch.arange(0, (nb + 1) * bq, bq, dtype=torch.int32)
        ck = torch.arange(0, (nb + 1) * bk, bk, dtype=torch.int32)
        ref, rlse = R.attn_varlen_ref(q.cpu(), k.cpu(), v.cpu(), cq, ck, scale, False)
    assert _rel_l2(out, ref) < 8e-3
    assert float((lse.float().cpu() - rlse).abs().max()) < 2e-2


@pytest.mark.parametrize("nwin,H,qscale", [(6, 8, 0.8), (70, 8, 0.8), (33, 3, 6.0), (300, 8, 2.0)])
def test_attn_window256_rows32(dev, nwin, H, qscale):
    """Hiera-L stage-3 windows (16 x 16 tokens, heads of 72; reference model/sam2.py:986-1033): 256-query windows at D > 64 run ONE 8-wave workgroup per window and
    head with 32 query rows per wave (attn_win_kernel<96, 8, 2, false, 5>: each K / V fragment read from LDS feeds two MFMAs, the output spans 5 of the 6 sixteen-column
    tiles).  Against the softmax oracle, against the 16-row form (impl 8), with the log-sum-exp, peaked scores (running-max rescale in every tile); bit-reproducible."""
    from rga3.hip import ops

    D, T = 72, 256 * nwin
    buf = _rand((T, 3 * H, D), dev, 0.8, seed=nwin)
    q, k, v = (buf[:, :H] * qscale).to(torch.bfloat16), buf[:, H:2 * H], buf[:, 2 * H:]
    qkv = torch.cat([q, k, v], 1).contiguous()                      # packed rows, as the model hands them over
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    cu = torch.arange(0, T + 1, 256, dtype=torch.int32)
    cud = cu.to(dev)
    scale = D ** -0.5
    out, lse = ops.attn_varlen(q, k, v, cud, cud, 256, scale, causal=False, return_lse=True, max_k=256)
    again = ops.attn_varlen(q, k, v, cud, cud, 256, scale, causal=False, max_k=256)
    assert torch.equal(out, again)
    o16 = ops.attn_varlen(q, k, v, cud, cud, 256, scale, causal=False, max_k=256, impl=8)
    assert _rel_l2(out, o16.float().cpu()) < 4e-3
    n = min(nwin, 40)                                                # the oracle on the first and the last windows
    for sl in (slice(0, 256 * n), slice(T - 256 * n, T)):
        ref, rlse = R.attn_varlen_ref(q[sl].cpu(), k[sl].cpu(), v[sl].cpu(), cu[:n + 1], cu[:n + 1], scale, False)
        assert _rel_l2(out[sl], ref) < 8e-3
        assert float((lse[:, sl].float().cpu() - rlse).abs().max()) < 2e-2


@pytest.mark.parametrize("D,T,seg", [(72, 1024, 512), (80, 640, 320), (80, 200, 100), (72, 48, 48)])
def test_attn_five_of_six_output_tiles_is_the_same_bits(dev, D, T, seg):
    """Heads of 72 (Hiera's global blocks, reference model/sam2.py:1021) and 80 (the ViT, HF modeling_qwen2_5_vl.py:211) sit in the DP = 96 kernels; the pipelined
    kernel now keeps 5 of the 6 sixteen-column output tiles for D <= 80 (one MFMA in twelve less, 248 registers and no scratch where six tiles spilled).  The dropped
    tile only ever held columns >= D that were never stored: bit-equal to the six-tile form (impl bit 16), and within tolerance of the softmax oracle."""
    from rga3.hip import ops

    H = 3
    q, k, v = _rand((T, H, D), dev, seed=5), _rand((T, H, D), dev, seed=6), _rand((T, H, D), dev, seed=7)
    cu = torch.arange(0, T + 1, seg, dtype=torch.int32)
    cud = cu.to(dev)
    scale = D ** -0.5
    out, lse = ops.attn_varlen(q, k, v, cud, cud, seg, scale, causal=False, return_lse=True)
    six, lse6 = ops.attn_varlen(q, k, v, cud, cud, seg, scale, causal=False, return_lse=True, impl=16)
    assert torch.equal(out, six) and torch.equal(lse, lse6)
    ref, rlse = R.attn_varlen_ref(q.cpu(), k.cpu(), v.cpu(), cu, cu, scale, False)
    assert _rel_l2(out, ref) < 8e-3
    assert float((lse.float().cpu() - rlse).abs().max()) < 2e-2


_LDS_GRANT_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
from oracle import kernels_ref as R
from rga3.hip import ops

dev = torch.device("cuda:0")
def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()
def rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(torch.bfloat16).to(dev)

D, H = 72, 2
scale = D ** -0.5
cu_q = torch.tensor([0, 64, 128], dtype=torch.int32)
q = rand((128, H, D), 5) * 0.8
for lk in (64, 192, 256):   # window kernel LDS: 18 688 B (no grant), 55 552 B (first grant), 73 984 B (a larger one)
    k, v = rand((2 * lk, H, D), 6 + lk) * 0.8, rand((2 * lk, H, D), 7 + lk) * 0.8
    cu_k = torch.tensor([0, lk, 2 * lk], dtype=torch.int32)
    out = ops.attn_varlen(q, k, v, cu_q.to(dev), cu_k.to(dev), 64, scale, causal=False, max_k=lk)
    old = ops.attn_varlen(q, k, v, cu_q.to(dev), cu_k.to(dev), 64, scale, causal=False, max_k=lk, impl=2)
    ref, _ = R.attn_varlen_ref(q.cpu(), k.cpu(), v.cpu(), cu_q, cu_k, scale, False)
    e_old, e_ref = rel_l2(out, old), rel_l2(out, ref)
    print("window lk", lk, "vs pipelined", e_old, "vs oracle", e_ref)
    assert e_old < 4e-3 and e_ref < 8e-3, lk

D, Hq, Hkv, T = 128, 4, 2, 320   # the 8-wave backward kernels, causal
scale = D ** -0.5
cu = torch.tensor([0, T], dtype=torch.int32)
q, k, v, do = rand((T, Hq, D), 1), rand((T, Hkv, D), 2), rand((T, Hkv, D), 3), rand((T, Hq, D), 4)
o, lse = ops.attn_varlen(q, k, v, cu.to(dev), cu.to(dev), T, scale, True, return_lse=True)
dq, dk, dv = ops.attn_varlen_bwd(q, k, v, o, do, lse, cu.to(dev), cu.to(dev), T, T, scale, True)
qf, kf, vf = (t.float().cpu().requires_grad_(True) for t in (q, k, v))
ref, _ = R.attn_varlen_ref(qf, kf, vf, cu, cu, scale, True)
ref.backward(do.float().cpu())
errs = rel_l2(dq, qf.grad), rel_l2(dk, kf.grad), rel_l2(dv, vf.grad)
print("bwd dq dk dv", *errs)
assert max(errs) < 2e-2
print("ok")
"""


def test_dynamic_lds_grant_grows_between_calls(dev):
    """The dynamic-LDS grant of a kernel whose need GROWS after a grant was made (launch_lds in csrc/common.h): in a fresh process -- no earlier test has granted the
    maximum -- the window kernel at D = 72 runs on key segments of 64, 192 and 256 (18 688 B: nothing to grant; 55 552 B: the first grant; 73 984 B: a larger one),
    each against the pipelined kernel (impl=2) and the softmax oracle at the bounds of test_attn_window_kernel; then one causal backward at D = 128 (the 8-wave
    kernels) against the oracle's autograd at the bound of test_attention_backward.  A grant that did not grow makes the launch fail (Rga3Error), not fault."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _LDS_GRANT_CHILD % (root, os.path.join(root, "rga3-release_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (r.stdout + r.stderr)[-3000:]


def test_attn_forced_rescale(dev):
    """Spike one key so the running max jumps at a later tile (exercises the alpha rescale path)."""
    from rga3.hip import ops

    T, H, D = 320, 2, 128
    q, k, v = _rand((T, H, D), dev, seed=21), _rand((T, H, D), dev, seed=22), _rand((T, H, D), dev, seed=23)
    k[200] = q[10] * 4.0
    cu = torch.tensor([0, T], dtype=torch.int32)
    out = ops.attn_varlen(q, k, v, cu.to(dev), cu.to(dev), T, D ** -0.5, False)
    ref, _ = R.attn_varlen_ref(q.cpu(), k.cpu(), v.cpu(), cu, cu, D ** -0.5, False)
    assert _rel_l2(out, ref) < 1e-2


@pytest.mark.parametrize("rows,dim", [(33, 1280), (2112, 3584), (7, 5120), (5, 256)])
def test_rmsnorm(dev, rows, dim):
    from rga3.hip import ops

    x, w = _rand((rows, dim), dev, 2.0, seed=31), (1 + 0.1 * torch.randn(dim)).to(torch.bfloat16).to(dev)
    y = ops.rmsnorm(x, w, 1e-6)
    assert _rel_l2(y, R.rmsnorm_ref(x.cpu(), w.cpu(), 1e-6)) < 6e-3
    add = _rand((rows, dim), dev, seed=32)
    y2, res = ops.rmsnorm(x, w, 1e-6, add=add, return_residual=True)
    s = (x.float() + add.float()).to(torch.bfloat16)
    assert torch.equal(res.cpu(), s.cpu())
    assert _rel_l2(y2, R.rmsnorm_ref(s.cpu(), w.cpu(), 1e-6)) < 6e-3


@pytest.mark.parametrize("rows,dim", [(65, 144), (10, 1152), (3, 256), (1001, 288), (77, 512), (5, 16), (130, 264), (33, 576), (9, 2304)])
def test_layernorm(dev, rows, dim):
    from rga3.hip import ops

    x = _rand((rows, dim), dev, 3.0, seed=33) + 0.5
    w, b = _rand((dim,), dev, seed=34), _rand((dim,), dev, seed=35)
    y = ops.layernorm(x, w, b, 1e-6)
    assert _rel_l2(y, R.layernorm_ref(x.cpu(), w.cpu(), b.cpu(), 1e-6)) < 6e-3
    wide = torch.zeros((rows, dim + 16), dtype=torch.bfloat16, device=dev)      # strided rows, no bias: every row path of the launcher
    wide[:, 8:8 + dim] = x
    y2 = ops.layernorm(wide[:, 8:8 + dim], w, None, 1e-6)
    assert _rel_l2(y2, R.layernorm_ref(x.cpu(), w.cpu(), None, 1e-6)) < 6e-3


@pytest.mark.parametrize("D,H", [(80, 16), (128, 32)])
def test_rope(dev, D, H):
    from rga3.hip import ops

    T = 77
    x = _rand((T, H + 3, D), dev, seed=41)
    ang = torch.rand(T, D // 2) * 6.0
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos().to(dev), emb.sin().to(dev)
    ref = x.float().cpu().clone()
    ref[:, 2:2 + H] = R.rope_ref(x[:, 2:2 + H].cpu(), cos.cpu(), sin.cpu())
    ops.rope_(x, cos, sin, 2, H)
    assert _rel_l2(x, ref) < 4e-3
    assert torch.equal(x[:, :2].float().cpu(), ref[:, :2]) and torch.equal(x[:, 2 + H:].float().cpu(), ref[:, 2 + H:])


def test_gather_scatter_pad(dev):
    from rga3.hip import ops

    table = _rand((40, 64), dev, seed=51)
    idx = torch.randperm(10)
    g = ops.gather_rows(table, idx.to(dev), rows_per_idx=4)
    ref = table.cpu().view(10, 4, 64)[idx].reshape(40, 64)
    assert torch.equal(g.cpu(), ref)
    out = torch.zeros_like(table)
    ops.scatter_rows_(out, idx.to(dev), g, rows_per_idx=4)
    assert torch.equal(out.cpu(), table.cpu())
    p = ops.pad_cols(table[:, :40], 64)
    assert torch.equal(p[:, :40].cpu(), table[:, :40].cpu()) and p[:, 40:].abs().sum().item() == 0
    q = ops.pad_cols(_rand((5, 24), dev)[:, :20], 32)
    assert q[:, 20:].abs().sum().item() == 0
    u = _rand((7, 147), dev, seed=52)  # rows not 16-byte aligned
    pu = ops.pad_cols(u, 152)
    assert torch.equal(pu[:, :147].cpu(), u.cpu()) and pu[:, 147:].abs().sum().item() == 0


def test_elementwise(dev):
    from rga3.hip import ops

    a, b = _rand((37, 100), dev, 2.0, seed=61), _rand((37, 100), dev, seed=62)
    assert _rel_l2(ops.silu_mul(a, b), torch.nn.functional.silu(a.float().cpu()) * b.float().cpu()) < 6e-3
    assert _rel_l2(ops.add(a, b), a.float().cpu() + b.float().cpu()) < 4e-3


@pytest.mark.parametrize("V", [5003, 5120, 152064])     # ragged width (scalar loads), 16-byte rows (vector loads), the real vocabulary
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_cross_entropy(dev, dtype, V):
    from rga3.hip import ops

    rows = 9
    logits = (torch.randn(rows, V) * 3).to(dtype).to(dev)
    labels = torch.randint(0, V, (rows,))
    labels[2] = -100
    loss, dl = ops.cross_entropy_rows(logits, labels.to(dev), want_grad=True, grad_scale=0.5)
    ref = R.ce_rows_ref(logits.cpu(), labels)
    assert (loss.cpu() - ref).abs().max().item() < 2e-3
    lf = logits.float().cpu().requires_grad_(True)
    (torch.nn.functional.cross_entropy(lf, labels, ignore_index=-100, reduction="sum") * 0.5).backward()
    assert _rel_l2(dl, lf.grad) < 1e-2


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 520, 384), (2112, 4608, 3584), (2112, 3584, 18944), (17, 24, 128),
                                   (4160, 4608, 3584), (4160, 3584, 18944), (4160, 37888, 3584)])   # M = 4160: configs[4] (32 frames, S = 4096 + 64): q|k|v, down, gate|up
def test_fp8_quant_and_gemm(dev, M, N, K):
    """e4m3 row quantiser bit-exact against torch's float8_e4m3fn cast; fp8 GEMM equal to the fp32 product of the quantised operands up to
    summation order; and the end-to-end error against the unquantised bf16 GEMM at the level per-row e4m3 quantisation implies."""
    from rga3.hip import ops

    a, w = _rand((M, K), dev, seed=21), _rand((N, K), dev, 0.05, seed=22)
    a[3, :] = 0                                  # a zero row: scale 1, all-zero codes
    a[5, 7] = 40.0                               # an outlier sets that row's scale
    qa, sa = ops.quant_fp8_rows(a)
    qw, sw = ops.quant_fp8_rows(w)
    ra, rsa = R.quant_fp8_rows_ref(a.cpu())
    assert torch.equal(sa.cpu(), rsa)
    assert torch.equal(qa.cpu().view(torch.float8_e4m3fn).float(), ra.float())
    rw, rsw = R.quant_fp8_rows_ref(w.cpu())
    bias, res = _rand((N,), dev, 0.5, seed=23), _rand((M, N), dev, seed=24)
    out = ops.gemm_fp8(qa, sa, qw, sw, bias=bias, residual=res)
    ref = R.gemm_fp8_ref(ra, rsa, rw, rsw, bias.cpu(), res.cpu())
    assert _rel_l2(out, ref) < 4e-3, (M, N, K)
    plain = ops.gemm_fp8(qa, sa, qw, sw)
    full = R.linear_ref(a.cpu(), w.cpu())
    assert _rel_l2(plain, full) < 6e-2           # two e4m3 operands: ~2^-4 relative per element, averaged over K


def test_fp8_quant_codes_equal_true_quotient_every_bf16_value(dev):
    """The row quantisers divide by the row scale with r = RN(1 / scale), q0 = x r, q = q0 + (x - q0 scale) r (two FMAs: Markstein's step) instead of the IEEE
    expansion.  Every e4m3 code must equal torch's cast of the TRUE quotient: all 65 280 finite bf16 values as one row each way round (the row's own amax fixes
    the scale), 600 rows of them against 600 different outliers (600 different scales, quotients anywhere between two codes), and a million random values."""
    from rga3.hip import ops

    bits = torch.arange(0, 65536, dtype=torch.int32)
    vals = bits.to(torch.int16).view(torch.bfloat16)
    vals = vals[torch.isfinite(vals.float())]
    n = (vals.numel() + 7) // 8 * 8
    row = torch.zeros(n, dtype=torch.bfloat16)
    row[:vals.numel()] = vals
    g = torch.Generator().manual_seed(5)
    rows = row[None].repeat(600, 1)
    small = rows.float().abs() < 1e30                                  # (the scale of a row is its outlier's: values above it are zeroed so the outlier IS the amax)
    out = (torch.rand(600, generator=g) * 6.0 - 3.0).exp() * 37.0      # amax between 1.8 and 740
    rows = torch.where(small & (rows.float().abs() <= out[:, None]), rows, torch.zeros((), dtype=torch.bfloat16))
    rows[:, 0] = out.to(torch.bfloat16)
    rnd = (torch.randn(128, 8192, generator=g) * torch.rand(128, 1, generator=g) * 10).to(torch.bfloat16)
    for x in (row[None].clone().masked_fill_(row[None].float().abs() > 3e38, 0), rows, rnd):
        q, sc = ops.quant_fp8_rows(x.to(dev))
        amax = x.float().abs().amax(1)
        want_sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        assert torch.equal(sc.cpu(), want_sc)
        want = (x.float() / want_sc[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
        got = q.cpu()
        assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("T,I", [(37, 512), (200, 18944), (3, 32)])
def test_swiglu_quant_fused_equals_unfused(dev, T, I):
    """rga3_swiglu_{fwd,bwd}_quant_fp8 == swiglu_{fwd,bwd} followed by quant_fp8_rows, bit for bit (codes and scales), incl. a zero row and an outlier row."""
    from rga3.hip import ops

    gu = _rand((T, 2 * I), dev, 1.5, seed=41)
    da = _rand((T, I), dev, 0.7, seed=42)
    gu[1] = 0
    da[1] = 0
    gu[2, 5] = 30.0
    q0, s0 = ops.quant_fp8_rows(ops.swiglu_fwd(gu))
    q1, s1 = ops.swiglu_fwd_quant(gu)
    assert torch.equal(s0, s1) and torch.equal(q0, q1)
    q2, s2 = ops.quant_fp8_rows(ops.swiglu_bwd(gu, da))
    q3, s3 = ops.swiglu_bwd_quant(gu, da)
    assert torch.equal(s2, s3)
    # the backward expression is long enough for the compiler to associate it differently in the two kernels on a few elements: those land on the
    # neighbouring e4m3 code (the bf16 value differed by one ulp before quantisation); everything else is identical
    diff = q2 != q3
    frac = float(diff.float().mean())
    print("SWIGLU_BWD_QUANT mismatching codes: %.2e" % frac)
    assert frac < 1e-3
    if frac > 0:
        a_, b_ = q2[diff].view(torch.float8_e4m3fn).float(), q3[diff].view(torch.float8_e4m3fn).float()
        assert float(((a_ - b_).abs() / a_.abs().clamp(min=2 ** -9)).max()) <= 0.13      # neighbouring codes: one step of a 3-bit mantissa


@pytest.mark.parametrize("M,N,K,f32", [(256, 256, 65536, False), (32, 256, 131072, True), (300, 520, 16384, False), (64, 64, 4096, False), (700, 256, 2048, False)])
def test_gemm_split_k_small_outputs(dev, M, N, K, f32):
    """Tile 25 (few tiles, huge K: the weight-gradient products): slices summed in f32 slabs by the reduce kernel; with bias and f32 output."""
    from rga3.hip import ops

    a, w = _rand((M, K), dev, 0.1, seed=31), _rand((N, K), dev, 0.1, seed=32)
    bias = _rand((N,), dev, 0.5, seed=33)
    odt = torch.float32 if f32 else torch.bfloat16
    out = ops.gemm(a, w, bias=bias, out_dtype=odt, tile=25)
    again = ops.gemm(a, w, bias=bias, out_dtype=odt, tile=25)
    assert torch.equal(out, again)
    ref = (a.float().cpu().double() @ w.float().cpu().double().t() + bias.float().cpu().double()).float()
    if not f32:
        ref = ref.to(torch.bfloat16).float()
    assert _rel_l2(out, ref) < (1e-4 if f32 else 5e-3), (M, N, K)


@pytest.mark.parametrize("K,M,N", [(2112, 128, 3584), (2112, 3584, 128), (6, 1024, 512), (300, 264, 136), (33, 8, 8), (4096, 512, 4608), (1000, 152064 // 8, 64)])
@pytest.mark.parametrize("f32", [False, True])
def test_gemm_tn_weight_gradient_product(dev, K, M, N, f32):
    """C = A^T B over row-major [K, M] / [K, N] operands (dW = dY^T X) vs fp32 matmul; strided views (column slices of a wider buffer) included."""
    from rga3.hip import ops

    torch.manual_seed(K + M + N)
    wide = torch.randn(K, M + 16, device=dev).to(torch.bfloat16)
    a = wide[:, 8:8 + M]                      # row stride M + 16, 16-byte aligned column offset
    b = torch.randn(K, N, device=dev).to(torch.bfloat16)
    got = ops.gemm_tn(a, b, out_dtype=torch.float32 if f32 else torch.bfloat16)
    want = a.float().T @ b.float()
    assert got.shape == (M, N)
    tol = (2e-5 if f32 else 6e-3)
    assert float((got.float() - want).norm() / want.norm()) < tol
    assert float((got.float() - want).abs().max()) <= (1e-3 if f32 else 2.0 ** -7) * float(want.abs().max()) + 1e-4
    again = ops.gemm_tn(a, b, out_dtype=torch.float32 if f32 else torch.bfloat16)
    assert torch.equal(got, again)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("act,N,K,bias,res", [("none", 4608, 3584, True, False), ("none", 3584, 3584, False, True), ("swiglu", 37888, 3584, False, False),
                                              ("none", 3584, 18944, False, True), ("gelu", 1000, 264, True, False), ("relu", 72, 64, True, False),
                                              ("swiglu", 96, 136, True, False)])
def test_gemv_decode_rows_match_tiled_gemm(dev, M, act, N, K, bias, res):
    """The skinny weight-stream kernel (tile 40, picked for M <= 4: the decode step of generate()) against the fp32 oracle and against the tiled
    kernel on the same rows embedded in a taller matrix: same epilogue semantics, so a decode row rounds like a prefill row (k-order differs)."""
    from rga3.hip import ops

    a, w = _rand((M, K), dev, seed=21), _rand((N, K), dev, 0.05, seed=22)
    b = _rand((N,), dev, 0.1, seed=23) if bias else None
    n_out = N // 2 if act == "swiglu" else N
    r = _rand((M, n_out), dev, seed=24) if res else None
    out = ops.gemm(a, w, b, residual=r, act=act)            # M <= 4 -> tile 40
    tall = torch.cat([a, _rand((128 - M, K), dev, seed=25)])
    rt = torch.cat([r, _rand((128 - M, n_out), dev, seed=26)]) if res else None
    ref = ops.gemm(tall, w, b, residual=rt, act=act, tile=12)[:M]
    assert out.shape == (M, n_out)
    assert _rel_l2(out, ref.float().cpu()) < 4e-3
    d = (out.float() - ref.float()).abs()
    assert float((d > 0).float().mean()) < 0.15 and float(d.max()) <= 2.0 ** -6 * float(ref.float().abs().max()) + 1e-3
    o32 = ops.gemm(a, w, b, out_dtype=torch.float32) if act == "none" and not res else None
    if o32 is not None:
        want = a.float() @ w.float().T + (b.float() if bias else 0)
        assert float((o32 - want).norm() / want.norm()) < 1e-5


def test_raw_ctypes_binding_as_in_integration_md(dev):
    """The binding a reference maintainer would write, with no help from rga3's own Python: plain ctypes on the C ABI."""
    import ctypes as C

    from rga3.hip import lib as L

    L.load()   # torch's HIP runtime first, as the document says
    so = C.CDLL(L.LIB_PATH)
    so.rga3_gemm_bf16.restype = C.c_int
    so.rga3_gemm_bf16.argtypes = [C.c_void_p] * 6 + [C.c_int64] * 7 + [C.c_int] * 3 + [C.c_void_p, C.c_int64, C.c_void_p]
    so.rga3_gemm_workspace_bytes.restype = C.c_int64
    ws = torch.zeros(so.rga3_gemm_workspace_bytes(), dtype=torch.uint8, device=dev)
    x, w, b = _rand((300, 264), dev, seed=31), _rand((520, 264), dev, 0.05, seed=32), _rand((520,), dev, 0.1, seed=33)
    out = torch.empty(300, 520, dtype=torch.bfloat16, device=dev)
    rc = so.rga3_gemm_bf16(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, None, out.data_ptr(), 300, 520, 264, x.stride(0), w.stride(0), out.stride(0), 0,
                           0, 0, -1, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert _rel_l2(out, R.linear_ref(x.cpu(), w.cpu(), b.cpu())) < 6e-3
    # errors come back as codes + a message, never as exceptions or aborts
    so.rga3_last_error.argtypes = [C.c_char_p, C.c_size_t]
    rc = so.rga3_gemm_bf16(x.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), 300, 520, 263, x.stride(0), w.stride(0), out.stride(0), 0,
                           0, 0, -1, None, 0, torch.cuda.current_stream().cuda_stream)
    buf = C.create_string_buffer(256)
    so.rga3_last_error(buf, 256)
    assert rc != 0 and b"multiple of 8" in buf.value


@pytest.mark.parametrize("seg_q,seg_k,nwin,H,D", [(16, 16, 64, 4, 72), (4, 16, 128, 8, 72), (8, 8, 32, 2, 64), (32, 32, 6, 3, 128), (2, 64, 64, 1, 32)])
def test_attention_block_diagonal_packing(dev, seg_q, seg_k, nwin, H, D):
    """Several tiny windows packed into one segment with block-diagonal visibility (block_q, block_k) == one segment per window, bit for bit
    (the same keys enter every row's softmax in the same order; masked scores contribute exact zeros)."""
    from rga3.hip import ops

    q = _rand((nwin * seg_q, H, D), dev, seed=41)
    k = _rand((nwin * seg_k, H, D), dev, seed=42)
    v = _rand((nwin * seg_k, H, D), dev, seed=43)
    cq = (torch.arange(nwin + 1, dtype=torch.int32) * seg_q).to(dev)
    ck = (torch.arange(nwin + 1, dtype=torch.int32) * seg_k).to(dev)
    ref = ops.attn_varlen(q, k, v, cq, ck, seg_q, D ** -0.5)
    g = 1
    while seg_q * g * 2 <= 64 and nwin % (g * 2) == 0:
        g *= 2
    assert g > 1
    cq2 = (torch.arange(nwin // g + 1, dtype=torch.int32) * seg_q * g).to(dev)
    ck2 = (torch.arange(nwin // g + 1, dtype=torch.int32) * seg_k * g).to(dev)
    got = ops.attn_varlen(q, k, v, cq2, ck2, seg_q * g, D ** -0.5, block=(seg_q, seg_k))
    assert torch.equal(got, ref)


@pytest.mark.parametrize("M,N,K", [(9, 256, 256), (9, 2048, 256), (9, 256, 2048), (16, 128, 256), (5, 24, 40), (13, 3584, 3584), (7, 250, 1176)])
@pytest.mark.parametrize("act", ["none", "gelu", "relu"])
def test_gemm_token_rows(dev, M, N, K, act):
    """Tile 41 (5 - 16 token rows, K split over the 8 waves of a workgroup): the mask decoder's token-side products (9 x 256 x 256, the 256 -> 2048 -> 256 MLP), ragged
    N / K (a last k-step of 8 columns, a last 16-column block of 8 / 10), a [SEG]-row sized product; bias, activation and residual with gemm_epilogue's rounding
    points -- against fp32, against the tiled kernel, reproducible, and picked automatically for these shapes."""
    from rga3.hip import ops

    a, w = _rand((M, K), dev, seed=M + N), _rand((N, K), dev, 0.05, seed=K)
    bias, res = _rand((N,), dev, 0.5, seed=5), _rand((M, N), dev, seed=6)
    out = ops.gemm(a, w, bias=bias, residual=res, act=act, tile=41)
    ref = R.linear_ref(a.cpu(), w.cpu(), bias.cpu(), res.cpu(), act)
    assert _rel_l2(out, ref) < 8e-3
    tiled = ops.gemm(a, w, bias=bias, residual=res, act=act, tile=12)
    assert _rel_l2(out, tiled) < 2e-3
    assert torch.equal(out, ops.gemm(a, w, bias=bias, residual=res, act=act, tile=41))
    if M * N * K < (1 << 24):
        assert torch.equal(out, ops.gemm(a, w, bias=bias, residual=res, act=act))          # tile = -1 routes here
    plain = ops.gemm(a, w, tile=41)
    assert _rel_l2(plain, R.linear_ref(a.cpu(), w.cpu())) < 6e-3
    buf = torch.zeros((M, N + 8), dtype=torch.bfloat16, device=dev)                        # strided output view
    ops.gemm(a, w, bias=bias, out=buf[:, :N], tile=41)
    assert torch.equal(buf[:, :N], ops.gemm(a, w, bias=bias, tile=41)) and float(buf[:, N:].abs().max()) == 0.0


def test_gemm_token_rows_grouped_with_operand_sum(dev):
    """gemm_rows16_many: several token-row products in one launch, some on the sum of two row operands (rounded to bf16 first, as a separate add launch would), mixed
    shapes / activations / residuals -- each equal, bit for bit, to tile 41 on the pre-added operand."""
    from rga3.hip import ops

    a, pe = _rand((9, 256), dev, seed=1), _rand((9, 256), dev, 0.5, seed=2)
    a5 = _rand((5, 2048), dev, seed=3)
    w1, b1 = _rand((256, 256), dev, 0.05, seed=4), _rand((256,), dev, 0.5, seed=5)
    w2, b2 = _rand((128, 256), dev, 0.05, seed=6), _rand((128,), dev, 0.5, seed=7)
    w3 = _rand((250, 2048), dev, 0.05, seed=8)
    res = _rand((9, 256), dev, seed=9)
    outs = ops.gemm_rows16_many([(a, pe, w1, b1), (a, None, w2, b2, None, "relu"), (a5, None, w3, None, None, "gelu"), (a, pe, w1, b1, res)])
    apre = ops.add(a, pe)
    assert torch.equal(outs[0], ops.gemm(apre, w1, b1, tile=41))
    assert torch.equal(outs[1], ops.gemm(a, w2, b2, act="relu", tile=41))
    assert torch.equal(outs[2], ops.gemm(a5, w3, act="gelu", tile=41))
    assert torch.equal(outs[3], ops.gemm(apre, w1, b1, residual=res, tile=41))
    assert _rel_l2(outs[0], R.linear_ref((a.float() + pe.float()).to(torch.bfloat16).cpu(), w1.cpu(), b1.cpu())) < 6e-3
