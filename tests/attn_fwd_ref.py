"""float64 reference of ops.attn_varlen / ops.attn_varlen_rope (csrc/attn_fwd.hip, csrc/attn_causal32.hip), the case table of their GPU tests and the
checkers those tests use (no tests in this module; tests/test_attn_fwd_ref_cpu.py tests the reference and the checkers, tests/test_attn_fwd_gpu.py the kernels).

The call, for every segment s with queries cu_q[s] .. cu_q[s + 1] and keys cu_k[s] .. cu_k[s + 1] (Lq and Lk of them), query head hq reading kv head
hq // (Hq // Hkv):  vis[q, key] = (!causal || key <= q + (Lk - Lq)) && (no block || (q >> log2 bq) == (key >> log2 bk));  lse[q] = logsumexp of scale * q.k over the
visible keys (-inf where none is visible);  o = softmax over the visible keys times V (0 where none is visible).  Everything runs on the CPU in float64 from the exact
values of the bf16 inputs and nothing is rounded; with model=True the roundings the kernels declare are applied (exp(S - rowmax) to bf16 before the P V product, the row
sum from the unrounded values, o to bf16): that is the yardstick a kernel's error is measured with, never the expectation."""
import collections
import functools

import torch

from tests.attn_bwd_ref import bf16_of, cu, rel_l2, row_errors, segment_of, visible

BF = torch.bfloat16
FACTOR = 3                                   # a kernel's worst row may be FACTOR x the model's worst row of the same case (the backward tests' constant)
FwdRef = collections.namedtuple("FwdRef", "o lse")   # o [Tq, Hq, D] float64, lse [Hq, Tq] float64


def seg_visible(Lq, Lk, causal, block=None):
    """[Lq, Lk] bool: the causal limit of attn_bwd_ref.visible and the block-diagonal packing (bq, bk), both powers of two."""
    vis = visible(Lq, Lk, causal)
    if block:
        bq, bk = block
        assert bq & (bq - 1) == 0 and bk & (bk - 1) == 0
        vis = vis & ((torch.arange(Lq)[:, None] // bq) == (torch.arange(Lk)[None, :] // bk))
    return vis


def attn_fwd_ref(q, k, v, cu_q, cu_k, scale, causal, block=None, model=False):
    """CPU tensors as ops.attn_varlen takes them (any float dtype: their exact values are used) -> FwdRef."""
    Tq, Hq, D = q.shape
    G = Hq // k.shape[1]
    o = torch.zeros((Tq, Hq, D), dtype=torch.float64)
    lse = torch.full((Hq, Tq), float("-inf"), dtype=torch.float64)
    for s in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[s]), int(cu_q[s + 1]), int(cu_k[s]), int(cu_k[s + 1])
        Lq, Lk = q1 - q0, k1 - k0
        if Lq == 0 or Lk == 0:
            continue
        Q = q[q0:q1].double().permute(1, 0, 2)                                      # [Hq, Lq, D]
        K = k[k0:k1].double().permute(1, 0, 2).repeat_interleave(G, 0)              # [Hq, Lk, D]
        V = v[k0:k1].double().permute(1, 0, 2).repeat_interleave(G, 0)
        vis = seg_visible(Lq, Lk, causal, block)[None]
        S = ((Q @ K.transpose(1, 2)) * float(scale)).masked_fill(~vis, float("-inf"))
        m = S.max(-1, keepdim=True).values
        seen = torch.isfinite(m)                                                    # [Hq, Lq, 1]: the row sees a key
        E = torch.where(vis & seen, torch.exp(S - torch.where(seen, m, torch.zeros_like(m))), torch.zeros_like(S))
        l = E.sum(-1, keepdim=True)
        O = ((bf16_of(E) if model else E) @ V) / torch.where(seen, l, torch.ones_like(l))
        o[q0:q1] = (bf16_of(O) if model else O).permute(1, 0, 2)
        lse[:, q0:q1] = torch.where(seen, m + torch.log(torch.where(seen, l, torch.ones_like(l))), torch.full_like(m, float("-inf")))[..., 0]
    return FwdRef(o, lse)


def rope_tables(lens, D, shift=0):
    """cos / sin [T, D] f32 of rotate-half RoPE, positions restarting in every segment (+ shift), rounded to multiples of 2^-6: with 7-bit table entries and 8-bit
    operands every product x cos is exact in f32 and so (but for operands ~2^9 apart) is the sum of two, so the kernels' f32 rotation and rope_rotate's float64 one
    round the SAME number to bf16 and the attention that follows is compared on identical operands."""
    pos = torch.cat([torch.arange(n, dtype=torch.float64) for n in lens]) + shift
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    fr = pos[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    rnd = lambda t: (torch.round(t * 64) / 64).float().contiguous()
    return rnd(emb.cos()), rnd(emb.sin())


def rope_rotate(x, cos, sin):
    """x [T, H, D] bf16, cos / sin [T, D] f32 -> bf16(x cos + rotate_half(x) sin), the rotation in float64 and ONE rounding (what rga3_attn_varlen_fwd_rope applies to
    q, and to k with rope_k, while it loads them)."""
    x = x.double()
    h = x.shape[-1] // 2
    rot = torch.cat([-x[..., h:], x[..., :h]], -1)
    return (x * cos.double()[:, None] + rot * sin.double()[:, None]).float().to(BF)


# ---------------------------------------------------------------------------------------------------------------- the case table
# The smallest shapes that reach each route of rga3_attn_varlen_fwd / rga3_attn_varlen_fwd_rope.  The comments name the instance as the dispatch code reads:
#   G<DP, QT, NWAVE, TR|SC, PAIR?, SPLIT?, ROPE?, KT, DTO> = attn_fwd_kernel (TR: transposing LDS reads, SC: impl bit 1's scalar reads); block of 16 QT NWAVE query rows
#   W<DP, NW, QT, ROPE?, DTO> = attn_win_kernel (non-causal, 0 < max_k <= 256, D <= 96, impl bits 1 and 2 clear);  C32 = attn_causal32_kernel (causal, D = 128,
#   max_q >= 256, 16-byte o, impl bits 1, 2, 4 clear).
# launch_dp: DP 64 / 128 take 8 waves x QT 1 above 64 query rows (impl 2: not), DP 96 takes 8 waves x QT 2 when non-causal and max_q is a multiple of 256 (impl 2: not),
# DP 256 always 4 waves x QT 1, everything else 4 waves x QT 1 up to 64 rows and 4 waves x QT 2 above.  launch_attn: PAIR only on 8 waves, causal, >= 4 query blocks
# (so never at DP 32 / 96 / 256); KT = 128 on <128, 1, 8> (paired or not), 64 elsewhere; SPLIT when the entry point set nsplit > 1; DTO = 5 at DP 96, D <= 80, not
# paired, impl bit 16 clear.
#   max_k: None = pass max(lk); 0 = pass none (keeps a short non-causal call away from the window kernel);  rope: None, "q" (keys arrive rotated) or "qk" (rope_k);
#   same_cu: hand the SAME device tensor as cu_q and cu_k (what the rope entry tests for its window form).
Case = collections.namedtuple("Case", "name family lq lk Hq Hkv D causal impl block max_k rope same_cu")


def _c(name, family, lq, lk, Hq, Hkv, D, causal, impl=0, block=None, max_k=None, rope=None, same_cu=False):
    return Case(name, family, list(lq), list(lk), Hq, Hkv, D, causal, impl, block, max_k, rope, same_cu)


RAGGED = [256, 100, 7, 129]
CASES = [
    # ---- general kernel, DP = 128
    _c("g128-130", "general", [130], [130], 4, 2, 128, False),                # G<128,1,8,TR,-,-,-,128,8>: one 128-key tile and a 2-key tail
    _c("g128-255-causal", "general", [255], [255], 4, 2, 128, True),          # G<128,1,8,TR,-,-,-,128,8>: one row short of C32, 2 query blocks: not paired
    _c("g128-513-d112-causal", "paired", [513], [513], 4, 2, 112, True),      # G<128,1,8,TR,PAIR,-,-,128,8>: 5 blocks (unpaired middle), last block one row, D < DP
    _c("g128-513-impl4", "paired", [513], [513], 4, 2, 128, True, impl=4),    # G<128,1,8,TR,PAIR,-,-,128,8>: impl 4 keeps C32's rows here
    _c("g128-300x437-d120-causal", "general", [300], [437], 4, 2, 120, True),  # G<128,1,8,TR,-,-,-,128,8>: 3 blocks, shift 137, zero-padded columns
    # ---- DP = 64
    _c("g64-512-gqa3-causal", "paired", [512], [512], 6, 2, 64, True),        # G<64,1,8,TR,PAIR,-,-,64,4>: 4 blocks = 2 pairs, group of 3
    _c("g64-400x437-d48-causal", "paired", [400], [437], 4, 2, 48, True),     # G<64,1,8,TR,PAIR,-,-,64,4>: shift 37, no multiple of a tile
    _c("g64-300", "general", [300], [300], 4, 2, 64, False),                  # G<64,1,8,TR,-,-,-,64,4>: 300 keys > 256 keep it off the window kernel
    _c("g64-9x300-d40", "general", [9, 9], [300, 300], 4, 2, 40, False),      # G<64,1,4,TR,-,-,-,64,4>: 4 waves, three of them without a row
    _c("g64-200-impl2", "general", [200], [200], 4, 2, 64, False, impl=2),    # G<64,2,4,TR,-,-,-,64,4>: impl 2 (wave4, QT = 2) where the window kernel would run
    _c("g64-100x150-impl1-causal", "general", [100], [150], 4, 2, 64, True, impl=1),   # G<64,1,8,SC,-,-,-,64,4>: the scalar-read form
    # ---- DP = 96
    _c("g96-512-d72", "general", [512], [512], 4, 2, 72, False),              # G<96,2,8,TR,-,-,-,64,5>: 8 waves x QT 2, five output tiles
    _c("g96-512-d72-impl16", "general", [512], [512], 4, 2, 72, False, impl=16),   # G<96,2,8,TR,-,-,-,64,6>: all six
    _c("g96-256x300-d96", "general", [256], [300], 4, 2, 96, False),          # G<96,2,8,TR,-,-,-,64,6>
    _c("g96-40x300-d80", "general", [40], [300], 4, 2, 80, False),            # G<96,1,4,TR,-,-,-,64,5>
    _c("g96-200x300-d88", "general", [200], [300], 4, 2, 88, False),          # G<96,2,4,TR,-,-,-,64,6>
    _c("g96-200x264-d72-causal", "general", [200], [264], 4, 2, 72, True),    # G<96,2,4,TR,-,-,-,64,5>: causal stays on 4 waves, never paired
    # ---- DP = 32
    _c("g32-385-causal", "general", [385], [385], 4, 2, 32, True),            # G<32,2,4,TR,-,-,-,64,2>: 4 blocks of 128, last one row
    _c("g32-64x300-d16", "general", [64], [300], 4, 2, 16, False),            # G<32,1,4,TR,-,-,-,64,2>
    _c("g32-70-d8-causal", "general", [70], [70], 4, 2, 8, True),             # G<32,2,4,TR,-,-,-,64,2>: one 16-byte chunk per row
    _c("g32-100x133-d24-causal", "general", [100], [133], 4, 2, 24, True),    # G<32,2,4,TR,-,-,-,64,2>
    # ---- DP = 256
    _c("g256-130x200", "general", [130], [200], 2, 1, 256, False),            # G<256,1,4,TR,-,-,-,64,16>: 3 blocks of 64
    _c("g256-100x133-d136-causal", "general", [100], [133], 2, 1, 136, True),  # G<256,1,4,TR,-,-,-,64,16>: D just above the 128 bucket
    _c("g256-70-d192", "general", [70], [70], 2, 1, 192, False),              # G<256,1,4,TR,-,-,-,64,16>
    # ---- split keys + attn_split_combine_kernel (non-causal, max_k >= 1024, few workgroups; slices = min(8, 256 / workgroups, max_k / 512) = 2 here, each
    #      ceil(tiles of the segment / 2) tiles of 64 keys)
    _c("split-9x1024-d16", "split", [9], [1024], 8, 8, 16, False),            # G<32,1,4,TR,-,SPLIT,-,64,2> + combine: 2 slices of 8 tiles
    _c("split-64x1024-d256", "split", [64], [1024], 1, 1, 256, False),        # G<256,1,4,TR,-,SPLIT,-,64,16> + combine
    _c("split-ragged-d64", "split", [9, 20], [1100, 40], 4, 2, 64, False),    # G<64,1,4,TR,-,SPLIT,-,64,4> + combine: the 40-key segment has 1 tile, its slice 1 holds no key
    # ---- window kernel, one case per instantiated form
    _c("w64-4-d8", "window", [64, 17, 40], [64, 17, 40], 4, 2, 8, False),     # W<64,4,1,-,4>: 16-byte LDS rows, padded-d reads 8 rows ahead
    _c("w64-4-d40", "window", [33, 64], [200, 70], 4, 2, 40, False),          # W<64,4,1,-,4>: 4 waves stage 256 rows in two passes
    _c("w96-4-5-d72", "window", [64, 30], [256, 100], 4, 2, 72, False),       # W<96,4,1,-,5>
    _c("w96-4-6-d88", "window", [50, 3], [70, 130], 4, 2, 88, False),         # W<96,4,1,-,6>
    _c("w64-8-ragged", "window", RAGGED, RAGGED, 4, 2, 64, False),            # W<64,8,1,-,4>: two workgroups per window, idle waves, partial last key tiles
    _c("w64-8-d24-cross", "window", [130, 64], [190, 33], 4, 2, 24, False),   # W<64,8,1,-,4>: Lq != Lk, 48-byte LDS rows
    _c("w96-8-1-5-d80", "window", [128, 70], [128, 70], 4, 2, 80, False),     # W<96,8,1,-,5>: 64 < max_q <= 128
    _c("w96-8-1-6-d96", "window", [100], [100], 4, 2, 96, False),             # W<96,8,1,-,6>
    _c("w96-8-2-5-ragged-d72", "window", RAGGED, RAGGED, 4, 2, 72, False),    # W<96,8,2,-,5>: 32 rows per wave
    _c("w96-8-2-6-d96", "window", [200, 129], [256, 60], 4, 2, 96, False),    # W<96,8,2,-,6>
    _c("w96-8-1-5-impl8", "window", [256], [256], 4, 2, 72, False, impl=8),   # W<96,8,1,-,5>: impl 8 keeps 256 queries on 16-row waves, two workgroups
    _c("w-block16", "window", [64] * 3, [64] * 3, 4, 2, 72, False, block=(16, 16)),        # W<96,4,1,-,5>, four 16-token windows packed per segment
    _c("w-block4x16", "window", [16] * 3, [64] * 3, 4, 2, 72, False, block=(4, 16)),       # W<96,4,1,-,5>, 4 pooled queries x 16 keys per window
    _c("g-block16-impl2", "general", [64] * 3, [64] * 3, 4, 2, 72, False, impl=2, block=(16, 16)),   # G<96,1,4,TR,-,-,-,64,5>: the same packing, masked-tile path
    _c("g-block4x16-impl2", "general", [16] * 3, [64] * 3, 4, 2, 72, False, impl=2, block=(4, 16)),  # G<96,1,4,TR,-,-,-,64,5>
    _c("w64-4-no-keys", "window", [40, 30, 50], [40, 0, 50], 4, 2, 64, False),               # W<64,4,1,-,4>: a segment without keys stages nothing, o = 0, lse = -inf
    # ---- attn_causal32_kernel
    _c("c32-256", "causal32", [256], [256], 4, 2, 128, True),                 # C32: two blocks, one pair
    _c("c32-257", "causal32", [257], [257], 4, 2, 128, True),                 # C32: three blocks, the unpaired middle, the last a single row
    _c("c32-385-1-300", "causal32", [385, 1, 300], [385, 1, 300], 4, 2, 128, True),   # C32: grid sized by the longest, a one-token segment
    _c("c32-300x437", "causal32", [300], [437], 4, 2, 128, True),             # C32: shift 137
    _c("c32-300x236", "causal32", [300], [236], 4, 2, 128, True),             # C32: shift -64, rows 0 .. 63 see no key
    # ---- rga3_attn_varlen_fwd_rope
    _c("rope-w64-qk", "rope", [64, 17, 40], [64, 17, 40], 4, 2, 64, False, rope="qk", same_cu=True),   # W<64,4,1,ROPE,4>
    _c("rope-w64-q", "rope", [64, 17, 40], [64, 17, 40], 4, 2, 64, False, rope="q", same_cu=True),     # W<64,4,1,ROPE,4>, keys arrive rotated
    _c("rope-w80-qk", "rope", [64, 17, 40], [64, 17, 40], 4, 2, 80, False, rope="qk", same_cu=True),   # W<96,4,1,ROPE,5>
    _c("rope-w80-q", "rope", [64, 17, 40], [64, 17, 40], 4, 2, 80, False, rope="q", same_cu=True),
    _c("rope-w96-qk", "rope", [64, 17, 40], [64, 17, 40], 4, 2, 96, False, rope="qk", same_cu=True),   # W<96,4,1,ROPE,6>
    _c("rope-w96-q", "rope", [64, 17, 40], [64, 17, 40], 4, 2, 96, False, rope="q", same_cu=True),
    _c("rope-g32-causal", "rope", [33] * 3, [33] * 3, 4, 2, 32, True, rope="qk", same_cu=True),        # G<32,1,4,TR,-,-,ROPE,64,2> (launch_rope_win): causal
    _c("rope-g128-causal", "rope", [33] * 3, [33] * 3, 4, 2, 128, True, rope="qk", same_cu=True),      # G<128,1,4,TR,-,-,ROPE,64,8>
    _c("rope-g32-other-cu", "rope", [33, 20], [33, 20], 4, 2, 32, False, rope="q"),                    # G<32,1,4,TR,-,-,ROPE,64,2>: non-causal, cu_k another tensor
    _c("rope-g128-other-cu", "rope", [33, 20], [33, 20], 4, 2, 128, False, rope="qk"),                 # G<128,1,4,TR,-,-,ROPE,64,8>
    _c("rope-c32-300", "rope", [300], [300], 4, 2, 128, True, rope="q"),                               # C32 rotating its query fragments
    # ---- degenerate segments and rows on the general kernel, below 256 rows
    _c("deg-no-queries-d64", "general", [100, 0, 50], [100, 40, 50], 4, 2, 64, True),     # G<64,1,8,TR,-,-,-,64,4>: 40 keys nobody queries
    _c("deg-no-queries-d128", "general", [100, 0, 50], [100, 40, 50], 4, 2, 128, True),   # G<128,1,8,TR,-,-,-,128,8>
    _c("deg-no-keys-d64", "general", [100, 30, 50], [100, 0, 50], 4, 2, 64, True),        # 30 queries without a key between two ordinary segments: o = 0, lse = -inf
    _c("deg-no-keys-d128", "general", [100, 30, 50], [100, 0, 50], 4, 2, 128, True),
    _c("deg-200x136-d64", "general", [200], [136], 4, 2, 64, True),                       # shift -64: rows 0 .. 63 see no key, the first query block walks no tile
    _c("deg-200x136-d128", "general", [200], [136], 4, 2, 128, True),
    # ---- multi-segment paired case for the "segment alone" test (all of its segments walk G<64,1,8,TR,PAIR,-,-,64,4> under max_q = 512)
    _c("g64-multi-causal", "paired", [512, 130, 1, 385], [512, 130, 1, 385], 4, 2, 64, True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = ("general", "paired", "split", "window", "causal32", "rope")


def make_operands(c, seed):
    """Seeded randn bf16 q [Tq, Hq, D], k, v [Tk, Hkv, D] of a case; rope cases also cos, sin [Tq, D] f32 and the rotated qr, kr the reference runs on."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *shape: torch.randn(shape, generator=g).to(BF)
    d = dict(q=mk(sum(c.lq), c.Hq, c.D), k=mk(sum(c.lk), c.Hkv, c.D), v=mk(sum(c.lk), c.Hkv, c.D))
    d["qr"], d["kr"] = d["q"], d["k"]
    if c.rope:
        d["cos"], d["sin"] = rope_tables(c.lq, c.D)
        d["qr"] = rope_rotate(d["q"], d["cos"], d["sin"])
        if c.rope == "qk":
            d["kr"] = rope_rotate(d["k"], d["cos"], d["sin"])
        else:
            d["k"] = d["kr"] = rope_rotate(d["k"], d["cos"], d["sin"])    # keys arrive rotated
    return d


@functools.lru_cache(maxsize=None)
def case_refs(name):
    """(operands dict, cu_q, cu_k, scale, exact FwdRef, model FwdRef) of a table case (seeded by its position): computed once, shared, never modified."""
    c = BY_NAME[name]
    d = make_operands(c, seed=500 + CASES.index(c))
    cq, ck, scale = cu(c.lq), cu(c.lk), c.D ** -0.5
    exact = attn_fwd_ref(d["qr"], d["kr"], d["v"], cq, ck, scale, c.causal, c.block)
    model = attn_fwd_ref(d["qr"], d["kr"], d["v"], cq, ck, scale, c.causal, c.block, model=True)
    return d, cq, ck, scale, exact, model


def model_worst_row(name):
    """The yardstick of a case: the worst row of its bf16 model against its exact result."""
    _, _, _, _, exact, model = case_refs(name)
    return float(row_errors(model.o, exact.o).max())


# ---------------------------------------------------------------------------------------------------------------- checkers
def lse_bound(q, k, cu_q, cu_k, scale, causal, block, lse):
    """[Hq, Tq] float64: what a kernel's f32 lse may differ from the float64 one by, derived:  D 2^-23 scale max_j sum_i |q_i| |k_ji| over the visible keys j (a score
    accumulated in f32 over D terms; the logsumexp moves by no more than its worst score) + 8 2^-23 max(1, |lse|) (exp2, the row sum, the logarithm, the final
    product and sum).  Rows without a visible key get 0: their lse is -inf exactly."""
    Tq, Hq, D = q.shape
    G = Hq // k.shape[1]
    out = torch.zeros((Hq, Tq), dtype=torch.float64)
    for s in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[s]), int(cu_q[s + 1]), int(cu_k[s]), int(cu_k[s + 1])
        if q1 == q0 or k1 == k0:
            continue
        Q = q[q0:q1].double().abs().permute(1, 0, 2)
        K = k[k0:k1].double().abs().permute(1, 0, 2).repeat_interleave(G, 0)
        A = (Q @ K.transpose(1, 2)).masked_fill(~seg_visible(q1 - q0, k1 - k0, causal, block)[None], 0.0)
        out[:, q0:q1] = D * 2.0 ** -23 * float(scale) * A.max(-1).values
    seen = torch.isfinite(lse)
    return torch.where(seen, out + 8 * 2.0 ** -23 * lse.abs().clamp_min(1.0).nan_to_num(posinf=1.0), torch.zeros_like(out))


def where(cu_q, tok, head):
    seg, row = segment_of(cu_q, tok)
    return f"token {tok} head {head} (segment {seg}, row {row}, 16-row tile {row // 16})"


def check_rows(what, o, lse, exact, yard, factor, cu_q, bound):
    """The per-row check of a forward result (o [Tq, Hq, D], lse [Hq, Tq] or None, CPU) against the float64 FwdRef `exact`:
      * o finite everywhere, lse finite except -inf exactly where exact.lse is;
      * rows that are zero in the reference (no visible key) exactly zero;
      * every row of o within factor x yard of the exact row (row_errors: relative to the row, floored at a tenth of the median row);
      * every lse within `bound` [Hq, Tq] (lse_bound) of the exact one.
    Raises AssertionError naming the token, head, segment, row and 16-row tile; prints and returns (worst row / yard, worst lse error / its bound)."""
    o = o.double()
    bad = (~torch.isfinite(o)).any(-1).nonzero()
    assert bad.numel() == 0, f"{what}: o not finite at {where(cu_q, *bad[0].tolist())} ({bad.shape[0]} rows)"
    dead = torch.isinf(exact.lse).t()                                               # [Tq, Hq]
    nz = ((o != 0).any(-1) & dead).nonzero()
    assert nz.numel() == 0, f"{what}: a row without a visible key is not zero at {where(cu_q, *nz[0].tolist())}"
    e = row_errors(o, exact.o)
    tok, head = divmod(int(e.argmax()), e.shape[1])
    ratio = float(e.max()) / yard
    frac = 0.0
    if lse is not None:
        lse = lse.double()
        wrong = (torch.isinf(exact.lse) != (lse == float("-inf"))) | torch.isnan(lse) | (lse == float("inf"))
        if wrong.any():
            h, t = wrong.nonzero()[0].tolist()
            raise AssertionError(f"{what}: lse {float(lse[h, t])} where the reference has {float(exact.lse[h, t])} at {where(cu_q, t, h)}")
        seen = torch.isfinite(exact.lse)
        err = torch.where(seen, (lse - exact.lse).abs(), torch.zeros_like(lse)).nan_to_num()
        rel = torch.where(seen, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        h, t = divmod(int(rel.argmax()), rel.shape[1])
        frac = float(rel.max())
        assert frac <= 1.0, f"{what}: lse off by {float(err[h, t]):.3e}, allowed {float(bound[h, t]):.3e}, at {where(cu_q, t, h)}"
    print(f"{what}: worst row {float(e.max()):.5f} = {ratio:.3f} x model {yard:.5f}; rel-L2 {rel_l2(o, exact.o):.5f}; worst lse error {frac:.3f} of its bound")
    assert float(e.max()) <= factor * yard, f"{what}: {where(cu_q, tok, head)} is off by {float(e.max()):.5f} of its norm, allowed {factor} x {yard:.5f}"
    return ratio, frac


def check_case(name, o, lse, what="kernel"):
    """check_rows of a table case with its own yardstick, factor (FACTOR, + 1 for the extra rounding of rotated operands) and lse bound."""
    c = BY_NAME[name]
    d, cq, ck, scale, exact, _ = case_refs(name)
    bound = lse_bound(d["qr"], d["kr"], cq, ck, scale, c.causal, c.block, exact.lse)
    return check_rows(f"{what} {name}", o, lse, exact, model_worst_row(name), FACTOR + (1 if c.rope else 0), cq, bound)


# ---- exact mask: one-hot values
def slice_starts(c):
    """Per segment, the first key of each split slice by the kernel's rule (SPLIT in attn_fwd_kernel): tiles of 64 keys, per = ceil(tiles / nsplit) tiles a slice,
    nsplit as rga3_attn_varlen_fwd sets it.  [] for a case that is not split."""
    if c.family != "split":
        return [[] for _ in c.lk]
    wgs = -(-max(c.lq) // 64) * c.Hq * len(c.lq)
    ns = min(256 // wgs, 8, max(c.lk) // 512)
    out = []
    for Lk in c.lk:
        tiles = -(-Lk // 64)
        per = -(-tiles // ns)
        out.append([i * per * 64 for i in range(ns) if i * per < tiles])
    return out


def needle_keys(c):
    """Global key indices worth a needle, sorted: around the causal diagonal of rows 0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, the last row of a block and of the
    segment (the diagonal key r + shift and the first one past it); key 0 and Lk - 1 of every segment (so also the first key of the NEXT one); keys 63, 64, 127, 128;
    the first key of each split slice; the first and last key of packed blocks."""
    keys = set()
    starts = slice_starts(c)
    k0 = 0
    for s, (Lq, Lk) in enumerate(zip(c.lq, c.lk)):
        local = {0, Lk - 1, 63, 64, 127, 128} | set(starts[s])
        if c.causal:
            for r in (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, Lq - 1):
                if r < Lq:
                    local |= {r + Lk - Lq, r + Lk - Lq + 1}
        if c.block:
            bk = c.block[1]
            local |= {0, bk - 1, bk, 2 * bk - 1, Lk - bk}
        keys |= {k0 + x for x in local if 0 <= x < Lk}
        k0 += Lk
    return sorted(keys)


def needle_values(c, keys, hk):
    """v [Tk, Hkv, D] bf16, zero except v[keys[n], hk, n] = 1: column n of o[r, h] IS P[r, keys[n]] for the query heads of kv head hk, and 0 for every other head.
    hk = None: in every kv head, so every query head shows its own P."""
    assert len(keys) <= c.D
    v = torch.zeros((sum(c.lk), c.Hkv, c.D), dtype=BF)
    for n, key in enumerate(keys):
        v[key, slice(None) if hk is None else hk, n] = 1.0
    return v


def check_needles(what, o, want, cu_q):
    """o against the float64 result `want` of the same one-hot call: exactly zero (either sign) wherever want is exactly zero -- a key the row cannot see, another
    segment, another block, the query heads of another kv group, the columns without a needle -- and within 2^-7 P + 1e-30 of P elsewhere (two bf16 roundings of at most
    2^-9 each, of the exponential and of the output, plus f32-level terms, times two; 1e-30 for exponentials the hardware flushes)."""
    o = o.double()
    assert torch.isfinite(o).all(), f"{what}: not finite"
    leak = ((want == 0) & (o != 0)).nonzero()
    if leak.numel():
        t, h, n = leak[0].tolist()
        raise AssertionError(f"{what}: needle {n} leaks {float(o[t, h, n]):.3e} into {where(cu_q, t, h)}, which cannot see it ({leak.shape[0]} such elements)")
    off = ((o - want).abs() > 2.0 ** -7 * want + 1e-30).nonzero()
    if off.numel():
        t, h, n = off[0].tolist()
        raise AssertionError(f"{what}: P of needle {n} is {float(o[t, h, n]):.6e}, float64 has {float(want[t, h, n]):.6e}, at {where(cu_q, t, h)} ({off.shape[0]} such elements)")
