"""CPU: the bf16 GEMM tile table (csrc/gemm_bf16.hip kTiles) as rga3_gemm_tiles reports it (host only, no device call): the tilings each entry point accepts, in the
order the tuner tries them, and their shapes.  The expected lists are the literals the entry points' validity checks and rga3.hip.ops spelled out by hand before the
table existed; the entry points now validate against the rows this query reads.  Likewise rga3_gemm_candidates (which of them the tuner times for one product, in
trial order) against the literal lists rga3.hip.tuner and rga3.hip.ops held before the rule moved into the library, and rga3_gemm_tn_slices (the K slices of a TN
product) against its closed form.
No reference counterpart (the reference's GEMMs are vendor BLAS calls: HF modeling_qwen2_5_vl.py:211-321 via reference model/qwen_2_5_vl_sam2.py:182-200)."""
import ctypes as C

import pytest

from rga3.hip import lib

PLAIN = [3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 20, 21, 22, 23, 25, 26, 27, 28, 31, 32, 40, 41]
EXPECTED = {
    "plain": PLAIN,
    "shared": [t for t in PLAIN if t not in (14, 25, 40, 41)],
    "ln": [20, 3, 5, 12, 13, 6, 7],
    "lnsum": [20, 3, 5, 12, 13, 23],
    "cat_k": [12, 3, 4, 5, 6, 13],
    "cat_n": [12, 3, 6, 13],
}
WIDTH = {3: 256, 6: 256, 20: 256, 4: 320, 5: 192, 7: 192, 23: 192, 13: 64, 12: 128}


def query(entry, cap=64):
    ids, bm, bn = ((C.c_int * max(cap, 1))() for _ in range(3))
    n = lib.load().rga3_gemm_tiles(entry, ids, bm, bn, cap)
    return n, [(ids[i], bm[i], bn[i]) for i in range(min(max(n, 0), cap))]


def test_entry_order_matches_the_accessor():
    assert list(lib._TILE_ENTRIES) == list(EXPECTED)


@pytest.mark.parametrize("entry", list(EXPECTED))
def test_each_entry_point_lists_its_tilings_in_order(entry):
    n, rows = query(list(EXPECTED).index(entry))
    assert n == len(EXPECTED[entry]) and [r[0] for r in rows] == EXPECTED[entry]
    assert list(lib.gemm_tiles(entry)) == EXPECTED[entry]           # what rga3.hip.ops reads: same ids, same order
    for t, _, bn in rows:
        assert lib.gemm_tiles(entry)[t] == bn and (t not in WIDTH or bn == WIDTH[t]), (t, bn)
    assert query(list(EXPECTED).index(entry), cap=0) == (n, [])       # the count alone
    assert query(list(EXPECTED).index(entry), cap=2) == (n, rows[:2])  # a short buffer is not overrun


def test_widths_and_shapes():
    rows = {t: (bm, bn) for t, bm, bn in query(0)[1]}
    assert all(rows[t][1] == w for t, w in WIDTH.items())
    assert rows[11] == rows[12] == (128, 128)        # 11 is an alias of the 128 x 128 kernel (the static heuristic scores it as 256 x 128, a kernel that does not exist)
    assert rows[3][0] == 128 and rows[13] == (64, 64) and rows[20] == (256, 256) and rows[23] == (256, 192) and rows[31] == (192, 256)


def test_lnsum_slices_follow_the_table():
    so = lib.load()
    for t in EXPECTED["lnsum"]:
        for N in (64, 192, 576, 1280):
            assert so.rga3_gemm_lnsum_slices(N, t) == -(-N // WIDTH[t]), (N, t)
    assert so.rga3_gemm_lnsum_slices(576, -1) == so.rga3_gemm_lnsum_slices(576, 12)       # -1 is the 128 x 128 tiling
    for t in [t for t in PLAIN if t not in EXPECTED["lnsum"]] + [0, 9, 24, 99, -2]:
        assert so.rga3_gemm_lnsum_slices(576, t) == -1, t
    assert so.rga3_gemm_lnsum_slices(0, 12) == -1


B = [20, 21, 22, 27, 28, 31, 32, 12, 13, 3, 4, 5, 6]
NONE, GELU, SWIGLU = 0, 1, 2
BF16, F32 = 0, 1
BIAS, RESIDUAL, COLSCALE = 1, 2, 4
# (entry, (M, N, K), act, out_dtype, epilogue bits) -> trial order
TRIALS = [
    (0, (2112, 3584, 3584), NONE, BF16, 0, B),
    (0, (256, 256, 8192), NONE, BF16, 0, B + [25, 14]),
    (0, (256, 256, 8192), NONE, BF16, BIAS, B + [25]),
    (0, (256, 256, 8192), NONE, BF16, RESIDUAL, B),
    (0, (1024, 1024, 4096), NONE, BF16, 0, B + [25]),           # M N = 2^20
    (0, (1024, 1032, 4096), NONE, BF16, 0, B),                  # just above
    (0, (256, 256, 4088), NONE, BF16, 0, B + [14]),             # K below 4096
    (0, (256, 256, 504), NONE, BF16, 0, B),                     # K below 512
    (0, (256, 20, 8192), NONE, BF16, 0, B + [25]),              # N % 8
    (0, (16, 1024, 4096), NONE, BF16, 0, B + [25, 14, 41]),
    (0, (16, 1024, 4096), NONE, F32, 0, B + [25, 14]),
    (0, (16, 1024, 4096), NONE, BF16, COLSCALE, B),
    (0, (16, 4096, 4096), GELU, BF16, BIAS, B + [41]),
    (0, (16, 4096, 4096), SWIGLU, BF16, 0, B),
    (0, (1024, 576, 576), NONE, BF16, 0, B + [23]),
    (0, (1023, 576, 576), NONE, BF16, 0, B),
    (0, (1024, 768, 576), NONE, BF16, 0, B),
    (0, (1024, 576, 576), GELU, BF16, 0, B),
    (0, (256, 256, 256), SWIGLU, BF16, BIAS, B),                # what gemm_swiglu_pre asks
    (1, (2112, 3584, 3584), NONE, BF16, 0, B),
    (1, (16, 1024, 4096), NONE, BF16, 0, B),                    # entry 1: no extras at any shape
    (1, (1024, 576, 576), NONE, BF16, BIAS | RESIDUAL, B),
    (2, (256, 256, 256), GELU, BF16, BIAS, [20, 3, 5, 12, 13, 6, 7]),
    (3, (1024, 576, 64), NONE, BF16, 0, [20, 3, 5, 12, 13, 23]),
    (3, (1023, 576, 64), NONE, BF16, RESIDUAL, [20, 3, 5, 12, 13]),
    (3, (1024, 768, 64), NONE, BF16, 0, [20, 3, 5, 12, 13]),
    (4, (256, 576, 64), NONE, BF16, 0, [12, 3, 4, 5, 6, 13]),   # a K side alone: every width
    (5, (256, 768, 64), NONE, BF16, 0, [12, 3, 6, 13]),
    (5, (256, 640, 64), NONE, BF16, BIAS, [12, 13]),
    (5, (256, 576, 64), NONE, BF16, 0, [13]),
]


def candidates(entry, shape, act, odt, epi, cap=64):
    ids = (C.c_int * (max(cap, 0) + 1))(*([-7] * (max(cap, 0) + 1)))
    n = lib.load().rga3_gemm_candidates(entry, *shape, act, odt, epi, ids, cap)
    assert ids[max(cap, 0)] == -7                               # nothing written behind `cap`
    return n, list(ids[:min(max(n, 0), max(cap, 0))])


@pytest.mark.parametrize("entry,shape,act,odt,epi,want", TRIALS)
def test_tuner_candidates_per_product(entry, shape, act, odt, epi, want):
    """The literal lists rga3.hip.ops handed to tuner.pick before the rule moved into the library (the tuner's base list + the `extra` block of ops.gemm, the filters of
    gemm_lnsum / gemm_cat), on both sides of every predicate."""
    assert candidates(entry, shape, act, odt, epi) == (len(want), want)
    assert candidates(entry, shape, act, odt, epi, cap=0) == (len(want), [])        # the count alone
    assert candidates(entry, shape, act, odt, epi, cap=1) == (len(want), want[:1])  # a short buffer is not overrun
    M, N, K = shape
    assert lib.gemm_candidates(lib._TILE_ENTRIES[entry], M, N, K, act, odt, bool(epi & BIAS), bool(epi & RESIDUAL), bool(epi & COLSCALE)) == tuple(want)


def test_tuner_candidates_are_plain_tilings():
    """Every tiling the tuner is told to time for an entry point is one that entry point has a kernel for (rga3_gemm_tiles of the same entry), at every product above
    and with every epilogue; for rga3_gemm_bf16 in particular they are plain tilings."""
    for entry, shape, act, odt, _, _ in TRIALS:
        for epi in range(8):
            n, ids = candidates(entry, shape, act, odt, epi)
            assert 0 < n == len(ids) == len(set(ids)) and set(ids) <= set(lib.gemm_tiles(lib._TILE_ENTRIES[entry])), (entry, shape, act, odt, epi, ids)


def test_candidates_of_bad_arguments_are_refused():
    for entry, shape in ((-1, (64, 64, 64)), (6, (64, 64, 64)), (0, (0, 64, 64)), (0, (64, -8, 64)), (2, (64, 64, 0))):
        assert candidates(entry, shape, NONE, BF16, 0)[0] < 0, (entry, shape)
        assert "gemm_candidates" in lib.last_error()
    assert lib.load().rga3_gemm_candidates(0, 64, 64, 64, NONE, BF16, 0, None, 4) < 0 and "gemm_candidates" in lib.last_error()   # room promised, no buffer


def tn_slices_closed_form(M, N, K):
    tiles, nk = -(-M // 128) * -(-N // 128), -(-K // 32)
    if tiles >= 128 or nk < 32:
        return 1
    z = min(64, 256 // tiles, nk // 8)
    return z if z >= 2 else 1


def test_tn_slices():
    """rga3_gemm_tn_slices = the slabs a TN product's workspace must hold: 256 CUs' worth of 128 x 128 tiles, at most 64 slices, at least 8 K-tiles of 32 each."""
    fn = lib.load().rga3_gemm_tn_slices
    for M, N in ((128, 128), (128, 3584), (1024, 1024), (1408, 1408)):
        for K in range(1, 5001):
            assert fn(M, N, K) == tn_slices_closed_form(M, N, K), (M, N, K)
    for K, z in ((1000, 4), (1024, 4), (1272, 5), (2112, 8), (4160, 16), (65536, 64), (992, 1)):
        assert fn(128, 128, K) == z == lib.gemm_tn_slices(128, 128, K), K
    for bad in ((0, 128, 128), (128, -8, 128), (128, 128, 0)):
        assert fn(*bad) < 0 and "gemm_tn_slices" in lib.last_error()


def test_unknown_ids_and_entries_are_rejected():
    for entry in (-1, 6, 99):
        assert query(entry)[0] < 0
        assert "gemm_tiles" in lib.last_error()
    known = set(PLAIN)
    for entry in range(6):
        assert {t for t, _, _ in query(entry)[1]} <= known      # no id outside the table: 0 - 2, 9, 15 - 19, 24, 29, 30, 33 - 39 and beyond stay unknown everywhere
    with pytest.raises(ValueError):
        lib.gemm_tiles("nope")
