"""CPU: the bf16 GEMM tile table (csrc/gemm_bf16.hip kTiles) as rga3_gemm_tiles reports it (host only, no device call): the tilings each entry point accepts, in the
order the tuner tries them, and their shapes.  The expected lists are the literals the entry points' validity checks and rga3.hip.ops spelled out by hand before the
table existed; the entry points now validate against the rows this query reads.
No reference counterpart (the reference's GEMMs are vendor BLAS calls: HF modeling_qwen2_5_vl.py:211-321 via reference model/qwen_2_5_vl_sam2.py:182-200)."""
import ctypes as C

import pytest

from rga3.hip import lib, tuner

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


def test_tuner_candidates_are_plain_tilings():
    assert set(tuner.CANDIDATES) <= set(lib.gemm_tiles("plain"))


def test_unknown_ids_and_entries_are_rejected():
    for entry in (-1, 6, 99):
        assert query(entry)[0] < 0
        assert "gemm_tiles" in lib.last_error()
    known = set(PLAIN)
    for entry in range(6):
        assert {t for t, _, _ in query(entry)[1]} <= known      # no id outside the table: 0 - 2, 9, 15 - 19, 24, 29, 30, 33 - 39 and beyond stay unknown everywhere
    with pytest.raises(ValueError):
        lib.gemm_tiles("nope")
