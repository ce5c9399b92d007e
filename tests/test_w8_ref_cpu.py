"""CPU: the properties of the weight-only e4m3 reference (tests/w8_ref.py) that the GPU tests of the decode path rely on."""
import pytest
import torch

from tests.w8_ref import SHAPES, dequant_ref, edge_matrix, quant_ref, snap_ref


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request):
    rows, K = request.param
    w = edge_matrix(rows, K, seed=rows + K)
    return w, quant_ref(w)


def test_scale_is_the_smallest_power_of_two_that_holds_the_row(case):
    w, (codes, scale) = case
    amax = w.float().abs().amax(dim=1)
    m, _ = torch.frexp(scale)
    assert bool((m == 0.5).all())                                   # powers of two
    nz = amax > 0
    r = amax[nz] / scale[nz]
    assert bool((r > 224).all()) and bool((r <= 448).all())
    assert bool((scale[~nz] == 1).all()) and bool((codes.view(torch.uint8)[~nz] == 0).all())
    if w.shape[0] > 2:
        assert scale[1].item() == 2.0 ** -12 and scale[2].item() == 2.0 ** -11      # amax = 448 * 2^-12 exactly, and one bf16 ulp above


def test_codes_are_never_nan_and_use_the_subnormals(case):
    w, (codes, _) = case
    c = codes.view(torch.uint8)
    assert not bool(((c & 0x7F) == 0x7F).any())
    if w.shape[0] > 3:
        assert bool((((c[3] & 0x78) == 0) & ((c[3] & 0x07) != 0)).any())            # exponent field 0, mantissa not: e4m3 subnormals
        assert int(c[3, 0]) == 0x7E                                                  # 448


def test_dequantised_values_are_bf16_numbers(case):
    _, (codes, scale) = case
    d = dequant_ref(codes, scale)
    assert torch.equal(d.to(torch.bfloat16).float(), d)


def test_requantising_reproduces_the_values(case):
    w, _ = case
    s1 = snap_ref(w)
    s2 = snap_ref(s1)
    assert torch.equal(s1.view(torch.int16), s2.view(torch.int16))
    # the (code, scale) pair may move: a row whose largest element rounded down to a binade boundary gets the smaller scale on the second pass
    assert bool((quant_ref(s1)[1] <= quant_ref(w)[1]).all())
