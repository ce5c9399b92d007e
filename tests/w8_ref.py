"""CPU reference of the weight-only e4m3 format of the decode step (no tests in this module): one power-of-two scale per row, OCP e4m3 codes.

scale = 2^k with k the smallest integer such that amax <= 448 * 2^k, clamped to k >= -126 (1 for a zero row): with amax = m * 2^e, m in [0.5, 1) (frexp),
448 = 0.875 * 2^9 gives k = e - 9 if m <= 0.875, else e - 8.  code = e4m3(x / scale), round to nearest even; the division by a power of two is exact.
Every dequantised value code * 2^k has at most 4 significant bits and a bf16 exponent, so it is a bf16 number.
"""
import torch

SHAPES = ((72, 272), (4608, 3584), (96, 176), (5, 16))     # (rows, K) of the matrices the properties are checked on
VALID_CODES = tuple(c for c in range(256) if c & 0x7F != 0x7F)   # the 254 codes that are not NaN


def quant_ref(w):
    """bf16 [rows, K] (CPU) -> (torch.float8_e4m3fn codes [rows, K], f32 scales [rows])."""
    assert w.dtype == torch.bfloat16 and w.dim() == 2
    wf = w.float().cpu()
    amax = wf.abs().amax(dim=1)
    m, e = torch.frexp(amax)
    k = torch.where(m <= 0.875, e - 9, e - 8).clamp(min=-126)
    k = torch.where(amax == 0, torch.zeros_like(k), k)
    scale = torch.ldexp(torch.ones_like(amax), k)
    return (wf / scale[:, None]).to(torch.float8_e4m3fn), scale


def dequant_ref(codes, scale):
    """f32 [rows, K] = code * scale (exact)."""
    return codes.float() * scale[:, None]


def snap_ref(w):
    """bf16 -> bf16: the value every weight has after one quantise / dequantise round trip."""
    return dequant_ref(*quant_ref(w)).to(torch.bfloat16)


def edge_matrix(rows, K, seed=0):
    """A bf16 [rows, K] matrix (CPU) whose rows span 16 binades, with the edge rows the format has (as many as fit):
    row 0 all zero; row 1 with amax exactly 448 * 2^-12; row 2 with amax the next bf16 above that; row 3 with amax 448 * 2^3 and, from column 1 on, the
    multiples of half of e4m3's smallest subnormal at that scale (subnormal codes and their round-to-even ties)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-14, 3, (rows, 1), generator=g).float())
    edge = 448.0 * 2.0 ** -12
    if rows > 0:
        w[0] = 0
    if rows > 1:
        w[1] = w[1].clamp(-edge, edge)
        w[1, K // 2] = edge
    if rows > 2:
        w[2] = w[2].clamp(-edge, edge)
        w[2, K - 1] = -edge * (1 + 2.0 ** -7 / 1.75)        # 448 = 1.75 * 2^8: one bf16 ulp (2^-7 of the leading bit) above
    if rows > 3:
        j = torch.arange(K - 1).float()
        w[3, 1:] = (j % 20) * 0.5 * 2.0 ** -9 * 8.0 * torch.where(j % 2 == 0, 1.0, -1.0)
        w[3, 0] = 448.0 * 8.0
    return w.to(torch.bfloat16)
