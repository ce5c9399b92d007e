"""float64 reference of ops.attn_varlen_bwd (csrc/attn_bwd.hip) and the builders its tests share (no tests in this module).

The call, for every segment s with queries cu_q[s] .. cu_q[s + 1] and keys cu_k[s] .. cu_k[s + 1] (Lq and Lk of them), query head hq reading kv head
hq // (Hq // Hkv):  vis[q, key] = !causal || key <= q + (Lk - Lq);  lse[q] = logsumexp of scale * q.k over the visible keys, rounded to f32 (-inf where none is
visible);  P = exp(scale * q.k - lse) on visible entries, 0 elsewhere;  o = bf16(P V).  The backward is the kernels' own formula:
delta = rowsum(dO * o) with that bf16 o,  dS = P * (dO V^T - delta) * scale,  dQ = dS K,  dK = sum over the group of dS^T Q,  dV = sum over the group of P^T dO.
Everything here runs on the CPU in float64 from the exact values of the bf16 inputs; with model=True the roundings the kernels declare are applied as well
(P and dS to bf16 before the three products, the three outputs to bf16): that is the yardstick a kernel's error is measured with, never the expectation."""
import collections

import torch

BF = torch.bfloat16

Ref = collections.namedtuple("Ref", "o lse dq dk dv")   # o [Tq, Hq, D] bf16, lse [Hq, Tq] f32, dq [Tq, Hq, D] / dk, dv [Tk, Hkv, D] float64


def bf16_of(x64):
    """float64 -> the nearest bf16 number (through f32), as float64."""
    return x64.float().to(BF).double()


def cu(lens):
    """Segment lengths -> int32 prefix sums [len(lens) + 1]."""
    out = torch.zeros(len(lens) + 1, dtype=torch.int32)
    out[1:] = torch.tensor(list(lens), dtype=torch.int64).cumsum(0).to(torch.int32)
    return out


def make_case(lq, lk, Hq, Hkv, D, seed):
    """Seeded randn bf16 operands of one call: dict(q, do [Tq, Hq, D], k, v [Tk, Hkv, D])."""
    g = torch.Generator().manual_seed(seed)
    Tq, Tk = sum(lq), sum(lk)
    mk = lambda *shape: torch.randn(shape, generator=g).to(BF)
    return dict(q=mk(Tq, Hq, D), k=mk(Tk, Hkv, D), v=mk(Tk, Hkv, D), do=mk(Tq, Hq, D))


def visible(Lq, Lk, causal):
    """[Lq, Lk] bool."""
    if not causal:
        return torch.ones((Lq, Lk), dtype=torch.bool)
    return torch.arange(Lk)[None, :] <= torch.arange(Lq)[:, None] + (Lk - Lq)


def attn_bwd_ref(q, k, v, do, cu_q, cu_k, scale, causal, model=False):
    """CPU bf16 tensors as ops.attn_varlen_bwd takes them -> Ref.  A segment without queries leaves the dk, dv of its keys at zero, one without keys leaves dq = 0,
    o = 0 and lse = -inf; a row that sees no key has lse = -inf, o = 0 and dq = 0."""
    Tq, Hq, D = q.shape
    Tk, Hkv, _ = k.shape
    G = Hq // Hkv
    rnd = bf16_of if model else (lambda x: x)
    o = torch.zeros((Tq, Hq, D), dtype=torch.float64)
    lse = torch.full((Hq, Tq), float("-inf"), dtype=torch.float64)
    dq = torch.zeros((Tq, Hq, D), dtype=torch.float64)
    dk = torch.zeros((Tk, Hkv, D), dtype=torch.float64)
    dv = torch.zeros((Tk, Hkv, D), dtype=torch.float64)
    for s in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[s]), int(cu_q[s + 1]), int(cu_k[s]), int(cu_k[s + 1])
        Lq, Lk = q1 - q0, k1 - k0
        if Lq == 0 or Lk == 0:
            continue
        Q = q[q0:q1].double().permute(1, 0, 2)                                      # [Hq, Lq, D]
        dO = do[q0:q1].double().permute(1, 0, 2)
        K = k[k0:k1].double().permute(1, 0, 2).repeat_interleave(G, 0)              # [Hq, Lk, D]
        V = v[k0:k1].double().permute(1, 0, 2).repeat_interleave(G, 0)
        vis = visible(Lq, Lk, causal)[None]
        S = (Q @ K.transpose(1, 2)) * float(scale)
        L = torch.logsumexp(S.masked_fill(~vis, float("-inf")), dim=-1).float().double()   # [Hq, Lq], -inf on rows without a visible key
        P = torch.where(vis & torch.isfinite(L)[..., None], torch.exp(S - torch.where(torch.isfinite(L), L, torch.zeros_like(L))[..., None]), torch.zeros_like(S))
        O = bf16_of(P @ V)
        delta = (dO * O).sum(-1, keepdim=True)
        dS = rnd(P * (dO @ V.transpose(1, 2) - delta) * float(scale))
        o[q0:q1] = O.permute(1, 0, 2)
        lse[:, q0:q1] = L
        dq[q0:q1] = (dS @ K).permute(1, 0, 2)
        dk[k0:k1] = (dS.transpose(1, 2) @ Q).view(Hkv, G, Lk, D).sum(1).permute(1, 0, 2)
        dv[k0:k1] = (rnd(P).transpose(1, 2) @ dO).view(Hkv, G, Lk, D).sum(1).permute(1, 0, 2)
    return Ref(o.to(BF), lse.float(), rnd(dq), rnd(dk), rnd(dv))


def row_errors(got, want):
    """[T, H, D] x 2 -> [T, H] float64: |got - want|_2 / max(|want|_2, 0.1 * median nonzero row norm of want) per (token, head).  The floor is there because some rows
    are exactly zero in the mathematics (dq of a causal row that sees one key: its softmax is constant)."""
    got, want = got.double().cpu(), want.double().cpu()
    n = want.norm(dim=-1)
    nz = n[n > 0]
    floor = 0.1 * float(nz.median()) if nz.numel() else 1.0
    return (got - want).norm(dim=-1) / n.clamp_min(floor)


def rel_l2(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).norm() / (want.norm() + 1e-300))


def segment_of(cu_, token):
    """(segment index, row inside it) of a token of the concatenated batch."""
    s = int(torch.searchsorted(cu_[1:].long(), int(token), right=True))
    return s, int(token) - int(cu_[s])


# The case table of tests/test_attn_bwd_gpu.py: the smallest shapes that reach each path of launch_bwd.  The dQ kernel's block is 128 query rows at every D; the dK / dV
# kernel's is 128 keys at D = 128 (8 waves) and 64 keys below (4 waves).  The paired causal route (PAIR) is taken when causal && cdiv(max_q, 128) >= 4 &&
# cdiv(max_k, dK / dV block) >= 4; the GQA split (SPLIT) whenever Hq > Hkv and a workspace is passed, as ops.attn_varlen_bwd does.
Case = collections.namedtuple("Case", "name lq lk Hq Hkv D causal")
MULTI = [640, 130, 1, 385]
CASES = [
    Case("513-gqa2-d128", [513], [513], 4, 2, 128, True),                 # PAIR + SPLIT, 5 blocks (unpaired middle), last block of 1 row
    Case("multi-mha-d128", MULTI, MULTI, 2, 2, 128, True),                # PAIR non-split, segments with 5 / 2 / 1 / 4 blocks under one grid
    Case("multi-gqa4-d128", MULTI, MULTI, 4, 1, 128, True),               # the same with SPLIT, group of 4 (also run with dkv_ws = NULL)
    Case("512-gqa3-d64", [512], [512], 6, 2, 64, True),                   # PAIR on the QT = 2, 4-wave kernels, 8 key blocks
    Case("400x464-d80", [400], [464], 2, 1, 80, True),                    # PAIR, shift +64, D < DP = 96
    Case("400x437-d72", [400], [437], 2, 1, 72, True),                    # PAIR, shift not a multiple of any tile
    Case("385-d32", [385], [385], 2, 2, 32, True),                        # PAIR, DP = 32
    Case("390-d16", [390], [390], 2, 1, 16, True),                        # PAIR, D < DP = 32
    Case("empty-q-segment", [300, 0, 77], [300, 40, 77], 4, 2, 128, True),  # 40 keys without a query: dk = dv = 0 exactly
    Case("negative-shift", [200], [136], 2, 2, 64, True),                 # 64 rows see no key (lse = -inf): all finite, those dq rows exactly 0
    Case("70-noncausal-d32", [70], [70], 2, 2, 32, False),                # non-PAIR baseline
    Case("cross-9x64-d16", [9, 9], [64, 64], 8, 8, 16, False),            # cross attention, max_k != max_q
    Case("300-77-1-gqa2-d128", [300, 77, 1], [300, 77, 1], 4, 2, 128, True),  # the first case of test_train_gpu.py::test_attention_backward, now per row
]
BY_NAME = {c.name: c for c in CASES}


def case_operands(c):
    """The operands of a table case (seeded by its position) and its cu_q, cu_k, scale."""
    d = make_case(c.lq, c.lk, c.Hq, c.Hkv, c.D, seed=100 + CASES.index(c))
    return d, cu(c.lq), cu(c.lk), c.D ** -0.5


def case_refs(c):
    """(operands dict, cu_q, cu_k, scale, exact Ref, model Ref) of a table case."""
    d, cq, ck, scale = case_operands(c)
    exact = attn_bwd_ref(d["q"], d["k"], d["v"], d["do"], cq, ck, scale, c.causal)
    model = attn_bwd_ref(d["q"], d["k"], d["v"], d["do"], cq, ck, scale, c.causal, model=True)
    return d, cq, ck, scale, exact, model
