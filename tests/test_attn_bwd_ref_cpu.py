"""CPU: the float64 reference of ops.attn_varlen_bwd (tests/attn_bwd_ref.py) against float64 autograd through a plain masked softmax attention, its edge cases
(a row that sees no key, segments without queries or without keys), its bf16 error model on every case of the GPU table, and row_errors on a planted fault."""
import functools

import pytest
import torch

from tests import attn_bwd_ref as R

MODEL_BOUND = 0.008     # worst-row error of the model=True yardstick against the exact result (measured 0.0032 .. 0.0056: essentially the final bf16 rounding)
GPU_FACTOR = 3          # tests/test_attn_bwd_gpu.py allows a kernel GPU_FACTOR times the model's worst row


@functools.lru_cache(maxsize=None)
def refs(name):
    return R.case_refs(R.BY_NAME[name])


def autograd_attention(d, cq, ck, scale, causal):
    """float64 autograd through softmax(mask(scale q k^T)) v, segment by segment -> (o, dq, dk, dv, P per segment as [Hq, Lq, Lk])."""
    q, k, v = (d[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    G = q.shape[1] // k.shape[1]
    outs, Ps = [], []
    for s in range(len(cq) - 1):
        q0, q1, k0, k1 = int(cq[s]), int(cq[s + 1]), int(ck[s]), int(ck[s + 1])
        Q = q[q0:q1].permute(1, 0, 2)
        K = k[k0:k1].permute(1, 0, 2).repeat_interleave(G, 0)
        V = v[k0:k1].permute(1, 0, 2).repeat_interleave(G, 0)
        S = (Q @ K.transpose(1, 2)) * scale
        P = torch.softmax(S.masked_fill(~R.visible(q1 - q0, k1 - k0, causal)[None], float("-inf")), dim=-1)
        outs.append((P @ V).permute(1, 0, 2))
        Ps.append(P.detach())
    o = torch.cat(outs, 0)
    o.backward(d["do"].double())
    return o.detach(), q.grad, k.grad, v.grad, Ps


def rounding_bounds(d, cq, ck, scale, o, lse, Ps):
    """Per-element bounds on |reference - autograd| for dq, dk, dv.  The reference differs from the mathematics in two places only:
      * it takes delta = rowsum(dO * bf16(o)).  A bf16 number has 8 significant bits, so |o - bf16(o)| <= half an ulp = 2^-9 * 2^e with 2^e the power of two above |o|
        (2^-9 |o| < that <= 2^-8 |o|); the reference's o is in addition formed from P (1 + d), below.  So |delta_ref - delta| <= sum_d |dO| (2^-9 2^e + 2 dl |o|).
      * it takes P = exp(s - f32(lse)): P_ref = P (1 + d) with |d| <= dl = expm1(2^-24 |lse|) (f32 rounds to nearest: 2^-24 relative).
    Hence |dS_ref - dS| <= scale (P dl |dO V^T - delta| + P (1 + dl) |delta_ref - delta|) and |P_ref - P| <= P dl, carried through the three products with absolute values.
    1e-12 absolute covers the float64 evaluation itself."""
    q, k, v, do = (d[n].double() for n in ("q", "k", "v", "do"))
    G = q.shape[1] // k.shape[1]
    bq, bk, bv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for s, P in enumerate(Ps):
        q0, q1, k0, k1 = int(cq[s]), int(cq[s + 1]), int(ck[s]), int(ck[s + 1])
        Hkv, Lk, D = k.shape[1], k1 - k0, q.shape[2]
        Q, dO, O = (t[q0:q1].permute(1, 0, 2) for t in (q, do, o))
        K = k[k0:k1].permute(1, 0, 2).repeat_interleave(G, 0)
        V = v[k0:k1].permute(1, 0, 2).repeat_interleave(G, 0)
        dl = torch.expm1(2.0 ** -24 * lse[:, q0:q1].double().abs())[..., None]                   # [Hq, Lq, 1]
        pow2 = torch.where(O == 0, torch.zeros_like(O), torch.ldexp(torch.ones_like(O), torch.frexp(O)[1]))
        ddelta = (dO.abs() * (2.0 ** -9 * pow2 + 2 * dl * O.abs())).sum(-1, keepdim=True)
        delta = (dO * O).sum(-1, keepdim=True)
        dds = scale * (P * dl * (dO @ V.transpose(1, 2) - delta).abs() + P * (1 + dl) * ddelta)
        bq[q0:q1] = (dds @ K.abs()).permute(1, 0, 2)
        bk[k0:k1] = (dds.transpose(1, 2) @ Q.abs()).view(Hkv, G, Lk, D).sum(1).permute(1, 0, 2)
        bv[k0:k1] = ((P * dl).transpose(1, 2) @ dO.abs()).view(Hkv, G, Lk, D).sum(1).permute(1, 0, 2)
    return bq + 1e-12, bk + 1e-12, bv + 1e-12


@pytest.mark.parametrize("lq,lk,Hq,Hkv,D,causal", [([37, 5, 1], [37, 5, 1], 4, 2, 16, True), ([9, 6], [20, 11], 3, 3, 8, False), ([12], [19], 2, 1, 24, True)])
def test_reference_equals_float64_autograd_up_to_the_rounding_of_o(lq, lk, Hq, Hkv, D, causal):
    d = R.make_case(lq, lk, Hq, Hkv, D, seed=sum(lq) + D)
    cq, ck, scale = R.cu(lq), R.cu(lk), D ** -0.5
    ref = R.attn_bwd_ref(d["q"], d["k"], d["v"], d["do"], cq, ck, scale, causal)
    o, dq, dk, dv, Ps = autograd_attention(d, cq, ck, scale, causal)
    assert ((ref.o.double() - o).abs() <= 2.0 ** -8 * (1 + 1e-5) * o.abs()).all()
    lse_want = torch.cat([torch.logsumexp(((d["q"][int(cq[s]):int(cq[s + 1])].double().permute(1, 0, 2)
                                            @ d["k"][int(ck[s]):int(ck[s + 1])].double().permute(1, 0, 2).repeat_interleave(Hq // Hkv, 0).transpose(1, 2)) * scale)
                                           .masked_fill(~R.visible(lq[s], lk[s], causal)[None], float("-inf")), -1) for s in range(len(lq))], 1)
    assert torch.equal(ref.lse, lse_want.float())
    bq, bk, bv = rounding_bounds(d, cq, ck, scale, o, ref.lse, Ps)
    for name, got, want, bound in (("dq", ref.dq, dq, bq), ("dk", ref.dk, dk, bk), ("dv", ref.dv, dv, bv)):
        err = (got - want).abs()
        assert (err <= bound).all(), (name, float((err - bound).max()))
        assert R.rel_l2(got, want) < 1e-2, name
    assert R.rel_l2(ref.dv, dv) < 1e-6                     # dV does not read o at all


def test_a_row_that_sees_no_key():
    """Lq = 7, Lk = 4, causal: shift = -3, rows 0 .. 2 see no key."""
    d = R.make_case([7], [4], 2, 1, 8, seed=1)
    for model in (False, True):
        ref = R.attn_bwd_ref(d["q"], d["k"], d["v"], d["do"], R.cu([7]), R.cu([4]), 0.3, True, model=model)
        assert all(torch.isfinite(t.double()).all() for t in (ref.o, ref.dq, ref.dk, ref.dv))
        assert (ref.lse[:, :3] == float("-inf")).all() and torch.isfinite(ref.lse[:, 3:]).all()
        assert (ref.dq[:3] == 0).all() and (ref.o[:3] == 0).all()
        assert (ref.dq[3] == 0).all()                      # one visible key: the softmax is constant
        assert (ref.dq[4:] != 0).any() and (ref.dk != 0).any() and (ref.dv != 0).any()


def test_zero_length_segments():
    lq, lk = [5, 0, 3, 4], [5, 6, 0, 4]
    d = R.make_case(lq, lk, 4, 2, 8, seed=2)
    ref = R.attn_bwd_ref(d["q"], d["k"], d["v"], d["do"], R.cu(lq), R.cu(lk), 0.35, True)
    assert (ref.dk[5:11] == 0).all() and (ref.dv[5:11] == 0).all()               # keys nobody queries
    assert (ref.dq[5:8] == 0).all() and (ref.o[5:8] == 0).all() and (ref.lse[:, 5:8] == float("-inf")).all()   # queries without a key
    # the segments around them equal the same segments run alone
    for qa, qb, ka, kb in ((0, 5, 0, 5), (8, 12, 11, 15)):
        alone = R.attn_bwd_ref(d["q"][qa:qb], d["k"][ka:kb], d["v"][ka:kb], d["do"][qa:qb], R.cu([qb - qa]), R.cu([kb - ka]), 0.35, True)
        assert torch.equal(alone.dq, ref.dq[qa:qb]) and torch.equal(alone.dk, ref.dk[ka:kb]) and torch.equal(alone.dv, ref.dv[ka:kb])
        assert torch.equal(alone.lse, ref.lse[:, qa:qb]) and torch.equal(alone.o, ref.o[qa:qb])


def test_cu_and_segment_of():
    c = R.cu([640, 130, 1, 385])
    assert c.dtype == torch.int32 and c.tolist() == [0, 640, 770, 771, 1156]
    assert R.segment_of(c, 0) == (0, 0) and R.segment_of(c, 639) == (0, 639) and R.segment_of(c, 640) == (1, 0) and R.segment_of(c, 770) == (2, 0)
    assert R.segment_of(c, 1155) == (3, 384)
    assert R.segment_of(R.cu([3, 0, 2]), 3) == (2, 0)      # an empty segment owns no token


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_model_error_stays_where_it_was_measured(name):
    """The yardstick of the GPU tests must not drift: the worst row of the bf16 model against the exact result is below MODEL_BOUND for every tensor of every case."""
    _, _, _, _, exact, model = refs(name)
    for t in ("dq", "dk", "dv"):
        worst = float(R.row_errors(getattr(model, t), getattr(exact, t)).max())
        assert 0 < worst < MODEL_BOUND, (name, t, worst)
        assert R.rel_l2(getattr(model, t), getattr(exact, t)) < 4e-3, (name, t)


def test_row_errors_flags_one_negated_element():
    """One element of one row replaced by its negation exceeds what the GPU tests allow (GPU_FACTOR times the model's worst row); the other rows stay at 0."""
    _, _, _, _, exact, model = refs("513-gqa2-d128")
    for t in ("dq", "dk", "dv"):
        want = getattr(exact, t)
        allowed = GPU_FACTOR * float(R.row_errors(getattr(model, t), want).max())
        got = want.clone()
        row = want[300, 1]
        i = int(row.abs().argsort()[row.numel() // 2])     # an element of median magnitude
        got[300, 1, i] = -got[300, 1, i]
        e = R.row_errors(got, want)
        assert e[300, 1] > allowed, (t, float(e[300, 1]), allowed)
        e[300, 1] = 0
        assert (e == 0).all()


def test_row_errors_floor():
    want = torch.zeros(4, 1, 8, dtype=torch.float64)
    want[1:] = 1.0                                          # row norms 0, sqrt(8) x 3: floor = 0.1 sqrt(8)
    got = want.clone()
    got[0, 0, 0] = 0.5
    got[2, 0, 0] = 1.5
    e = R.row_errors(got, want)
    assert torch.allclose(e[:, 0], torch.tensor([0.5 / (0.1 * 8 ** 0.5), 0.0, 0.5 / 8 ** 0.5, 0.0], dtype=torch.float64))
