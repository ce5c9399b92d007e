"""float64 reference of ops.decode_attn (csrc/decattn.hip) and the builders its tests share (no tests in this module).

The call, for every sequence b: rotate the Hq query heads and the Hkv new key heads of the fused qkv row (rotate-half: o1 = a c1 - b s1, o2 = b c2 + a s2, one bf16
rounding), store the rotated k row and the v row at cache position lens[b], and return softmax(scale q K^T) V over cache rows 0 .. lens[b] inclusive, query head hq
reading kv head hq // (Hq // Hkv).  Everything here runs on the CPU in float64 from the exact values of the bf16 / f32 inputs."""
import torch


def rotate_ref(x, cos, sin):
    """x [B, H, D], cos / sin [B, D] -> (exact rotation in float64, sum of the two products' magnitudes |a c| + |b s| per element)."""
    x, c, s = x.double(), cos.double()[:, None, :], sin.double()[:, None, :]
    h = x.shape[-1] // 2
    a, b = x[..., :h], x[..., h:]
    exact = torch.cat((a * c[..., :h] - b * s[..., :h], b * c[..., h:] + a * s[..., h:]), dim=-1)
    mag = torch.cat(((a * c[..., :h]).abs() + (b * s[..., :h]).abs(), (b * c[..., h:]).abs() + (a * s[..., h:]).abs()), dim=-1)
    return exact, mag


def rotation_bound(exact, mag):
    """Per element: |got - exact| <= 2^-8 |exact| + 2^-20 (|a c| + |b s|) -- one bf16 rounding (half an ulp of an 8-bit significand: at most 2^-8 relative) plus the f32
    evaluation of two products and a sum in either contraction (at most three roundings of 2^-24 each of magnitudes bounded by |a c| + |b s|)."""
    return 2.0 ** -8 * exact.abs() + 2.0 ** -20 * mag


def bf16_of(x64):
    """float64 -> the nearest bf16 number (through f32: the double rounding moves no value the tests use across a tie), as float64."""
    return x64.float().to(torch.bfloat16).double()


def decode_attn_ref(qkv, cos, sin, k_cache, v_cache, lens, Hq, Hkv, scale):
    """CPU tensors as ops.decode_attn takes them (k_cache / v_cache [B, cap, Hkv, D] BEFORE the call; rows at and beyond lens[b] are ignored).
    -> dict(out [B, Hq, D] float64 (NaN rows where lens[b] >= cap), k_exact / k_mag [B, Hkv, D] float64 (rotation of the new key row and its bound's magnitude term),
    v_row [B, Hkv, D] bf16 (the row to be stored bit for bit))."""
    B, H, D = qkv.shape
    cap = k_cache.shape[1]
    G = Hq // Hkv
    rot, mag = rotate_ref(qkv[:, :Hq + Hkv], cos, sin)
    q = bf16_of(rot[:, :Hq])
    k_new = bf16_of(rot[:, Hq:])
    v_new = qkv[:, Hq + Hkv:]
    out = torch.full((B, Hq, D), float("nan"), dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        if n < 0 or n >= cap:
            continue
        K = torch.cat((k_cache[b, :n].double(), k_new[b][None]), 0)      # [n + 1, Hkv, D]
        V = torch.cat((v_cache[b, :n].double(), v_new[b].double()[None]), 0)
        for hq in range(Hq):
            h = hq // G
            sc = (K[:, h] @ q[b, hq]) * float(scale)
            p = torch.exp(sc - sc.max())
            out[b, hq] = (p[:, None] * V[:, h]).sum(0) / p.sum()
    return dict(out=out, k_exact=rot[:, Hq:], k_mag=mag[:, Hq:], v_row=v_new)


def mrope_tables(pos3, D, theta=1000000.0):
    """cos / sin [B, D] f32 of TextModel.mrope_tables for positions pos3 [3, B] (int64), with the section split (D/8, 3D/16, 3D/16) -- (16, 24, 24) at D = 128 and the
    tiny model's (2, 3, 3) at D = 16."""
    sec = [D // 8, 3 * D // 16, D // 2 - D // 8 - 3 * D // 16]
    axis = torch.tensor(sum([[i] * s for i, s in enumerate(sec)], []))
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    fr = pos3[axis, :].t().float() * inv
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def random_case(B, Hq, Hkv, D, cap, seed):
    """Random bf16 operands of a call: dict(qkv [B, Hq + 2 Hkv, D], k_cache, v_cache [B, cap, Hkv, D], cos, sin [B, D] f32 at positions up to 5000)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B, Hq + 2 * Hkv, D), generator=g).to(torch.bfloat16)
    kc = torch.randn((B, cap, Hkv, D), generator=g).to(torch.bfloat16)
    vc = torch.randn((B, cap, Hkv, D), generator=g).to(torch.bfloat16)
    pos3 = torch.randint(0, 5001, (3, B), generator=g)
    cos, sin = mrope_tables(pos3, D)
    return dict(qkv=qkv, k_cache=kc, v_cache=vc, cos=cos, sin=sin)
