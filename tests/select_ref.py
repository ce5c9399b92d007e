"""The semantics of rga3_select_token (include/rga3_hip.h) restated in torch on the CPU (no tests in this module).

Per row, every step in ``dtype``: float32 is the exact restatement of the kernel (one IEEE operation per step), float64 is the yardstick.

  1. s = logit; where seen: s < 0 ? s * penalty : s / penalty; s = s / temperature
  2. candidates ordered by (s descending, index ascending), -0.0 == +0.0; the first K = min(top_k, V)
  3. w_j = exp(s_j - s_0), Z = sum of w_j in candidate order
  4. j is kept iff j == 0 or tail_j > (1 - top_p) * Z, tail_j = sum_{i >= j} w_i taken from the last candidate upwards (HF's cumsum over the ascending sort):
     a prefix of n candidates
  5. u None: candidate 0.  Else Z_n = sum_{i < n} w_i and the first kept j with sum_{i <= j} w_i > u * Z_n, the last kept if there is none

Alongside the token, ``select_row`` returns the two decision margins: how close u * Z_n came to a cumulative sum (over Z_n) and how close a tail sum came to the
top-p threshold (over Z).  A draw whose margin is below the rounding of the sums may legitimately fall on either side.
"""
import math

import torch


def scores(logits, seen=None, penalty=1.0, temperature=1.0, dtype=torch.float32):
    """[..., V] scores after penalty and temperature, in ``dtype`` (scalars rounded to it first, as the kernel's float arguments are)."""
    s = logits.to(dtype)
    p = torch.tensor(penalty, dtype=dtype)
    t = torch.tensor(temperature, dtype=dtype)
    if seen is not None:
        s = torch.where(seen.bool(), torch.where(s < 0, s * p, s / p), s)
    return s / t


def _seq_sum(w):
    """Sum in index order, one rounding per addition, starting from 0 (torch.cumsum's order is not specified)."""
    acc = torch.zeros((), dtype=w.dtype)
    out = []
    for x in w:
        acc = acc + x
        out.append(acc)
    return torch.stack(out) if out else w


def select_row(logits, seen=None, penalty=1.0, temperature=1.0, top_k=1, top_p=1.0, u=None, dtype=torch.float32):
    """One row.  Returns dict(token, order [K] candidate indices, kept = order[:n], scores [V], margin_u, margin_p)."""
    V = logits.shape[0]
    s = scores(logits, seen, penalty, temperature, dtype)
    order = torch.sort(s, descending=True, stable=True).indices[: min(int(top_k), V)]     # stable: equal scores (and -0.0 / +0.0) keep index order
    sk = s[order]
    w = torch.exp(sk - sk[0])
    csum = _seq_sum(w)
    Z = csum[-1]
    tail = torch.flip(_seq_sum(torch.flip(w[1:], (0,))), (0,)) if len(w) > 1 else w[:0]
    thr = (torch.tensor(1.0, dtype=dtype) - torch.tensor(top_p, dtype=dtype)) * Z
    n = 1 + int((tail > thr).sum())
    margin_p = float(((tail - thr).abs() / Z).min()) if len(tail) else math.inf
    Zn = csum[n - 1]
    token, margin_u = int(order[0]), math.inf
    if u is not None:
        t = torch.tensor(u, dtype=torch.float32).to(dtype) * Zn
        hit = (csum[:n] > t).nonzero()
        token = int(order[int(hit[0, 0]) if len(hit) else n - 1])
        margin_u = float(((csum[:n] - t).abs() / Zn).min())
    return {"token": token, "order": order, "kept": order[:n], "scores": s, "margin_u": margin_u, "margin_p": margin_p}


def select(logits, seen=None, penalty=1.0, temperature=1.0, top_k=1, top_p=1.0, u=None, dtype=torch.float32):
    """[B, V] logits -> list of select_row results; seen [B, V] or None, u [B] or None.  Nothing is modified."""
    return [select_row(logits[b], None if seen is None else seen[b], penalty, temperature, top_k, top_p, None if u is None else float(u[b]), dtype)
            for b in range(logits.shape[0])]


def draws(logits, u, seen=None, penalty=1.0, temperature=1.0, top_k=1, top_p=1.0, dtype=torch.float32):
    """Many draws of ONE row at once: u [N] f32 -> (tokens [N] int64, margin_u [N], margin_p float).  Same arithmetic as select_row."""
    r = select_row(logits, seen, penalty, temperature, top_k, top_p, None, dtype)
    n = len(r["kept"])
    sk = r["scores"][r["order"]]
    csum = _seq_sum(torch.exp(sk - sk[0]))[:n]
    t = u.to(torch.float32).to(dtype) * csum[-1]
    above = csum[None, :] > t[:, None]
    first = torch.where(above.any(1), above.to(torch.int8).argmax(1), torch.full((len(u),), n - 1))
    margin_u = ((csum[None, :] - t[:, None]).abs() / csum[-1]).min(1).values
    return r["kept"][first], margin_u, r["margin_p"]
