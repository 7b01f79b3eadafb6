"""The reference for BatchTopK selection (pure torch, any device; the tests run it on the CPU).

Score: the fp32 product float(a) * weight[latent] (weight None: float(a)).  Key: the score where the activation and
the score are both > 0, else 0.  Order: larger key first, among equal keys the smaller flat index row * h + latent
first -- a stable descending sort of the flattened key -- and the selected set is the first n_keep positions whose
key is > 0.
"""
import struct

import torch


def batch_topk_key(v, weight=None):
    """[B, h] fp32 keys (0: ineligible).  NaN > 0 is false."""
    a = v.float()
    s = a if weight is None else a * weight.float()[None, :]
    return torch.where((v > 0) & (s > 0), s, torch.zeros((), dtype=torch.float32, device=v.device))


def batch_topk_order(v, weight=None):
    """The stable descending sort of the flattened key: (sorted keys [B * h] fp32, flat indices [B * h])."""
    order = torch.sort(batch_topk_key(v, weight).flatten(), descending=True, stable=True)
    return order.values, order.indices


def batch_topk_ref(v, n_keep, weight=None, order=None):
    """v [B, h] -> dict: dense [B, h] (selected elements keep their bits, the rest +0), mask [B, h] bool,
    row_count [B] int64, T (the smallest selected score as a 0-dim fp32 tensor, 0 when nothing is selected),
    selected, ties (selected elements whose score is T), ties_total (elements whose score is T), eligible.
    order: batch_topk_order(v, weight), to share one sort among several n_keep."""
    B, h = v.shape
    keys, indices = batch_topk_order(v, weight) if order is None else order
    n = min(int(n_keep), B * h)
    keep = keys[:n] > 0
    mask = torch.zeros(B * h, dtype=torch.bool, device=v.device)
    mask[indices[:n]] = keep
    mask = mask.view(B, h)
    dense = torch.where(mask, v, torch.zeros((), dtype=v.dtype, device=v.device))
    selected = int(keep.sum())
    eligible = int((keys > 0).sum())
    T = keys[selected - 1].clone() if selected else torch.zeros((), dtype=torch.float32)
    ties_total = int((keys == T).sum()) if selected else 0
    ties = int((keys[:selected] == T).sum()) if selected else 0
    return {"dense": dense, "mask": mask, "row_count": mask.sum(1), "T": T, "selected": selected, "ties": ties,
            "ties_total": ties_total, "eligible": eligible}


def threshold_ref(v, theta, weight=None):
    """The inference form: eligible and score >= theta."""
    key = batch_topk_key(v, weight)
    mask = (key > 0) & (key >= theta)
    return {"dense": torch.where(mask, v, torch.zeros((), dtype=v.dtype, device=v.device)), "mask": mask,
            "row_count": mask.sum(1)}


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def batch_topk_brute(rows, n_keep, weight=None):
    """rows: lists of Python floats (values an fp32 holds exactly) -> the selected flat indices, ascending, by a
    plain Python loop.  The product of two fp32 values is exact in a double, so rounding it once to fp32 is the
    IEEE single multiply."""
    h = len(rows[0])
    cand = []
    for b, row in enumerate(rows):
        for i, a in enumerate(row):
            if not a > 0:
                continue
            s = a if weight is None else (_f32(a * weight[i]) if abs(a * weight[i]) < 3e38 else a * weight[i])
            if s > 0:
                cand.append((s, b * h + i))
    chosen = []
    for _ in range(min(n_keep, len(cand))):
        best = None
        for s, i in cand:
            if (s, i) in chosen:
                continue
            if best is None or s > best[0] or (s == best[0] and i < best[1]):
                best = (s, i)
        chosen.append(best)
    return sorted(i for _, i in chosen)
