"""The reference for per-row top-k selection (pure torch, any device; the tests run it on the CPU).

Order: larger value first, among equal values the smaller index first -- a stable descending sort of the key
(the value where it is > 0, else 0) -- and the selected set is the first k positions whose key is > 0.
"""
import torch


def topk_order(v):
    """The stable descending sort of the key: (sorted keys [B, h] fp32, indices [B, h]).  NaN > 0 is false."""
    key = torch.where(v > 0, v.float(), torch.zeros((), dtype=torch.float32, device=v.device))
    order = torch.sort(key, dim=1, descending=True, stable=True)
    return order.values, order.indices


def topk_ref(v, k, order=None):
    """v [B, h] -> dict: dense [B, h] (selected elements keep their bits, the rest +0), idx [B, k] int32 and
    val [B, k] (v's dtype) in ascending index padded with (-1, 0), count [B] int64, mask [B, h] bool.
    order: topk_order(v), to share one sort among several k."""
    B, h = v.shape
    keys, indices = topk_order(v) if order is None else order
    idx, keep = indices[:, :k], keys[:, :k] > 0
    mask = torch.zeros(B, h, dtype=torch.bool, device=v.device)
    mask.scatter_(1, idx, keep)
    dense = torch.where(mask, v, torch.zeros((), dtype=v.dtype, device=v.device))
    count = keep.sum(1)
    sidx = torch.where(keep, idx, torch.full_like(idx, h)).sort(dim=1).values  # selected first, ascending
    real = sidx < h
    val = torch.where(real, v.gather(1, sidx.clamp(max=h - 1)), torch.zeros((), dtype=v.dtype, device=v.device))
    return {"dense": dense, "idx": torch.where(real, sidx, torch.full_like(sidx, -1)).to(torch.int32), "val": val,
            "count": count, "mask": mask}


def topk_brute(row, k):
    """One row (a list of floats) by a plain Python loop: the selected indices, ascending."""
    cand = [(x, i) for i, x in enumerate(row) if x > 0]
    chosen = []
    for _ in range(min(k, len(cand))):
        best = None
        for x, i in cand:
            if (x, i) in chosen:
                continue
            if best is None or x > best[0] or (x == best[0] and i < best[1]):
                best = (x, i)
        chosen.append(best)
    return sorted(i for _, i in chosen)


def tie_straddles(v, k):
    """Rows whose k-th and (k+1)-th elements under the order are equal and positive: the tie rule decides."""
    keys, _ = topk_order(v)
    if k >= v.shape[1]:
        return torch.zeros(v.shape[0], dtype=torch.bool)
    return (keys[:, k - 1] == keys[:, k]) & (keys[:, k] > 0)
