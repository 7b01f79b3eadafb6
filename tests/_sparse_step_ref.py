"""CPU restatements of the sparse TopK step's kernels (cc_pairs_group, cc_decode_pairs_partial, cc_pairs_wgrad:
include/crosscoder_hip.h) and the inputs their tests share.

fma32(a, b, c) is the fp32 fused multiply-add on CPU tensors: the product a b of two fp32 values is exact in fp64 (48
significant bits), the sum with c is formed in fp64 with its rounding error (TwoSum), rounded to odd (if the sum was
inexact and its last bit is even, the neighbour towards the error: it is odd), and that rounds to fp32 once -- fp64
keeps 29 more bits than fp32, so rounding to odd first makes the second rounding the only one that counts.

group_cells is cc_pairs_group's algorithm (count per (latent, row block) cell, exclusive scan in (latent, block) order,
arbitrary placement inside a cell, rank by slot number); ops.pairs_by_latent and a plain loop must give the same.
decode_partial_f32 is the slot-order fma chain from +0.  lists_f32 is cc_pairs_grad_decoder's order for any coefficient
and row matrix (a list of at most L entries one chain from +0, a longer one in pieces of L added in piece order),
lists_sum_f32 the same order with plain adds (db_enc).  sq_partials is the squared-sum partial of every workgroup of
cc_pairs_wgrad's second launch in its lane order.

The squared-sum bound.  A partial is a sum of non-negative terms r^2; every addition on the way from a term to the
partial rounds once (fma: the square itself does not round), relative 2^-24 of a partial sum that is at most the
total.  A term passes through at most D additions, so the partial is within D 2^-24 of its exact value, relative, to
first order; (D + 1) 2^-24 leaves room for the second-order terms.  sq_chain_depth gives D: 8 additions per 8-column
group a lane stores (ceil(K / 8 / 256) groups per row, ceil(h / parts) rows), 6 for the butterfly, 4 for the waves.
"""
import torch

from tests import _pairs_grad_ref as pref
from tests._topk_ref import topk_ref

SPLIT = pref.SPLIT
GROUP_ROWS = 256   # PG_ROWS: rows of a row block of cc_pairs_group
THREADS = 256      # lanes of a workgroup of cc_pairs_wgrad
MAX_PARTS = 1 << 16


def fma32(a, b, c):
    """fp32 fma(a, b, c) of fp32 tensors (broadcast), correctly rounded"""
    p = a.double() * b.double()                       # exact
    c = c.double()
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                   # exact: s + err == p + c
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.where(err > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    s = torch.where((err != 0) & even & torch.isfinite(s), torch.nextafter(s, toward), s)
    return s.float()


def group_cells(idx, h, rows=GROUP_ROWS, shuffle_seed=0):
    """(perm int32 [B k], seg int64 [h + 1]) by the kernel's algorithm; the placement inside a cell is shuffled (the
    arrival order of the atomics), the rank restores the slot order.  Positions from seg[h] on are 0."""
    B, k = idx.shape
    flat = idx.reshape(-1).tolist()
    nblk = -(-B // rows)
    cells = [0] * (h * nblk)
    for p, j in enumerate(flat):
        if 0 <= j < h:
            cells[j * nblk + (p // k) // rows] += 1
    start, run, seg = [], 0, []
    for c, n in enumerate(cells):
        if c % nblk == 0:
            seg.append(run)
        start.append(run)
        run += n
    seg.append(run)
    gen = torch.Generator().manual_seed(shuffle_seed)
    order = torch.randperm(len(flat), generator=gen).tolist()
    cursor, tmp = list(start), [0] * len(flat)
    for p in order:
        j = flat[p]
        if 0 <= j < h:
            c = j * nblk + (p // k) // rows
            tmp[cursor[c]] = p
            cursor[c] += 1
    perm = [0] * len(flat)
    for p, j in enumerate(flat):
        if 0 <= j < h:
            c = j * nblk + (p // k) // rows
            rank = sum(1 for q in range(start[c], cursor[c]) if tmp[q] < p)
            perm[start[c] + rank] = p
    return torch.tensor(perm, dtype=torch.int32), torch.tensor(seg, dtype=torch.int64)


def decode_partial_f32(val, idx, W, h, K):
    """fp32 [B, K]: per element the fma chain from +0 over the slots in order, a slot outside [0, h) skipped"""
    B, k = val.shape
    acc = torch.zeros(B, K, dtype=torch.float32)
    for s in range(k):
        i = idx[:, s].long()
        ok = ((i >= 0) & (i < h)).unsqueeze(1)
        w = W[i.clamp(0, h - 1), :K].float()
        acc = torch.where(ok, fma32(val[:, s].float().unsqueeze(1), w, acc), acc)
    return acc


def decode_partial_f64(val, idx, W, h, K):
    B, k = val.shape
    i = idx.long()
    ok = (i >= 0) & (i < h)
    acts = torch.zeros(B, h, dtype=torch.float64)
    acts.scatter_add_(1, i.clamp(0, h - 1), torch.where(ok, val.double(), torch.zeros((), dtype=torch.float64)))
    return acts @ W[:h, :K].double()


def _clamped(seg, P):
    return [min(max(int(s), 0), P) for s in seg]


def _chain(entries, coef, M, k, Bk, K):
    acc = torch.zeros(K, dtype=torch.float32)
    for slot in entries:
        if 0 <= slot < Bk:
            acc = fma32(coef[slot], M[slot // k, :K].float(), acc)
    return acc


def lists_f32(perm, seg, coef, M, K, L=SPLIT):
    """fp32 [h, K] before the one rounding: row j = sum over latent j's list of coef[slot] * M[slot // k] in
    cc_pairs_grad_decoder's order.  coef [B, k] (any float dtype; used as fp32), M [B, >= K]."""
    perm = [int(p) for p in perm]
    B, k = coef.shape
    P, h = len(perm), len(seg) - 1
    seg = _clamped(seg, P)
    cf = coef.reshape(-1).float()
    out = torch.zeros(h, K, dtype=torch.float32)
    for j in range(h):
        b, e = seg[j], seg[j + 1]
        if e - b <= L:
            out[j] = _chain(perm[b:e], cf, M, k, B * k, K)
        else:
            acc = torch.zeros(K, dtype=torch.float32)
            for p0 in range(b, e, L):
                acc = acc + _chain(perm[p0:min(p0 + L, e)], cf, M, k, B * k, K)
            out[j] = acc
    return out


def lists_sum_f32(perm, seg, coef, L=SPLIT):
    """fp32 [h] before the one rounding: db_enc's order -- plain adds of coef[slot] from +0, pieces as lists_f32"""
    perm = [int(p) for p in perm]
    P, h = len(perm), len(seg) - 1
    seg = _clamped(seg, P)
    cf = coef.reshape(-1).float()
    Bk = cf.numel()
    out = torch.zeros(h, dtype=torch.float32)

    def chain(entries):
        acc = torch.zeros((), dtype=torch.float32)
        for slot in entries:
            if 0 <= slot < Bk:
                acc = acc + cf[slot]
        return acc

    for j in range(h):
        b, e = seg[j], seg[j + 1]
        if e - b <= L:
            out[j] = chain(perm[b:e])
        else:
            acc = torch.zeros((), dtype=torch.float32)
            for p0 in range(b, e, L):
                acc = acc + chain(perm[p0:min(p0 + L, e)])
            out[j] = acc
    return out


def wgrad_parts(h):
    return min(h, MAX_PARTS)


def sq_chain_depth(h, K):
    """D of the squared-sum bound (module docstring)"""
    return 8 * -(-(K // 8) // THREADS) * -(-h // wgrad_parts(h)) + 6 + 4


def sq_partials(stored):
    """fp32 [parts]: the squared-sum partial of each workgroup over `stored` [h, K] (the rounded values; a vector [h]
    counts as b_enc's: thread 0 alone holds a term per row)"""
    vec = stored.dim() == 1
    h = stored.shape[0]
    parts = wgrad_parts(h)
    lanes = torch.zeros(parts, THREADS, dtype=torch.float32)
    sf = stored.float()
    for j in range(h):
        g = j % parts
        if vec:
            lanes[g, 0] = fma32(sf[j], sf[j], lanes[g, 0])
            continue
        ng = sf.shape[1] // 8
        for G0 in range(0, ng, THREADS):
            n = min(THREADS, ng - G0)
            blk = sf[j, G0 * 8:(G0 + n) * 8].view(n, 8)
            for c in range(8):
                lanes[g, :n] = fma32(blk[:, c], blk[:, c], lanes[g, :n])
    w = lanes.view(parts, THREADS // 64, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ o]
    out = torch.zeros(parts, dtype=torch.float32)
    for q in range(THREADS // 64):
        out = out + w[:, q, 0]
    return out


def make_case(B, n, d, h, k, dtype, skew=False, seed=0):
    """Seeded CPU operands of one step's backward: x, g_recon [B, K], W_enc, W_dec [h, K], b_enc [h] in `dtype`; acts =
    dtype(relu(x W_enc^T + b_enc)) (fp32 arithmetic), its reference top-k pairs idx / val [B, k] (tests/_topk_ref.py) and
    g_pre fp32 [B, k] (random; +0 at the padding slots, as cc_pairs_grad_values leaves them).
    skew: latent 3's b_enc is raised so that it is selected in every row, the last 24 latents' is lowered so that they
    never fire, and everyone else's is lowered until some rows hold fewer than k positive activations."""
    g = torch.Generator().manual_seed(1000 * seed + B + 7 * k + 13 * h + 31 * d)
    K = n * d
    x = torch.randn(B, K, generator=g).to(dtype)
    g_recon = (torch.randn(B, K, generator=g) / B).to(dtype)
    W_enc = (torch.randn(h, K, generator=g) / K ** 0.5).to(dtype)
    W_dec = (0.5 * torch.randn(h, K, generator=g)).to(dtype)
    b_enc = (0.1 * torch.randn(h, generator=g))
    if skew:
        b_enc = b_enc - 1.6
        b_enc[3] = 50.0
        b_enc[h - 24:] = -50.0
    b_enc = b_enc.to(dtype)
    acts = torch.relu(x.float() @ W_enc.float().t() + b_enc.float()).to(dtype)
    sel = topk_ref(acts, k)
    g_pre = torch.randn(B, k, generator=g) / B
    g_pre = torch.where(sel["idx"] >= 0, g_pre, torch.zeros(()))
    return {"x": x, "g_recon": g_recon, "W_enc": W_enc, "W_dec": W_dec, "b_enc": b_enc, "acts": acts,
            "idx": sel["idx"], "val": sel["val"], "count": sel["count"], "g_pre": g_pre}


def assert_skewed(idx, h, k, hot=3):
    """The three conditions of the skewed case, on its pairs"""
    B = idx.shape[0]
    assert bool((idx == hot).any(1).all()), "latent %d is not in every row" % hot
    assert B > 2 * SPLIT and B % SPLIT != 0, "its list must span two full pieces and a rest"
    fired = torch.zeros(h, dtype=torch.bool)
    fired[idx[idx >= 0].long()] = True
    assert int((~fired).sum()) >= 24, "at least 24 latents never fire"
    assert bool(((idx >= 0).sum(1) < k).any()), "some rows hold fewer than k eligible latents"
