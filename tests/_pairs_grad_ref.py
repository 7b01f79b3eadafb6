"""CPU restatements of the sparse decode's backward (cc_pairs_grad_values, cc_pairs_grad_decoder, cc_pairs_latent_sums:
include/crosscoder_hip.h) and of ops.pairs_by_latent, with the bounds their tests use.  The operands are
tests/_decode_pairs_ref.make_case's: its x serves as g, the gradient on the reconstruction.

cc_pairs_grad_values.  dot[r][s][m] is an fp32 sum of d products g_c w_c.  Whatever the order, a term passes through at
most d - 1 additions, each rounding by 2^-24 of a partial sum that is at most M = sum_c |g_c w_c| in magnitude; with
fma no product rounds, without it each rounds once more (2^-24 |g_c w_c|):  |dot - exact| <= d 2^-24 M to first order,
and values_tol = (d + 1) 2^-23 M leaves a factor 2.  total adds the n models' sums: the same bound with n d in place of
d over the whole row's M.  The multiplication by val rounds once: dot_val == fl(val * dot) is checked bitwise instead.
A dyadic case (small integers times 2^-q) makes every product and partial sum exact, so the kernel must equal fp64 bit
for bit there in any order.

cc_pairs_grad_decoder.  decoder_f32 is the documented order executed in fp32: per latent one accumulator per column
from +0, updated entry by entry in segment order; a segment longer than L as consecutive pieces of L, each from +0, the
piece sums added in piece order onto +0.  For bf16 operands the product v g is exact in fp32, so `acc + v * g` rounds
once like the kernel's fmaf: bit-equal.  For fp32 operands the kernel is compared with fp64 within
decoder_tol = (len + 1) 2^-23 sum |v g|: a chain of len fmas rounds len times by 2^-24 of at most sum |v g|; the
split replaces some of those additions by as many piece additions, so the count does not grow.

cc_pairs_latent_sums.  latent_sums_f64 is the same fp64 loop; the kernel must give its bits.

The identity that ties attribution to cc_decode_pairs (fp32, b_dec = 0).  For one row with pairs (v_s, i_s), a group G of
latents, r1 = decode_pairs(v) and r0 = decode_pairs(v with G's slots zeroed):
    exactly,  <g, r1 - r0> = sum_c g_c sum_{s in G} v_s W[i_s][c] = sum_{s in G} v_s <g, W[i_s]> = sum_{s in G} total_s.
    left:   r1_c and r0_c are fma chains of k steps from b_c = 0; each step rounds by 2^-24 of a partial sum of at most
            S_c = sum_s |v_s W[i_s][c]|:  |r_c - exact| <= k 2^-24 S_c each, so the left side, with the inner product in
            fp64, is within 2 k 2^-24 sum_c |g_c| S_c = k 2^-23 T of its exact value, T = sum_{s, c} |v_s g_c W[i_s][c]|.
            (A non-zero b_dec would add |b_c| to S_c: the test keeps the crosscoder's initial zero b_dec.)
    right:  total_s = the n model sums (each within d 2^-24 of its M, above), each multiplied by v_s (one rounding) and
            added in model order (n roundings):  (n d + n + 1) 2^-24 |v_s| sum_c |g_c W[i_s][c]| <= (n d + 2) 2^-23 of it
            (n + 1 <= n d + 4); summed over G's slots in fp64 that is at most (n d + 2) 2^-23 T.
    together  |left - right| <= (k + n d + 2) 2^-23 T = identity_tol.
"""
import torch

EPS32 = 2.0 ** -23
SPLIT = 128  # CC_PAIRS_GRAD_SPLIT


def by_latent_loop(idx, h):
    """(perm list, seg list of h + 1) by a plain loop: the valid slots in (latent, r, s) order"""
    B, k = idx.shape
    lists = [[] for _ in range(h)]
    flat = idx.reshape(-1).tolist()
    for slot, i in enumerate(flat):  # (slot order is (r, s) order)
        if 0 <= i < h:
            lists[i].append(slot)
    perm, seg = [], [0]
    for lst in lists:
        perm += lst
        seg.append(len(perm))
    return perm, seg


def values_f64(idx, W, g, n, d, h, val=None):
    """(dot fp64 [B, k, n] -- times val where given --, M fp64 [B, k, n] = sum_c |g_c w_c| (times |val|)); an invalid
    slot gives 0 in both"""
    B, k = idx.shape
    i = idx.long()
    ok = (i >= 0) & (i < h)
    Wr = W[i.clamp(0, h - 1)].double().view(B, k, n, d)
    p = Wr * g.double().view(B, 1, n, d)
    dot, M = p.sum(-1), p.abs().sum(-1)
    if val is not None:
        dot, M = dot * val.double().unsqueeze(-1), M * val.double().abs().unsqueeze(-1)
    z = torch.zeros((), dtype=torch.float64)
    return torch.where(ok.unsqueeze(-1), dot, z), torch.where(ok.unsqueeze(-1), M, z)


def values_tol(terms, M):
    return (terms + 1) * EPS32 * M


def _chain_f32(entries, val_flat, g, k, Bk, K):
    acc = torch.zeros(K, dtype=torch.float32)
    for slot in entries:
        if 0 <= slot < Bk:
            acc = acc + val_flat[slot].float() * g[slot // k, :K].float()
    return acc


def decoder_f32(perm, seg, val, g, K, L=SPLIT):
    """fp32 [h, K]: the documented order (before the one rounding to the dtype).  perm / seg: lists or tensors."""
    perm, seg = [int(p) for p in perm], [int(s) for s in seg]
    B, k = val.shape
    P, h = len(perm), len(seg) - 1
    vf = val.reshape(-1)
    out = torch.zeros(h, K, dtype=torch.float32)
    for j in range(h):
        b, e = min(max(seg[j], 0), P), min(max(seg[j + 1], 0), P)
        if e - b <= L:
            out[j] = _chain_f32(perm[b:e], vf, g, k, B * k, K)
        else:
            acc = torch.zeros(K, dtype=torch.float32)
            for p0 in range(b, e, L):
                acc = acc + _chain_f32(perm[p0:min(p0 + L, e)], vf, g, k, B * k, K)
            out[j] = acc
    return out


def decoder_f64(perm, seg, val, g, K):
    """(exact fp64 [h, K], S fp64 [h, K] = sum |v g|, len int64 [h]) over the segments"""
    perm, seg = [int(p) for p in perm], [int(s) for s in seg]
    B, k = val.shape
    h = len(seg) - 1
    lat = torch.repeat_interleave(torch.arange(h), torch.tensor(seg[1:]) - torch.tensor(seg[:-1]))
    slots = torch.tensor(perm[:seg[-1]], dtype=torch.int64)
    contrib = val.reshape(-1)[slots].double().unsqueeze(1) * g[slots // k, :K].double()
    exact = torch.zeros(h, K, dtype=torch.float64).index_add_(0, lat, contrib)
    S = torch.zeros(h, K, dtype=torch.float64).index_add_(0, lat, contrib.abs())
    return exact, S, torch.tensor(seg[1:]) - torch.tensor(seg[:-1])


def decoder_tol(length, S):
    return (length.double().unsqueeze(1) + 1) * EPS32 * S


def latent_sums_f64(a, perm, seg, sum_, abs_, count):
    """The fp64 loop, in place on sum_ / abs_ [h, n] (fp64) and count [h] (int64); a fp32 [B, k, n]"""
    perm, seg = [int(p) for p in perm], [int(s) for s in seg]
    n = a.shape[-1]
    af = a.reshape(-1, n)
    P, Bk = len(perm), af.shape[0]
    for j in range(len(seg) - 1):
        b, e = min(max(seg[j], 0), P), min(max(seg[j + 1], 0), P)
        for p in range(b, e):
            if 0 <= perm[p] < Bk:
                x = af[perm[p]].double()
                sum_[j] = sum_[j] + x
                abs_[j] = abs_[j] + x.abs()
                count[j] += 1


def dense_autograd(val, idx, W, b, g, h):
    """fp64 autograd of the dense restatement  recon = scatter(val, idx) @ W[:h] + b,  metric = <g, recon>:
    (recon, d val [B, k] (0 at invalid slots), d W [h, K], d b [K])"""
    B, k = val.shape
    i = idx.long()
    ok = (i >= 0) & (i < h)
    v = val.double().clone().requires_grad_(True)
    Wd = W[:h].double().clone().requires_grad_(True)
    bd = b.double().clone().requires_grad_(True)
    acts = torch.zeros(B, h, dtype=torch.float64).scatter_add(1, i.clamp(0, h - 1), torch.where(ok, v, torch.zeros_like(v)))
    recon = acts @ Wd + bd
    (recon * g.double()).sum().backward()
    return recon.detach(), v.grad, Wd.grad, bd.grad


def identity_tol(k, n, d, T):
    return (k + n * d + 2) * EPS32 * T
