"""CPU restatements of cc_decode_pairs (include/crosscoder_hip.h) and the inputs its tests share.

decode_f32 is the kernel's definition executed in torch on the CPU: one fp32 accumulator per output element, started
at b_dec and updated slot by slot in slot order, a slot outside [0, h) skipped, rounded once to the dtype.  For bf16
operands it is bit-exact: the product of two bf16 values has at most 16 significant bits, so it is exact in fp32 and
`acc + v * w` rounds once, like the kernel's fmaf.  For fp32 operands the product rounds too, so the kernel is compared
with decode_f64 instead, within chain_tol:

    an fma chain of k steps from b:  every step rounds once, relative 2^-24 of a partial sum that is at most
    S = |b| + sum |v w| in magnitude, so |acc - exact| <= k 2^-24 S; the multiply-then-add loop of decode_f32 rounds
    twice per step: 2 k 2^-24 S.  (k + 1) 2^-23 S covers both, and an fp32 output needs no further rounding.

sq_err sums d non-negative terms (r - x)^2 in fp32: the difference rounds once (relative 2^-24, so 2^-23 on its
square), each of the d adds rounds once (2^-24 of a partial sum that is at most the total): relative error at most
(d + 2) 2^-24 to first order; sq_tol = (d + 4) 2^-23 times the value leaves a factor 2.
"""
import torch

EPS32 = 2.0 ** -23


def decode_f32(val, idx, W, b, h, rounded=True):
    """[B, K] in val's dtype: the fp32 slot-order loop (rows and columns vectorised, slots in order); rounded=False:
    the fp32 accumulators before the one rounding."""
    B, k = val.shape
    acc = b.float().unsqueeze(0).expand(B, -1).clone()
    for s in range(k):
        i = idx[:, s].long()
        ok = (i >= 0) & (i < h)
        w = W[i.clamp(0, h - 1)].float()
        acc = torch.where(ok.unsqueeze(1), acc + val[:, s].float().unsqueeze(1) * w, acc)
    return acc.to(val.dtype) if rounded else acc


def decode_f64(val, idx, W, b, h):
    """(exact [B, K] fp64, S [B, K] fp64 = |b| + sum |v w| over the valid slots)"""
    B, k = val.shape
    acc = b.double().unsqueeze(0).expand(B, -1).clone()
    S = acc.abs()
    for s in range(k):
        i = idx[:, s].long()
        ok = ((i >= 0) & (i < h)).unsqueeze(1)
        p = val[:, s].double().unsqueeze(1) * W[i.clamp(0, h - 1)].double()
        acc = torch.where(ok, acc + p, acc)
        S = torch.where(ok, S + p.abs(), S)
    return acc, S


def dense_f64(val, idx, W, b, h):
    """fp64 acts @ W[:h] + b with the valid pairs scattered (added) into a dense [B, h] matrix"""
    B, k = val.shape
    i = idx.long()
    ok = (i >= 0) & (i < h)
    acts = torch.zeros(B, h, dtype=torch.float64)
    acts.scatter_add_(1, i.clamp(0, h - 1), torch.where(ok, val.double(), torch.zeros((), dtype=torch.float64)))
    return acts @ W[:h].double() + b.double()


def sq_err_f64(recon, x, n, d):
    """fp64 [B, n] from a reconstruction already rounded to its dtype"""
    B = recon.shape[0]
    return (recon.double() - x.double()).pow(2).view(B, n, d).sum(-1)


def chain_tol(k, S):
    return (k + 1) * EPS32 * S


def sq_tol(d, value):
    return (d + 4) * EPS32 * value


def make_case(rows, n, d, h, k, dtype, seed=0):
    """Seeded random operands on the CPU -> dict(val [rows, k], idx int32 [rows, k], W [h, n d], b [n d],
    x [rows, n d]).  The indices, by row r (where k and rows allow it):
      every row      in-range latents drawn with replacement
      r % 3 == 1     slot 1 repeats slot 0 (a duplicate)
      r % 4 == 2     the last (k + 2) // 3 slots are -1 (padding at the end)
      r % 5 == 3     the middle slot is -1;  r % 5 == 4: the middle slot is another negative value
      the last row   no valid slot at all (rows >= 2)
    Skipped slots keep non-zero values: a kernel that read them would show."""
    g = torch.Generator().manual_seed(1000 * seed + rows + 7 * k + 13 * h)
    K = n * d
    W = (0.5 * torch.randn(h, K, generator=g)).to(dtype)
    b = torch.randn(K, generator=g).to(dtype)
    x = torch.randn(rows, K, generator=g).to(dtype)
    val = torch.randn(rows, k, generator=g).to(dtype)
    idx = torch.randint(0, h, (rows, k), generator=g, dtype=torch.int32)
    r = torch.arange(rows)
    if k >= 2:
        dup = r % 3 == 1
        idx[dup, 1] = idx[dup, 0]
        idx[r % 4 == 2, k - (k + 2) // 3:] = -1
    if k >= 3:
        idx[r % 5 == 3, k // 2] = -1
        neg = torch.nonzero(r % 5 == 4).flatten()
        idx[neg, k // 2] = torch.where(neg % 2 == 0, -7, -2 ** 31).to(torch.int32)
    if rows >= 2:
        idx[rows - 1] = -1
    return {"val": val, "idx": idx, "W": W, "b": b, "x": x}
