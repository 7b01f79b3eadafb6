"""CPU restatements (fp64, torch) of the dead-latent resampling kernels (include/crosscoder_hip.h: cc_row_norms,
cc_resample_pick, cc_resample_write) and the bounds their GPU tests use.  u = 2^-24 (fp32), U = 2^-53 (fp64),
v = 2^-8 (bf16: 8 significant bits): the unit roundoffs of round-to-nearest, whose relative error is at most
v / (1 + v) (Higham, Theorem 2.3).

Row norms.  The kernel sums K non-negative squares in fp32 in a fixed order: a lane folds the 8 columns it owns of
every 512-column chunk into one fma chain (8 ceil(K / 512) roundings; for bf16 input a square is exact in fp32, for
fp32 input fmaf rounds the exact x^2 + q once: one rounding per term either way), then 6 butterfly adds.  A sum of
non-negative terms in which every term passes through at most m roundings has relative error at most
(1 + u)^m - 1 <= m u / (1 - m u) (Higham, Accuracy and Stability, section 4.2: each term's factor is a product of at
most m factors (1 + delta), |delta| <= u, and all terms have one sign).  The square root halves a relative error
(sqrt(1 + e) <= 1 + e / 2 for e >= 0, and >= 1 - e / 2 - e^2 / 2 below) and rounds once more.  With
m = 8 ceil(K / 512) + 6:
    row_norm_tol(K) = (m / 2 + 2) u
-- m / 2 + 1 to first order, one more u for every second-order term (m u < 2^-15 for K <= 2^17): of order K 2^-24 / 128.

Pick.  cdf is an inclusive prefix sum of non-negative fp64 weights in which an element passes through at most
16 + 256 + ceil(R / 4096) + 2 additions, so a computed cdf[r] is within pick_scan_tol(R) = that many times U,
relatively, of the exact prefix sum -- and so is the reference's own torch.cumsum (at most R additions: R U).  A test
that places u_j at the midpoint of row r's interval of the reference CDF and only uses rows whose weight is at least
1e-6 of the total is therefore safe: the target and both interval ends move by at most ~(R + 300) U * total
< 1e-11 * total for R <= 70001, against a half-width of at least 5e-7 * total.

Write.  s = sum x_c^2 as above with 2048-column chunks and the four waves added in order: m = 8 ceil(K / 2048) + 6 + 3
roundings.  root = sqrtf(s): relative m u / 2 + u.  scale = norm / root: + u.  value = x_c * scale: + u.  Against the
fp64 value x_c norm / ||x||, to first order (m / 2 + 3) u; one more u for the second-order terms:
    write_tol(K) = (m / 2 + 4) u                   fp32 parameters and fp32 masters, relative per element
    write_tol_bf16(K) = v / (1 + v) + write_tol(K) (1 + v)   bf16 parameters: one more rounding to nearest
which is below 2^-8 while write_tol(K) < 2^-16 / (1 + v)^2, i.e. for K <= 2^16 (write_tol(2^16) = 136.5 u).  The norm handed to the kernel is the
fp32 rounding of the caller's float: the reference uses that fp32 value, so it adds nothing.
"""
import math

import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
UBF = 2.0 ** -8


def row_norm_tol(K):
    m = 8 * math.ceil(K / 512) + 6
    return (m / 2 + 2) * U32


def write_tol(K):
    m = 8 * math.ceil(K / 2048) + 6 + 3
    return (m / 2 + 4) * U32


def write_tol_bf16(K):
    return UBF / (1 + UBF) + write_tol(K) * (1 + UBF)


def pick_scan_tol(R):
    return (16 + 256 + math.ceil(R / 4096) + 2) * U64


def row_norms(W):
    """fp64 [rows]"""
    return W.double().pow(2).sum(1).sqrt()


def weights(loss):
    """fp64 [R]: loss^2, 0 for a loss that is negative (sign set) or not finite"""
    l = loss.double()
    ok = torch.isfinite(l) & ~torch.signbit(l)
    return torch.where(ok, l * l, torch.zeros_like(l))


def cdf(loss):
    """fp64 [R]: the inclusive prefix sum of weights(loss), one addition after the other"""
    return torch.cumsum(weights(loss), 0)


def pick_loop(c, u):
    """The definition in plain loops: for each u_j the smallest r with c[r] > u_j * c[-1]; -1 everywhere if c[-1] is
    not > 0.  c fp64 [R], u fp64 [J] -> list of ints."""
    total = float(c[-1])
    R = c.shape[0]
    out = []
    for uj in u.tolist():
        if not total > 0:
            out.append(-1)
            continue
        t = uj * total
        r = 0
        while r < R - 1 and not float(c[r]) > t:
            r += 1
        out.append(r)
    return out


def pick(c, u):
    """pick_loop by binary search (torch.searchsorted on the prefix sums) -> int64 [J]"""
    total = c[-1]
    if not float(total) > 0:
        return torch.full((u.shape[0],), -1, dtype=torch.int64)
    # right=True: the first index whose value is > the target
    return torch.searchsorted(c, u * total, right=True).clamp(max=c.shape[0] - 1)


def midpoints(c, rows):
    """u_j at the midpoint of row rows[j]'s interval (c[r-1], c[r]] of the prefix sums c, as a fraction of c[-1]"""
    lo = torch.where(rows > 0, c[(rows - 1).clamp(min=0)], torch.zeros((), dtype=torch.float64))
    return (lo + c[rows]) / 2 / c[-1]


def safe_rows(loss, floor=1e-6):
    """the rows whose weight is at least `floor` of the total"""
    w = weights(loss)
    return torch.nonzero(w >= floor * w.sum()).flatten()


def reseed(x, norm):
    """fp64 [K]: x * norm / ||x|| for the fp32 value of norm the kernel is handed"""
    x = x.double()
    n32 = float(torch.tensor(norm, dtype=torch.float32))
    return x * n32 / x.pow(2).sum().sqrt()


def pattern(numel, dtype, seed):
    """A seeded arena fill with no zero element (so that a zeroed element is told from an untouched one) and no
    element whose bits the kernel could reproduce by accident: values in +-[0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(numel, generator=g) + 0.5
    s = torch.where(torch.rand(numel, generator=g) < 0.5, -1.0, 1.0)
    return (v * s).to(dtype)
