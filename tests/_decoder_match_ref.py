"""fp64 reference for decoder matching (crosscoder_amd.match_decoders, cc_decoder_match) and a pure-Python statement
of the key order.

`cosines` is the whole similarity matrix from the tensors actually given to the kernel (their bits upcast to fp64 on
the CPU).  `tol` is the derived bound on one fp32 score: with K the contraction length, the fp32 accumulation of exact
products costs at most K 2^-24 sum|ab| / (|a||b|) <= K 2^-24, each of the two fp32 norms is within about
(K/2 + 2) 2^-24 relative, and the two multiplies follow: (2K + 16) 2^-23.  An indexing error shows as 0.1 to 1."""
import struct

import torch


def tol(K):
    return (2 * K + 16) * 2.0 ** -23


def cosines(Wc, Wq):
    """Wc [M, K], Wq [N, K] (any dtype, any device) -> (cos [M, N] fp64 on the CPU, ok_c [M], ok_q [N]): cos[i][j] of
    candidate i and query j, 0 where either vector is zero; ok_* = the vector is not zero."""
    c, q = Wc.detach().cpu().double(), Wq.detach().cpu().double()
    nc, nq = c.norm(dim=1), q.norm(dim=1)
    ok_c, ok_q = nc > 0, nq > 0
    cos = (c @ q.t()) / (nc.clamp(min=1e-300)[:, None] * nq.clamp(min=1e-300)[None, :])
    return cos, ok_c, ok_q


def masked(cos, ok_c, exclude_diag=False):
    """The matrix the argmax runs over: -inf on candidates that give no key (zero rows; the diagonal)."""
    m = cos.clone()
    m[~ok_c] = float("-inf")
    if exclude_diag:
        k = min(m.shape)
        m[torch.arange(k), torch.arange(k)] = float("-inf")
    return m


def key(score, index):
    """The 64-bit key of one (fp32 score, candidate index) pair: high word = the bits b of score + 0.0 (so -0 is +0)
    mapped to unsigned order, b ^ 0xffffffff for a set sign bit and b ^ 0x80000000 otherwise; low word = ~index.
    The unsigned max of two keys is the larger score and, on equal scores, the smaller index; 0 = no candidate."""
    b = struct.unpack("<I", struct.pack("<f", score + 0.0))[0]
    hi = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)
    return (hi << 32) | (~index & 0xFFFFFFFF)


def unkey(k):
    """key's inverse -> (score, index), or (nan, -1) for key 0."""
    if k == 0:
        return float("nan"), -1
    hi = k >> 32
    b = hi ^ 0x80000000 if hi >> 31 else hi ^ 0xFFFFFFFF
    return struct.unpack("<f", struct.pack("<I", b))[0], ~k & 0xFFFFFFFF


def as_unsigned(keys):
    """An int64 key tensor as Python unsigned integers."""
    return [k & 0xFFFFFFFFFFFFFFFF for k in keys.cpu().tolist()]
