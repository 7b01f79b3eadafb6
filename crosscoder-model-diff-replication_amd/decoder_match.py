"""Nearest latents across dictionaries by decoder cosine: for every latent of crosscoder A, the latent of crosscoder
B whose decoder vector has the largest cosine with it, and the other way round.

This is how dictionaries are compared: the mean of the best cosines ("MMCS") measures seed-to-seed stability, the
matches tell whether the chat-only latents of an L1 crosscoder reappear in a BatchTopK one (Minder et al. 2025), and
within one dictionary (cc_b=None, the diagonal excluded) they find duplicated or split latents.

The similarity matrix is never stored and the weights are never normalised or copied: cc_decoder_match runs the GEMM
of the two decoders on their arenas, scales the accumulator by the two inverse norms in its epilogue, and keeps per
query only the best (cosine, candidate) pair as a 64-bit key whose unsigned order is (cosine descending, candidate
index ascending); cc_match_reduce merges the keys of each candidate chunk into the running best.  An integer max:
the result does not depend on chunk_rows, and ties go to the smaller index.

    r = match_decoders(cc_a, cc_b)            # or match_decoders(cc) for the nearest other latent of the same one
    r["index"], r["cosine"]                   # [dict_size of A]: best latent of B and its cosine
    r["index_rev"], r["cosine_rev"]           # [dict_size of B]: best latent of A
    r["mutual"], r["mmcs"], r["mmcs_rev"]
"""
import torch

from . import ops

CHUNK_ROWS = 4096


def decode_keys(best, q_scale=None):
    """best [N] int64 keys (ops.match_reduce's state) -> (index [N] int64, cosine [N] fp32); (-1, NaN) where the key
    is 0 (no candidate) or the query's q_scale is 0 (a zero vector: every score is +0).  The inverse of the key map:
    high word = the score's bits in unsigned order, low word = the complement of the candidate index."""
    hi = (best >> 32) & 0xFFFFFFFF
    idx = ~best & 0xFFFFFFFF
    bits = torch.where(hi >= 0x80000000, hi ^ 0x80000000, hi ^ 0xFFFFFFFF)
    bits = torch.where(bits >= 0x80000000, bits - 0x100000000, bits)  # as the int32 of the same bits
    cos = bits.to(torch.int32).view(torch.float32)
    none = best == 0
    if q_scale is not None:
        none = none | (q_scale == 0)
    return (torch.where(none, torch.full_like(idx, -1), idx),
            torch.where(none, torch.full_like(cos, float("nan")), cos))


def match_keys(Wc, c_scale, Wq, q_scale, chunk_rows=CHUNK_ROWS, exclude_diag=False, slab=None):
    """The running-best keys [N] (int64) of the queries Wq [N, K] over all candidates Wc [M, K], chunk_rows candidates
    at a time into one reused slab of col_part_rows(chunk_rows) x N keys."""
    M, N = Wc.shape[0], Wq.shape[0]
    best = torch.zeros(N, dtype=torch.int64, device=Wq.device)
    rows = min(chunk_rows, M)
    R = ops.col_part_rows(rows)
    if slab is None or tuple(slab.shape) != (R, N) or slab.device != Wq.device:
        slab = torch.empty(R, N, dtype=torch.int64, device=Wq.device)
    for r0 in range(0, M, rows):
        r1 = min(M, r0 + rows)
        part = slab[:ops.col_part_rows(r1 - r0)]
        ops.decoder_match(Wc[r0:r1], Wq, c_scale, q_scale, part, row0=r0, exclude_diag=exclude_diag)
        ops.match_reduce(part, best)
    return best


def inverse_norms(W, n, d, model=None):
    """fp32 inverse norms [rows] of the rows of W [rows, n * d] (cc_dec_norms' per-model norms): model m's slice, or
    (None) the whole row, rsqrt of the summed squared per-model norms; 0 where the norm is 0."""
    rows = W.shape[0]
    norms = torch.empty(rows, n, dtype=torch.float32, device=W.device)
    inv = torch.empty(rows, n, dtype=torch.float32, device=W.device)
    ops.dec_norms(W, rows, n, d, norms=norms, inv_norms=inv)
    if model is not None:
        return inv[:, model].contiguous()
    sq = (norms * norms).sum(1)
    return torch.where(sq > 0, torch.rsqrt(sq), torch.zeros_like(sq))


def _operand(cc, model):
    """(W [kernel h, K], its inverse norms) of one crosscoder: model m's slice of the arena's W_dec (K = kernel d)
    or, model None, the whole rows (K = n * kernel d, the cosine over all models).  Padding latents are zero rows:
    scale 0."""
    a = cc.arena()
    a.wait_pending()
    W = a.W_dec_hk if model is None else a.W_dec_hk[:, model * a.d:(model + 1) * a.d]
    return W, inverse_norms(a.W_dec_hk, a.n, a.d, model)


def _mean(cos):
    ok = ~cos.isnan()
    return float(cos[ok].double().mean()) if bool(ok.any()) else float("nan")


def match_decoders(cc_a, cc_b=None, model=None, chunk_rows=CHUNK_ROWS):
    """Nearest latents by decoder cosine.  cc_b=None: cc_a against itself with the diagonal excluded.  model=None:
    the concatenated decoder vectors of all models; model=m: model m's slice only.  Returns a dict of tensors on the
    crosscoder's device:
        index [h_a] int64      best latent of B for each latent of A (ties: the smaller index); -1 if the latent's
                               decoder vector is zero or B has no valid candidate
        cosine [h_a] fp32      its cosine; NaN where index is -1
        index_rev, cosine_rev  [h_b]: the same for each latent of B over A (self mode: the forward tensors)
        mutual [h_a] bool      index_rev[index[j]] == j
        mmcs, mmcs_rev         Python floats: the mean of the non-NaN cosines"""
    n = cc_a.n_models
    self_mode = cc_b is None
    if self_mode:
        cc_b = cc_a
    if model is not None and (isinstance(model, bool) or not isinstance(model, int) or not -n <= model < n):
        raise ValueError(f"model must be None or an int in {-n}..{n - 1}, got {model!r}")
    if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1:
        raise ValueError(f"chunk_rows must be an int >= 1, got {chunk_rows!r}")
    if (cc_b.n_models, cc_b.cfg["d_in"], cc_b.dtype) != (n, cc_a.cfg["d_in"], cc_a.dtype):
        raise ValueError(f"the crosscoders differ: n_models {n} / {cc_b.n_models}, d_in {cc_a.cfg['d_in']} / "
                         f"{cc_b.cfg['d_in']}, dtype {cc_a.dtype} / {cc_b.dtype}")
    if not self_mode and cc_a.arena().data.device != cc_b.arena().data.device:
        raise ValueError(f"the crosscoders are on different devices: {cc_a.arena().data.device} / "
                         f"{cc_b.arena().data.device}")
    if model is not None:
        model %= n
    with torch.no_grad():
        Wa, sa = _operand(cc_a, model)
        Wb, sb = (Wa, sa) if self_mode else _operand(cc_b, model)
        h_a, h_b = cc_a.d_hidden, cc_b.d_hidden
        # A's latents as queries over B's as candidates, then the operands swapped
        index, cosine = decode_keys(match_keys(Wb, sb, Wa, sa, chunk_rows, exclude_diag=self_mode)[:h_a], sa[:h_a])
        if self_mode:
            index_rev, cosine_rev = index, cosine
        else:
            index_rev, cosine_rev = decode_keys(match_keys(Wa, sa, Wb, sb, chunk_rows)[:h_b], sb[:h_b])
        j = torch.arange(h_a, device=index.device)
        mutual = (index >= 0) & (index_rev[index.clamp(min=0)] == j)
    return {"index": index, "cosine": cosine, "index_rev": index_rev, "cosine_rev": cosine_rev, "mutual": mutual,
            "mmcs": _mean(cosine), "mmcs_rev": _mean(cosine_rev)}
