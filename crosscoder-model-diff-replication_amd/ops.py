"""Tensor-level wrappers over the C ABI (include/crosscoder_hip.h).

Every function takes torch tensors that already live on a ROCm device, checks shapes on
the host, and launches on torch's current stream.  Nothing here computes on the CPU.
"""
import ctypes

import torch

from . import _lib
from ._lib import CC_BF16, CC_F32, CC_LAYOUT_KC, CC_LAYOUT_MN

_DT = {torch.bfloat16: CC_BF16, torch.float32: CC_F32}


def dtype_code(dtype):
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"crosscoder_amd supports bf16 and fp32 storage, got {dtype}") from None


def lib():
    return _lib.load()


def _stream(t):
    if t.device.type != "cuda":
        raise RuntimeError(
            f"crosscoder_amd kernels run on a ROCm GPU; got a tensor on {t.device} "
            "(the CPU restatement lives in oracle/ and is test-only)")
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _vptr(p):
    """an optional raw device address (int, ctypes.c_void_p or None) as a c_void_p"""
    return p if isinstance(p, ctypes.c_void_p) else ctypes.c_void_p(p or 0)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


TILE_CTR_WORDS = 8  # CC_TILE_CTR_WORDS (include/crosscoder_hip.h)


def _ctr(t):
    """A persistent launch's per-XCD tile counters: int32 [TILE_CTR_WORDS] (zero; every launch leaves them zero),
    or None (static tile order)."""
    if t is None:
        return None
    if t.dtype != torch.int32 or t.numel() < TILE_CTR_WORDS:
        raise ValueError("tile counters: int32 tensor of at least TILE_CTR_WORDS elements")
    return _ptr(t)


def _offsets(offsets):
    """(the int64 array of a squared-sum segment list's offsets, its number of segments)"""
    return (ctypes.c_int64 * len(offsets))(*[int(o) for o in offsets]), len(offsets) - 1


def _wgrad_operands(acts, g_recon, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec, sq_dec, g_pre, x, grad_enc, sq_enc,
                    n, d, tr):
    """cc_wgrad_both*'s first 16 arguments: the 12 weight-gradient operands, then B, h, n, d (tr: the batch operands are
    transposed, acts [h][B])"""
    B, h = acts.shape[::-1] if tr else acts.shape
    return (_ptr(acts), _ptr(g_recon), _ptr(W_dec_hk), _ptr(norms), _ptr(colsum_acts), l1_scale, _ptr(grad_dec),
            _ptr(sq_dec), _ptr(g_pre), _ptr(x), _ptr(grad_enc), _ptr(sq_enc), B, h, n, d)


def _bias_tail(gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, cols):
    """The grad tail's bias operands in the C ABI's order: per slab its pointer, rows (and, cols: the stand-alone
    entries, columns), the bias gradient and its sq partials"""
    out = []
    for slab, g, sq in ((gpre_colpart, g_b_enc, sq_b_enc), (loss_colpart, g_b_dec, sq_b_dec)):
        out += [_ptr(slab), *slab.shape[:2 if cols else 1], _ptr(g), _ptr(sq)]
    return out


def _contig(t, name):
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")
    return t


def _rows_ld(t, name):
    """(rows, row pitch) of a 2-D tensor with contiguous rows"""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be [rows, width] with contiguous rows")
    return t.shape[0], t.stride(0) if t.stride(0) >= t.shape[1] else t.shape[1]


def _like(t, ref, name, ref_name):
    """an optional tensor laid out as `ref`"""
    if t is not None and (t.dtype != ref.dtype or t.shape != ref.shape or t.stride() != ref.stride()
                          or t.device != ref.device):
        raise ValueError(f"{name} must have {ref_name}'s dtype, shape, strides and device")


def _dense(t, dt, shape, dev, name):
    """an optional contiguous tensor of one dtype, shape and device"""
    if t is not None and (t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {dev}")


def check(rc):
    _lib.check(rc)


# ---------------------------------------------------------------- sizing helpers
def col_part_rows(M):
    return int(lib().cc_col_part_rows(M))


def wave_parts(M, N):
    return int(lib().cc_wave_parts(M, N))


def wgrad_parts(h, K, dtype):
    return int(lib().cc_wgrad_parts(h, K, dtype_code(dtype)))


def prep_part_rows(B):
    return int(lib().cc_prep_part_rows(B))


def loss_part_rows(B):
    return int(lib().cc_loss_part_rows(B))


def loss_col_blocks(d):
    return int(lib().cc_loss_col_blocks(d))


def loss_scalars_len(B):
    return int(lib().cc_loss_scalars_len(B))


# ---------------------------------------------------------------- kernels
def gemm_f32out(A, a_layout, Bm, b_layout, M, N, K, out=None):
    """Generic MFMA GEMM (test/diagnostic): see cc_gemm_f32out."""
    lda = A.shape[-1]
    ldb = Bm.shape[-1]
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    check(lib().cc_gemm_f32out(_ptr(A), a_layout, lda, _ptr(Bm), b_layout, ldb, _ptr(out), out.shape[-1],
                               M, N, K, dtype_code(A.dtype), _stream(A)))
    return out


def prep_input(x_in, factor, dtype, out=None, colsum_part=None, out_t=None):
    """x_out[B, n*d] = dtype(x_in * factor[model]) (Buffer.next normalisation + get_losses cast);
    out_t (optional, bf16): also x_out^T [n*d, B]."""
    B, n, d = x_in.shape
    _contig(x_in, "x")
    if out is None:
        out = torch.empty(B, n * d, device=x_in.device, dtype=dtype)
    fdt = dtype_code(factor.dtype) if factor is not None else CC_F32
    if out_t is not None:
        if out_t.shape != (n * d, B) or not out_t.is_contiguous():
            raise ValueError("out_t must be a contiguous [n*d, B] tensor")
        check(lib().cc_prep_input_t(_ptr(x_in), dtype_code(x_in.dtype), _ptr(factor), fdt, _ptr(out), _ptr(out_t),
                                    _ptr(colsum_part), B, n, d, dtype_code(dtype), _stream(x_in)))
    else:
        check(lib().cc_prep_input(_ptr(x_in), dtype_code(x_in.dtype), _ptr(factor), fdt, _ptr(out),
                                  _ptr(colsum_part), B, n, d, dtype_code(dtype), _stream(x_in)))
    return out


def reduce_rows(part, R, C, scale=1.0, out_f32=None, out_t=None, sq_part=None, ld=None, dot_w=None, dot_part=None):
    dt = dtype_code(out_t.dtype) if out_t is not None else CC_F32
    check(lib().cc_reduce_rows(_ptr(part), R, C, C if ld is None else ld, scale, _ptr(out_f32), _ptr(out_t),
                               dt, _ptr(sq_part), _ptr(dot_w), _ptr(dot_part), _stream(part)))


def reduce_parts(C):
    return int(lib().cc_reduce_parts(C))


def dec_norms(W_dec_hk, h, n, d, norms=None, total=None, inv_norms=None):
    if norms is None:
        norms = torch.empty(h, n, device=W_dec_hk.device, dtype=torch.float32)
    if total is None:
        total = torch.empty(h, device=W_dec_hk.device, dtype=torch.float32)
    check(lib().cc_dec_norms(_ptr(W_dec_hk), _ptr(norms), _ptr(total), _ptr(inv_norms), h, n, d,
                             dtype_code(W_dec_hk.dtype), _stream(W_dec_hk)))
    return norms, total


def encode_fwd(x, W_enc_hk, b_enc, acts, apply_relu=True, tn=None, colsum_part=None, l1_part=None,
               l0_part=None):
    B, K = x.shape
    h = W_enc_hk.shape[0]
    check(lib().cc_encode_fwd(_ptr(x), _ptr(W_enc_hk), _ptr(b_enc), _ptr(tn), _ptr(acts), int(apply_relu),
                              _ptr(colsum_part), _ptr(l1_part), _ptr(l0_part), B, K, h, dtype_code(x.dtype),
                              _stream(x)))
    return acts


def mask_bits_words(B, h):
    return int(lib().cc_mask_bits_words(B, h))


def colsum_job(part, rows, cols, scale=1.0, out=None):
    """A column reduction a GEMM launch carries in its prologue (cc_colsum_job: reduce_rows(part, rows, cols,
    scale=scale, out_f32=out) with the same bits), passed by reference."""
    return ctypes.byref(_lib.ColsumJob(part.data_ptr(), rows, cols, part.stride(0) if part.dim() == 2 else cols,
                                       scale, out.data_ptr()))


def encode_fwd_t(x, W_enc_hk, b_enc, acts, acts_t, apply_relu=True, tn=None, colsum_part=None, l1_part=None,
                 l0_part=None, mask_bits=None, tile_ctr=None, pre=None):
    """encode_fwd that also stores acts_t [h][B] = acts^T (bf16, B % 8 == 0) and, optionally, the activation
    mask bits (int32 [mask_bits_words(B, h)]) that dacts_bwd_t reads instead of acts.  tile_ctr: int32
    [TILE_CTR_WORDS] zeroed counters -> dynamic per-XCD tile order (same bits).  pre: a colsum_job the launch
    runs first."""
    B, K = x.shape
    h = W_enc_hk.shape[0]
    if mask_bits is not None and mask_bits.numel() < mask_bits_words(B, h):
        raise ValueError("mask_bits too small")
    check(lib().cc_encode_fwd_t(_ptr(x), _ptr(W_enc_hk), _ptr(b_enc), _ptr(tn), _ptr(acts), _ptr(acts_t),
                                int(apply_relu), _ptr(colsum_part), _ptr(l1_part), _ptr(l0_part), _ptr(mask_bits),
                                _ctr(tile_ctr), pre, B, K, h, dtype_code(x.dtype), _stream(x)))
    return acts


def decode_fwd(acts, W_dec_hk, b_dec=None, recon_f32=None, recon_t=None):
    B, h = acts.shape
    K = W_dec_hk.shape[1]
    check(lib().cc_decode_fwd(_ptr(acts), _ptr(W_dec_hk), _ptr(b_dec), _ptr(recon_f32), _ptr(recon_t), B, h, K,
                              dtype_code(acts.dtype), _stream(acts)))


def decode_ws_floats(B, h, K, dtype):
    return int(lib().cc_decode_ws_floats(B, h, K, dtype_code(dtype)))


def decode_partial(acts, W_dec_hk, recon_f32, ws=None):
    """fp32 acts . W_dec without bias, whole-wave schedule + split-K leftover (cc_decode_fwd_ws)."""
    B, h = acts.shape
    K = W_dec_hk.shape[1]
    check(lib().cc_decode_fwd_ws(_ptr(acts), _ptr(W_dec_hk), _ptr(recon_f32), _ptr(ws),
                                 0 if ws is None else ws.numel(), B, h, K, dtype_code(acts.dtype), _stream(acts)))


def decode_partial_jobs(acts, W_dec_hk, recon_f32, ws, n, d, norm_fin=None, pre=None, wait=None):
    """decode_partial (the same recon_f32 bits) carrying the step's small jobs (cc_decode_partial): pre, an
    ops.colsum_job run before the tiles; norm_fin = (part, norms, total, inv_norms), the decoder norms' finaliser
    (dec_norms_finalize) as extra blocks of the split-K reduction launch; wait = (ctr, target, err_addr): the launch
    waits in the kernel for a done counter of adam_dec_norms on another stream (as decode_loss)."""
    B, h = acts.shape
    part, norms, total, inv = norm_fin if norm_fin is not None else (None, None, None, None)
    wctr, wtarget, werr = wait if wait is not None else (None, 0, None)
    check(lib().cc_decode_partial(_ptr(acts), _ptr(W_dec_hk), _ptr(recon_f32), _ptr(ws), 0 if ws is None else ws.numel(),
                                  _ptr(part), _ptr(norms), _ptr(total), _ptr(inv), pre, _ptr(wctr),
                                  int(wtarget) & 0xFFFFFFFF, werr, B, h, n, d, dtype_code(acts.dtype), _stream(acts)))


def decode_partial_t(acts, W_dec_t, recon_f32, ws=None):
    """decode_partial from the transposed decoder copy W_dec_t [K][h] (cc_decode_fwd_ws_t); same results."""
    B, h = acts.shape
    K = W_dec_t.shape[0]
    check(lib().cc_decode_fwd_ws_t(_ptr(acts), _ptr(W_dec_t), _ptr(recon_f32), _ptr(ws),
                                   0 if ws is None else ws.numel(), B, h, K, dtype_code(acts.dtype), _stream(acts)))


def decode_loss_ncb(B, h, n, d, dtype):
    """Row-term column blocks per model of decode_loss_t's row_part (d / 64), 0 if it does not serve the shape."""
    return int(lib().cc_decode_loss_ncb(B, h, n, d, dtype_code(dtype)))


def decode_loss_t(acts, W_dec_t, b_dec, x, x_mean, grad_scale, g_recon, g_recon_t, row_part, col_part, ws, n, d):
    """G2 + the reconstruction loss in one pass (cc_decode_loss_t): g_recon / g_recon_t bit-identical to
    decode_partial_t + loss_fwd_bwd(g_recon_t=...); row_part [2, n * d/64, B], col_part [B/128, K]."""
    B, h = acts.shape
    check(lib().cc_decode_loss_t(_ptr(acts), _ptr(W_dec_t), _ptr(b_dec), _ptr(x), _ptr(x_mean), grad_scale,
                                 _ptr(g_recon), _ptr(g_recon_t), _ptr(row_part), _ptr(col_part), _ptr(ws),
                                 0 if ws is None else ws.numel(), B, h, n, d, dtype_code(acts.dtype), _stream(acts)))


def decode_loss(acts, W_dec_hk, b_dec, x, x_mean, grad_scale, g_recon, g_recon_t, row_part, col_part, ws, n, d,
                norm_fin=None, pre=None, wait=None):
    """decode_loss_t reading W_dec [h, K] itself (cc_decode_loss, transposed LDS reads of the B operand): the same
    bits without the W_dec^T copy.  g_recon_t may be None.  norm_fin = (part, norms, total, inv_norms): the decoder
    norms' finaliser (dec_norms_finalize) rides in the launch.  wait = (ctr, target, err_addr): the launch waits in
    the kernel for a done counter of adam_dec_norms on another stream (err_addr: host-visible word set on a
    timeout)."""
    B, h = acts.shape
    part, norms, total, inv = norm_fin if norm_fin is not None else (None, None, None, None)
    wctr, wtarget, werr = wait if wait is not None else (None, 0, None)
    check(lib().cc_decode_loss(_ptr(acts), _ptr(W_dec_hk), _ptr(b_dec), _ptr(x), _ptr(x_mean), grad_scale,
                               _ptr(g_recon), _ptr(g_recon_t), _ptr(row_part), _ptr(col_part), _ptr(ws),
                               0 if ws is None else ws.numel(), _ptr(part), _ptr(norms), _ptr(total), _ptr(inv), pre,
                               _ptr(wctr), int(wtarget) & 0xFFFFFFFF, werr, B, h, n, d, dtype_code(acts.dtype),
                               _stream(acts)))


def loss_fwd_bwd(recon_f32, b_dec, x, x_mean, g_recon, row_part, col_part, grad_scale, B, n, d, row0=0, rows=None,
                 g_recon_t=None):
    """Loss terms + g_recon for batch rows [row0, row0 + rows) (default: all B rows);
    g_recon_t (optional, bf16 [n*d, B]): also those rows of g_recon^T."""
    rows = B - row0 if rows is None else rows
    if g_recon_t is not None:
        if g_recon_t.shape != (n * d, B) or not g_recon_t.is_contiguous():
            raise ValueError("g_recon_t must be a contiguous [n*d, B] tensor")
        check(lib().cc_loss_fwd_bwd_rows_t(_ptr(recon_f32), _ptr(b_dec), _ptr(x), _ptr(x_mean), _ptr(g_recon),
                                           _ptr(g_recon_t), _ptr(row_part), _ptr(col_part), grad_scale, row0, rows,
                                           B, n, d, dtype_code(x.dtype), _stream(x)))
        return
    check(lib().cc_loss_fwd_bwd_rows(_ptr(recon_f32), _ptr(b_dec), _ptr(x), _ptr(x_mean), _ptr(g_recon),
                                     _ptr(row_part), _ptr(col_part), grad_scale, row0, rows, B, n, d,
                                     dtype_code(x.dtype), _stream(x)))


def loss_finalize(row_part, l1_part, n_l1, l0_part, n_l0, ev, ev_a, ev_b, scalars, B, n, d, l1l0_out=None,
                  host=None, seq=0, ncb=None):
    """host (optional): a _hip.MappedHostBuffer that also receives scalars[0:8] and then `seq` in word 8.
    ncb: row_part's column blocks per model when it is not loss_fwd_bwd's layout (decode_loss_t's)."""
    if ncb is not None:
        check(lib().cc_loss_finalize_nb(_ptr(row_part), ncb, _ptr(l1_part), n_l1, _ptr(l0_part), n_l0, _ptr(ev),
                                        _ptr(ev_a), _ptr(ev_b), _ptr(scalars), _ptr(l1l0_out),
                                        host.device_ptr if host is not None else None, seq, B, n, d,
                                        _stream(row_part)))
        return
    if host is not None:
        check(lib().cc_loss_finalize_mapped(_ptr(row_part), _ptr(l1_part), n_l1, _ptr(l0_part), n_l0, _ptr(ev),
                                            _ptr(ev_a), _ptr(ev_b), _ptr(scalars), _ptr(l1l0_out), host.device_ptr,
                                            seq, B, n, d, _stream(row_part)))
        return
    check(lib().cc_loss_finalize(_ptr(row_part), _ptr(l1_part), n_l1, _ptr(l0_part), n_l0, _ptr(ev), _ptr(ev_a),
                                 _ptr(ev_b), _ptr(scalars), _ptr(l1l0_out), B, n, d, _stream(row_part)))


def loss_tail(colsum_acts, tn, l1_part, row_part, l0_part, n_l0, ev, ev_a, ev_b, scalars, B, n, d, counter,
              l1l0_out=None, host=None, seq=0, ncb=None):
    """The l1 dot partials from the reduced activation column sums + loss_finalize as one launch whose
    workgroups fit beside a persistent GEMM (cc_loss_tail; the same bits as reduce_rows(.., dot_part) +
    loss_finalize).  ncb: row_part's column blocks per model (default loss_fwd_bwd's layout)."""
    h = colsum_acts.numel()
    check(lib().cc_loss_tail(_ptr(colsum_acts), _ptr(tn), h, _ptr(l1_part), _ptr(row_part),
                             loss_col_blocks(d) if ncb is None else ncb, _ptr(l0_part), n_l0, _ptr(ev), _ptr(ev_a),
                             _ptr(ev_b), _ptr(scalars), _ptr(l1l0_out), host.device_ptr if host is not None else None,
                             seq, B, n, d, _ptr(counter), _stream(colsum_acts)))


def grad_tail(gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, sq, offsets, max_norm, emulate_bf16,
              out, counter):
    """The two bias-gradient reduce_rows (+ sq partials) + clip_finalize as one launch (same bits)."""
    arr, nparams = _offsets(offsets)
    check(lib().cc_grad_tail(*_bias_tail(gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, True),
                             dtype_code(g_b_enc.dtype), _ptr(sq), arr, nparams, max_norm, int(emulate_bf16), _ptr(out),
                             _ptr(counter), _stream(sq)))


def grad_tail_sums(gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, sq, offsets, out, counter,
                   zero_mask=0):
    """The two bias-gradient reduce_rows (+ sq partials) + segment_sums as one launch (same bits)."""
    arr, nparams = _offsets(offsets)
    check(lib().cc_grad_tail_sums(*_bias_tail(gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, True),
                                  dtype_code(g_b_enc.dtype), _ptr(sq), arr, nparams, int(zero_mask), _ptr(out),
                                  _ptr(counter), _stream(sq)))


def segment_sums(sq, offsets, out, zero_mask=0):
    """out[p] = sum(sq[offsets[p]:offsets[p+1]]) (0 where bit p of zero_mask is set)."""
    arr, nparams = _offsets(offsets)
    check(lib().cc_segment_sums(_ptr(sq), arr, nparams, int(zero_mask), _ptr(out), _stream(sq)))


def dacts_bwd(g_recon, W_dec_hk, acts, tn, l1_scale, g_pre, colsum_part=None):
    B, K = g_recon.shape
    h = W_dec_hk.shape[0]
    check(lib().cc_dacts_bwd(_ptr(g_recon), _ptr(W_dec_hk), _ptr(acts), _ptr(tn), l1_scale, _ptr(g_pre),
                             _ptr(colsum_part), B, K, h, dtype_code(g_recon.dtype), _stream(g_recon)))


def loss_tail_job(colsum_acts, tn, l1_part, row_part, l0_part, n_l0, ev, ev_a, ev_b, scalars, B, n, d, counter,
                  l1l0_out=None, host=None, seq=0, ncb=None):
    """loss_tail's arguments as a cc_loss_tail_job a d_acts launch carries (dacts_bwd_t(tail=...)), by reference."""
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    return ctypes.byref(_lib.LossTailJob(
        p(colsum_acts), p(tn), colsum_acts.numel(), p(l1_part), p(row_part), loss_col_blocks(d) if ncb is None else ncb,
        p(l0_part), n_l0, p(ev), p(ev_a), p(ev_b), p(scalars), p(l1l0_out),
        host.device_ptr.value if host is not None else None, seq, B, n, p(counter)))


def dacts_bwd_t(g_recon, W_dec_hk, acts, tn, l1_scale, g_pre_t, colsum_part=None, mask_bits=None, tile_ctr=None,
                tail=None):
    """dacts_bwd storing g_pre transposed only: g_pre_t [h][>= B] view (column slice allowed, row stride
    g_pre_t.stride(0)).  mask_bits: encode_fwd_t's bits of these rows (see mask_bits_rows)."""
    B, K = g_recon.shape
    h = W_dec_hk.shape[0]
    if g_pre_t.shape[0] != h or g_pre_t.shape[1] != B or g_pre_t.stride(1) != 1:
        raise ValueError("g_pre_t must be an [h, B] view with unit column stride")
    if mask_bits is not None and mask_bits.numel() < mask_bits_words(B, h):
        raise ValueError("mask_bits too small")
    check(lib().cc_dacts_bwd_t(_ptr(g_recon), _ptr(W_dec_hk), _ptr(acts), _ptr(tn), l1_scale, _ptr(mask_bits),
                               _ptr(g_pre_t), g_pre_t.stride(0), _ptr(colsum_part), _ctr(tile_ctr), tail, B, K, h,
                               dtype_code(g_recon.dtype), _stream(g_recon)))


def mask_bits_rows(mask_bits, h, r0, r1):
    """The mask bits of batch rows [r0, r1) (r0 % 256 == 0) of encode_fwd_t's [B][h] bits."""
    if r0 % 256:
        raise ValueError("mask bits slices start on a 256-row tile")
    w = mask_bits_words(256, h)
    return mask_bits[(r0 // 256) * w:]


def transpose(src, out=None):
    """out [cols, rows] = src^T for a 2-D 16-bit tensor (rows, cols % 8 == 0); out may be a column slice view."""
    rows, cols = src.shape
    if src.element_size() != 2 or src.stride(1) != 1:
        raise ValueError("transpose: 2-D 16-bit tensor with unit column stride")
    if out is None:
        out = torch.empty(cols, rows, dtype=src.dtype, device=src.device)
    if out.shape != (cols, rows) or out.stride(1) != 1 or out.dtype != src.dtype:
        raise ValueError("transpose: out must be [cols, rows] of the same dtype, unit column stride")
    check(lib().cc_transpose_b16(_ptr(src), rows, cols, src.stride(0), _ptr(out), out.stride(0), _stream(src)))
    return out


def dec_norms_part_floats(h, n, d):
    return int(lib().cc_dec_norms_part_floats(h, n, d))


def transpose_dec_norms(W_dec_hk, n, d, W_dec_t, part, norms, total, inv_norms=None):
    """W_dec_t = W_dec^T and dec_norms' outputs (same bits) from one pass over W_dec (d % 64 == 0)."""
    h = W_dec_hk.shape[0]
    check(lib().cc_transpose_dec_norms(_ptr(W_dec_hk), h, n, d, _ptr(W_dec_t), _ptr(part), _ptr(norms), _ptr(total),
                                       _ptr(inv_norms), _stream(W_dec_hk)))


def dec_norms_finalize(part, h, n, d, norms, total, inv_norms=None):
    check(lib().cc_dec_norms_finalize(_ptr(part), h, n, d, _ptr(norms), _ptr(total), _ptr(inv_norms),
                                      _stream(part)))


def adam_dec_norms(p, g, m, v, h, K, lr, beta1, beta2, eps, step, part, coef=None, clip_sums=None, emulate=True,
                   max_blocks=0, done_ctr=None):
    """Adam over the decoder half p/g/m/v (flat views, W_dec [h, K] first) that also writes the decoder-norm
    partials of the updated W_dec into `part` (cc_adam_dec_norms; dec_norms_finalize completes them).
    coef: the clip coefficient tensor; or clip_sums = (sums, max_norm): formed in the kernel.  done_ctr (int32
    device word, max_blocks > 0): each workgroup adds 1 when its results are released; returns the number of
    workgroups (adam_capped_blocks) then, else None."""
    sums, max_norm = clip_sums if clip_sums is not None else (None, 0.0)
    check(lib().cc_adam_dec_norms(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(coef), _ptr(sums),
                                  0 if sums is None else sums.numel(), float(max_norm), int(emulate), lr, beta1, beta2,
                                  eps, int(step), int(max_blocks), _ptr(part), h, K, dtype_code(p.dtype),
                                  _ptr(done_ctr), _stream(p)))
    return adam_capped_blocks(p.numel(), max_blocks) if done_ctr is not None else None


def adam_capped_blocks(numel, max_blocks):
    """Workgroups of the capped-grid Adam launch (cc_adam_capped_blocks)."""
    return int(lib().cc_adam_capped_blocks(int(numel), int(max_blocks)))


def adam_dec_transposed(p, g, m, v, coef, lr, beta1, beta2, eps, step, W_dec_t, part, max_blocks=0):
    """Adam over the decoder matrix p/g/m/v [h, K] (views into the arenas) + W_dec_t = p^T and the
    decoder-norm partials from the same pass."""
    h, K = p.shape
    check(lib().cc_adam_dec_transposed(_ptr(p), _ptr(g), _ptr(m), _ptr(v), h, K, _ptr(coef), lr, beta1, beta2, eps,
                                       int(step), int(max_blocks), _ptr(W_dec_t), _ptr(part), dtype_code(p.dtype),
                                       _stream(p)))


def wgrad_dec(acts, g_recon, W_dec_hk, norms, colsum_acts, l1_scale, grad, sq_part, n, d):
    B, h = acts.shape
    check(lib().cc_wgrad_dec(_ptr(acts), _ptr(g_recon), _ptr(W_dec_hk), _ptr(norms), _ptr(colsum_acts), l1_scale,
                             _ptr(grad), _ptr(sq_part), B, h, n, d, dtype_code(acts.dtype), _stream(acts)))


def wgrad_enc(g_pre, x, grad, sq_part):
    B, h = g_pre.shape
    K = x.shape[1]
    check(lib().cc_wgrad_enc(_ptr(g_pre), _ptr(x), _ptr(grad), _ptr(sq_part), B, h, K, dtype_code(g_pre.dtype),
                             _stream(g_pre)))


def wgrad_both(acts, g_recon, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec, sq_dec, g_pre, x, grad_enc, sq_enc,
               n, d):
    """wgrad_dec + wgrad_enc (same results), one launch where the ping-pong GEMM serves both."""
    check(lib().cc_wgrad_both(*_wgrad_operands(acts, g_recon, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec, sq_dec,
                                               g_pre, x, grad_enc, sq_enc, n, d, False),
                              dtype_code(acts.dtype), _stream(acts)))


def wgrad_both_t(actsT, g_reconT, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec, sq_dec, g_preT, xT, grad_enc,
                 sq_enc, n, d):
    """wgrad_both from transposed batch operands (actsT / g_preT [h][B], g_reconT / xT [n*d][B]); same results."""
    check(lib().cc_wgrad_both_t(*_wgrad_operands(actsT, g_reconT, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec,
                                                 sq_dec, g_preT, xT, grad_enc, sq_enc, n, d, True),
                                dtype_code(actsT.dtype), _stream(actsT)))


def wgrad_tile_sums(h, K):
    """floats of the per-tile squared-sum scratch of wgrad_both_clip_t / wgrad_both_sums_t (the tile sums, then the
    launch clock words: see wgrad_clock)"""
    return int(lib().cc_wgrad_tile_sums(h, K))


WGRAD_CLOCK_WORDS = 8  # floats at the end of the tile-sum scratch: 4 uint64 clock words (gemm.hip WgradTail::clock)


def wgrad_clock(tile_sum):
    """The clock words the fused G4G5 launches accumulate at the end of their tile-sum scratch, as a view
    [shader-clock ticks, 100 MHz ticks, launches, reserved] (int64; zero them to start a window).  The scratch is
    exactly cc_wgrad_tile_sums floats (_check_tile_sum), so the kernel's clock words are its last 8."""
    return tile_sum[-WGRAD_CLOCK_WORDS:].view(torch.int64)


def _check_tile_sum(tile_sum, h, K):
    # (exactly: the launch writes its clock words after the tile sums, and wgrad_clock reads the buffer's last 8)
    if tile_sum.dtype != torch.float32 or not tile_sum.is_contiguous() or tile_sum.numel() != wgrad_tile_sums(h, K):
        raise ValueError(f"tile_sum must be a contiguous fp32 buffer of exactly {wgrad_tile_sums(h, K)} floats "
                         f"(cc_wgrad_tile_sums({h}, {K})), got {tuple(tile_sum.shape)} {tile_sum.dtype}")


def wgrad_both_clip_t(actsT, g_reconT, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec, sq_dec, g_preT, xT, grad_enc,
                      sq_enc, n, d, gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, sq, offsets,
                      max_norm, emulate_bf16, out, counter, tile_sum, tile_ctr=None, abort_ptr=None):
    """wgrad_both_t + grad_tail in one launch (the bias sums before the GEMM tiles, the clip coefficient
    in the last workgroup); same outputs.  abort_ptr: device address of the step's abort word (when set, out[0] is
    written as CLIP_ABORTED and the Adam launches reading it apply nothing)."""
    _check_tile_sum(tile_sum, actsT.shape[0], n * d)
    arr, nparams = _offsets(offsets)
    check(lib().cc_wgrad_both_clip_t(
        *_wgrad_operands(actsT, g_reconT, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec, sq_dec, g_preT, xT,
                         grad_enc, sq_enc, n, d, True),
        *_bias_tail(gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, False), _ptr(sq), arr, nparams,
        max_norm, int(emulate_bf16), _ptr(out), _ptr(counter), _ptr(tile_sum), _ctr(tile_ctr), _vptr(abort_ptr),
        dtype_code(actsT.dtype), _stream(actsT)))


CLIP_ABORTED = -1.0  # clip_out[0] of a step whose update was not applied (include/crosscoder_hip.h)


def wgrad_both_sums_t(actsT, g_reconT, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec, sq_dec, g_preT, xT, grad_enc,
                      sq_enc, n, d, gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, sq, offsets, out,
                      counter, tile_sum, zero_mask=0, tile_ctr=None, abort_ptr=None):
    """wgrad_both_t + grad_tail_sums in one launch (the latent-sharded step); same outputs.  abort_ptr: device address
    of the step's abort word (when set, every out[p] is -inf: the all-reduced sums abort every rank's Adam)."""
    _check_tile_sum(tile_sum, actsT.shape[0], n * d)
    arr, nparams = _offsets(offsets)
    check(lib().cc_wgrad_both_sums_t(
        *_wgrad_operands(actsT, g_reconT, W_dec_hk, norms, colsum_acts, l1_scale, grad_dec, sq_dec, g_preT, xT,
                         grad_enc, sq_enc, n, d, True),
        *_bias_tail(gpre_colpart, g_b_enc, sq_b_enc, loss_colpart, g_b_dec, sq_b_dec, False), _ptr(sq), arr, nparams,
        int(zero_mask), _ptr(out), _ptr(counter), _ptr(tile_sum), _ctr(tile_ctr), _vptr(abort_ptr),
        dtype_code(actsT.dtype), _stream(actsT)))


def clip_finalize(sq, offsets, max_norm, emulate_bf16, out):
    arr, nparams = _offsets(offsets)
    check(lib().cc_clip_finalize(_ptr(sq), arr, nparams, max_norm, int(emulate_bf16), _ptr(out), _stream(sq)))


def adam_step(p, g, m, v, coef, lr, beta1, beta2, eps, step, max_blocks=0):
    check(lib().cc_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(coef), lr, beta1, beta2, eps,
                             int(step), int(max_blocks), dtype_code(p.dtype), _stream(p)))


def adam_master_step(p32, g16, m32, v32, p16, coef, lr, beta1, beta2, eps, step, max_blocks=0):
    """The master-weight Adam step (cc_adam_master_step): fp32 p32 / m32 / v32 updated in place from the bf16
    gradient g16 with the bits of the fp32 adam_step on g16.float(), and p16 = p32 rounded to bf16.  All flat,
    contiguous, of one length and on one device; max_blocks as adam_step's."""
    n = p32.numel()
    for name, t, dt in (("p32", p32, torch.float32), ("g16", g16, torch.bfloat16), ("m32", m32, torch.float32),
                        ("v32", v32, torch.float32), ("p16", p16, torch.bfloat16)):
        if t.dtype != dt or t.numel() != n or t.device != p32.device:
            raise ValueError(f"adam_master_step: {name} must be a {dt} tensor of {n} elements on {p32.device}")
        _contig(t, name)
    check(lib().cc_adam_master_step(_ptr(p32), _ptr(g16), _ptr(m32), _ptr(v32), _ptr(p16), n, _ptr(coef), lr, beta1,
                                    beta2, eps, int(step), int(max_blocks), _stream(p32)))


def prep_job_ok(x_in, factor, dtype, out_t):
    """Whether prep_input(x_in, factor, dtype, out_t=out_t) can ride in an Adam launch (prep_job)."""
    return (out_t is not None and dtype == torch.bfloat16 and x_in.dim() == 3 and x_in.shape[0] % 8 == 0
            and x_in.shape[2] % 8 == 0 and x_in.dtype in _DT and x_in.is_contiguous() and x_in.data_ptr() % 16 == 0
            and (factor is None or factor.dtype in _DT))


def prep_job(x_in, factor, out, colsum_part, out_t):
    """prep_input(x_in, factor, bf16, out=out, colsum_part=colsum_part, out_t=out_t) as a job an Adam launch carries
    (cc_prep_job, adam_step_prep), passed by reference."""
    B, n, d = x_in.shape
    _contig(x_in, "x")
    if out.shape != (B, n * d) or out.dtype != torch.bfloat16 or not out.is_contiguous():
        raise ValueError("out must be a contiguous bf16 [B, n*d] tensor")
    if out_t.shape != (n * d, B) or out_t.dtype != torch.bfloat16 or not out_t.is_contiguous():
        raise ValueError("out_t must be a contiguous bf16 [n*d, B] tensor")
    fdt = dtype_code(factor.dtype) if factor is not None else CC_F32
    return ctypes.byref(_lib.PrepJob(x_in.data_ptr(), dtype_code(x_in.dtype),
                                     factor.data_ptr() if factor is not None else None, fdt, out.data_ptr(),
                                     out_t.data_ptr(), colsum_part.data_ptr() if colsum_part is not None else None,
                                     B, n, d))


def adam_step_prep(p, g, m, v, coef, lr, beta1, beta2, eps, step, prep):
    """adam_step (one-pass form, bf16, numel % 8 == 0) whose launch also runs the prep_job `prep`: the same bits as
    the two launches."""
    check(lib().cc_adam_step_prep(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(coef), lr, beta1, beta2, eps,
                                  int(step), dtype_code(p.dtype), prep, _stream(p)))


def adam_step_clip(p, g, m, v, sums, max_norm, emulate_bf16, lr, beta1, beta2, eps, step, max_blocks=0,
                   clip_out=None):
    """adam_step with the clip coefficient formed in the kernel from per-parameter squared sums (fp32 [nparams])."""
    check(lib().cc_adam_step_clip(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(sums), sums.numel(),
                                  float(max_norm), int(emulate_bf16), _ptr(clip_out), lr, beta1, beta2, eps, int(step),
                                  int(max_blocks), dtype_code(p.dtype), _stream(p)))


# ---------------------------------------------------------------- around the step
def gather_rows(src, perm, out=None):
    """out[i] = src[perm[i]] over dim 0 (Buffer.refresh's shuffle); perm int64 on the same device."""
    _contig(src, "src")
    if perm.dtype != torch.int64 or perm.device != src.device:
        raise ValueError("perm must be an int64 tensor on the source's device")
    rows = perm.numel()
    if out is None:
        out = torch.empty((rows,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    _contig(out, "out")
    row_bytes = src.element_size()
    for s_ in src.shape[1:]:
        row_bytes *= s_
    check(lib().cc_gather_rows(_ptr(src), src.shape[0], _ptr(perm.contiguous()), _ptr(out), rows, row_bytes,
                               _stream(src)))
    return out


def fold_scaling(W_enc_hk, W_dec_hk, b_dec_flat, scale, n, d):
    """In place W_enc[m] *= s[m], W_dec[:, m] /= s[m], b_dec[m] /= s[m] (scale: fp32 device [n];
    W_dec_hk / b_dec_flat may be None: encoder-only fold)."""
    h = W_enc_hk.shape[0]
    check(lib().cc_fold_scaling(_ptr(W_enc_hk), _ptr(W_dec_hk), _ptr(b_dec_flat), _ptr(scale), h, n, d,
                                dtype_code(W_enc_hk.dtype), _stream(W_enc_hk)))


def decoder_stats(W_dec_hk, n, d):
    """norms [h, n], relative norms [h], cosine similarities [h] (fp32) of W_dec."""
    h = W_dec_hk.shape[0]
    dev = W_dec_hk.device
    norms = torch.empty(h, n, device=dev, dtype=torch.float32)
    rel = torch.empty(h, device=dev, dtype=torch.float32)
    cos = torch.empty(h, device=dev, dtype=torch.float32)
    check(lib().cc_decoder_stats(_ptr(W_dec_hk), h, n, d, dtype_code(W_dec_hk.dtype), _ptr(norms), _ptr(rel),
                                 _ptr(cos), _stream(W_dec_hk)))
    return norms, rel, cos


# ---------------------------------------------------------------- latent statistics (latent_stats.py)
def latent_stats_max_k():
    return int(lib().cc_latent_stats_max_k())


def latent_stats_update(acts, h, k, count, sum_, hist, topk_val, topk_row, row_ids=None, row0=0):
    """One pass over acts [B, ld >= h] (rows contiguous) folded into the state tensors for latents 0..h-1:
    count [h] int64, sum_ [h] fp32, hist [h, 32] int64 or None, topk_val [h, k] fp32, topk_row [h, k] int64
    (cc_latent_stats_update; fresh state: zeros, topk_row -1).  Row b has id row_ids[b] (int64 [B] on the
    device) or row0 + b."""
    B, ld = _rows_ld(acts, "acts")
    dev = acts.device
    for name, t, dt, shape in (("count", count, torch.int64, (h,)), ("sum", sum_, torch.float32, (h,)),
                               ("hist", hist, torch.int64, (h, 32)), ("topk_val", topk_val, torch.float32, (h, k)),
                               ("topk_row", topk_row, torch.int64, (h, k))):
        if t is None and name == "hist":
            continue
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {dev}")
    if row_ids is not None:
        if row_ids.dtype != torch.int64 or row_ids.device != dev or tuple(row_ids.shape) != (B,):
            raise ValueError(f"row_ids must be an int64 tensor of shape ({B},) on {dev}")
        row_ids = row_ids.contiguous()
    check(lib().cc_latent_stats_update(_ptr(acts), ld, B, h, dtype_code(acts.dtype), _ptr(row_ids), int(row0), int(k),
                                       _ptr(count), _ptr(sum_), _ptr(hist), _ptr(topk_val), _ptr(topk_row),
                                       _stream(acts)))


# ---------------------------------------------------------------- latent scaling (latent_scaling.py)
def _pitched(t, cols, name):
    """(pointer, row pitch) of a 2-D operand with contiguous rows of at least `cols` elements; a column slice
    of a wider matrix (one model of [.., n*d]) keeps the wide matrix's pitch."""
    if t.dim() != 2 or t.shape[1] < cols or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name} must be [rows, >= {cols}] with contiguous rows, got {tuple(t.shape)}")
    return _ptr(t), t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _int_at_least(v, name, least=1):
    """a Python int (not a bool) >= least"""
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError(f"{name} must be an int >= {least}, got {v!r}")
    return v


def _mult8(v, name):
    """a Python int (not a bool), a multiple of 8, >= 8"""
    if isinstance(v, bool) or not isinstance(v, int) or v < 8 or v % 8:
        raise ValueError(f"{name} must be an int multiple of 8, got {v!r}")
    return v


def _rows(t, rows, K, dt, dev, name, optional=False):
    """(pointer, row pitch) of the operand t [rows, >= K] of dt on dev (_pitched: a column slice keeps its pitch);
    optional: (None, 0) for None"""
    if t is None and optional:
        return None, 0
    if t is None or t.dim() != 2 or t.shape[0] != rows or t.shape[1] < K or t.dtype != dt or t.device != dev:
        raise ValueError(f"{name} must be [{rows}, >= {K}] of {dt} on {dev}"
                         + ("" if t is None else f", got {t.dtype} {tuple(t.shape)}"))
    return _pitched(t, K, name)


def _decoder(W_dec, K, dt, dev, h):
    """(pointer, row pitch, h) of the decoder operand W_dec [>= h, >= K] of dt on dev; h defaults to W_dec's rows"""
    if W_dec.dim() != 2 or W_dec.shape[1] < K or W_dec.dtype != dt or W_dec.device != dev:
        raise ValueError(f"W_dec must be [h, >= {K}] of {dt} on {dev}, got {W_dec.dtype} {tuple(W_dec.shape)}")
    h = W_dec.shape[0] if h is None else h
    if isinstance(h, bool) or not isinstance(h, int) or not 1 <= h <= W_dec.shape[0]:
        raise ValueError(f"h must be an int in 1..{W_dec.shape[0]} (W_dec's rows), got {h!r}")
    return (*_pitched(W_dec, K, "W_dec"), h)


def _scratch(ws, dt, need, dev, name="ws"):
    """an optional contiguous scratch buffer of dt with at least `need` elements on dev"""
    if ws is not None and (ws.dtype != dt or ws.device != dev or not ws.is_contiguous() or ws.numel() < need):
        raise ValueError(f"{name} must be a contiguous {dt} tensor of at least {need} elements on {dev}")


def latent_scaling(Y, W, acts, dot_part, sq_part=None):
    """dot_part [col_part_rows(B), h] fp32 <- per 128-row group, sum_i acts[i, j] * (W[j] . Y[i]); sq_part (same
    shape, optional) <- sum_i acts[i, j]^2 (cc_latent_scaling; reduce_rows over the slab rows gives the sums).
    Y [B, d], W [h, d] and acts [B, >= h] may be column slices of wider matrices (their row pitch is kept)."""
    B, d = Y.shape
    h = W.shape[0]
    if W.shape[1] != d or acts.shape[0] != B or Y.dtype != W.dtype or Y.dtype != acts.dtype:
        raise ValueError("latent_scaling: Y [B, d], W [h, d], acts [B, >= h] of one dtype")
    R = col_part_rows(B)
    for name, t in (("dot_part", dot_part), ("sq_part", sq_part)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (R, h) or not t.is_contiguous()
                              or t.device != Y.device):
            raise ValueError(f"{name} must be a contiguous fp32 tensor of shape ({R}, {h}) on {Y.device}")
    (py, ldy), (pw, ldw), (pa, lda) = _pitched(Y, d, "Y"), _pitched(W, d, "W"), _pitched(acts, h, "acts")
    check(lib().cc_latent_scaling(py, ldy, pw, ldw, pa, lda, _ptr(dot_part), _ptr(sq_part), B, d, h,
                                  dtype_code(Y.dtype), _stream(Y)))


# ---------------------------------------------------------------- decoder matching (decoder_match.py)
def _keys(t, shape, name, dev):
    if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
        raise ValueError(f"{name} must be a contiguous int64 tensor of shape {shape} on {dev}")
    return _ptr(t)


def decoder_match(Wc, Wq, c_scale, q_scale, key_part, row0=0, exclude_diag=False):
    """key_part [col_part_rows(M), N] int64 <- per 128-row group of the M candidates Wc [M, K] (global indices
    row0 .. row0 + M - 1) and per query row of Wq [N, K], the best (cosine, candidate) pair as a 64-bit key
    (cc_decoder_match; match_reduce folds the slab rows into the running best).  c_scale [>= row0 + M] is the whole
    candidate set's fp32 inverse norms, q_scale [N] the queries'.  Wc and Wq may be row or column slices of wider
    matrices (their row pitch is kept)."""
    M, K = Wc.shape
    N = Wq.shape[0]
    if Wq.shape[1] != K or Wc.dtype != Wq.dtype or Wc.device != Wq.device:
        raise ValueError("decoder_match: Wc [M, K] and Wq [N, K] of one dtype on one device")
    _int_at_least(row0, "row0", 0)
    for name, t, least in (("c_scale", c_scale, row0 + M), ("q_scale", q_scale, N)):
        if (t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.device != Wc.device
                or (t.shape[0] < least if name == "c_scale" else t.shape[0] != least)):
            raise ValueError(f"{name} must be a contiguous fp32 vector of {'at least ' if name == 'c_scale' else ''}"
                             f"{least} elements on {Wc.device}")
    pk = _keys(key_part, (col_part_rows(M), N), "key_part", Wc.device)
    (pc, ldc), (pq, ldq) = _pitched(Wc, K, "Wc"), _pitched(Wq, K, "Wq")
    check(lib().cc_decoder_match(pc, ldc, pq, ldq, _ptr(c_scale), _ptr(q_scale), pk, M, N, K, row0,
                                 1 if exclude_diag else 0, dtype_code(Wc.dtype), _stream(Wc)))


def match_reduce(key_part, best):
    """best [N] int64 (in/out; zeros = nothing seen) <- max(best, max over the rows of key_part [R, N]) as unsigned
    64-bit keys (cc_match_reduce)."""
    if key_part.dim() != 2 or key_part.shape[0] < 1:
        raise ValueError(f"key_part must be [R >= 1, N], got {tuple(key_part.shape)}")
    R, N = key_part.shape
    pk = _keys(key_part, (R, N), "key_part", key_part.device)
    pb = _keys(best, (N,), "best", key_part.device)
    check(lib().cc_match_reduce(pk, R, N, pb, _stream(key_part)))


# ---------------------------------------------------------------- per-row top-k (TopK crosscoders)
def topk_part_rows(B, h):
    return int(lib().cc_topk_part_rows(B, h))


def topk_l0_parts(B, h):
    return int(lib().cc_topk_l0_parts(B, h))


def topk_rows(acts, h, k, out=None, idx_out=None, val_out=None, colsum_part=None, l0_part=None):
    """Each row of acts [B, ld >= h] (rows contiguous), first h columns, reduced to its k largest positive values
    (ties: the smaller latent first; cc_topk_rows).  out: the masked activations (may be `acts` itself: in place);
    idx_out int32 [B, k] / val_out [B, k] (acts' dtype): the selected pairs by ascending latent, padded with
    (-1, 0); colsum_part fp32 [topk_part_rows(B, h), h] / l0_part fp32 [topk_l0_parts(B, h)]: column-sum partials
    and selected counts of the masked activations."""
    B, ld = _rows_ld(acts, "acts")
    dev = acts.device
    _like(out, acts, "out", "acts")
    if (idx_out is None) != (val_out is None):
        raise ValueError("idx_out and val_out go together")
    _dense(idx_out, torch.int32, (B, k), dev, "idx_out")
    _dense(val_out, acts.dtype, (B, k), dev, "val_out")
    _dense(colsum_part, torch.float32, (topk_part_rows(B, h), h), dev, "colsum_part")
    _dense(l0_part, torch.float32, (topk_l0_parts(B, h),), dev, "l0_part")
    check(lib().cc_topk_rows(_ptr(acts), ld, B, h, dtype_code(acts.dtype), int(k), _ptr(out), _ptr(idx_out),
                             _ptr(val_out), _ptr(colsum_part), _ptr(l0_part), _stream(acts)))
    return out


# ---------------------------------------------------------------- sparse decode from pairs (the pairs' consumer)
def decode_pairs(val, idx, W_dec, b_dec, n, d, h=None, recon=None, x=None, sq_err=None):
    """The decode of k (value, latent) pairs per row, topk_rows' val_out / idx_out (cc_decode_pairs): per row r and
    column c an fp32 fma chain  b_dec[c] + sum_s val[r, s] * W_dec[idx[r, s], c]  over the slots in order, rounded
    once to the dtype.  A slot whose index is outside [0, h) adds nothing (h defaults to W_dec's rows).
    val [B, k] (bf16 / fp32) and idx [B, k] int32, contiguous; W_dec [>= h, >= n * d], b_dec [n * d]; recon and x
    [B, >= n * d] of val's dtype (W_dec, recon and x may be column slices of wider matrices: their row pitch is
    kept); sq_err fp32 [B, n]: per row and model, the squared error of the rounded reconstruction against x.
    Without x: writes (and returns) recon, allocated if not given.  With x: writes sq_err (allocated if not given),
    and recon only if given.  -> (recon or None, sq_err or None)."""
    B, k = _pairs_idx(idx, val)
    _int_at_least(n, "n")
    _mult8(d, "d")
    K, dt, dev = n * d, val.dtype, val.device
    pw, ldw, h = _decoder(W_dec, K, dt, dev, h)
    _dense(b_dec, dt, (K,), dev, "b_dec")
    if sq_err is not None and x is None:
        raise ValueError("sq_err needs x")
    _dense(sq_err, torch.float32, (B, n), dev, "sq_err")
    (pr, ldr), (px, ldx) = _rows(recon, B, K, dt, dev, "recon", True), _rows(x, B, K, dt, dev, "x", True)
    stream = _stream(val)
    if x is None and recon is None:
        recon = torch.empty(B, K, dtype=dt, device=dev)
        pr, ldr = _ptr(recon), K
    if x is not None and sq_err is None:
        sq_err = torch.empty(B, n, dtype=torch.float32, device=dev)
    check(lib().cc_decode_pairs(_ptr(val), _ptr(idx), B, k, pw, ldw, h, _ptr(b_dec), n, d, dtype_code(dt), pr, ldr,
                                px, ldx, _ptr(sq_err), stream))
    return recon, sq_err


# ---------------------------------------------------------------- the sparse decode's backward (pair gradients)
PAIRS_GRAD_SPLIT = 128  # CC_PAIRS_GRAD_SPLIT (include/crosscoder_hip.h)


def _pairs_idx(idx, val, name="val"):
    """(B, k) of idx [B, k] int32, contiguous; an optional val of the same shape, bf16 / fp32, contiguous, beside it"""
    if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1 or (val is not None and val.shape != idx.shape):
        raise ValueError(f"idx (and {name}) must be [rows >= 1, k >= 1], got {tuple(idx.shape)}"
                         + ("" if val is None else f" and {tuple(val.shape)}"))
    if idx.dtype != torch.int32:
        raise ValueError(f"idx must be int32, got {idx.dtype}")
    if val is not None and val.dtype not in _DT:
        raise ValueError(f"{name} must be bf16 or fp32, got {val.dtype}")
    if not idx.is_contiguous() or (val is not None and not val.is_contiguous()):
        raise ValueError(f"idx and {name} must be contiguous")
    if val is not None and val.device != idx.device:
        raise ValueError(f"{name} must be on {idx.device}")
    return idx.shape


def _pairs_val(val):
    """(B, k) of val [B, k], bf16 / fp32, contiguous"""
    if val.dim() != 2 or val.shape[0] < 1 or val.shape[1] < 1 or val.dtype not in _DT or not val.is_contiguous():
        raise ValueError(f"val must be a contiguous bf16 or fp32 [rows >= 1, k >= 1] tensor, got {val.dtype} "
                         f"{tuple(val.shape)}")
    return val.shape


def _grouped(perm, seg, dev):
    """(P, h) of the pairs grouped by latent: perm [P] int32, seg [h + 1] int64, contiguous on dev"""
    if perm.dtype != torch.int32 or perm.dim() != 1 or not perm.is_contiguous() or perm.device != dev:
        raise ValueError(f"perm must be a contiguous int32 vector on {dev}")
    if seg.dtype != torch.int64 or seg.dim() != 1 or seg.shape[0] < 2 or not seg.is_contiguous() or seg.device != dev:
        raise ValueError(f"seg must be a contiguous int64 vector of dict_size + 1 >= 2 elements on {dev}")
    return perm.shape[0], seg.shape[0] - 1


def pairs_by_latent(idx, h):
    """The pairs idx [B, k] (int32 or int64) grouped by latent -> (perm int32 [B k], seg int64 [h + 1]): the first seg[h]
    entries of perm are the flat slot numbers r * k + s of the valid pairs (0 <= idx < h) sorted by (latent, r, s), and
    latent j's are perm[seg[j] : seg[j + 1]]; the remaining entries (the invalid slots, in slot order) belong to no
    segment.  torch on idx's device, no host synchronisation: a sort of the unique int64 keys latent * (B k) + slot
    (an invalid slot counts as latent h), a count per latent and a cumsum.  Deterministic: the keys are distinct, so
    every sort gives one order, and the counts are integers."""
    if idx.dim() != 2 or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"idx must be an int32 or int64 [rows, k] tensor, got {idx.dtype} {tuple(idx.shape)}")
    _int_at_least(h, "h")
    Bk = idx.numel()
    if Bk > 2 ** 31 - 1:
        raise ValueError(f"rows * k must stay below 2^31, got {Bk}")
    lat = idx.reshape(-1).to(torch.int64)
    lat = torch.where((lat >= 0) & (lat < h), lat, torch.full_like(lat, h))
    keys = lat * Bk + torch.arange(Bk, dtype=torch.int64, device=idx.device)
    perm = (torch.sort(keys).values % max(Bk, 1)).to(torch.int32)
    count = torch.zeros(h + 1, dtype=torch.int64, device=idx.device).scatter_add_(0, lat, torch.ones_like(lat))
    seg = torch.zeros(h + 1, dtype=torch.int64, device=idx.device)
    torch.cumsum(count[:h], 0, out=seg[1:])
    return perm, seg


def pairs_grad_values(idx, W_dec, g, n, d, val=None, h=None, dot=None, total=None, want_dot=True, want_total=False):
    """The sampled dot products of g [B, >= n * d] with the decoder rows the pairs name (cc_pairs_grad_values): dot fp32
    [B, k, n], per slot and model  sum_c g[r, c] * W_dec[idx[r, s], c];  with val [B, k] (g's dtype) multiplied once in
    fp32 by val[r, s]: the pair's attribution.  total fp32 [B, k]: dot summed over the models in model order.  An
    output is computed when it is given or wanted (want_dot, want_total: it is then allocated), at least one of them.
    A slot whose index is outside [0, h) gives +0 (h defaults to W_dec's rows).  idx [B, k] int32, contiguous; W_dec
    [>= h, >= n * d] and g may be column slices of wider matrices.  -> (dot or None, total or None)."""
    B, k = _pairs_idx(idx, val)
    _int_at_least(n, "n")
    _mult8(d, "d")
    K, dt, dev = n * d, g.dtype, idx.device
    if dt not in _DT:
        raise ValueError(f"g must be bf16 or fp32, got {dt}")
    pg, ldg = _rows(g, B, K, dt, dev, "g")
    pw, ldw, h = _decoder(W_dec, K, dt, dev, h)
    if val is not None and val.dtype != dt:
        raise ValueError(f"val must have g's dtype {dt}, got {val.dtype}")
    _dense(dot, torch.float32, (B, k, n), dev, "dot")
    _dense(total, torch.float32, (B, k), dev, "total")
    if dot is None and total is None and not want_dot and not want_total:
        raise ValueError("at least one of dot and total is needed")
    stream = _stream(idx)
    if total is None and want_total:
        total = torch.empty(B, k, dtype=torch.float32, device=dev)
    if dot is None and want_dot:
        dot = torch.empty(B, k, n, dtype=torch.float32, device=dev)
    check(lib().cc_pairs_grad_values(_ptr(idx), _ptr(val), B, k, pw, ldw, h, pg, ldg, n, d, dtype_code(dt), _ptr(dot),
                                     _ptr(total), stream))
    return dot, total


def pairs_grad_decoder_ws_floats(P, K):
    return int(lib().cc_pairs_grad_decoder_ws_floats(P, K))


def pairs_grad_decoder(perm, seg, val, g, K, out=None, ws=None):
    """dW [h, K] (val's dtype) <- pairs^T . g from the pairs grouped by latent (pairs_by_latent; cc_pairs_grad_decoder):
    row j = sum over latent j's pairs, in perm's order, of val[r, s] * g[r, :K] -- one fp32 fma chain per element (a
    list longer than PAIRS_GRAD_SPLIT in pieces of that length, added in order), rounded once; a latent without pairs
    gets a row of +0.  val [B, k] contiguous, g [B, >= K] and out [h, >= K] of its dtype (column slices keep their
    pitch); ws: fp32, at least pairs_grad_decoder_ws_floats(len(perm), K) elements (allocated when None)."""
    B, k = _pairs_val(val)
    dt, dev = val.dtype, val.device
    P, h = _grouped(perm, seg, dev)
    _mult8(K, "K")
    pg, ldg = _rows(g, B, K, dt, dev, "g")
    po, ldo = _rows(out, h, K, dt, dev, "out", True)
    need = (P // PAIRS_GRAD_SPLIT) * K
    _scratch(ws, torch.float32, need, dev)
    stream = _stream(val)
    if out is None:
        out = torch.empty(h, K, dtype=dt, device=dev)
        po, ldo = _ptr(out), K
    if ws is None and need:
        ws = torch.empty(pairs_grad_decoder_ws_floats(P, K), dtype=torch.float32, device=dev)
    check(lib().cc_pairs_grad_decoder(_ptr(perm), P, _ptr(seg), h, _ptr(val), B, k, pg, ldg, K, dtype_code(dt), po, ldo,
                                      _ptr(ws), stream))
    return out


def pairs_latent_sums(a, perm, seg, sum, abs_sum, count):
    """The per-pair values a fp32 [B, k, n] folded into the per-latent state sum / abs_sum fp64 [h, n] and count int64
    [h], in place (cc_pairs_latent_sums): for latent j and its pairs in perm's order, plain fp64 adds of a, of |a|, and
    of 1."""
    if a.dim() != 3 or a.dtype != torch.float32 or not a.is_contiguous() or min(a.shape) < 1:
        raise ValueError(f"a must be a contiguous fp32 [rows, k, n] tensor, got {a.dtype} {tuple(a.shape)}")
    B, k, n = a.shape
    dev = a.device
    P, h = _grouped(perm, seg, dev)
    _dense(sum, torch.float64, (h, n), dev, "sum")
    _dense(abs_sum, torch.float64, (h, n), dev, "abs_sum")
    _dense(count, torch.int64, (h,), dev, "count")
    if sum is None or abs_sum is None or count is None:
        raise ValueError("sum, abs_sum and count are all needed")
    check(lib().cc_pairs_latent_sums(_ptr(a), B, k, n, _ptr(perm), P, _ptr(seg), h, _ptr(sum), _ptr(abs_sum),
                                     _ptr(count), _stream(a)))


# ---------------------------------------------------------------- the sparse TopK step's kernels (sparse_step.hip)
def pairs_group_ws_bytes(B, k, h):
    return int(lib().cc_pairs_group_ws_bytes(B, k, h))


def pairs_group(idx, h, perm=None, seg=None, ws=None):
    """pairs_by_latent as one kernel sequence in stream order (cc_pairs_group): idx [B, k] int32, contiguous -> (perm
    int32 [B k], seg int64 [h + 1]); seg and perm[:seg[h]] equal pairs_by_latent's, the rest of perm is unspecified
    inside [0, B k).  ws: uint8, at least pairs_group_ws_bytes(B, k, h) bytes, 16-byte aligned (allocated when None)."""
    B, k = _pairs_idx(idx, None)
    dev = idx.device
    _int_at_least(h, "h")
    _dense(perm, torch.int32, (B * k,), dev, "perm")
    _dense(seg, torch.int64, (h + 1,), dev, "seg")
    need = pairs_group_ws_bytes(B, k, h)
    if need == 0:
        raise ValueError(f"pairs_group: (rows, k, h) = ({B}, {k}, {h}) is out of the kernel's range")
    _scratch(ws, torch.uint8, need, dev)
    stream = _stream(idx)
    if perm is None:
        perm = torch.empty(B * k, dtype=torch.int32, device=dev)
    if seg is None:
        seg = torch.empty(h + 1, dtype=torch.int64, device=dev)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    check(lib().cc_pairs_group(_ptr(idx), B, k, h, _ptr(perm), _ptr(seg), _ptr(ws), stream))
    return perm, seg


def decode_pairs_partial(val, idx, W_dec, K, h=None, recon=None):
    """The fp32 partial reconstruction of k (value, latent) pairs per row (cc_decode_pairs_partial): recon fp32 [B, >= K]
    <- the fp32 fma chain +0 + sum_s val[r, s] * W_dec[idx[r, s], c] over the slots in order -- decode_pairs' chain
    without the bias and the rounding, what decode_partial hands to loss_fwd_bwd.  val [B, k] (bf16 / fp32) and idx
    int32, contiguous; W_dec [>= h, >= K] of val's dtype (column slices keep their pitch)."""
    B, k = _pairs_idx(idx, val)
    dt, dev = val.dtype, val.device
    _mult8(K, "K")
    pw, ldw, h = _decoder(W_dec, K, dt, dev, h)
    pr, ldr = _rows(recon, B, K, torch.float32, dev, "recon", True)
    stream = _stream(val)
    if recon is None:
        recon = torch.empty(B, K, dtype=torch.float32, device=dev)
        pr, ldr = _ptr(recon), K
    check(lib().cc_decode_pairs_partial(_ptr(val), _ptr(idx), B, k, pw, ldw, h, K, dtype_code(dt), pr, ldr, stream))
    return recon


def pairs_wgrad_ws_floats(P, K):
    return int(lib().cc_pairs_wgrad_ws_floats(P, K))


def pairs_wgrad_parts(h):
    return int(lib().cc_pairs_wgrad_parts(h))


def pairs_wgrad(perm, seg, val, g_pre, g_recon, x, K, dW_dec, dW_enc, db_enc, sq_dec, sq_enc, sq_b_enc, ws=None,
                add=None):
    """The sparse step's weight gradients from the pairs grouped by latent (cc_pairs_wgrad): per latent j and its list
    in perm's order, dW_dec[j] = sum val * g_recon[row], dW_enc[j] = sum p * x[row], db_enc[j] = sum p with p = g_pre
    rounded to the dtype -- pairs_grad_decoder's order for all three, rounded once -- plus the squared sums of the
    stored values, pairs_wgrad_parts(h) fp32 partials per parameter.  val [B, k] (bf16 / fp32) and g_pre fp32 [B, k],
    contiguous; g_recon, x [B, >= K] and dW_dec, dW_enc [h, >= K] of val's dtype (pitches kept); db_enc [h] of it; ws:
    fp32, at least pairs_wgrad_ws_floats(len(perm), K) elements (allocated when None).
    add (pairs_wgrad_add's (slot, aWd, aWe, ab)): the compact addends, through cc_pairs_wgrad_add."""
    B, k = _pairs_val(val)
    dt, dev = val.dtype, val.device
    P, h = _grouped(perm, seg, dev)
    _dense(g_pre, torch.float32, (B, k), dev, "g_pre")
    _mult8(K, "K")
    (pg, ldg), (px, ldx) = _rows(g_recon, B, K, dt, dev, "g_recon"), _rows(x, B, K, dt, dev, "x")
    (pd, ldd), (pe, lde) = _rows(dW_dec, h, K, dt, dev, "dW_dec"), _rows(dW_enc, h, K, dt, dev, "dW_enc")
    _dense(db_enc, dt, (h,), dev, "db_enc")
    parts = pairs_wgrad_parts(h)
    for name, t in (("sq_dec", sq_dec), ("sq_enc", sq_enc), ("sq_b_enc", sq_b_enc)):
        _dense(t, torch.float32, (parts,), dev, name)
    if g_pre is None or db_enc is None or sq_dec is None or sq_enc is None or sq_b_enc is None:
        raise ValueError("g_pre, db_enc and the three sq partials are all needed")
    need = (P // PAIRS_GRAD_SPLIT) * (2 * K + 8)
    _scratch(ws, torch.float32, need, dev)
    stream = _stream(val)
    if ws is None and need:
        ws = torch.empty(pairs_wgrad_ws_floats(P, K), dtype=torch.float32, device=dev)
    args = (_ptr(perm), P, _ptr(seg), h, _ptr(val), _ptr(g_pre), B, k, pg, ldg, px, ldx, K, dtype_code(dt), pd, ldd, pe,
            lde, _ptr(db_enc), _ptr(sq_dec), _ptr(sq_enc), _ptr(sq_b_enc), _ptr(ws))
    if add is None:
        check(lib().cc_pairs_wgrad(*args, stream))
        return
    slot, aWd, aWe, ab = add
    _dense(slot, torch.int32, (h,), dev, "slot")
    if slot is None or aWd is None or aWe is None or ab is None:
        raise ValueError("slot and the three addends are all needed")
    Dp = aWd.shape[0] if aWd.dim() == 2 else 0
    (pad, lad), (pae, lae) = _rows(aWd, Dp, K, dt, dev, "aWd"), _rows(aWe, Dp, K, dt, dev, "aWe")
    _dense(ab, dt, (Dp,), dev, "ab")
    check(lib().cc_pairs_wgrad_add(*args, _ptr(slot), Dp, pad, lad, pae, lae, _ptr(ab), stream))


def pairs_wgrad_add(perm, seg, val, g_pre, g_recon, x, K, dW_dec, dW_enc, db_enc, sq_dec, sq_enc, sq_b_enc, slot, aWd,
                    aWe, ab, ws=None):
    """pairs_wgrad with the compact addends of the AuxK loss's dead set (cc_pairs_wgrad_add): for a latent j with
    s = slot[j] >= 0 (int32 [h]; ops.dead_compact's), rows s of aWd, aWe [D_pad, >= K] and element s of ab [D_pad]
    (val's dtype) are added to the fp32 sums of dW_dec[j], dW_enc[j] and db_enc[j] before their one rounding.  The
    squared sums are those of the stored values."""
    pairs_wgrad(perm, seg, val, g_pre, g_recon, x, K, dW_dec, dW_enc, db_enc, sq_dec, sq_enc, sq_b_enc, ws=ws,
                add=(slot, aWd, aWe, ab))


# ---------------------------------------------------------------- BatchTopK (one selection over the whole batch)
def batch_topk_part_rows(B, h):
    return int(lib().cc_batch_topk_part_rows(B, h))


def batch_topk_l0_parts(B, h):
    return int(lib().cc_batch_topk_l0_parts(B, h))


def batch_topk_ws_bytes(B, h, dtype, weighted):
    return int(lib().cc_batch_topk_ws_bytes(B, h, dtype_code(dtype), int(bool(weighted))))


def _batch_topk_args(acts, h, weight, out, colsum_part, l0_part, row_count):
    B, ld = _rows_ld(acts, "acts")
    dev = acts.device
    _like(out, acts, "out", "acts")
    _dense(weight, torch.float32, (h,), dev, "weight")
    _dense(colsum_part, torch.float32, (batch_topk_part_rows(B, h), h), dev, "colsum_part")
    _dense(l0_part, torch.float32, (batch_topk_l0_parts(B, h),), dev, "l0_part")
    _dense(row_count, torch.int32, (B,), dev, "row_count")
    return B, ld


def batch_topk(acts, h, n_keep, weight=None, out=None, colsum_part=None, l0_part=None, row_count=None, info=None,
               ws=None, threshold=None, beta=0.0):
    """acts [B, ld >= h] (rows contiguous), first h columns, reduced to the n_keep best (row, latent) pairs of the
    whole batch under score = act * weight[latent] (weight fp32 [h]; None: the activation itself); ties: the
    smaller flat index row * h + latent first (cc_batch_topk).  out: the masked activations (may be `acts` itself:
    in place); colsum_part fp32 [batch_topk_part_rows(B, h), h] / l0_part fp32 [batch_topk_l0_parts(B, h)]:
    column-sum partials and selected counts of the masked activations; row_count int32 [B]: every row's selected
    count; info uint32-as-int32 [4]: (threshold score bits, selected, ties at the threshold admitted, eligible).
    ws: a uint8 tensor of at least batch_topk_ws_bytes(...) bytes (allocated when None).  threshold (an fp32 tensor
    of one element on the device) with beta in [0, 1): the running threshold the last selection launch folds T into
    (T itself while it is < 0).  Returns out."""
    B, ld = _batch_topk_args(acts, h, weight, out, colsum_part, l0_part, row_count)
    _int_at_least(n_keep, "n_keep")
    if out is None and info is None and row_count is None:
        raise ValueError("at least one of out, info and row_count is needed")
    dev = acts.device
    _dense(info, torch.int32, (4,), dev, "info")
    if threshold is not None and (threshold.dtype != torch.float32 or threshold.numel() != 1
                                  or threshold.device != dev or not 0 <= beta < 1):
        raise ValueError(f"threshold must be an fp32 tensor of one element on {dev}, beta a float in [0, 1)")
    need = batch_topk_ws_bytes(B, h, acts.dtype, weight is not None)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    if ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"ws must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    check(lib().cc_batch_topk(_ptr(acts), ld, B, h, dtype_code(acts.dtype), _ptr(weight), int(n_keep), _ptr(out),
                              _ptr(colsum_part), _ptr(l0_part), _ptr(row_count), _ptr(info), _ptr(threshold), float(beta), _ptr(ws), ws.numel(),
                              _stream(acts)))
    return out


def threshold_mask(acts, h, theta, weight=None, out=None, colsum_part=None, l0_part=None, row_count=None):
    """The inference form of batch_topk, one pass: keeps an element iff it is eligible and its score is >= theta
    (an fp32 tensor of one element on the device: never read on the host; cc_threshold_mask).  The same outputs
    without info."""
    B, ld = _batch_topk_args(acts, h, weight, out, colsum_part, l0_part, row_count)
    if out is None and row_count is None:
        raise ValueError("at least one of out and row_count is needed")
    if theta.dtype != torch.float32 or theta.numel() != 1 or theta.device != acts.device:
        raise ValueError(f"theta must be an fp32 tensor of one element on {acts.device}")
    check(lib().cc_threshold_mask(_ptr(acts), ld, B, h, dtype_code(acts.dtype), _ptr(weight), _ptr(theta), _ptr(out),
                                  _ptr(colsum_part), _ptr(l0_part), _ptr(row_count), _stream(acts)))
    return out


# ---------------------------------------------------------------- the AuxK dead-latent loss
def auxk_rows(acts, h, k_aux, since_fired, dead_after, out, row_count=None):
    """Each row of acts [B, ld >= h], first h columns, reduced to its k_aux largest positive values among the dead
    latents only (since_fired [>= h] int64 on the device; dead: since_fired >= dead_after), into `out` (acts' dtype,
    shape and strides, another buffer): topk_rows with a column predicate (cc_auxk_rows).  row_count int32 [B]:
    every row's selected count."""
    B, ld = _rows_ld(acts, "acts")
    dev = acts.device
    _like(out, acts, "out", "acts")
    if out.data_ptr() == acts.data_ptr():
        raise ValueError("out must not be acts")
    if since_fired.dtype != torch.int64 or since_fired.device != dev or since_fired.dim() != 1 \
            or since_fired.numel() < h or not since_fired.is_contiguous():
        raise ValueError(f"since_fired must be a contiguous int64 tensor of at least {h} elements on {dev}")
    _dense(row_count, torch.int32, (B,), dev, "row_count")
    check(lib().cc_auxk_rows(_ptr(acts), ld, B, h, dtype_code(acts.dtype), int(k_aux), _ptr(since_fired),
                             int(dead_after), _ptr(out), _ptr(row_count), _stream(acts)))
    return out


def dead_update(colsum_acts, since_fired, h_real, B, dead_after, count_out, was_dead=None, host_ptr=None):
    """since_fired [h] int64 <- 0 where colsum_acts [h] fp32 > 0, else + B; count_out (int32 [1]) = the latents
    below h_real that are dead (>= dead_after) under the new state; was_dead (uint8 [h], optional): the dead mask
    under the old state; host_ptr (optional): device address of a host-visible int32 word that also receives the
    count (cc_dead_update)."""
    h = colsum_acts.numel()
    dev = colsum_acts.device
    _dense(colsum_acts, torch.float32, (h,), dev, "colsum_acts")
    _dense(since_fired, torch.int64, (h,), dev, "since_fired")
    _dense(was_dead, torch.uint8, (h,), dev, "was_dead")
    if count_out.dtype != torch.int32 or count_out.numel() != 1 or count_out.device != dev:
        raise ValueError(f"count_out must be an int32 tensor of one element on {dev}")
    check(lib().cc_dead_update(_ptr(colsum_acts), _ptr(since_fired), h, int(h_real), int(B), int(dead_after),
                               _ptr(was_dead), _ptr(count_out), _vptr(host_ptr), _stream(colsum_acts)))


def auxk_part_floats(B, K):
    return int(lib().cc_auxk_part_floats(B, K))


def auxk_loss(recon_f32, b_dec, x, ehat_f32, g_aux, part, scalars, auxk_coeff, host_ptr=None):
    """The aux loss of ehat_f32 [B, K] (fp32, = aux_acts . W_dec) against e = x - (recon_f32 + b_dec), and
    g_aux [B, K] (x's dtype) = dtype(2 auxk_coeff / (B den) (ehat - e)) (cc_auxk_loss).  part: fp32
    [auxk_part_floats(B, K)]; scalars: fp32 [4] <- {auxk_loss, den, scale, valid}; host_ptr (optional): device address
    of a host-visible fp32 word that also receives auxk_loss."""
    B, K = x.shape
    dev = x.device
    for name, t, dt in (("recon_f32", recon_f32, torch.float32), ("x", x, x.dtype), ("ehat_f32", ehat_f32, torch.float32),
                        ("g_aux", g_aux, x.dtype)):
        if t.dtype != dt or tuple(t.shape) != (B, K) or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape ({B}, {K}) on {dev}")
    if b_dec.dtype != x.dtype or b_dec.numel() != K or not b_dec.is_contiguous():
        raise ValueError(f"b_dec must be a contiguous {x.dtype} tensor of {K} elements")
    if part.dtype != torch.float32 or part.numel() < auxk_part_floats(B, K) or not part.is_contiguous():
        raise ValueError(f"part must be a contiguous fp32 tensor of at least {auxk_part_floats(B, K)} elements")
    if scalars.dtype != torch.float32 or scalars.numel() < 4 or not scalars.is_contiguous():
        raise ValueError("scalars must be a contiguous fp32 tensor of at least 4 elements")
    check(lib().cc_auxk_loss(_ptr(recon_f32), _ptr(b_dec), _ptr(x), _ptr(ehat_f32), _ptr(g_aux), _ptr(part),
                             _ptr(scalars), _vptr(host_ptr), float(auxk_coeff), B, K, dtype_code(x.dtype), _stream(x)))


def add_rows(dst, src):
    """dst = dtype(float(dst) + float(src)) for two [rows, cols] views of the same dtype and row stride
    (cc_add_rows)."""
    rows, ld = _rows_ld(dst, "dst")
    _like(src, dst, "src", "dst")
    check(lib().cc_add_rows(_ptr(dst), _ptr(src), rows, dst.shape[1], ld, dtype_code(dst.dtype), _stream(dst)))


# ---------------------------------------------------------------- the compacted dead set (the sparse step's AuxK)
def dead_compact(since_fired, h_real, dead_after, ids, slot, count):
    """The dead latents of since_fired [h] (int64; dead: >= dead_after, latents >= h_real never) in ascending order
    (cc_dead_compact): ids int32 [D_pad] (D_pad a multiple of 8) <- the c-th dead latent, -1 from their number D on;
    slot int32 [h] <- every latent's compact index or -1; count (int32 [1]) <- D.  Dead latents from D_pad on are
    dropped."""
    h, dev = since_fired.numel(), since_fired.device
    _dense(since_fired, torch.int64, (h,), dev, "since_fired")
    _dense(slot, torch.int32, (h,), dev, "slot")
    if ids is None or ids.dtype != torch.int32 or ids.dim() != 1 or ids.device != dev or not ids.is_contiguous():
        raise ValueError(f"ids must be a contiguous int32 vector on {dev}")
    _mult8(ids.numel(), "len(ids)")
    if slot is None or count is None or count.dtype != torch.int32 or count.numel() != 1 or count.device != dev:
        raise ValueError(f"slot is needed, and count must be an int32 tensor of one element on {dev}")
    check(lib().cc_dead_compact(_ptr(since_fired), h, int(h_real), int(dead_after), _ptr(ids), ids.numel(), _ptr(slot),
                                _ptr(count), _stream(since_fired)))


def compact_gather(ids, h, W=None, Wc=None, acts=None, acts_c=None):
    """Bit copies through ids (int32 [D_pad], ops.dead_compact's) of latents below h (cc_compact_gather): rows,
    Wc[c] = W[ids[c]] for W [>= h, >= K] and Wc [D_pad, K]; columns, acts_c[r][c] = acts[r][ids[c]] for acts
    [B, >= h] (rows contiguous) and acts_c [B, D_pad] contiguous.  An ids[c] < 0 gives a +0 row / column.  Either
    pair may be left out."""
    dev = ids.device
    Dp = _mult8(ids.numel(), "len(ids)")
    if ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError("ids must be a contiguous int32 vector")
    if (W is None) != (Wc is None) or (acts is None) != (acts_c is None) or (W is None and acts is None):
        raise ValueError("W goes with Wc and acts with acts_c; one pair at least")
    _int_at_least(h, "h")
    pw = pc = pa = po = None
    ldw = ldc = K = lda = B = 0
    dt = (W if W is not None else acts).dtype
    if W is not None:
        K = _mult8(Wc.shape[1] if Wc.dim() == 2 else 0, "Wc's columns")
        pw, ldw, _ = _decoder(W, K, dt, dev, h)
        pc, ldc = _rows(Wc, Dp, K, dt, dev, "Wc")
    if acts is not None:
        B, lda = _rows_ld(acts, "acts")
        if acts.shape[1] < h or acts.device != dev:
            raise ValueError(f"acts must be [B, >= {h}] on {dev}")
        _dense(acts_c, dt, (B, Dp), dev, "acts_c")
        pa, po = _ptr(acts), _ptr(acts_c)
    check(lib().cc_compact_gather(_ptr(ids), Dp, h, pw, ldw, K, pc, ldc, pa, lda, B, po, dtype_code(dt), _stream(ids)))


# ---------------------------------------------------------------- JumpReLU (one learned threshold per latent)
CLIP_EMULATE_MIXED = 2  # clip_finalize / grad_tail's emulate_bf16 for four bf16 gradients followed by fp32 ones


def jumprelu_part_rows(B, h):
    return int(lib().cc_jumprelu_part_rows(B, h))


def jumprelu_l0_parts(B, h):
    return int(lib().cc_jumprelu_l0_parts(B, h))


def _jumprelu_args(a, h, theta, same, slabs):
    B, ld = _rows_ld(a, "acts")
    dev = a.device
    for name, t in same:
        _like(t, a, name, "acts")
    _dense(theta, torch.float32, (h,), dev, "theta")
    for name, t in slabs:
        _dense(t, torch.float32, (jumprelu_part_rows(B, h), h), dev, name)
    return B, ld


def jumprelu_mask(acts, h, theta, eps, out, gate=None, colsum_part=None, l0_part=None):
    """acts [B, ld >= h] (rows contiguous), first h columns, masked to the elements that are > 0 and > theta[latent]
    (theta fp32 [h]; strictly) into `out` (may be `acts` itself: in place); gate (optional, another buffer): the
    elements that are > 0 with a - theta > -eps / 2, which dacts_bwd masks with in a JumpReLU step; colsum_part fp32
    [jumprelu_part_rows(B, h), h] / l0_part fp32 [jumprelu_l0_parts(B, h)]: column-sum partials and counts of the
    kept elements (cc_jumprelu_mask).  Returns out."""
    B, ld = _jumprelu_args(acts, h, theta, (("out", out), ("gate", gate)), (("colsum_part", colsum_part),))
    if gate is not None and gate.data_ptr() == acts.data_ptr():
        raise ValueError("gate must not be acts")
    _dense(l0_part, torch.float32, (jumprelu_l0_parts(B, h),), acts.device, "l0_part")
    check(lib().cc_jumprelu_mask(_ptr(acts), ld, B, h, dtype_code(acts.dtype), _ptr(theta), float(eps), _ptr(out),
                                 _ptr(gate), _ptr(colsum_part), _ptr(l0_part), _stream(acts)))
    return out


def jumprelu_bwd(g_pre, gate, h, theta, eps, l0_scale, gpre_colsum_part=None, thr_part=None):
    """One pass over g_pre [B, ld >= h] (dacts_bwd's output under `gate`, in/out) and gate (jumprelu_mask's): thr_part
    fp32 [jumprelu_part_rows(B, h), h] <- partial sums over the window (gated, a - theta < eps / 2) of
    -(theta / eps) g_pre - l0_scale / eps; g_pre <- +0 where gated but not kept; gpre_colsum_part (same shape) <- the
    column-sum partials of the resulting g_pre (cc_jumprelu_bwd)."""
    B, ld = _jumprelu_args(g_pre, h, theta, (("gate", gate),),
                           (("gpre_colsum_part", gpre_colsum_part), ("thr_part", thr_part)))
    check(lib().cc_jumprelu_bwd(_ptr(g_pre), _ptr(gate), ld, B, h, dtype_code(g_pre.dtype), _ptr(theta), float(eps),
                                float(l0_scale), _ptr(gpre_colsum_part), _ptr(thr_part), _stream(g_pre)))


# ---------------------------------------------------------------- dead-latent resampling (resample.py)
def row_norms(W, out=None):
    """out fp32 [rows] <- the 2-norm of every row of W [rows, K] (bf16 / fp32, K % 8 == 0; a column slice of a wider
    matrix keeps its row pitch), one pass in a fixed order (cc_row_norms): no fp32 copy of W is made."""
    if W.dim() != 2 or W.shape[0] < 1:
        raise ValueError(f"W must be [rows >= 1, K], got {tuple(W.shape)}")
    rows, K = W.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=W.device)
    _dense(out, torch.float32, (rows,), W.device, "out")
    pw, ld = _pitched(W, K, "W")
    check(lib().cc_row_norms(pw, ld, rows, K, dtype_code(W.dtype), _ptr(out), _stream(W)))
    return out


def resample_pick(loss, u, cdf=None, rows_out=None):
    """rows_out int64 [J] <- for every uniform u[j] (fp64 in [0, 1)) a row of loss (fp32 [R]) drawn with probability
    proportional to loss^2 (fp64; a negative or non-finite loss never), with replacement: the smallest r whose
    inclusive prefix sum cdf[r] exceeds u[j] * cdf[R - 1] (cc_resample_pick).  cdf: fp64 [R] scratch that receives
    the prefix sums.  No row has weight: every entry is -1.  -> (rows_out, cdf)"""
    dev = loss.device
    if loss.dim() != 1 or loss.shape[0] < 1 or u.dim() != 1 or u.shape[0] < 1:
        raise ValueError(f"loss [R >= 1] and u [J >= 1] expected, got {tuple(loss.shape)} and {tuple(u.shape)}")
    R, J = loss.shape[0], u.shape[0]
    _dense(loss, torch.float32, (R,), dev, "loss")
    _dense(u, torch.float64, (J,), dev, "u")
    if cdf is None:
        cdf = torch.empty(R, dtype=torch.float64, device=dev)
    if rows_out is None:
        rows_out = torch.empty(J, dtype=torch.int64, device=dev)
    _dense(cdf, torch.float64, (R,), dev, "cdf")
    _dense(rows_out, torch.int64, (J,), dev, "rows_out")
    check(lib().cc_resample_pick(_ptr(loss), R, _ptr(u), J, _ptr(cdf), _ptr(rows_out), _stream(loss)))
    return rows_out, cdf


def resample_write(X, rows, latents, h, enc_norm, dec_norm, params, master=None, exp_avg=None, exp_avg_sq=None,
                   done=None):
    """Re-seed latent latents[j] from the pool row X[rows[j]] for every j (cc_resample_write): its W_dec row becomes
    x * dec_norm / ||x||, its W_enc row x * enc_norm / ||x||, its b_enc 0, in `params` (the flat arena
    [W_enc [h][K] | b_enc [h] | W_dec [h][K] | b_dec [K]] of X's dtype) and unrounded in `master` (fp32, the same
    layout); the latent's rows and b_enc entries of exp_avg / exp_avg_sq (one dtype, together) become 0.  X [R, K]
    (rows contiguous); rows, latents int64 [J], latents distinct and in [0, h) (the caller's check); a row index
    outside [0, R) or a source row of zeros leaves its latent untouched.  done (int32 [J], allocated if not given)
    says which were written.  -> done"""
    R, ldx = _rows_ld(X, "X")
    K, dev = X.shape[1], X.device
    numel = 2 * h * K + h + K
    J = rows.shape[0] if rows.dim() == 1 else -1
    if J < 1:
        raise ValueError(f"rows must be int64 [J >= 1], got {tuple(rows.shape)}")
    _dense(rows, torch.int64, (J,), dev, "rows")
    _dense(latents, torch.int64, (J,), dev, "latents")
    _dense(params, X.dtype, (numel,), dev, "params")
    _dense(master, torch.float32, (numel,), dev, "master")
    if (exp_avg is None) != (exp_avg_sq is None):
        raise ValueError("exp_avg and exp_avg_sq go together")
    sdt = CC_F32
    if exp_avg is not None:
        sdt = dtype_code(exp_avg.dtype)
        _dense(exp_avg, exp_avg.dtype, (numel,), dev, "exp_avg")
        _dense(exp_avg_sq, exp_avg.dtype, (numel,), dev, "exp_avg_sq")
    if done is None:
        done = torch.empty(J, dtype=torch.int32, device=dev)
    _dense(done, torch.int32, (J,), dev, "done")
    check(lib().cc_resample_write(_ptr(X), ldx, R, _ptr(rows), _ptr(latents), J, h, K, dtype_code(X.dtype),
                                  float(enc_norm), float(dec_norm), _ptr(params), _ptr(master), _ptr(exp_avg),
                                  _ptr(exp_avg_sq), sdt, _ptr(done), _stream(X)))
    return done
