"""fp64 references, error bounds and the comparator for the training-step kernels (cc_prep_input, cc_encode_fwd,
cc_decode_fwd, cc_loss_fwd_bwd, cc_loss_finalize, cc_dacts_bwd, cc_wgrad_dec, cc_wgrad_enc, cc_dec_norms,
cc_reduce_rows, cc_clip_finalize, cc_gemm_f32out).

Every function takes the tensors actually handed to the kernel (any dtype, any device), upcasts their bits to fp64 on
the CPU and returns the fp64 result with, per output element, the magnitude sum A its error bound scales with: the sum
of the absolute values of the terms the kernel adds up for that element.  Only torch is imported.

The bounds are derived, not measured.

acc_bound(L, A) = (L + 16) 2^-23 A.  An fp32 accumulation of L terms in any order (sequential, pairwise, MFMA blocks,
lane butterflies) errs by at most L 2^-24 A to first order (each of at most L - 1 additions rounds a partial sum of
magnitude <= A by 2^-24 relative).  The factor 2 covers the rounding of the L products themselves where the operands
are fp32 (bf16 products are exact in fp32) and the second-order terms; the + 16 covers the few epilogue operations (a
bias add, a scale, the L1 term's multiplies, a square root) and the (1 + 2^-8) by which a following bf16 rounding
stretches the accumulated error.  L is the contraction length; for a column sum it is the number of rows summed.

store_bound(v64, dtype) = 2^-8 |v64| for bf16 -- one rounding to nearest even of an 8-bit significand is off by at
most half an ulp, and an ulp is at most 2^-7 of the value -- and 0 for fp32 (the accumulator is stored as it is).

An output passes when |ours - v64| <= acc_bound + store_bound.  |relu(a) - relu(b)| <= |a - b|, so activations are
checked against relu(pre64) under the pre-activation's bound with no guard band.  An indexing error, a dropped term,
a wrong mask or a wrong scale is of order A: 2^8 to 2^20 times these bounds.

Reference lines (mitroitskii/crosscoder-model-diff-replication): each function names what it restates, as
include/crosscoder_hip.h does."""
import torch

EPS23 = 2.0 ** -23


def f64(t):
    """The bits of t as fp64 on the CPU."""
    return t.detach().to("cpu").to(torch.float64)


def round_dt(v64, dtype):
    """fp64 -> dtype as the kernels store: through fp32 (the accumulator), then to nearest even.  fp64: as it is."""
    if dtype == torch.float64:
        return v64
    return v64.to(torch.float32).to(dtype)


def acc_bound(L, A):
    return (L + 16) * EPS23 * A


def store_bound(v64, dtype):
    return v64.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else torch.zeros_like(v64)


def check(ours, v64, bound, name):
    """Asserts |ours - v64| <= bound element-wise (a NaN fails); the message names the worst element.  Returns
    max(err / bound) over the elements with a non-zero bound (0.0 if there is none)."""
    ours = f64(ours)
    v64 = f64(v64) if torch.is_tensor(v64) else torch.tensor(float(v64), dtype=torch.float64)
    bound = f64(bound) if torch.is_tensor(bound) else torch.tensor(float(bound), dtype=torch.float64)
    assert ours.shape == v64.shape, f"{name}: shape {tuple(ours.shape)} against {tuple(v64.shape)}"
    bound = bound.expand_as(v64)
    err = (ours - v64).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    bad = ~(err <= bound)
    if bool(bad.any()):
        excess = torch.where(bad, torch.where(err.isnan(), torch.full_like(err, float("inf")), err - bound),
                             torch.full_like(err, -1.0))
        flat = int(excess.argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), err.shape)) if err.dim() else ()
        raise AssertionError(
            f"{name}: {int(bad.sum())} of {err.numel()} elements out of bound; worst at {idx}: ours "
            f"{ours.reshape(-1)[flat].item():.9g}, fp64 {v64.reshape(-1)[flat].item():.9g}, err "
            f"{err.reshape(-1)[flat].item():.3e}, bound {bound.reshape(-1)[flat].item():.3e}")
    return float(ratio.max()) if ratio.numel() else 0.0


# ----------------------------------------------------------------------------- the forward
def prep(x_in, factor, dtype):
    """buffer.py:115-124 + crosscoder.py:99: x[b, m d + j] = round_dt(float(x_in[b, m, j]) * float(factor[m])),
    factor None = 1.  The product of two fp32 values is exact in fp64, so the one rounding to fp32 is the fp32
    multiply's: x is bit-exact.  -> (x [B, n d] in dtype, its fp64 column sums [n d], A = sum_b |x|)."""
    B, n, d = x_in.shape
    v = f64(x_in)
    if factor is not None:
        v = v * f64(factor)[None, :, None]
    x = round_dt(v, dtype).reshape(B, n * d)
    return x, f64(x).sum(0), f64(x).abs().sum(0)


def encode(x, W_enc_hk, b_enc):
    """crosscoder.py:69-80 before the ReLU: pre64 [B, h] = x W_enc^T + b_enc (W_enc h-major [h, K]);
    A = sum_k |x| |W| + |b|."""
    x, W, b = f64(x), f64(W_enc_hk), f64(b_enc)
    return x @ W.t() + b, x.abs() @ W.abs().t() + b.abs()


def decode(acts, W_dec_hk, b_dec=None):
    """crosscoder.py:82-89: recon64 [B, K] = acts W_dec (+ b_dec); A = sum_h |acts| |W| (+ |b|)."""
    a, W = f64(acts), f64(W_dec_hk)
    r, A = a @ W, a.abs() @ W.abs()
    if b_dec is not None:
        r, A = r + f64(b_dec), A + f64(b_dec).abs()
    return r, A


def loss(recon_f32, b_dec, x, x_mean, grad_scale, n, d, dtype):
    """crosscoder.py:104-121 and the autograd of :104-106.  With r = recon + b_dec (b_dec None = 0):
      g64 [B, K] = grad_scale (r - x),  Ag = grad_scale (|recon| + |b_dec| + |x|)
      l2 [B, n]  = sum_j (r - x)^2 per (row, model),  A_l2 = sum_j (|recon| + |b_dec| + |x|)^2
      tv [B, n]  = sum_j (x - x_mean)^2,              A_tv = sum_j (|x| + |x_mean|)^2
      colsum [K] = the column sums of round_dt(g64, dtype) (the b_dec gradient),  A_colsum = sum_b |round_dt(g64)|.
    The magnitudes carry the operands of the subtraction, so the bounds hold where recon is close to x."""
    r0, xx, mu = f64(recon_f32), f64(x), f64(x_mean)
    b = f64(b_dec) if b_dec is not None else torch.zeros_like(mu)
    B = xx.shape[0]
    diff = (r0 + b) - xx
    mag = r0.abs() + b.abs() + xx.abs()
    g = grad_scale * diff
    gr = f64(round_dt(g, dtype))
    per = lambda t: t.reshape(B, n, d).sum(-1)  # noqa: E731
    return {"g": g, "Ag": abs(grad_scale) * mag, "l2": per(diff * diff), "A_l2": per(mag * mag),
            "tv": per((xx - mu) ** 2), "A_tv": per((xx.abs() + mu.abs()) ** 2), "colsum": gr.sum(0),
            "A_colsum": gr.abs().sum(0)}


def loss_scalars(l2_rm, tv_rm, B_l1, active, B):
    """crosscoder.py:106-128, trainer.py:51-61 (oracle.cpu_reference.get_losses) from the per-(row, model) sums
    l2_rm / tv_rm [B, n], B * l1_loss and the active count: l2, l1, l0, ev [B], ev_a / ev_b [B] (models 0 and 1 as
    get_losses indexes them, whatever n is; ev_b = 0 for a single model, where the reference has nothing to index)
    and their means."""
    l2_rm, tv_rm = f64(l2_rm), f64(tv_rm)
    eps = 1e-8
    l2_row = l2_rm.sum(1)
    ev = 1 - l2_row / (tv_rm.sum(1) + eps)
    ev_a = 1 - l2_rm[:, 0] / (tv_rm[:, 0] + eps)
    ev_b = 1 - l2_rm[:, 1] / (tv_rm[:, 1] + eps) if l2_rm.shape[1] > 1 else torch.zeros_like(ev)
    return {"l2": l2_row.sum() / B, "l1": float(B_l1) / B, "l0": float(active) / B, "ev": ev, "ev_a": ev_a,
            "ev_b": ev_b, "mean_ev": ev.sum() / B, "mean_ev_a": ev_a.sum() / B, "mean_ev_b": ev_b.sum() / B}


# ----------------------------------------------------------------------------- the backward
def dacts(g_recon, W_dec_hk, acts, tn, l1_scale):
    """Autograd of crosscoder.py:77,84-89,126: g_pre64 [B, h] = (g_recon W_dec^T + l1_scale tn) * (acts > 0);
    A = sum_k |g| |W| + |l1_scale tn| (unmasked: the bound of an element the mask must have zeroed)."""
    g, W, t = f64(g_recon), f64(W_dec_hk), f64(tn)
    full = g @ W.t() + l1_scale * t
    return full * (f64(acts) > 0), g.abs() @ W.abs().t() + abs(l1_scale) * t.abs()


def wgrad_dec(acts, g_recon, W_dec_hk, inv_norms, colsum_acts, l1_scale, n, d):
    """Autograd of crosscoder.py:84-89 and :123-126: grad64 [h, K] = acts^T g_recon + l1_scale colsum_acts[h]
    W_dec[h, m, :] inv_norms[h, m], with the GIVEN inv_norms (0 where the norm is 0: the norm backward's masked
    value), so the L1 term is 0 there; A = |acts|^T |g| + |the L1 term|.  Also returns the L1 term."""
    a, g, W = f64(acts), f64(g_recon), f64(W_dec_hk)
    h = W.shape[0]
    l1 = l1_scale * f64(colsum_acts)[:, None] * (W.reshape(h, n, d) * f64(inv_norms).reshape(h, n, 1)).reshape(h, n * d)
    return a.t() @ g + l1, a.abs().t() @ g.abs() + l1.abs(), l1


def wgrad_enc(g_pre, x):
    """Autograd of crosscoder.py:69-76: grad64 [h, K] = g_pre^T x (W_enc's h-major layout); A = |g_pre|^T |x|."""
    g, xx = f64(g_pre), f64(x)
    return g.t() @ xx, g.abs().t() @ xx.abs()


def dec_norms(W_dec_hk, n, d):
    """crosscoder.py:123-125: norms [h, n] = ||W_dec[h, m, :]||, totals [h] = sum_m, inverse norms [h, n] with 0
    where the norm is 0."""
    W = f64(W_dec_hk)
    norms = W.reshape(W.shape[0], n, d).pow(2).sum(-1).sqrt()
    inv = torch.where(norms > 0, 1.0 / norms.clamp(min=1e-300), torch.zeros_like(norms))
    return norms, norms.sum(1), inv


def colsum(v):
    """Column sums of v [rows, C] and their magnitude sums."""
    v = f64(v)
    return v.sum(0), v.abs().sum(0)


def clip(sq_sums, max_norm):
    """torch/nn/utils/clip_grad.py in fp64 (the fp32 mode's reference): per-parameter norms from their squared sums,
    total = the norm of the norms, coef = min(1, max_norm / (total + 1e-6)) -> (total, coef, norms)."""
    norms = torch.tensor([float(s) for s in sq_sums], dtype=torch.float64).sqrt()
    total = norms.pow(2).sum().sqrt()
    return float(total), min(1.0, max_norm / (float(total) + 1e-6)), norms
