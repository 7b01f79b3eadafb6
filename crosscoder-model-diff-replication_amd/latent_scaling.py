"""Latent Scaling (Minder et al. 2025, "Robustly identifying concepts introduced during chat fine-tuning using
crosscoders"): per latent and model, the closed-form least-squares scale at which the latent's activation times
its decoder direction explains that model's reconstruction error, and that model's reconstruction.

The relative decoder norm (analysis.decoder_stats) calls a latent "chat-only" when one model's decoder vector is
near zero; L1 shrinkage produces that picture even for latents that explain both models equally well.  The ratios
nu_err / nu_rec of the fitted scales between the models tell the two apart.

Per batch of rows x [B, n, d], in the crosscoder's dtype T, with r = decoder_model:
    f = cc.encode(x)                          the crosscoder's own activations (as LatentStats.update obtains them)
    R = cc.decode(f)                          the reconstruction with b_dec, rounded to T
    E = T(float(x) - float(R))                one fp32 subtraction, rounded once
accumulated over the stream in fp64 (each batch's fp32 sums added), per latent j and model m:
    S_err[m][j] = sum_i f_ij (W_dec[j, r] . E_i^m)     S_rec[m][j] = sum_i f_ij (W_dec[j, r] . R_i^m)
    Q[j] = sum_i f_ij^2
Each S is one GEMM whose [B, h] product is never stored (cc_latent_scaling: the epilogue multiplies the accumulator
by the activation tile and keeps only its column sums); Q comes out of one of those launches.  result() adds, from
the weights alone, G[m][j] = W_dec[j, r] . W_dec[j, m] and the leave-one-out scales (`betas`).

    ls = LatentScaling(cc)                    # decoder direction: the last model (chat in [base, chat])
    for x in batches:                         # [rows, n_models, d_in], as cc.encode takes it
        ls.update(x)
    r = ls.result()                           # r["nu_err"], r["nu_rec"], r["beta_err"], ...
"""
import torch

from . import ops

CHUNK_ROWS = 4096


def betas(S_err, S_rec, Q, G, decoder_model):
    """The leave-one-out least-squares scales from the accumulators (S_err, S_rec, G [n, h]; Q [h]; any device,
    computed in fp64).  With r = decoder_model and latent j's own contribution removed from each target,
        error target E^m + f_j W_dec[j, m]:            beta_err[m] = (S_err[m] + Q G[m]) / (Q G[r])
        reconstruction target R^m - f_j W_dec[j, m]:   beta_rec[m] = (S_rec[m] - Q G[m]) / (Q G[r])
        nu_err[m] = beta_err[m] / beta_err[r],   nu_rec[m] = beta_rec[m] / beta_rec[r].
    NaN where the latent never fired (Q = 0) or G[r] = 0.  -> (beta_err, beta_rec, nu_err, nu_rec), each [n, h]."""
    S_err, S_rec, Q, G = (torch.as_tensor(t).to(torch.float64) for t in (S_err, S_rec, Q, G))
    n = G.shape[0]
    r = decoder_model + n if decoder_model < 0 else decoder_model
    if not 0 <= r < n:
        raise ValueError(f"decoder_model must name one of the {n} models, got {decoder_model}")
    den = Q * G[r]
    ok = (Q > 0) & (G[r] != 0)
    den = torch.where(ok, den, torch.full_like(den, float("nan")))
    beta_err = (S_err + Q * G) / den
    beta_rec = (S_rec - Q * G) / den
    return beta_err, beta_rec, beta_err / beta_err[r], beta_rec / beta_rec[r]


class LatentScaling:
    def __init__(self, cc, decoder_model=-1, chunk_rows=CHUNK_ROWS):
        n = cc.n_models
        if isinstance(decoder_model, bool) or not isinstance(decoder_model, int) or not -n <= decoder_model < n:
            raise ValueError(f"decoder_model must be an int in {-n}..{n - 1}, got {decoder_model!r}")
        if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1:
            raise ValueError(f"chunk_rows must be an int >= 1, got {chunk_rows!r}")
        self.cc = cc
        self.decoder_model = decoder_model % n
        self.chunk_rows = chunk_rows
        self._buf = None  # update()'s reused buffers (acts, R, E) for chunk_rows rows
        self._slab = None  # the launches' partial slabs and their reduced rows, for one chunk size
        self.reset()

    def reset(self):
        """Forget everything seen so far (fresh state on the crosscoder's current device)."""
        cc = self.cc
        dev = cc.arena().data.device
        self.rows_seen = 0
        # rows 0..n-1: S_err, n..2n-1: S_rec, 2n: Q (fp64, over the kernel's h)
        self._state = torch.zeros(2 * cc.n_models + 1, cc._hp, dtype=torch.float64, device=dev)

    def _slabs(self, rows, dev):
        R = ops.col_part_rows(rows)
        s = self._slab
        if s is None or s[0].shape[1] != R or s[0].device != dev:
            k = 2 * self.cc.n_models + 1
            s = self._slab = (torch.empty(k, R, self.cc._hp, dtype=torch.float32, device=dev),
                              torch.empty(k, self.cc._hp, dtype=torch.float32, device=dev))
        return s

    def update_from_parts(self, acts, err, rec):
        """The kernel path without encode / decode: acts [rows, >= kernel h], err / rec [rows, n * kernel d], device
        tensors in the crosscoder's dtype with contiguous rows (the kernel dims are dict_size / d_in rounded up to
        multiples of 8, engine.padded_dims).  2 n cc_latent_scaling launches (the first also gives Q), their
        reductions, and the fp64 accumulation."""
        cc = self.cc
        a = cc.arena()
        a.wait_pending()
        n, dp, hp = cc.n_models, cc._dp, cc._hp
        dev = self._state.device
        rows = acts.shape[0]
        if acts.dim() != 2 or acts.shape[1] < hp:
            raise ValueError(f"expected acts of shape [rows, >= {hp}], got {tuple(acts.shape)}")
        for name, t in (("err", err), ("rec", rec)):
            if t.dim() != 2 or tuple(t.shape) != (rows, n * dp):
                raise ValueError(f"expected {name} of shape [{rows}, {n * dp}], got {tuple(t.shape)}")
        for name, t in (("acts", acts), ("err", err), ("rec", rec)):
            if t.dtype != cc.dtype or t.device != dev:
                raise ValueError(f"{name} must be a {cc.dtype} tensor on {dev}")
        if rows == 0:
            return
        part, red = self._slabs(rows, dev)
        R = part.shape[1]
        r = self.decoder_model
        W = a.W_dec_hk[:, r * dp:(r + 1) * dp]
        for t, Y in enumerate((err, rec)):
            for m in range(n):
                k = t * n + m
                ops.latent_scaling(Y[:, m * dp:(m + 1) * dp], W, acts, part[k], part[2 * n] if k == 0 else None)
        for k in range(2 * n + 1):
            ops.reduce_rows(part[k], R, hp, out_f32=red[k])
        self._state += red
        self.rows_seen += rows

    def update(self, x):
        """x [rows, n_models, d_in] as CrossCoder.encode takes it, any row count, chunk_rows at a time."""
        cc = self.cc
        cc._check_x(x)
        a = cc.arena()
        a.wait_pending()
        dev, rows = a.data.device, x.shape[0]
        b = self._buf
        if b is None or b[0].device != dev or b[0].dtype != cc.dtype:
            K = cc.n_models * cc._dp
            b = self._buf = (torch.empty(self.chunk_rows, cc._hp, dtype=cc.dtype, device=dev),
                             torch.empty(self.chunk_rows, K, dtype=cc.dtype, device=dev),
                             torch.empty(self.chunk_rows, K, dtype=cc.dtype, device=dev))
        for r0 in range(0, rows, self.chunk_rows):
            r1 = min(rows, r0 + self.chunk_rows)
            acts, rec, err = (t[:r1 - r0] for t in b)
            xf = cc._flat_x(x[r0:r1])
            ops.encode_fwd(xf, a.W_enc_hk, a.b_enc, acts, True)
            cc.activate_(acts)  # the crosscoder's own activations, as cc.encode gives them for these rows
            ops.decode_fwd(acts, a.W_dec_hk, a.b_dec_flat, recon_t=rec)
            # E = T(float(x) - float(R)): torch subtracts two T values in fp32 and rounds once
            torch.sub(xf, rec, out=err)
            self.update_from_parts(acts, err, rec)

    def _gram(self):
        """G [n, kernel h] fp64: G[m][j] = W_dec[j, r] . W_dec[j, m], one pass over W_dec."""
        a = self.cc.arena()
        a.wait_pending()
        W = a.W_dec_hk.view(a.h, a.n, a.d).to(torch.float64)
        return torch.einsum("hd,hmd->mh", W[:, self.decoder_model], W)

    def result(self):
        """dict of tensors over the reference's dict_size latents (padding latents dropped): beta_err, beta_rec,
        nu_err, nu_rec [n, h] (fp64; NaN where the latent never fired or G[r] = 0), the raw accumulators S_err,
        S_rec, G [n, h] and Q [h] (fp64), fired [h] (bool) and rows_seen."""
        h, n = self.cc.d_hidden, self.cc.n_models
        st = self._state[:, :h]
        S_err, S_rec, Q = st[:n].clone(), st[n:2 * n].clone(), st[2 * n].clone()
        G = self._gram()[:, :h].contiguous()
        beta_err, beta_rec, nu_err, nu_rec = betas(S_err, S_rec, Q, G, self.decoder_model)
        return {"beta_err": beta_err, "beta_rec": beta_rec, "nu_err": nu_err, "nu_rec": nu_rec, "S_err": S_err,
                "S_rec": S_rec, "Q": Q, "G": G, "fired": Q > 0, "rows_seen": self.rows_seen}
