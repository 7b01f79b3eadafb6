"""fp64 references for latent scaling (crosscoder_amd.LatentScaling, cc_latent_scaling).

`accumulators` restates what one cc_latent_scaling launch sums, from the operands' own bits upcast to fp64, with
the magnitude sum A that the tests' error bound is stated in.  `brute_force_betas` builds every leave-one-out
target explicitly and solves the one-unknown least squares with torch.linalg.lstsq: it shares no formula with
latent_scaling.betas."""
import torch

EPS24 = 2.0 ** -24


def accumulators(acts, Y, W):
    """acts [B, >= h], Y [B, d], W [h, d] (any dtype; their bits upcast) ->
    S64[j] = sum_i f_ij (W_j . Y_i),  A[j] = sum_i |f_ij| sum_k |W_jk| |Y_ik|,  Q64[j] = sum_i f_ij^2."""
    W, Y = W.double(), Y.double()
    f = acts[:, :W.shape[0]].double()
    S = (f * (Y @ W.t())).sum(0)
    A = (f.abs() * (Y.abs() @ W.abs().t())).sum(0)
    return S, A, (f * f).sum(0)


def s_bound(B, d, A):
    """|S - S64| allowed for one launch over B rows: any order of at most d + B fp32 operations over exact products
    errs by (d + B) 2^-24 A to first order; twice that (second-order terms, the MFMA's internal accumulation,
    fp32 operands' product roundings), plus 8 ulp of slack."""
    return (d + B + 8) * 2 * EPS24 * A


def q_bound(B, Q64):
    return (B + 2) * 2 * EPS24 * Q64


def brute_force_betas(f, E, R, W_dec, decoder_model):
    """f [rows, h], E / R [rows, n, d], W_dec [h, n, d] (fp64) -> (beta_err, beta_rec) [n, h]: for every latent j
    and model m, the scalar beta minimising || beta f_j W_dec[j, r] - target ||_F over the rows, with the targets
    E^m + f_j W_dec[j, m] and R^m - f_j W_dec[j, m] built explicitly.  NaN where the regressor is all zero."""
    rows, h = f.shape
    n = W_dec.shape[1]
    r = decoder_model % n
    out = torch.full((2, n, h), float("nan"), dtype=torch.float64)
    for j in range(h):
        X = (f[:, j, None] * W_dec[j, r][None, :]).reshape(-1, 1)  # the regressor, rows * d stacked
        if not bool((X != 0).any()):
            continue
        for m in range(n):
            own = f[:, j, None] * W_dec[j, m][None, :]
            for t, target in enumerate((E[:, m] + own, R[:, m] - own)):
                out[t, m, j] = torch.linalg.lstsq(X, target.reshape(-1, 1)).solution[0, 0]
    return out[0], out[1]
