"""The reference for the AuxK dead-latent loss (pure torch, runs on the CPU).

Dead latents: tokens_since_fired >= dead_after.  Aux activations: per row the k_aux largest eligible activations
among the dead latents only, in cc_topk_rows' order -- topk_ref(where(dead, v, 0), k_aux).  Aux loss: with e = x - r
(detached) and e^ = aux_acts . W_dec (no bias), (1/B) sum (e^ - e)^2 over (1/B) sum (e - mean_b e)^2, and 0 when the
denominator is 0 or the quotient is not finite.
"""
import torch

from tests._topk_ref import topk_ref


def aux_select(v, dead, k_aux):
    """v [B, h], dead [h] bool -> topk_ref's dict for the dead columns only."""
    return topk_ref(torch.where(dead[None, :], v, torch.zeros((), dtype=v.dtype)), k_aux)


def aux_select_brute(rows, dead, k_aux):
    """The same by a plain Python loop: per row the selected indices, ascending."""
    out = []
    for row in rows:
        cand = [(x, i) for i, x in enumerate(row) if dead[i] and x > 0]
        chosen = []
        while cand and len(chosen) < k_aux:
            best = cand[0]
            for x, i in cand[1:]:
                if x > best[0] or (x == best[0] and i < best[1]):
                    best = (x, i)
            cand.remove(best)
            chosen.append(best[1])
        out.append(sorted(chosen))
    return out


def dead_update_ref(colsum, since_fired, B, dead_after, h_real):
    """-> (new since_fired, dead count among the first h_real latents under the new state, the old dead mask)."""
    fired = colsum > 0
    new = torch.where(fired, torch.zeros_like(since_fired), since_fired + B)
    return new, int((new[:h_real] >= dead_after).sum()), since_fired >= dead_after


def auxk_loss_ref(e, ehat):
    """e, ehat [B, K] (any float dtype; e carries no gradient) -> (auxk_loss, den, valid) as 0-dim tensors / bool."""
    B = e.shape[0]
    e = e.detach()
    num = (ehat - e).pow(2).sum() / B
    den = (e - e.mean(0)).pow(2).sum() / B
    loss = num / den
    valid = bool(den > 0) and bool(torch.isfinite(loss))
    return (loss if valid else torch.zeros((), dtype=e.dtype)), den, valid


def g_aux_ref(e, ehat, auxk_coeff, dtype):
    """d(auxk_coeff * auxk_loss)/d e^ rounded to dtype: dtype(2 auxk_coeff / (B den) (e^ - e)), +0 when forced."""
    _, den, valid = auxk_loss_ref(e, ehat)
    if not valid:
        return torch.zeros(e.shape, dtype=dtype)
    return (2.0 * auxk_coeff / (e.shape[0] * den) * (ehat - e)).to(dtype)


def step_loss_ref(x, P, M, A, l1_coeff, auxk_coeff):
    """The step's objective with the two masks imposed, in the dtype of x and P (leaves for autograd):
    acts = relu(pre) * M, aux_acts = relu(pre) * A; l2 + l1_coeff * l1 + auxk_coeff * auxk_loss.
    -> (total, {"l2_loss", "l1_loss", "auxk_loss"})."""
    B = x.shape[0]
    dt = x.dtype
    pre = torch.einsum("bnd,ndh->bh", x, P["W_enc"]) + P["b_enc"]
    relu = torch.relu(pre)
    acts = relu * M.to(dt)
    recon = torch.einsum("bh,hnd->bnd", acts, P["W_dec"]) + P["b_dec"]
    l2 = (recon.float() - x.float()).pow(2).sum(dim=(1, 2)).mean() if dt != torch.float64 else \
        (recon - x).pow(2).sum(dim=(1, 2)).mean()
    tn = P["W_dec"].norm(dim=-1).sum(dim=1)
    l1 = (acts * tn[None, :]).sum(-1).mean(0)
    wide = torch.float64 if dt == torch.float64 else torch.float32
    e = (x.to(wide) - recon.to(wide)).detach().reshape(B, -1)
    ehat = torch.einsum("bh,hnd->bnd", relu * A.to(dt), P["W_dec"]).to(wide).reshape(B, -1)
    auxk, _, _ = auxk_loss_ref(e, ehat)
    total = l2 + l1_coeff * l1 + auxk_coeff * auxk
    return total, {"l2_loss": l2, "l1_loss": l1, "auxk_loss": auxk}
