"""Latent ablation over a token stream: how much each model's reconstruction loses when a group of latents is
switched off (the intervention that follows the model-diffing analyses: decoder-norm statistics, LatentScaling,
match_decoders and LatentStats say which latents are model-specific; this measures what they carry).

`LatentAblation(cc, groups, k)` encodes each batch once into k (value, latent) pairs per row
(CrossCoder.encode_pairs) and measures, per model, the squared reconstruction error of the unedited pairs (the
baseline) and of the pairs with each group's values set to zero (CrossCoder.pairs_sq_err: the sparse decode, which
gathers k decoder rows per token).  No dense [rows, dict_size] activation matrix and no reconstruction is stored,
whatever the number of groups.

    ab = LatentAblation(cc, {"chat_only": chat_mask, "shared": shared_idx}, k=128)
    for x in batches:            # [rows, n_models, d_in], as cc.encode takes it
        ab.update(x)
    r = ab.result()              # r["chat_only"]["delta_mse"], r["baseline"]["explained_variance"], r["full_rows"]

The numbers are those of the k-pair form: exact for the rows with at most k non-zero activations; `full_rows`
counts the rows that use all k slots and may have been truncated to their k largest.
"""
import torch

RESERVED = ("baseline", "rows", "full_rows")
EPS = 1e-8  # the reference's guard of the explained-variance quotient (crosscoder.py:110)


def _group_mask(name, g, h, dev):
    """a group -- a bool mask [dict_size] or a tensor / sequence of latent indices -- as a bool mask on dev"""
    g = torch.as_tensor(g)
    if g.dtype == torch.bool:
        if g.dim() != 1 or g.shape[0] != h:
            raise ValueError(f"group {name!r}: a bool mask must have shape [{h}] (dict_size), got {tuple(g.shape)}")
        return g.to(dev).clone()
    if g.dtype not in (torch.int32, torch.int64) and g.numel():
        raise ValueError(f"group {name!r}: expected a bool mask or int32 / int64 latent indices, got {g.dtype}")
    if g.dim() != 1:
        raise ValueError(f"group {name!r}: latent indices must be one-dimensional, got shape {tuple(g.shape)}")
    g = g.to(torch.int64)
    if g.numel() and not (0 <= int(g.min()) and int(g.max()) < h):
        raise ValueError(f"group {name!r}: latent indices must lie in 0..{h - 1}")
    mask = torch.zeros(h, dtype=torch.bool, device=dev)
    mask[g.to(dev)] = True
    return mask


class LatentAblation:
    def __init__(self, cc, groups, k=None):
        k = cc.k if k is None else k
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= cc.d_hidden:
            raise ValueError(f"k must be an int in 1..dict_size ({cc.d_hidden}), got {k!r} (pairs kept per row; a "
                             "crosscoder whose cfg has no 'k' needs one)")
        if not isinstance(groups, dict):
            raise ValueError("groups must be a dict: name -> bool mask [dict_size] or latent indices")
        dev = cc.arena().data.device
        self.cc = cc
        self.k = k
        self.names = []
        self._masks = []
        for name, g in groups.items():
            if not isinstance(name, str) or name in RESERVED:
                raise ValueError(f"a group's name must be a string other than {RESERVED}, got {name!r}")
            self.names.append(name)
            self._masks.append(_group_mask(name, g, cc.d_hidden, dev))
        self.reset()

    def reset(self):
        """Forget everything seen so far."""
        dev = self.cc.arena().data.device
        e, n = 1 + len(self.names), self.cc.n_models
        self.rows = 0
        self._sq = torch.zeros(e, n, dtype=torch.float64, device=dev)  # sum over rows of the squared error
        self._ev = torch.zeros(e, n, dtype=torch.float64, device=dev)  # ... of 1 - sq_err / (total variance + eps)
        self._full = torch.zeros((), dtype=torch.int64, device=dev)

    def update(self, x):
        """x [rows, n_models, d_in] as CrossCoder.encode takes it.  The total variance is about this batch's mean."""
        cc = self.cc
        vals, idx = cc.encode_pairs(x, self.k)
        if x.shape[0] == 0:
            return
        xf = x.to(vals.device).float()
        tv = (xf - xf.mean(0)).pow(2).sum(-1) + EPS  # fp32 [rows, n_models]
        slot_latent = idx.clamp(min=0).long()  # (a padding slot's value is 0 already)
        for e, mask in enumerate([None] + self._masks):
            v = vals if mask is None else vals.masked_fill(mask[slot_latent], 0)
            sq = cc.pairs_sq_err(v, idx, x)
            self._sq[e] += sq.sum(0, dtype=torch.float64)
            self._ev[e] += (1 - sq / tv).sum(0, dtype=torch.float64)
        self._full += (idx[:, -1] >= 0).sum()  # (the pairs are padded at the end)
        self.rows += x.shape[0]

    def result(self):
        """{"baseline": e, <group>: e, ..., "rows": int, "full_rows": int} with e = {"mse", "explained_variance",
        "delta_mse"}: fp64 [n_models] on the host -- the mean per-row squared error, the mean per-row explained
        variance, and mse minus the baseline's.  Synchronises."""
        if self.rows == 0:
            raise ValueError("result(): no rows seen yet")
        mse, ev = (self._sq / self.rows).cpu(), (self._ev / self.rows).cpu()
        out = {"rows": self.rows, "full_rows": int(self._full)}
        for e, name in enumerate(["baseline"] + self.names):
            out[name] = {"mse": mse[e], "explained_variance": ev[e], "delta_mse": mse[e] - mse[0]}
        return out
