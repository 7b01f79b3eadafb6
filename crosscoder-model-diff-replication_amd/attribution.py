"""Latent attribution over a token stream: the first-order effect of every latent on a behavioural metric, per model,
in one pass (the twin of LatentAblation, which measures a few groups exactly at one sparse decode each).

The user supplies, per batch, the activations x and the gradient g = d metric / d reconstruction their LMs give by
hooks (the crosscoder's reconstruction patched in at the hook point).  `LatentAttribution(cc, k, groups)` encodes the
batch once into k (value, latent) pairs per row (CrossCoder.encode_pairs) and takes, per pair and model,

    attribution = value * <g[row, model], W_dec[latent, model]>

-- zeroing the pair changes the linearised metric by minus that -- from a gather kernel (CrossCoder.pairs_attribution:
k decoder rows per token; no dense [rows, dict_size] matrix and no [rows, dict_size] GEMM), then folds the pairs into
per-latent fp64 sums in a fixed order (ops.pairs_by_latent, ops.pairs_latent_sums): two runs over the same stream give
equal bits.  update() never synchronises with the host.

    at = LatentAttribution(cc, k=128, groups={"chat_only": chat_mask})
    for x, g in batches:         # both [rows, n_models, d_in]
        at.update(x, g)
    r = at.result()              # r["mean"], r["mean_abs"] fp64 [dict_size, n_models]; r["count"]; r["chat_only"]
    latents, summed = at.top(20, model=1)

The numbers are those of the k-pair form: exact for the rows with at most k non-zero activations; `full_rows` counts
the rows that use all k slots and may have been truncated to their k largest.
"""
import torch

from . import ops
from .ablation import _group_mask

RESERVED = ("rows", "full_rows", "mean", "mean_abs", "count")


def group_sums(total, masks):
    """fp64 [groups, n_models]: the per-latent summed attributions total [dict_size, n_models] added over each
    group's latents (masks: bool [dict_size] each)"""
    zero = torch.zeros((), dtype=total.dtype, device=total.device)
    return torch.stack([torch.where(m.unsqueeze(1), total, zero).sum(0) for m in masks]) if masks \
        else total.new_zeros(0, total.shape[1])


class LatentAttribution:
    def __init__(self, cc, k=None, groups=None):
        k = cc.k if k is None else k
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= cc.d_hidden:
            raise ValueError(f"k must be an int in 1..dict_size ({cc.d_hidden}), got {k!r} (pairs kept per row; a "
                             "crosscoder whose cfg has no 'k' needs one)")
        groups = {} if groups is None else groups
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
        h, n = self.cc.d_hidden, self.cc.n_models
        self.rows = 0
        self._sum = torch.zeros(h, n, dtype=torch.float64, device=dev)  # per latent and model: sum of attributions
        self._abs = torch.zeros(h, n, dtype=torch.float64, device=dev)  # ... of their absolute values
        self._count = torch.zeros(h, dtype=torch.int64, device=dev)     # pairs of the latent
        self._full = torch.zeros((), dtype=torch.int64, device=dev)

    def update(self, x, g):
        """x and g [rows, n_models, d_in]: the activations, as CrossCoder.encode takes them, and the gradient of the
        metric with respect to the reconstruction at the same rows."""
        cc = self.cc
        if g.shape != x.shape:
            raise ValueError(f"g must have x's shape {tuple(x.shape)}, got {tuple(g.shape)}")
        vals, idx = cc.encode_pairs(x, self.k)
        if x.shape[0] == 0:
            return
        a = cc.pairs_attribution(vals, idx, g)
        perm, seg = ops.pairs_by_latent(idx, cc.d_hidden)
        ops.pairs_latent_sums(a, perm, seg, self._sum, self._abs, self._count)
        self._full += (idx[:, -1] >= 0).sum()  # (the pairs are padded at the end)
        self.rows += x.shape[0]

    def result(self):
        """{"mean", "mean_abs": fp64 [dict_size, n_models] -- the attribution and the absolute attribution per token
        (summed over the latent's pairs, divided by the rows seen); "count": int64 [dict_size], the latent's pairs;
        <group>: {"attribution": fp64 [n_models]}, the group's latents' attributions summed over all rows: minus the
        first-order estimate of what zeroing the group does to the summed metric; "rows", "full_rows"}, on the host.
        Synchronises."""
        if self.rows == 0:
            raise ValueError("result(): no rows seen yet")
        out = {"rows": self.rows, "full_rows": int(self._full), "mean": (self._sum / self.rows).cpu(),
               "mean_abs": (self._abs / self.rows).cpu(), "count": self._count.cpu()}
        per_group = group_sums(self._sum, self._masks).cpu()
        for e, name in enumerate(self.names):
            out[name] = {"attribution": per_group[e]}
        return out

    def top(self, n, model=None):
        """(latents int64 [n], summed attribution fp64 [n]) on the host: the n latents with the largest absolute
        summed attribution, of one model or (None) added over the models; ties: the smaller latent."""
        h = self.cc.d_hidden
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= h:
            raise ValueError(f"n must be an int in 1..dict_size ({h}), got {n!r}")
        if model is not None and (isinstance(model, bool) or not isinstance(model, int)
                                  or not 0 <= model < self.cc.n_models):
            raise ValueError(f"model must be None or an int in 0..{self.cc.n_models - 1}, got {model!r}")
        s = (self._sum.sum(1) if model is None else self._sum[:, model]).cpu()
        order = torch.sort(s.abs(), descending=True, stable=True).indices[:n]
        return order, s[order]
