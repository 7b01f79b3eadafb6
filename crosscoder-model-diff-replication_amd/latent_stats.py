"""Per-latent activation statistics over a token stream (the notebook's latent dashboards: "Computing feature
acts", "histograms", "sequences"; the dead / dense latent counts of a training log).

`LatentStats(cc)` keeps, per latent, how often it fires, the sum and a log2 histogram of its non-zero
activations and the k rows where it fires hardest.  Each batch costs one HBM pass over the activations
(cc_latent_stats_update) into a small state that lives on the crosscoder's device and persists across
batches; results are bit-reproducible and do not depend on how the stream is cut into batches, except `sum`
(an fp32 sum per batch, added batch by batch).

    st = LatentStats(cc, k=16)
    for x in batches:            # [rows, n_models, d_in], as cc.encode takes it
        st.update(x)
    r = st.result()              # r["frequency"], r["dead"], r["topk_rows"], ...

`Trainer(cfg, ..., latent_stats=st)` feeds it every step's activations (trainer.py).
"""
import torch

from . import ops

HIST_BINS = 32
HIST_MIN_EXP = -16  # bin i holds 2^(i-16) <= v < 2^(i-15); bins 0 and 31 also take what lies beyond
CHUNK_ROWS = 4096   # update() encodes at most this many rows at a time
FREQ_BINS, FREQ_RANGE = 50, (-10.0, 0.0)


def hist_edges():
    """The 33 edges of the activation histogram: 2^-16 .. 2^16 (fp32, exact)."""
    return torch.pow(2.0, torch.arange(HIST_MIN_EXP, HIST_MIN_EXP + HIST_BINS + 1, dtype=torch.float64)).float()


def log10_frequency_hist(count, rows_seen, bins=FREQ_BINS, range_=FREQ_RANGE):
    """The across-latent density histogram the dashboards plot: log10(count / rows_seen) of the latents that
    fired at all, in `bins` equal bins over `range_` (numpy.histogram's convention: the last bin includes
    its right edge, 0 = fires on every row).  Host computation.  -> (counts int64 [bins], edges fp64 [bins + 1])."""
    c = torch.as_tensor(count).detach().to("cpu", torch.float64)
    alive = c[c > 0]
    edges = torch.linspace(range_[0], range_[1], bins + 1, dtype=torch.float64)
    if rows_seen <= 0 or alive.numel() == 0:
        return torch.zeros(bins, dtype=torch.int64), edges
    hist, edges = torch.histogram(torch.log10(alive / float(rows_seen)), bins=bins, range=tuple(range_))
    return hist.to(torch.int64), edges


class LatentStats:
    def __init__(self, cc, k=16, hist=True):
        max_k = ops.latent_stats_max_k()
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= max_k:
            raise ValueError(f"k must be an integer in 1..{max_k}, got {k!r}")
        self.cc = cc
        self.k = k
        self.with_hist = bool(hist)
        self._acts = None  # update()'s reused activation buffer [CHUNK_ROWS, kernel h]
        self.reset()

    def reset(self):
        """Forget everything seen so far (fresh state on the crosscoder's current device)."""
        dev = self.cc.arena().data.device
        hp = self.cc._hp
        self.rows_seen = 0
        self._count = torch.zeros(hp, dtype=torch.int64, device=dev)
        self._sum = torch.zeros(hp, dtype=torch.float32, device=dev)
        self._hist = torch.zeros(hp, HIST_BINS, dtype=torch.int64, device=dev) if self.with_hist else None
        self._topk_val = torch.zeros(hp, self.k, dtype=torch.float32, device=dev)
        self._topk_row = torch.full((hp, self.k), -1, dtype=torch.int64, device=dev)

    def _row_ids(self, row_ids, rows):
        if row_ids is None:
            return None
        row_ids = torch.as_tensor(row_ids)
        if row_ids.dim() != 1 or row_ids.shape[0] != rows:
            raise ValueError(f"row_ids must hold one id per row ({rows}), got shape {tuple(row_ids.shape)}")
        return row_ids.to(self._count.device, torch.int64).contiguous()

    def update_from_acts(self, acts, row_ids=None, row0=None):
        """acts [rows, width >= dict_size] already on the device (bf16 or fp32, rows contiguous; the kernels'
        padded width is fine, as is apply_relu=False output: only values > 0 count).  Row b gets the id
        row_ids[b], or row0 + b (row0 defaults to rows_seen)."""
        if acts.dim() != 2 or acts.shape[1] < self.cc.d_hidden:
            raise ValueError(f"expected acts of shape [rows, >= {self.cc.d_hidden}], got {tuple(acts.shape)}")
        if acts.device != self._count.device:
            raise ValueError(f"acts live on {acts.device}, the statistics on {self._count.device}")
        rows = acts.shape[0]
        ids = self._row_ids(row_ids, rows)
        if rows == 0:
            return
        h = min(acts.shape[1], self.cc._hp)  # (latents past h keep their state: padding latents never fire)
        ops.latent_stats_update(acts, h, self.k, self._count[:h], self._sum[:h],
                                None if self._hist is None else self._hist[:h], self._topk_val[:h],
                                self._topk_row[:h], row_ids=ids, row0=self.rows_seen if row0 is None else int(row0))
        self.rows_seen += rows

    def update(self, x, row_ids=None):
        """x [rows, n_models, d_in] as CrossCoder.encode takes it, any row count.  Without row_ids the rows
        are numbered on from rows_seen."""
        cc = self.cc
        cc._check_x(x)
        rows = x.shape[0]
        ids = self._row_ids(row_ids, rows)
        a = cc.arena()
        a.wait_pending()
        if self._acts is None or self._acts.device != a.data.device or self._acts.dtype != cc.dtype:
            self._acts = torch.empty(CHUNK_ROWS, cc._hp, dtype=cc.dtype, device=a.data.device)
        for r0 in range(0, rows, CHUNK_ROWS):
            r1 = min(rows, r0 + CHUNK_ROWS)
            acts = self._acts[:r1 - r0]
            ops.encode_fwd(cc._flat_x(x[r0:r1]), a.W_enc_hk, a.b_enc, acts, True)
            cc.activate_(acts)  # a TopK / BatchTopK crosscoder's activations, as cc.encode gives them for these rows
            self.update_from_acts(acts, row_ids=None if ids is None else ids[r0:r1])

    def result(self):
        """dict of tensors over the reference's dict_size latents (padding latents dropped)."""
        h = self.cc.d_hidden
        count, s = self._count[:h], self._sum[:h]
        tv, tr = self._topk_val[:h], self._topk_row[:h]
        n = max(self.rows_seen, 1)
        fh, fe = log10_frequency_hist(count, self.rows_seen)
        out = {
            "count": count.clone(),
            "frequency": (count.double() / n).float(),
            "dead": count == 0,
            "sum": s.clone(),
            "mean_active": torch.where(count > 0, s / count.clamp(min=1).float(), torch.zeros_like(s)),
            "max": tv[:, 0].clone(),
            "topk_values": tv.clone(),
            "topk_rows": tr.clone(),
            "hist_edges": hist_edges().to(count.device),
            "log10_frequency_hist": fh,
            "log10_frequency_edges": fe,
        }
        if self._hist is not None:
            out["hist"] = self._hist[:h].clone()
        return out
