"""Dead-latent resampling for L1 (ReLU) dictionaries, and for TopK / BatchTopK ones: Anthropic's neuron resampling
("Towards Monosemanticity", appendix "Neuron resampling").

A ReLU latent whose pre-activation is negative on every token gets no gradient through the reconstruction, and the L1
term only shrinks it further.  `LatentResampler` keeps a pool of inputs with their reconstruction losses and the
latents' firing counts, and re-seeds each dead latent from a pool row drawn with probability proportional to the
squared loss: its decoder row becomes the row's direction at the alive latents' mean decoder norm, its encoder row
the same direction at `enc_scale` times their mean encoder norm, its encoder bias 0, its Adam state 0.

    rs = LatentResampler(cc, rows=64 * 4096)
    for x in batches:            # [B, n_models, d_in], as cc.get_losses takes it
        rs.add(x)
    out = rs.apply(optimizer)    # out["resampled"], out["latents"], out["rows"], ...
    rs.reset()

`Trainer.resample_dead_latents(rs)` applies it between steps with the trainer's optimizer and AuxK counters;
cfg["resample_every"] makes `Trainer.step` do all of it by itself (trainer.py).
"""
import math

import torch

from . import engine, ops


def _positive(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
        raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    return float(v)


class LatentResampler:
    def __init__(self, cc, rows, enc_scale=0.2, dec_scale=1.0, seed=0):
        """rows: the pool's capacity (allocated here, once: rows x n_models x d_in of the crosscoder's dtype, plus 12
        bytes per row and 24 per latent).  enc_scale / dec_scale: the re-seeded rows' norms as multiples of the alive
        latents' mean encoder-row / decoder-row norm.  seed: of apply()'s default uniforms."""
        if cc.activation == "jumprelu":
            raise ValueError("LatentResampler does not serve activation 'jumprelu': what a re-seeded latent's "
                             "threshold should be reset to is open, and a JumpReLU latent is revived by its "
                             "threshold falling")
        if isinstance(rows, bool) or not isinstance(rows, int) or rows < 1:
            raise ValueError(f"rows must be an int >= 1, got {rows!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int, got {seed!r}")
        self.cc = cc
        self.rows = rows
        self.enc_scale = _positive(enc_scale, "enc_scale")
        self.dec_scale = _positive(dec_scale, "dec_scale")
        self.seed = seed
        dev = cc.arena().data.device
        hp, K = cc._hp, cc.n_models * cc._dp
        self._x = torch.zeros(rows, K, dtype=cc.dtype, device=dev)
        self._loss = torch.zeros(rows, dtype=torch.float32, device=dev)
        self._cdf = torch.empty(rows, dtype=torch.float64, device=dev)
        # cc_latent_stats_update's state, of which the counts are what is read (k = 1, no histogram)
        self._count = torch.zeros(hp, dtype=torch.int64, device=dev)
        self._sum = torch.zeros(hp, dtype=torch.float32, device=dev)
        self._top_val = torch.zeros(hp, 1, dtype=torch.float32, device=dev)
        self._top_row = torch.full((hp, 1), -1, dtype=torch.int64, device=dev)
        self.filled = 0

    def reset(self):
        """Empty the pool and forget the firing counts (the storage stays)."""
        self.filled = 0
        self._count.zero_()
        self._sum.zero_()
        self._top_val.zero_()
        self._top_row.fill_(-1)

    def add(self, x):
        """x [B, n_models, d_in] as get_losses takes it: one forward of the crosscoder (get_losses' launches), after
        which the pool keeps the rows in the crosscoder's dtype, each row's squared reconstruction error summed over
        models and columns (the loss pass's per-row partials, summed on the device in a fixed order) and which latents
        fired on them (cc_latent_stats_update on the forward's activations).  ValueError past the capacity."""
        cc = self.cc
        cc._check_x(x)
        B = x.shape[0]
        if self.filled + B > self.rows:
            raise ValueError(f"LatentResampler.add: {B} more rows do not fit (capacity {self.rows}, {self.filled} "
                             "filled); reset() first or build it with more rows")
        if B == 0:
            return
        ws = cc._workspace(B)
        a = cc.arena()
        if a.data.device != self._x.device:
            raise ValueError(f"the crosscoder moved to {a.data.device}; the pool is on {self._x.device}")
        engine.forward(ws, a, cc.pad_input(x).contiguous(), None)
        r0, r1 = self.filled, self.filled + B
        self._x[r0:r1].copy_(ws.x)
        part = engine._row_part(ws)[0]  # [n * ncb][B]: sum (r - x)^2 per (model, column block, row)
        ops.reduce_rows(part, part.shape[0], B, out_f32=self._loss[r0:r1])
        ops.latent_stats_update(ws.acts, cc._hp, 1, self._count, self._sum, None, self._top_val, self._top_row,
                                row0=r0)
        self.filled = r1

    def dead(self):
        """bool [dict_size]: the latents that never fired on the rows added so far."""
        return self._count[:self.cc.d_hidden] == 0

    def _latents(self, dead):
        """`dead` (None: dead(); a bool mask [dict_size]; or an integer index tensor of distinct latents) as sorted
        int64 indices on the pool's device."""
        hr = self.cc.d_hidden
        if dead is None:
            dead = self.dead()
        dead = torch.as_tensor(dead)
        if dead.dtype == torch.bool:
            if tuple(dead.shape) != (hr,):
                raise ValueError(f"a dead mask must have shape ({hr},), got {tuple(dead.shape)}")
            return torch.nonzero(dead.to(self._x.device)).flatten()
        if dead.dtype.is_floating_point or dead.dtype.is_complex or dead.dim() != 1:
            raise ValueError("dead must be a bool mask [dict_size] or a 1-D integer tensor of latent indices")
        idx = dead.to(torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= hr):
            raise ValueError(f"latent indices must lie in [0, {hr})")
        uniq = torch.unique(idx)  # (sorted)
        if uniq.numel() != idx.numel():
            raise ValueError("latent indices must be distinct: a latent is re-seeded from one row")
        return uniq.to(self._x.device)

    def apply(self, optimizer=None, dead=None, u=None):
        """Re-seed the `dead` latents (default: dead()) from pool rows drawn with probability proportional to the
        squared loss, with replacement: latent j's row is the one whose interval of the losses' cumulative sum holds
        u[j] (u: J fp64 uniforms in [0, 1), J = the number of dead latents, in ascending latent order; default: drawn
        from a torch.Generator seeded with `seed`).  optimizer: the trainer's FusedAdam -- its moments of the
        re-seeded rows (and b_enc entries) are zeroed and its fp32 masters, if any, receive the unrounded rows -- or
        None: only the parameters are written.
        -> {"latents" int64 [J], "rows" int64 [J] (-1: nothing drawn), "written" bool [J] (False where the source row
        was all zeros), "enc_norm", "dec_norm" (floats: the re-seeded rows' norms), "resampled" (int)}.  An empty pool,
        no dead latent, no alive latent or an all-zero loss resample nothing: "resampled" is 0 and nothing is written.
        Synchronises with the device (the norms and the count are read)."""
        cc = self.cc
        latents = self._latents(dead)
        if optimizer is not None and getattr(optimizer, "cc", None) is not cc:
            raise ValueError("optimizer must be the FusedAdam of this resampler's crosscoder")
        J, hr, dev = latents.numel(), cc.d_hidden, self._x.device
        if u is not None:
            u = torch.as_tensor(u)
            if tuple(u.shape) != (J,) or not u.dtype.is_floating_point:
                raise ValueError(f"u must hold one float per dead latent ({J}), got {tuple(u.shape)} {u.dtype}")
        out = {"latents": latents, "rows": torch.full((J,), -1, dtype=torch.int64, device=dev),
               "written": torch.zeros(J, dtype=torch.bool, device=dev), "enc_norm": 0.0, "dec_norm": 0.0,
               "resampled": 0}
        if self.filled == 0 or J == 0 or J == hr:
            return out
        a = cc.arena()
        a.wait_pending()  # the decoder half may still be updating on the trainer's side stream
        alive = torch.ones(hr, dtype=torch.bool, device=dev)
        alive[latents] = False
        norms = torch.stack([ops.row_norms(a.W_enc_hk)[:hr], ops.row_norms(a.W_dec_hk)[:hr]]).double()
        mean = ((norms * alive).sum(1) / (hr - J)).tolist()
        enc_norm, dec_norm = self.enc_scale * mean[0], self.dec_scale * mean[1]
        if u is None:
            gen = torch.Generator(device="cpu").manual_seed(self.seed)
            u = torch.rand(J, dtype=torch.float64, generator=gen)
        u = u.to(dev, torch.float64).contiguous()
        loss = self._loss[:self.filled]
        rows, cdf = ops.resample_pick(loss, u, cdf=self._cdf[:self.filled])
        out["rows"] = rows
        if not float(cdf[-1]) > 0.0:  # (no row has weight: every pick is -1)
            return out
        master = m = v = None
        if optimizer is not None:
            # (before the write: a master arena out of date with the parameters is re-seeded from them now)
            master = optimizer.master_for_update()
            m, v = optimizer.exp_avg.data, optimizer.exp_avg_sq.data
        done = ops.resample_write(self._x[:self.filled], rows, latents, cc._hp, enc_norm, dec_norm, a.data,
                                  master=None if master is None else master.data, exp_avg=m, exp_avg_sq=v)
        # The kernel wrote the arenas without bumping a version counter: what is derived from the parameters is
        # re-keyed with Arena.updates (params_written): the selection weights and every step workspace's carried decoder
        # norms, norm partials and W_dec^T are derived again by their next reader; the masters are already the
        # unrounded rows, so their token moves along and they are not rebuilt from the rounded parameters
        cc.params_written()
        if master is not None:
            optimizer.master_updated()
        out["written"] = done.bool()
        out["enc_norm"], out["dec_norm"] = enc_norm, dec_norm
        out["resampled"] = int(done.sum())
        return out
