"""The crosscoder training step as a fixed sequence of HIP launches over resident HBM buffers.

Data layout in HBM (one arena per role, all views of single allocations):
  params  [ W_enc h-major [h][K] | b_enc [h] | W_dec [h][K] | b_dec [K] ]   (dtype)
  grads   same layout (dtype)        exp_avg / exp_avg_sq   same layout (dtype)
  x [B][K], acts [B][h], g_recon [B][K] (dtype); recon [B][K] fp32 (latent-sharded step / two-pass form only).
  bf16 (transposed_wgrad): also x^T [K][B], acts^T [h][B], g_recon^T [K][B], and g_pre only as
  g_pre^T [h][B] -- G4/G5 contract over the batch, so these make both of their operands
  row-contiguous.  acts^T / g_pre^T come from G1's / G3's epilogues, x^T from the prep kernel, g_recon^T
  from G2's loss epilogue (LDS-staged transposed stores).  G2 reads W_dec [h][K] itself (transposed LDS
  reads of its B operand); the decoder norms come from the partial sums the decoder-half Adam writes.
W_enc's logical shape is [n, d, h] with strides (d, 1, K) exactly like the reference's
rearranged view (crosscoder.py:55-58), so both weight matrices are [h][K] row-major and
every GEMM streams 128-byte rows.

Step (reference trainer.py:41-63 -> crosscoder.py:96-130 -> autograd -> clip -> Adam), single GPU:
  prep      x = dtype(buf * factor), x^T, column sums for x.mean(0)          buffer.py:124, crosscoder.py:99
            (the Trainer's steady state: carried by the previous step's encoder-half Adam launch, PREP_IN_ADAM)
  G1        (prologue: x.mean(0)) acts = relu(x W_enc + b_enc), acts^T, mask bits, colsum/l0 slabs
                                                                            crosscoder.py:69-80,112,128
  (rest)    the decoder-half Adam's last rows of the previous step (+ their norm partials; none at
            DEC_SIDE_ROWS = 1.0, where the side launch takes b_dec along), then a wait for the side stream's rows
  G2+loss   (prologue: sum_b acts) acts W_dec + b_dec - x -> l2/tv row terms, g_recon = 2(r-x)/B,
            g_recon^T, db_dec slab (no fp32 reconstruction); its split-K leftover launch also finalises
            ||W_dec[h,m]||, their sum over m and inverses from the Adam's partials
                                                                            crosscoder.py:82-89,104-126
  G3        (prologue of its first workgroups: the loss tail -- l1 partials, EV, the loss scalars into
            mapped host memory) g_pre = (g_recon W_dec^T + l1c tn/B) * (acts>0), stored as g_pre^T
                                                                            crosscoder.py:106-128, autograd
  G4G5      dW_dec = acts^T g_recon + l1c/B colsum(acts) W_dec/||W_dec||,
            dW_enc = g_pre^T x, db_enc / db_dec, the clip coefficient        autograd, trainer.py:46
  adam      encoder half on this stream (+ the next batch's prep); the decoder half's first rows on the side
            stream beside the next step's G1 (with the next step's norm partials)   trainer.py:47
G1, G3 and G4G5 are persistent launches that hand out their tiles per XCD from counters (DYNAMIC_TILES).
The sparse TopK step (forward_sparse / backward_sparse, a StepWorkspace built with sparse=True; cfg["sparse_step"]) keeps
prep, G1, the loss kernels and adam, and runs G2 and the whole backward on the selection's k (value, latent) pairs per
row (csrc/sparse_step.hip, csrc/pairs_grad.hip) instead of G2, G3 and G4G5.
"""
import contextlib
import itertools

import torch

from . import _hip, ops

# Optional per-launch timer (bench.py installs one): an object with .span(name) -> context
# manager recording HIP events on torch's current stream around the launch.
TIMER = None


def _span(name):
    return TIMER.span(name) if TIMER is not None else contextlib.nullcontext()


# The persistent GEMMs (G1, G3, G4G5) hand out their tiles from per-XCD counters, so workgroups that start late
# (CUs held by the side stream's or RCCL's kernels) take fewer tiles; False: the static tile order.  The same
# bits either way (every partial-sum slot is indexed by tile; tests compare the two).
DYNAMIC_TILES = True


# The Trainer's loss tail rides in the backward's G3 launch (its first workgroups run it before their tiles, the
# dynamic tile order evens out their late start; cc_dacts_bwd_t's tail job), instead of a side-stream launch
# forked from the compute stream before G3.  The same bits either way.
LOSS_TAIL_IN_G3 = True


# G2 (the step's first reader of the decoder half) waits for the side-stream decoder-half Adam inside its kernel
# (a done counter the Adam's workgroups increment; cc_decode_loss' wait_ctr) instead of the compute stream
# waiting for the Adam's event: the ~10 us a cross-stream dependency takes to release the next kernel go away.
# Other readers still wait for the event.  The same bits either way.
G2_WAITS_IN_KERNEL = True


# The next batch's prep (x, x^T, the column-sum partials) rides in the step's encoder-half Adam launch (its first
# workgroups; cc_adam_step_prep) where the caller can name that batch (adam's next_batch, the Trainer's
# buffer.peek_raw()); the next forward() then skips its prep launch if it is handed exactly that batch (ws.prep_token)
# and runs prep as always otherwise.  The same bits either way.
PREP_IN_ADAM = True


# The side-stream decoder-half Adam takes b_dec along when it takes every row of W_dec (DEC_SIDE_ROWS = 1.0), so the
# first reader launches nothing after G1: it only waits (in G2's kernel, or for the event).  The same bits either way.
BDEC_IN_SIDE_ADAM = True


def _prep_token(x_in, factor, tag):
    """What identifies a raw batch handed to forward() as the one an Adam launch already prepped: the storage, layout
    and version counters of the batch and the factors, the caller's tag (the buffer's refresh count: a refresh rewrites
    rows without touching a version counter) and the stream both launches run on."""
    f = None if factor is None else (factor.data_ptr(), factor.dtype, tuple(factor.shape), factor._version)
    return (x_in.data_ptr(), x_in.dtype, tuple(x_in.shape), x_in.stride(), x_in._version, f, tag,
            torch.cuda.current_stream(x_in.device).cuda_stream)


def _tile_ctr(ws, k):
    return ws.tile_ctr[k] if DYNAMIC_TILES else None


def padded_dims(h, d):
    """Kernel dims (h, d) of a crosscoder with dict_size h and d_in d: both rounded up to a multiple of 8
    (the kernels move 16-byte rows).  The padding latents / columns are zero in every arena and stay
    zero through the step (their pre-activations, reconstructions, gradients and Adam updates are 0),
    so the reference-shaped views see exactly the reference crosscoder."""
    return -(-h // 8) * 8, -(-d // 8) * 8


class Arena:
    """Flat storage for the four parameters (or their grads / Adam moments):
    [ W_enc h-major [h][K] | b_enc [h] | W_dec [h][K] | b_dec [K] ] -- the encoder half and the
    decoder half are contiguous, so Adam can update them as two launches (enc_part / dec_part).
    h, d are the kernel dims (padded_dims); ref = (dict_size, d_in) of the reference-shaped views
    when they differ."""

    _serials = itertools.count()

    def __init__(self, h, n, d, dtype, device, data=None, ref=None):
        self.h, self.n, self.d = h, n, d
        self.h_ref, self.d_ref = ref if ref is not None else (h, d)
        self.padded = (self.h_ref, self.d_ref) != (h, d)
        K = n * d
        self.K = K
        self.numel = 2 * h * K + h + K
        self.data = data if data is not None else torch.zeros(self.numel, dtype=dtype, device=device)
        o = 0
        self.W_enc_hk = self.data[o:o + h * K].view(h, K)
        o += h * K
        self.b_enc = self.data[o:o + h]
        o += h
        self.split = o  # enc_part = data[:split], dec_part = data[split:]
        self.W_dec_hk = self.data[o:o + h * K].view(h, K)
        o += h * K
        self.b_dec_flat = self.data[o:o + K]
        self.pending = None  # event the decoder half's Adam (side stream) records; see clip_and_adam
        # the decoder half's last rows, launched by the first reader on its own stream (engine.adam)
        self.pending_rest = None
        # a stream already ordered after `pending` by a launch that waited for the Adam in its kernel
        self.pending_ordered = None
        # kernel writes of this arena so far (Adam launches, the scaling-factor fold, the resampler: whoever calls
        # CrossCoder.params_written): they bump no torch version counter, so everything cached from the params is
        # keyed on this as well (_norms_token, FusedAdam._arena_token, CrossCoder's selection weights)
        self.updates = 0
        self.serial = next(Arena._serials)  # (a re-packed arena may get a freed arena's address back)

    def enc_part(self):
        return self.data[:self.split]

    def dec_part(self):
        return self.data[self.split:]

    def wait_pending(self, kernel_wait=False):
        """Order torch's current stream after the decoder half's Adam if it ran on a side stream (launching
        its deferred last rows first, if any).  kernel_wait (the caller is a cc_decode_loss launch that can wait
        in its kernel): returns that wait's (counter, target) instead of ordering the stream, where the Adam
        signals one; the stream then counts as ordered once that launch is enqueued (pending_ordered)."""
        tok = None
        if self.pending_rest is not None:
            rest, self.pending_rest = self.pending_rest, None
            tok = rest(kernel_wait)
        if tok is not None:
            return tok
        if self.pending is not None:
            cur = torch.cuda.current_stream(self.data.device)
            if cur != self.pending_ordered:
                self.pending.wait(cur)
            self.pending = None
            self.pending_ordered = None
        return None

    def like(self, dtype=None, device=None):
        """A zeroed arena of the same dims (grads / Adam moments)."""
        return Arena(self.h, self.n, self.d, dtype or self.data.dtype, device or self.data.device,
                     ref=(self.h_ref, self.d_ref))

    # reference-shaped views ([:h_ref] latents, [:d_ref] columns per model of the kernel layout)
    def W_enc(self):  # [n, d, h], strides (d, 1, K)
        v = self.W_enc_hk.view(self.h, self.n, self.d)
        if self.padded:
            v = v[:self.h_ref, :, :self.d_ref]
        return v.permute(1, 2, 0)

    def W_dec(self):  # [h, n, d]
        v = self.W_dec_hk.view(self.h, self.n, self.d)
        return v[:self.h_ref, :, :self.d_ref] if self.padded else v

    def b_enc_ref(self):  # [h]
        return self.b_enc[:self.h_ref] if self.padded else self.b_enc

    def b_dec(self):  # [n, d]
        v = self.b_dec_flat.view(self.n, self.d)
        return v[:, :self.d_ref] if self.padded else v

    def views(self):
        return {"W_enc": self.W_enc(), "W_dec": self.W_dec(), "b_enc": self.b_enc_ref(), "b_dec": self.b_dec()}


class StepWorkspace:
    """All activations / partial-sum slabs of one step, allocated once per (B, shape, dtype)."""

    def __init__(self, B, n, d, h, dtype, device, transposed=None, topk=None, batch_topk=None, auxk=None,
                 jumprelu=None, sparse=False):
        """topk (a TopK crosscoder's k): forward() masks G1's activations in place to each row's k largest (one
        cc_topk_rows launch) and the step runs in its batch-major form, whose G3 / G4 read ws.acts itself.
        batch_topk ((k, weighted) of a BatchTopK crosscoder): instead, to the batch's B * k best pairs (cc_batch_topk,
        scored with the decoder norms ws.tn when weighted), in the same step form.
        auxk ((k_aux,), the AuxK dead-latent loss of a TopK / BatchTopK trainer): acts, g_recon, g_pre and the fp32
        reconstruction get 2 B rows and the g_pre column-partial slab twice its rows; the bottom halves are the aux
        rows (aux activations, g_aux, their g_pre, e^), the top halves what every B-row consumer sees as before.
        jumprelu (a JumpReLU crosscoder's bandwidth eps): forward() masks G1's activations in place to those above
        their latent's threshold (one cc_jumprelu_mask launch, which also writes ws.gate, G3's mask operand), in the
        batch-major form; the workspace owns the gate, the backward pass' two slabs (the threshold gradient's partials
        and g_pre's recomputed column partials) and a fifth segment of ws.sq for the threshold's squared gradient.
        sparse (with topk, the Trainer's sparse step: forward_sparse / backward_sparse): the workspace owns the pairs
        (pair_idx, pair_val), their d_acts (pair_gpre, fp32), perm / seg and the grouping's and the list gradients'
        scratch; it allocates no g_pre, no g_pre column partials and no G2 split-K workspace, and the first three
        segments of ws.sq take cc_pairs_wgrad's partials.
        sparse with auxk ((k_aux,)): no aux halves; the aux problem is a dense one over the D
        dead latents alone.  The workspace owns slot [h], the fp32 e^ and g_aux, the aux loss's parts and scalars,
        was_dead, dead_count, the device's D, and -- flat, of a capacity that aux_reserve grows geometrically and never
        shrinks, viewed per step by aux_views as [B][D_pad] / [D_pad][K] -- ids, acts_c (the selection runs in place and
        leaves aux_c there), g_pre_c and its column partials, Wc_dec, the addends aWd / aWe / ab, the squared-sum
        scratch nobody reads and the aux decode's split-K workspace."""
        f32 = torch.float32
        self.topk = topk
        self.sparse = bool(sparse)
        if self.sparse and topk is None:
            raise ValueError("a sparse workspace needs topk")
        self.batch_topk, self.bt_weighted = batch_topk if batch_topk is not None else (None, False)
        if topk is not None and batch_topk is not None:
            raise ValueError("topk and batch_topk exclude each other")
        self.jumprelu = None if jumprelu is None else float(jumprelu)
        if jumprelu is not None and (topk is not None or batch_topk is not None or auxk is not None):
            raise ValueError("jumprelu excludes topk, batch_topk and auxk")
        if topk is not None or batch_topk is not None or jumprelu is not None:
            transposed = False
        elif auxk is not None:
            raise ValueError("auxk needs topk or batch_topk")
        self.k_aux = auxk[0] if auxk is not None else None
        # rows of the buffers that carry an aux half (a sparse workspace carries none: its aux problem is compact)
        R = 2 * B if auxk is not None and not self.sparse else B
        K = n * d
        self.B, self.n, self.d, self.h, self.K, self.dtype = B, n, d, h, K, dtype
        E = lambda *s, dt=f32: torch.empty(*s, dtype=dt, device=device)  # noqa: E731
        # batch-contiguous copies for the weight gradients (G4/G5 then read row-contiguous KC tiles on
        # both operands: ~20 % faster than the batch-major MN/MN form at config 2).  transposed=False
        # forces the batch-major form (same results; the parity test compares the two)
        self.tr = transposed_wgrad(B, K, h, dtype) if transposed is None else bool(transposed) and \
            transposed_wgrad(B, K, h, dtype)
        self.x = E(B, K, dt=dtype)
        self.x_t = E(K, B, dt=dtype) if self.tr else None
        self.x_colpart = E(ops.prep_part_rows(B), K)
        self.x_mean = E(K)
        self.norms = E(h, n)
        self.tn = E(h)
        self.acts_full = E(R, h, dt=dtype)
        self.acts = self.acts_full[:B]
        # G2 + loss in one pass (decode_loss) when it serves the shape: its row terms come per 64-column
        # block and its b_dec-gradient partials per 128-row group; one storage holds either layout
        self.fused_ncb = ops.decode_loss_ncb(B, h, n, d, dtype) if self.tr else 0
        # the fused G2 reads W_dec [h][K] itself (transposed LDS reads); elsewhere in the transposed mode G2 reads
        # W_dec^T [K][h] (both operands h-contiguous), refreshed with the decoder norms after Adam
        self.W_dec_t = E(K, h, dt=dtype) if self.tr and not self.fused_ncb else None
        npart = ops.dec_norms_part_floats(h, n, d) if self.tr else 0
        # per-(row, 64-column block) squared sums of W_dec (d % 64 == 0): written by the decoder-half Adam
        # (cc_adam_dec_norms) or by the fused W_dec^T + norms pass
        self.norm_part = E(npart) if npart else None
        # the decoder-norm partials are complete but not yet finalised into norms / tn / inv_norms: the next G2
        # launch carries the finaliser (decode_loss), or flush_norms runs it before the first reader
        self.norms_fin_pending = False
        self.fork_events = [None, None]  # the step's last stream-fork events (loss tail, decoder-half Adam)
        self.tail_deferred = None  # (host, seq, l1l0_out) of a loss tail the G3 launch of the batch's last rows carries
        self.acts_t = E(h, B, dt=dtype) if self.tr else None
        # G1's activation mask as bits in the GEMM accumulator order: G3 reads 16 B per thread and tile instead
        # of the 128 KB acts tile (1/16 of the bytes, no LDS staging)
        self.mask_bits = E(ops.mask_bits_words(B, h), dt=torch.int32) if self.tr else None
        # G1's activation column-sum / l0 partial slabs, double-buffered: the loss tail that reads a
        # step's slabs runs on the side stream, which nothing orders before the NEXT step's G1 on torch's
        # stream; alternating slots orders every rewrite after that tail (the step after next waits for
        # this step's decoder-half Adam before G2, and the side stream runs the tail before that Adam)
        # (and the column sums reduced from them, which the side stream's loss tail reads: the NEXT step's
        # reduce runs on torch's stream before that step waits for the side stream)
        # (TopK: the slabs are the mask kernel's -- column sums and selected counts of the masked activations -- and
        # G1 writes none)
        if batch_topk is not None:
            self.n_wave, col_rows = ops.batch_topk_l0_parts(B, h), ops.batch_topk_part_rows(B, h)
            # the selection's workspace, its info words (threshold score bits, selected, ties admitted, eligible) and
            # every row's selected count
            self.bt_ws = E(ops.batch_topk_ws_bytes(B, h, dtype, self.bt_weighted), dt=torch.uint8)
            self.bt_info = torch.zeros(4, dtype=torch.int32, device=device)
            self.bt_row_count = torch.zeros(B, dtype=torch.int32, device=device)
        elif jumprelu is not None:
            self.n_wave, col_rows = ops.jumprelu_l0_parts(B, h), ops.jumprelu_part_rows(B, h)
            self.gate = E(B, h, dt=dtype)
            self.thr_part = E(col_rows, h)
            self.jr_gpre_colpart = E(col_rows, h)
            self.theta = None  # the thresholds the last forward masked with (fp32 [h]); the backward's too
        else:
            self.n_wave = ops.wave_parts(B, h) if topk is None else ops.topk_l0_parts(B, h)
            col_rows = ops.col_part_rows(B) if topk is None else ops.topk_part_rows(B, h)
        self._slots = [(E(col_rows, h), E(self.n_wave), E(h)) for _ in range(2)]
        self._slot = 1
        self.acts_colpart, self.l0_part, self.colsum_acts = self._slots[1]
        self.n_l1 = ops.reduce_parts(h)
        self.l1_part = E(self.n_l1)  # per 64-latent block: sum_h colsum_acts[h] * tn[h] (= B * l1)
        self.recon_full = E(R, K)
        self.recon = self.recon_full[:B]
        nws = 0 if self.sparse else ops.decode_ws_floats(B, h, K, dtype)
        self.dec_ws = E(nws) if nws else None  # G2 split-K partials
        self.g_recon_full = E(R, K, dt=dtype)
        self.g_recon = self.g_recon_full[:B]
        self.g_recon_t = E(K, B, dt=dtype) if self.tr else None
        self.ncb = ops.loss_col_blocks(d)
        rp = E(2 * n * max(self.ncb, self.fused_ncb) * B)
        self.row_part = rp[:2 * n * self.ncb * B].view(2, n * self.ncb, B)  # loss_fwd_bwd's layout
        self.row_part_fused = rp[:2 * n * self.fused_ncb * B].view(2, n * self.fused_ncb, B) if self.fused_ncb \
            else None
        # b_dec-gradient partial rows: the two-pass loss kernel writes one per 32 batch rows, the fused
        # G2 + loss epilogue one per 128-row wave half of every 256-row tile (more rows when B <= 32)
        self.loss_colpart = E(max(ops.loss_part_rows(B), ops.col_part_rows(B)), K)
        self.row_ncb = None         # layout of the row terms last written (None: loss_fwd_bwd's)
        self.loss_col_rows = ops.loss_part_rows(B)  # rows of loss_colpart last written
        self.ev = E(B)
        self.ev_a = E(B)
        self.ev_b = E(B)
        self.scalars = E(ops.loss_scalars_len(B))
        # transposed mode stores g_pre only as g_pre_t [h][B]; ws.g_pre is then its [B][h] view
        self.g_pre_t = E(h, B, dt=dtype) if self.tr else None
        self.g_pre_full = None if self.tr or self.sparse else E(R, h, dt=dtype)
        self.g_pre = self.g_pre_t.t() if self.tr else self.g_pre_full[:B] if not self.sparse else None
        cpr = ops.col_part_rows(B)
        self.gpre_colpart_full = None if self.sparse else E(cpr * (R // B), h)
        self.gpre_colpart = None if self.sparse else self.gpre_colpart_full[:cpr]
        if self.sparse:
            k = int(topk)
            self.pair_idx = E(B, k, dt=torch.int32)
            self.pair_val = E(B, k, dt=dtype)
            self.pair_gpre = E(B, k)  # d_acts at the pairs, fp32: the list gradients round it where they read it
            self.perm = E(B * k, dt=torch.int32)
            self.seg = E(h + 1, dt=torch.int64)
            self.group_ws = E(ops.pairs_group_ws_bytes(B, k, h), dt=torch.uint8)
            nwg = ops.pairs_wgrad_ws_floats(B * k, K)
            self.wgrad_ws = E(nwg) if nwg else None
        if auxk is not None and self.sparse:
            self.ehat, self.g_aux = E(B, K), E(B, K, dt=dtype)
            self.auxk_part = E(ops.auxk_part_floats(B, K))
            self.auxk_scalars = torch.zeros(4, dtype=f32, device=device)
            self.was_dead = torch.zeros(h, dtype=torch.uint8, device=device)
            self.dead_count = torch.zeros(1, dtype=torch.int32, device=device)
            self.slot = E(h, dt=torch.int32)
            self.aux_count = torch.zeros(1, dtype=torch.int32, device=device)  # D as cc_dead_compact counted it
            self.aux_cap = 0  # compact columns the flat buffers hold
            self.aux_D = self.aux_Dp = 0  # the last active step's dead count (the host's) and D_pad
            self.aux_dec_ws = None
            self.aux_reserve(-(-h // AUX_CAP_FRACTION))
        elif auxk is not None:
            # the aux halves, and the aux loss's partial slabs, scalars {auxk_loss, den, scale, valid}, the rows'
            # selected counts, the dead mask the step's selection used and the dead count after the step
            self.aux_acts, self.ehat, self.g_aux = self.acts_full[B:], self.recon_full[B:], self.g_recon_full[B:]
            self.g_pre_aux, self.gpre_colpart_aux = self.g_pre_full[B:], self.gpre_colpart_full[cpr:]
            self.auxk_part = E(ops.auxk_part_floats(B, K))
            self.auxk_scalars = torch.zeros(4, dtype=f32, device=device)
            self.aux_row_count = torch.zeros(B, dtype=torch.int32, device=device)
            self.was_dead = torch.zeros(h, dtype=torch.uint8, device=device)
            self.dead_count = torch.zeros(1, dtype=torch.int32, device=device)
        self.aux_active = False  # the last step issued the aux launches
        nw_w = ops.wgrad_parts(h, K, dtype)
        self.inv_norms = E(h, n)
        sizes = [nw_w, nw_w, ops.reduce_parts(h), ops.reduce_parts(K)]
        if self.sparse:
            sizes[:3] = [ops.pairs_wgrad_parts(h)] * 3
        if jumprelu is not None:
            sizes.append(ops.reduce_parts(h))  # the thresholds' gradient
        self.sq_off = [0]
        for s in sizes:
            self.sq_off.append(self.sq_off[-1] + s)
        self.sq = E(self.sq_off[-1])
        self.clip_out = E(8)
        self.tile_sum = E(ops.wgrad_tile_sums(h, K))  # per-tile squared sums of the fused G4G5 + grad tail
        ops.wgrad_clock(self.tile_sum).zero_()  # + the clock words the launch accumulates (bench: effective sclk)
        # per-XCD tile counters of the persistent G1 / G3 / G4G5 launches (dynamic tile order, DYNAMIC_TILES);
        # every launch leaves its counters at zero
        self.tile_ctr = torch.zeros(3, ops.TILE_CTR_WORDS, dtype=torch.int32, device=device)
        self.clip_ready = False  # backward(clip=...) already wrote clip_out (fused grad tail)
        self.acts_pending = False  # forward deferred the activation column sums to loss_finalize
        # arrival counters of the fused tail launches (loss tail, grad tail); each launch leaves 0
        self.tail_ctr = torch.zeros(2, dtype=torch.int32, device=device)
        # the side-stream decoder-half Adam's done counter (each workgroup adds 1; never reset) and the count
        # G2 waits for in its kernel (G2_WAITS_IN_KERNEL); wait_err: a mapped host word G2 sets if that wait
        # ever times out (checked by the next forward)
        self.adam_done = torch.zeros(8, dtype=torch.int32, device=device)
        self.adam_done_target = 0
        self.wait_err = None
        self.norms_token = None
        # the raw batch whose prep the last Adam launch carried (_prep_token; PREP_IN_ADAM), into a second set of
        # (x, x_t, x_colpart) allocated with the first such launch: ws.x stays the step's own batch for whoever reads
        # it after the step.  Any forward() consumes the token; the one handed that batch swaps the two sets
        self.prep_token = None
        self.x_next = None
        self.busy = None  # weakref to the token of an autograd graph whose backward still needs this workspace

    def aux_reserve(self, D):
        """A sparse AuxK workspace: room for D dead latents.  The capacity doubles until it holds aux_pad(D) (at most
        the kernel h) and never shrinks; a torch allocation, for between steps.  -> whether it grew."""
        need = min(aux_pad(D), self.h)
        if need <= self.aux_cap:
            return False
        cap = max(self.aux_cap, AUX_GRANULE)
        while cap < need:
            cap *= 2
        cap = self.aux_cap = min(cap, self.h)
        B, K, dt, dev = self.B, self.K, self.dtype, self.x.device
        E = lambda n, t=torch.float32: torch.empty(n, dtype=t, device=dev)  # noqa: E731
        self._ids = E(cap, torch.int32)
        self._acts_c, self._g_pre_c = E(B * cap, dt), E(B * cap, dt)
        self._Wc_dec, self._aWd, self._aWe, self._ab = E(cap * K, dt), E(cap * K, dt), E(cap * K, dt), E(cap, dt)
        self._gpre_colpart_c = E(ops.col_part_rows(B) * cap)
        self._aux_sq = E(2 * ops.wgrad_parts(cap, K, dt) + ops.reduce_parts(cap))
        return True

    def aux_views(self, D):
        """The step's views of the compact buffers for the host's dead count D (1 <= D, aux_pad(D) within the capacity):
        ids [D_pad], acts_c = aux_c and g_pre_c [B][D_pad], Wc_dec, aWd, aWe [D_pad][K], ab [D_pad], the g_pre column
        partials [col_part_rows(B)][D_pad].  ids and slot are rebuilt by every active step: nothing here is carried."""
        Dp = min(aux_pad(D), self.h)
        if Dp > self.aux_cap:
            raise ValueError(f"the compact aux buffers hold {self.aux_cap} latents, {Dp} are needed: aux_reserve first")
        B, K = self.B, self.K
        self.aux_D, self.aux_Dp = int(D), Dp
        self.ids = self._ids[:Dp]
        self.acts_c = self.aux_c = self._acts_c[:B * Dp].view(B, Dp)
        self.g_pre_c = self._g_pre_c[:B * Dp].view(B, Dp)
        self.Wc_dec, self.aWd, self.aWe = (t[:Dp * K].view(Dp, K) for t in (self._Wc_dec, self._aWd, self._aWe))
        self.ab = self._ab[:Dp]
        cpr = ops.col_part_rows(B)
        self.gpre_colpart_c = self._gpre_colpart_c[:cpr * Dp].view(cpr, Dp)
        need = ops.decode_ws_floats(B, Dp, K, self.dtype)
        if need and (self.aux_dec_ws is None or self.aux_dec_ws.numel() < need):
            self.aux_dec_ws = torch.empty(need, dtype=torch.float32, device=self.x.device)
        return Dp

    def next_slot(self):
        """Switch G1's partial slabs (acts_colpart, l0_part, colsum_acts) to the other slot (once per forward)."""
        self._slot ^= 1
        self.acts_colpart, self.l0_part, self.colsum_acts = self._slots[self._slot]

    def sq_slice(self, i):
        return self.sq[self.sq_off[i]:self.sq_off[i + 1]]


# The compact aux problem's latent extent D_pad is the dead count rounded up to AUX_GRANULE (a multiple of 8: the
# kernels move 16-byte rows), and a sparse AuxK workspace starts with room for 1 / AUX_CAP_FRACTION of the latents
# (DESIGN.md section 3.22).
AUX_GRANULE = 8
AUX_CAP_FRACTION = 32


def aux_pad(D):
    return max(1, -(-int(D) // AUX_GRANULE)) * AUX_GRANULE


def transposed_wgrad(B, K, h, dtype):
    """Whether the step keeps batch-contiguous operand copies for G4/G5 (bf16 ping-pong shapes)."""
    return bool(ops.lib().cc_transposed_ok(B, K, h, ops.dtype_code(dtype)))


def _norms_token(P):
    # what the workspace carries from W_dec (norms, norm partials, W_dec^T) stays valid while W_dec is the same storage
    # of the same arena, has not been written in place through torch (every such write bumps the version counter all
    # views of the arena share) and no kernel has written the arena since (Arena.updates: the step's Adam, which
    # derives the carry right after, and every other kernel writer -- CrossCoder.params_written)
    return (P.serial, P.W_dec_hk.data_ptr(), P.W_dec_hk._version, P.updates)


def norms_for_next(ws, P):
    """Launch the next step's decoder norms (and W_dec^T) now, right after Adam wrote W_dec, so they
    run while the host turns this step's loss scalars into the loss dict; forward() then skips them.
    (clip_and_adam(side_stream=...) launches them on the side stream itself.)"""
    if ws.norms_token == _norms_token(P):
        return
    ws.norms_fin_pending = False  # (as decoder_norms: nothing finalises over what is derived here)
    _decoder_derived(ws, P)
    ws.norms_token = _norms_token(P)


def _decoder_derived(ws, P):
    if ws.W_dec_t is not None and ws.norm_part is not None:  # W_dec^T and the norms from one pass over W_dec
        with _span("dec_norms_T"):
            ops.transpose_dec_norms(P.W_dec_hk, ws.n, ws.d, ws.W_dec_t, ws.norm_part, ws.norms, ws.tn, ws.inv_norms)
        return
    if ws.W_dec_t is not None:
        ops.transpose(P.W_dec_hk, out=ws.W_dec_t)
    ops.dec_norms(P.W_dec_hk, ws.h, ws.n, ws.d, norms=ws.norms, total=ws.tn, inv_norms=ws.inv_norms)


def flush_norms(ws):
    """Finalise pending decoder norms on torch's current stream (where no G2 launch carried the finaliser)."""
    if ws.norms_fin_pending:
        ws.norms_fin_pending = False
        with _span("dec_norms"):
            ops.dec_norms_finalize(ws.norm_part, ws.h, ws.n, ws.d, ws.norms, ws.tn, ws.inv_norms)


def decoder_norms(ws, P):
    """||W_dec[h, m]||, their sum over m and inverses (crosscoder.py:123-125), unless still fresh.  Call it after
    Arena.wait_pending(): the first reader's wait for the side-stream Adam sets norms_fin_pending, and norm partials
    pending their finaliser are Adam's, of the W_dec it wrote -- where W_dec was written since (the token moved), they
    are dropped with the token, or the next G2 launch / flush_norms would finalise them over the re-derived norms."""
    fresh = getattr(ws, "norms_token", None) == _norms_token(P)
    ws.norms_token = None  # consumed: W_dec changes with this step's Adam
    if fresh:
        return
    ws.norms_fin_pending = False
    _decoder_derived(ws, P)


def _take_or_prep(ws, x_in, factor, prep_tag):
    """ws.x / x_t / x_colpart <- the prepped batch: the one the last Adam launch carried where that was exactly this
    batch's (PREP_IN_ADAM; the buffers are swapped in), else a prep launch"""
    prepped, ws.prep_token = ws.prep_token, None
    if prepped is not None and prepped == _prep_token(x_in, factor, prep_tag):
        (ws.x, ws.x_t, ws.x_colpart), ws.x_next = ws.x_next, (ws.x, ws.x_t, ws.x_colpart)
    else:
        with _span("prep"):
            ops.prep_input(x_in, factor, ws.dtype, out=ws.x, colsum_part=ws.x_colpart, out_t=ws.x_t)


def forward(ws, P, x_in, factor=None, grad_scale=None, want_grad=True, loss=True, finalize=True, bt_threshold=None,
            aux=None, theta=None, prep_tag=None):
    """Forward + reconstruction-loss gradient.  P: params Arena.  x_in [B, n, d] any of
    fp32/bf16, factor [n] or None.  Leaves losses in ws.scalars / ws.ev*, g_recon ready
    (loss=False: stops at the fp32 reconstruction, for loss_rows / loss_finalize by slices;
    finalize=False: stops after the loss rows, for loss_finalize_with_g3 / loss_finalize_beside).  Where the fused entry
    serves the shape, G2 and the loss rows are one pass (decode_loss_t; no fp32 reconstruction).
    bt_threshold ((tensor, beta), BatchTopK, the Trainer's): the running threshold the selection folds its T into.
    aux ((since_fired, dead_after), the Trainer's, a workspace built with auxk): the AuxK selection of G1's activations
    among the dead latents goes into ws.aux_acts, before the main mask overwrites them.
    theta (fp32 [h], a workspace built with jumprelu): the thresholds of the JumpReLU mask.
    prep_tag: the tag of adam's next_batch, where x_in may be that batch (the Trainer's: its buffer's refresh count)."""
    B, n, d, h, K = ws.B, ws.n, ws.d, ws.h, ws.K
    ws.next_slot()
    _take_or_prep(ws, x_in, factor, prep_tag)
    # G1 reads only the encoder half: it may overlap the previous step's decoder-half Adam.  x.mean(0) (first
    # read by the loss) and sum_b acts (G4's L1 term and the l1 loss, crosscoder.py:112,126): column reductions
    # of the prep / G1 partial slabs -- carried in the prologues of G1 and G2 where the step's fused path runs
    # (cc_colsum_job: no launches of their own), else two reduce_rows launches after G1
    fused = bool(loss and ws.fused_ncb)  # (fused_ncb: the transposed-operand step only)
    # (the latent-sharded step's G1 -- loss=False -- carries x.mean(0) too; its G2, decode_partial_jobs, carries
    # sum_b acts and the decoder norms' finaliser)
    x_job = ops.colsum_job(ws.x_colpart, ws.x_colpart.shape[0], K, 1.0 / B, ws.x_mean) if ws.tr else None
    with _span("G1_encode"):
        if ws.tr:
            ops.encode_fwd_t(ws.x, P.W_enc_hk, P.b_enc, ws.acts, ws.acts_t, True, colsum_part=ws.acts_colpart,
                             l0_part=ws.l0_part, mask_bits=ws.mask_bits, tile_ctr=_tile_ctr(ws, 0), pre=x_job)
        elif ws.topk is None and ws.batch_topk is None and ws.jumprelu is None:
            ops.encode_fwd(ws.x, P.W_enc_hk, P.b_enc, ws.acts, True, colsum_part=ws.acts_colpart,
                           l0_part=ws.l0_part)
        else:
            ops.encode_fwd(ws.x, P.W_enc_hk, P.b_enc, ws.acts, True)
    if aux is not None:
        with _span("auxk_rows"):
            ops.auxk_rows(ws.acts, h, ws.k_aux, aux[0], aux[1], out=ws.aux_acts, row_count=ws.aux_row_count)
    if ws.topk is not None:
        # TopK: the mask in place, before anything else reads the activations; G2, the loss tail, G3 and G4 then see
        # the masked activations, their column sums and the selected count
        with _span("topk"):
            ops.topk_rows(ws.acts, h, ws.topk, out=ws.acts, colsum_part=ws.acts_colpart, l0_part=ws.l0_part)
    if ws.jumprelu is not None:
        # JumpReLU: the same, one streaming pass; it also leaves the gate (the kept elements plus the lower half of the
        # straight-through window), G3's mask operand
        if theta is None:
            raise ValueError("a jumprelu workspace's forward needs theta")
        ws.theta = theta
        with _span("jumprelu"):
            ops.jumprelu_mask(ws.acts, h, theta, ws.jumprelu, out=ws.acts, gate=ws.gate, colsum_part=ws.acts_colpart,
                              l0_part=ws.l0_part)
    norms_done = False
    if ws.batch_topk is not None:
        # BatchTopK: the same, one selection over the batch.  Weighted, it is scored with the decoder norms ws.tn (the
        # L1 term's own), which therefore have to be current before the mask: the wait for the decoder-half Adam and
        # the norms move ahead of it (G1 above still overlaps that Adam).  Unweighted, they stay where TopK has them
        if ws.bt_weighted:
            P.wait_pending()
            decoder_norms(ws, P)
            flush_norms(ws)
            norms_done = True
        thr, beta = bt_threshold if bt_threshold is not None else (None, 0.0)
        with _span("batch_topk"):
            ops.batch_topk(ws.acts, h, B * ws.batch_topk, weight=ws.tn if ws.bt_weighted else None, out=ws.acts,
                           colsum_part=ws.acts_colpart, l0_part=ws.l0_part, row_count=ws.bt_row_count,
                           info=ws.bt_info, ws=ws.bt_ws, threshold=thr, beta=beta)
    if x_job is None:
        ops.reduce_rows(ws.x_colpart, ws.x_colpart.shape[0], K, scale=1.0 / B, out_f32=ws.x_mean)
    acts_job = ops.colsum_job(ws.acts_colpart, ws.acts_colpart.shape[0], h, 1.0, ws.colsum_acts)
    fused_g2 = bool(loss and ws.fused_ncb)
    # the latent-sharded step's G2 (decode_partial_jobs: W_dec read as stored, bf16) waits in its kernel too
    partial_g2 = bool(not loss and ws.tr and ws.W_dec_t is None)
    # (only while the decoder norms are the Adam's own: otherwise decoder_norms below reads W_dec on this stream)
    wait = None if norms_done else P.wait_pending(kernel_wait=(fused_g2 or partial_g2) and G2_WAITS_IN_KERNEL
                                                  and ws.norms_token == _norms_token(P))
    if wait is not None:
        wait = (*wait, _wait_err(ws))
    if not norms_done:
        decoder_norms(ws, P)  # (+ W_dec^T), unless launched already after the last Adam
    if fused_g2:
        # (carries a pending norm finaliser and, fused, the activation column sums; waits in its kernel for the
        # side-stream Adam where `wait`)
        decode_loss(ws, P, grad_scale, pre=acts_job, wait=wait)
        ws.acts_pending = True
        if finalize:
            loss_finalize(ws)
        return
    with _span("G2_decode"):
        if ws.W_dec_t is not None:
            ops.reduce_rows(ws.acts_colpart, ws.acts_colpart.shape[0], h, out_f32=ws.colsum_acts)
            ops.decode_partial_t(ws.acts, ws.W_dec_t, ws.recon, ws.dec_ws)
        else:
            nf = (ws.norm_part, ws.norms, ws.tn, ws.inv_norms) if ws.norms_fin_pending else None
            ws.norms_fin_pending = False
            ops.decode_partial_jobs(ws.acts, P.W_dec_hk, ws.recon, ws.dec_ws, ws.n, ws.d, norm_fin=nf, pre=acts_job,
                                    wait=wait)
            if wait is not None:
                P.pending_ordered = torch.cuda.current_stream(ws.x.device)
    # (G2 does not read the norms: their finaliser after it, where the latent-sharded step's collective on the
    # reconstruction hides it)
    flush_norms(ws)
    # B * l1 = sum_h colsum_acts[h] * tn[h] (crosscoder.py:126) rides in the loss finaliser's launch
    # (loss_tail)
    ws.acts_pending = True
    if loss:
        loss_rows(ws, P, 0, ws.B, grad_scale)
        if finalize:
            loss_finalize(ws)


def forward_sparse(ws, P, x_in, factor=None, prep_tag=None, aux=None):
    """forward(finalize=False) of the sparse TopK step (a workspace built with sparse=True): prep
    and G1 as the dense TopK step, then the selection as k (value, latent) pairs per row with the same column-sum and
    count slabs (no dense masked write: ws.acts keeps G1's activations), the pairs grouped by latent (ws.perm, ws.seg),
    the plain event wait for the decoder-half Adam, the sparse G2 into ws.recon and the loss rows.  The caller forks
    the loss tail (loss_finalize_beside, or loss_finalize on this stream).
    aux ((since_fired, h_real, dead_after, D), the Trainer's, a workspace built with auxk, D >= 1 the host's dead count
    and within ws.aux_reserve): the dead set of since_fired is compacted (ws.ids, ws.slot), G1's activations of those
    latents gathered into ws.acts_c and reduced in place to each row's min(k_aux, D) largest (ws.aux_c), and -- after
    the wait for the decoder-half Adam -- their decoder rows gathered into ws.Wc_dec."""
    B, h, K = ws.B, ws.h, ws.K
    ws.next_slot()
    _take_or_prep(ws, x_in, factor, prep_tag)
    with _span("G1_encode"):
        ops.encode_fwd(ws.x, P.W_enc_hk, P.b_enc, ws.acts, True)
    if aux is not None:
        since_fired, h_real, dead_after, D = aux
        Dp = ws.aux_views(D)
        with _span("dead_compact"):
            ops.dead_compact(since_fired, h_real, dead_after, ws.ids, ws.slot, ws.aux_count)
        with _span("compact_cols"):
            ops.compact_gather(ws.ids, h, acts=ws.acts, acts_c=ws.acts_c)
        with _span("auxk_topk"):
            # (ids ascends, so the tie order in the compact index is the tie order in the latent)
            ops.topk_rows(ws.acts_c, Dp, min(ws.k_aux, int(D)), out=ws.acts_c)
    with _span("topk_pairs"):
        ops.topk_rows(ws.acts, h, ws.topk, out=None, idx_out=ws.pair_idx, val_out=ws.pair_val,
                      colsum_part=ws.acts_colpart, l0_part=ws.l0_part)
    with _span("pairs_group"):
        ops.pairs_group(ws.pair_idx, h, perm=ws.perm, seg=ws.seg, ws=ws.group_ws)
    ops.reduce_rows(ws.x_colpart, ws.x_colpart.shape[0], K, scale=1.0 / B, out_f32=ws.x_mean)
    ops.reduce_rows(ws.acts_colpart, ws.acts_colpart.shape[0], h, out_f32=ws.colsum_acts)
    P.wait_pending()
    decoder_norms(ws, P)
    if aux is not None:
        with _span("compact_rows"):
            ops.compact_gather(ws.ids, h, W=P.W_dec_hk, Wc=ws.Wc_dec)
    with _span("G2_decode_pairs"):
        ops.decode_pairs_partial(ws.pair_val, ws.pair_idx, P.W_dec_hk, K, h=h, recon=ws.recon)
    flush_norms(ws)
    ws.acts_pending = True
    loss_rows(ws, P, 0, B)


def auxk_forward_sparse(ws, P, since_fired, h_real, dead_after, auxk_coeff, active, host=None):
    """auxk_forward for the sparse step, after forward_sparse and before the loss tail is forked: the dead update
    (always; the dead count also into word 10 of `host`), then -- active: forward_sparse(aux=...) ran -- the aux decode
    e^ = aux_c . Wc_dec over the compact extent and the aux loss against the sparse step's fp32 ws.recon, with g_aux
    (auxk_loss also into word 9 of `host`)."""
    word = (lambda i: host.device_ptr.value + 4 * i) if host is not None else (lambda i: None)
    with _span("dead_update"):
        ops.dead_update(ws.colsum_acts, since_fired, h_real, ws.B, dead_after, ws.dead_count, was_dead=ws.was_dead,
                        host_ptr=word(10))
    ws.aux_active = bool(active)
    if not active:
        return
    with _span("auxk_decode"):
        ops.decode_partial(ws.aux_c, ws.Wc_dec, ws.ehat, ws.aux_dec_ws)
    with _span("auxk_loss"):
        ops.auxk_loss(ws.recon, P.b_dec_flat, ws.x, ws.ehat, ws.g_aux, ws.auxk_part, ws.auxk_scalars, auxk_coeff,
                      host_ptr=word(9))


def backward_sparse(ws, P, G, aux=False):
    """The sparse TopK step's backward, for l2 alone (l1_coeff = 0): d_acts at the pairs (the sampled dot products of
    g_recon with the selected decoder rows; a selected activation is > 0, so the straight-through mask is 1), the three
    list gradients with their squared-sum partials in one grouped launch pair, and b_dec's gradient from the loss's
    column partials.  clip_and_adam then runs its clip_finalize over ws.sq.
    aux (an active AuxK step: auxk_forward_sparse left g_aux): the aux loss's gradients as a dense problem over the
    compact extent -- G3 on the aux rows (no L1 term), G4 and G5 into the addends, the column sums of g_pre_c into ab,
    their squared sums into scratch nobody reads -- which the list gradients' launch adds, row slot[j] to latent j, into
    its fp32 sums before the one rounding (cc_pairs_wgrad_add).  Nothing of the aux loss reaches b_dec."""
    P.wait_pending()
    with _span("pairs_dacts"):
        ops.pairs_grad_values(ws.pair_idx, P.W_dec_hk, ws.g_recon, ws.n, ws.d, h=ws.h, total=ws.pair_gpre,
                              want_dot=False)
    add = None
    if aux:
        Dp = ws.aux_Dp
        nw = ops.wgrad_parts(Dp, ws.K, ws.dtype)
        sq_d, sq_e, sq_b = ws._aux_sq[:nw], ws._aux_sq[nw:2 * nw], ws._aux_sq[2 * nw:2 * nw + ops.reduce_parts(Dp)]
        with _span("G3_dacts_aux"):
            ops.dacts_bwd(ws.g_aux, ws.Wc_dec, ws.aux_c, ws.tn, 0.0, ws.g_pre_c, colsum_part=ws.gpre_colpart_c)
        with _span("G4_wgrad_dec_aux"):
            ops.wgrad_dec(ws.aux_c, ws.g_aux, ws.Wc_dec, ws.inv_norms, ws.colsum_acts, 0.0, ws.aWd, sq_d, ws.n, ws.d)
        with _span("G5_wgrad_enc_aux"):
            ops.wgrad_enc(ws.g_pre_c, ws.x, ws.aWe, sq_e)
        with _span("b_enc_grad_aux"):
            ops.reduce_rows(ws.gpre_colpart_c, ws.gpre_colpart_c.shape[0], Dp, out_t=ws.ab, sq_part=sq_b)
        add = (ws.slot, ws.aWd, ws.aWe, ws.ab)
    with _span("pairs_wgrad"):
        ops.pairs_wgrad(ws.perm, ws.seg, ws.pair_val, ws.pair_gpre, ws.g_recon, ws.x, ws.K, G.W_dec_hk, G.W_enc_hk,
                        G.b_enc, ws.sq_slice(1), ws.sq_slice(0), ws.sq_slice(2), ws=ws.wgrad_ws, add=add)
    with _span("b_dec_grad"):
        ops.reduce_rows(loss_colpart(ws), ws.loss_col_rows, ws.K, out_t=G.b_dec_flat, sq_part=ws.sq_slice(3))
    ws.clip_ready = False


STEP_ABORTED_MSG = ("crosscoder_hip: the step was aborted -- G2's in-kernel wait for the previous step's decoder-half "
                    "Adam (side stream) timed out, so G2 ran none of its tiles and this step's Adam launches applied no "
                    "update (params and Adam moments are those before the step; its batch was consumed).  If that "
                    "Adam was still running when this step's backward wrote its gradients, the decoder half of the "
                    "previous update may be inconsistent: reload a checkpoint.")


def check_step_abort(ws):
    """Raise (once: the word is cleared) if a G2 launch of this workspace timed out in its in-kernel wait.  The
    step's clip finaliser (after G3, which wrote the loss scalars the host just read) still has to see the word, so
    the device is drained before it is cleared (an error path: the sync costs nothing that matters)."""
    if ws is not None and ws.wait_err is not None and ws.wait_err.u32[0]:
        torch.cuda.synchronize(ws.x.device)
        ws.wait_err.u32[0] = 0
        raise RuntimeError(STEP_ABORTED_MSG)


def _wait_err(ws):
    """The mapped host word a G2 launch sets if its in-kernel wait times out.  The Trainer raises in the same step
    (check_step_abort after its loss read); other callers see it here, at the next forward, at the latest."""
    if ws.wait_err is None:
        ws.wait_err = _hip.MappedHostBuffer(4)
    check_step_abort(ws)
    return ws.wait_err.device_ptr


def decode_loss(ws, P, grad_scale=None, pre=None, wait=None):
    """G2 + loss rows + g_recon (and g_recon^T) in one pass over the whole batch (decode_loss: W_dec read
    directly).  pre: an ops.colsum_job the launch runs first; wait: (counter, target, err) of the side-stream
    Adam it waits for in the kernel."""
    gs = 2.0 / ws.B if grad_scale is None else grad_scale
    nf = (ws.norm_part, ws.norms, ws.tn, ws.inv_norms) if ws.norms_fin_pending else None
    ws.norms_fin_pending = False
    with _span("G2_decode"):
        ops.decode_loss(ws.acts, P.W_dec_hk, P.b_dec_flat, ws.x, ws.x_mean, gs, ws.g_recon, ws.g_recon_t,
                        ws.row_part_fused, ws.loss_colpart, ws.dec_ws, ws.n, ws.d, norm_fin=nf, pre=pre, wait=wait)
    if wait is not None:
        P.pending_ordered = torch.cuda.current_stream(ws.x.device)
    ws.row_ncb = ws.fused_ncb
    ws.loss_col_rows = ops.col_part_rows(ws.B)


def loss_rows(ws, P, r0, r1, grad_scale=None):
    """Loss row terms + g_recon for batch rows [r0, r1) (r0 % 32 == 0); slabs keep the batch layout."""
    gs = 2.0 / ws.B if grad_scale is None else grad_scale
    with _span("loss"):
        ops.loss_fwd_bwd(ws.recon, P.b_dec_flat, ws.x, ws.x_mean, ws.g_recon, ws.row_part, ws.loss_colpart, gs, ws.B,
                         ws.n, ws.d, row0=r0, rows=r1 - r0, g_recon_t=ws.g_recon_t)
    ws.row_ncb = None
    ws.loss_col_rows = ops.loss_part_rows(ws.B)


def _row_part(ws):
    return ws.row_part if ws.row_ncb is None else ws.row_part_fused


def loss_colpart(ws):
    """The b_dec-gradient partial rows the last loss producer wrote."""
    return ws.loss_colpart[:ws.loss_col_rows]


def loss_finalize(ws, l1l0_out=None, host=None, seq=0):
    """Loss scalars / EV vectors.  After a forward (which left the l1 partials to be formed against the
    decoder norms) one launch does both (cc_loss_tail); a re-formed loss (same activations) only the
    finaliser.  host (a _hip.MappedHostBuffer): the scalars also land there, then `seq` in word 8."""
    flush_norms(ws)  # (no-op after forward(), which ran the finaliser with or before G2)
    ws.tail_deferred = None
    if ws.acts_pending:
        ops.loss_tail(ws.colsum_acts, ws.tn, ws.l1_part, _row_part(ws), ws.l0_part, ws.n_wave, ws.ev, ws.ev_a,
                      ws.ev_b, ws.scalars, ws.B, ws.n, ws.d, ws.tail_ctr[0:1], l1l0_out=l1l0_out, host=host, seq=seq,
                      ncb=ws.row_ncb)
        ws.acts_pending = False
        return
    ops.loss_finalize(_row_part(ws), ws.l1_part, ws.n_l1, ws.l0_part, ws.n_wave, ws.ev, ws.ev_a, ws.ev_b, ws.scalars,
                      ws.B, ws.n, ws.d, l1l0_out=l1l0_out, host=host, seq=seq,
                      ncb=ws.row_ncb if ws.row_ncb is not None else ops.loss_col_blocks(ws.d))


def loss_from_recon(ws, P, grad_scale=None):
    """Re-form g_recon (+ the loss slabs) for another grad_scale, from the forward's operands: after the
    fused pass (no fp32 reconstruction kept) G2 runs again on the same acts / W_dec^T."""
    if ws.row_ncb is not None:
        decode_loss(ws, P, grad_scale)
    else:
        loss_rows(ws, P, 0, ws.B, grad_scale)
    loss_finalize(ws)


def loss_finalize_beside(ws, side_stream, on_losses=None, host=None, seq=0):
    """loss_finalize (+ on_losses(ws.scalars), e.g. a host copy) on `side_stream`, after everything
    queued so far on torch's stream: the backward's G3 does not read the tail's outputs, so it starts
    right after the loss kernel (the tail's workgroups fit beside G3's), and nothing on torch's stream
    reads the tail's outputs (G4's activation column sums come from forward()).  host / seq: the scalars
    go straight to mapped host memory (loss_finalize); then no event is recorded and None is returned,
    else the event that marks the tail's end."""
    dev = ws.x.device
    # (device-scope events for every stream-to-stream hand-off of the step: a torch event's system-scope release
    # idles the recording stream ~1.7 us longer, profiles/r04_event_probe.txt)
    ready = _hip.DeviceEvent().record(torch.cuda.current_stream(dev))
    ws.fork_events[0] = ready  # (kept alive until the next step's fork: the side stream's wait references it)
    with torch.cuda.stream(side_stream):
        ready.wait(side_stream)
        loss_finalize(ws, host=host, seq=seq)
        if on_losses is not None:
            on_losses(ws.scalars)
        if host is not None and on_losses is None:
            return None
        return _hip.DeviceEvent().record(side_stream)


def loss_finalize_with_g3(ws, side_stream, host=None, seq=0):
    """The loss tail of loss_finalize(ws, host=host, seq=seq), carried by the backward's G3 launch where it serves the
    shape (LOSS_TAIL_IN_G3, the transposed-operand step); otherwise loss_finalize_beside on `side_stream`.  Returns
    None (G3 carries it; the host reads the scalars through `host`) or loss_finalize_beside's event."""
    if LOSS_TAIL_IN_G3 and ws.tr and ws.acts_pending and host is not None:
        ws.tail_deferred = (host, seq, None)
        return None
    return loss_finalize_beside(ws, side_stream, host=host, seq=seq)


def row_chunks(B, n_chunks):
    """Batch slices [r0, r1) for the chunked (comm-overlapped) step: boundaries on 256-row GEMM
    tiles, so each slice's d_acts launch owns whole column-partial rows."""
    step = -(-B // max(1, n_chunks))
    step = -(-step // 256) * 256
    return [(r0, min(B, r0 + step)) for r0 in range(0, B, step)]


def dacts_rows(ws, P, l1_coeff, r0, r1, l1_grad_weight=1.0):
    """G3 over batch rows [r0, r1) (r0 % 256 == 0): g_pre rows + their column-sum partial rows."""
    l1_scale = float(l1_coeff) * l1_grad_weight / ws.B
    c0, c1 = ops.col_part_rows(r0), ops.col_part_rows(r1)
    flush_norms(ws)
    tail = None
    # a deferred loss tail rides in the launch of the batch's LAST rows: every loss row is written by then (the
    # latent-sharded step's per-slice loss rows precede their slice's G3 on this stream)
    if ws.tail_deferred is not None and r1 == ws.B:
        host, seq, l1l0_out = ws.tail_deferred
        ws.tail_deferred = None
        if ws.tr:
            tail = ops.loss_tail_job(ws.colsum_acts, ws.tn, ws.l1_part, _row_part(ws), ws.l0_part, ws.n_wave, ws.ev,
                                     ws.ev_a, ws.ev_b, ws.scalars, ws.B, ws.n, ws.d, ws.tail_ctr[0:1],
                                     l1l0_out=l1l0_out, host=host, seq=seq, ncb=ws.row_ncb)
            ws.acts_pending = False
        else:
            loss_finalize(ws, l1l0_out=l1l0_out, host=host, seq=seq)
    with _span("G3_dacts"):
        if ws.tr:
            ops.dacts_bwd_t(ws.g_recon[r0:r1], P.W_dec_hk, ws.acts[r0:r1], ws.tn, l1_scale, ws.g_pre_t[:, r0:r1],
                            colsum_part=ws.gpre_colpart[c0:c1], mask_bits=ops.mask_bits_rows(ws.mask_bits, ws.h, r0, r1),
                            tile_ctr=_tile_ctr(ws, 1), tail=tail)
        else:
            mask = ws.acts if ws.jumprelu is None else ws.gate
            ops.dacts_bwd(ws.g_recon[r0:r1], P.W_dec_hk, mask[r0:r1], ws.tn, l1_scale, ws.g_pre[r0:r1],
                          colsum_part=ws.gpre_colpart[c0:c1])


def _wgrad_operands(ws, P, G, l1_scale, tr):
    """ops.wgrad_both*'s weight-gradient operands (through n, d) for this workspace: the transposed batch operands
    (tr) or the batch-major ones"""
    batch = (ws.acts_t, ws.g_recon_t, ws.g_pre_t, ws.x_t) if tr else (ws.acts, ws.g_recon, ws.g_pre, ws.x)
    return (*batch[:2], P.W_dec_hk, ws.inv_norms, ws.colsum_acts, l1_scale, G.W_dec_hk, ws.sq_slice(1), *batch[2:],
            G.W_enc_hk, ws.sq_slice(0), ws.n, ws.d)


def _bias_operands(ws, G, gpre_colpart):
    """the grad tail's bias operands: the g_pre column-partial slab -> b_enc.grad, the loss's -> b_dec.grad"""
    return gpre_colpart, G.b_enc, ws.sq_slice(2), loss_colpart(ws), G.b_dec_flat, ws.sq_slice(3)


def _bias_grads(ws, G, gpre_colpart, offsets, clip=None, sums_out=None, zero_mask=0, emulate=None):
    """The backward's end after G4 / G5: the bias gradients (+ their sq partials) from the two column-partial slabs,
    with -- sums_out -- the per-parameter squared sums or -- clip -- clip_grad_norm_'s coefficient (then ws.clip_ready)
    in the same launch; neither: the two reductions alone.  offsets: the segments of ws.sq the sums / the clip cover;
    emulate: the clip's emulate_bf16 (default: torch's roundings for a bf16 crosscoder's four parameters)."""
    bias = _bias_operands(ws, G, gpre_colpart)
    if sums_out is not None:
        ops.grad_tail_sums(*bias, ws.sq, offsets, sums_out, ws.tail_ctr[1:2], zero_mask=zero_mask)
    elif clip is not None:
        ops.grad_tail(*bias, ws.sq, offsets, clip, ws.dtype == torch.bfloat16 if emulate is None else emulate,
                      ws.clip_out, ws.tail_ctr[1:2])
        ws.clip_ready = True
    else:
        ops.reduce_rows(gpre_colpart, gpre_colpart.shape[0], ws.h, out_t=G.b_enc, sq_part=ws.sq_slice(2))
        ops.reduce_rows(loss_colpart(ws), ws.loss_col_rows, ws.K, out_t=G.b_dec_flat, sq_part=ws.sq_slice(3))


def backward(ws, P, G, l1_coeff, l1_grad_weight=1.0, dacts_done=False, clip=None, sums_out=None, zero_mask=0,
             tail_done=None, l0_coeff=0.0, theta_grad=None):
    """Gradients of l2 + l1_coeff * l1 into the grads Arena G (+ squared-sum partials).
    dacts_done: G3 already ran per batch slice (dacts_rows).  tail_done: the event of a loss tail
    running beside (loss_finalize_beside), waited for before G4.  clip (max_norm, single-GPU step): the
    bias-gradient sums and clip_grad_norm_'s coefficient in one launch (clip_and_adam then skips
    its clip_finalize).  sums_out (latent-sharded step): instead, the per-parameter squared sums in
    the same launch (segment_sums semantics, zero_mask), for the all-reduce.
    A jumprelu workspace: backward_jumprelu (l0_coeff, theta_grad: its arguments)."""
    if ws.jumprelu is not None:
        if dacts_done or sums_out is not None or l1_grad_weight != 1.0:
            raise ValueError("the JumpReLU step has no sliced or sharded form")
        return backward_jumprelu(ws, P, G, l1_coeff, l0_coeff, theta_grad, clip, tail_done)
    l1_scale = float(l1_coeff) * l1_grad_weight / ws.B
    # (a deferred decoder-half Adam launch of the last step reads the clip coefficient this launch rewrites)
    P.wait_pending()
    if not dacts_done:
        dacts_rows(ws, P, l1_coeff, 0, ws.B, l1_grad_weight)
    if tail_done is not None:
        tail_done.wait(torch.cuda.current_stream(ws.x.device))
    wgrad = _wgrad_operands(ws, P, G, l1_scale, ws.tr)
    abort_ptr = ws.wait_err.device_ptr if ws.wait_err is not None else None
    if sums_out is not None and ws.tr:
        # G4 + G5 and the grad tail's per-parameter squared sums (for the all-reduce) in one launch
        with _span("G4G5_wgrad"):
            ops.wgrad_both_sums_t(*wgrad, *_bias_operands(ws, G, ws.gpre_colpart), ws.sq, ws.sq_off, sums_out,
                                  ws.tail_ctr[1:2], ws.tile_sum, zero_mask=zero_mask, tile_ctr=_tile_ctr(ws, 2),
                                  abort_ptr=abort_ptr)
        return
    if clip is not None and ws.tr:
        # G4 + G5 and the grad tail (bias sums + clip coefficient) in one launch
        with _span("G4G5_wgrad"):
            ops.wgrad_both_clip_t(*wgrad, *_bias_operands(ws, G, ws.gpre_colpart), ws.sq, ws.sq_off, clip,
                                  ws.dtype == torch.bfloat16, ws.clip_out, ws.tail_ctr[1:2], ws.tile_sum,
                                  tile_ctr=_tile_ctr(ws, 2), abort_ptr=abort_ptr)
        ws.clip_ready = True
        return
    with _span("G4G5_wgrad"):
        (ops.wgrad_both_t if ws.tr else ops.wgrad_both)(*wgrad)
    _bias_grads(ws, G, ws.gpre_colpart, ws.sq_off, clip, sums_out, zero_mask)


def backward_jumprelu(ws, P, G, l1_coeff, l0_coeff=0.0, theta_grad=None, clip=None, tail_done=None):
    """backward() of the batch-major step of a JumpReLU crosscoder, for l2 + l1_coeff l1 + l0_coeff l0: G3 with the gate
    as its mask operand (it leaves dL/d acts at the kept elements and in the lower half of the window); one pass
    (cc_jumprelu_bwd) that forms the threshold gradient's partials from the window, zeroes g_pre where gated but not
    kept and recomputes g_pre's column partials; the reduce that gives theta_grad (fp32 [h]) and segment 4 of ws.sq;
    then G4G5 and the grad tail as always, the tail over the recomputed column partials and -- theta_grad given --
    five parameters.  theta_grad None (get_losses' autograd, which serves the four reference parameters): the pass
    only restores the straight-through g_pre, and the clip is over four."""
    B, h = ws.B, ws.h
    l1_scale = float(l1_coeff) / B
    P.wait_pending()
    dacts_rows(ws, P, l1_coeff, 0, B)
    with _span("jumprelu_bwd"):
        ops.jumprelu_bwd(ws.g_pre, ws.gate, h, ws.theta, ws.jumprelu, float(l0_coeff) / B,
                         gpre_colsum_part=ws.jr_gpre_colpart, thr_part=ws.thr_part if theta_grad is not None else None)
    if theta_grad is not None:
        with _span("theta_grad"):
            ops.reduce_rows(ws.thr_part, ws.thr_part.shape[0], h, out_t=theta_grad, sq_part=ws.sq_slice(4))
    if tail_done is not None:
        tail_done.wait(torch.cuda.current_stream(ws.x.device))
    with _span("G4G5_wgrad"):
        ops.wgrad_both(*_wgrad_operands(ws, P, G, l1_scale, False))
    off = ws.sq_off if theta_grad is not None else ws.sq_off[:5]
    _bias_grads(ws, G, ws.jr_gpre_colpart, off, clip, emulate=clip_emulation(ws, len(off) - 1))


def clip_emulation(ws, nparams=4):
    """clip_finalize / grad_tail's emulate_bf16 for this workspace: torch's bf16 roundings for a bf16 crosscoder's four
    parameters; with the fp32 threshold as a fifth, torch's arithmetic on that mixed list (bf16 norms of the four,
    fp32 total and coefficient)."""
    if ws.dtype != torch.bfloat16:
        return 0
    return ops.CLIP_EMULATE_MIXED if nparams > 4 else 1


def auxk_forward(ws, P, since_fired, h_real, dead_after, auxk_coeff, active, host=None):
    """The AuxK part of the forward, after G2 and the loss rows (the step's column sums ws.colsum_acts exist) and
    before the loss tail is forked: the dead update (always; the dead count also into word 10 of `host`, a
    _hip.MappedHostBuffer), then -- active: forward(aux=...) selected the aux activations -- the aux decode
    e^ = aux_acts . W_dec and the aux loss with g_aux (auxk_loss also into word 9 of `host`)."""
    word = (lambda i: host.device_ptr.value + 4 * i) if host is not None else (lambda i: None)
    with _span("dead_update"):
        ops.dead_update(ws.colsum_acts, since_fired, h_real, ws.B, dead_after, ws.dead_count, was_dead=ws.was_dead,
                        host_ptr=word(10))
    ws.aux_active = bool(active)
    if not active:
        return
    with _span("auxk_decode"):
        # (cc_decode_fwd(aux_acts, W_dec, NULL, e^) in the main G2's whole-wave / split-K schedule; its workspace is free)
        ops.decode_partial(ws.aux_acts, P.W_dec_hk, ws.ehat, ws.dec_ws)
    with _span("auxk_loss"):
        ops.auxk_loss(ws.recon, P.b_dec_flat, ws.x, ws.ehat, ws.g_aux, ws.auxk_part, ws.auxk_scalars, auxk_coeff,
                      host_ptr=word(9))


def backward_auxk(ws, P, G, l1_coeff, clip):
    """backward(clip=...) of the batch-major step with the aux rows of an active AuxK step: G3 on the main rows as
    always, G3 on the aux rows (no L1 term) into the bottom halves, the aux half of g_pre folded into the main half,
    G4 over the 2 B concatenated rows (acts^T g_recon + aux_acts^T g_aux; the L1 term from the main column sums), G5
    over the folded rows, and the grad tail over both halves of the g_pre column-partial slab."""
    B, n, d = ws.B, ws.n, ws.d
    l1_scale = float(l1_coeff) / B
    P.wait_pending()
    dacts_rows(ws, P, l1_coeff, 0, B)
    with _span("G3_dacts_aux"):
        ops.dacts_bwd(ws.g_aux, P.W_dec_hk, ws.aux_acts, ws.tn, 0.0, ws.g_pre_aux, colsum_part=ws.gpre_colpart_aux)
    with _span("add_rows"):
        ops.add_rows(ws.g_pre, ws.g_pre_aux)
    with _span("G4_wgrad_dec"):
        ops.wgrad_dec(ws.acts_full, ws.g_recon_full, P.W_dec_hk, ws.inv_norms, ws.colsum_acts, l1_scale, G.W_dec_hk,
                      ws.sq_slice(1), n, d)
    with _span("G5_wgrad_enc"):
        ops.wgrad_enc(ws.g_pre, ws.x, G.W_enc_hk, ws.sq_slice(0))
    _bias_grads(ws, G, ws.gpre_colpart_full, ws.sq_off, clip)


# workgroups of the decoder-half Adam that runs beside the next step's G1 (128 / 192 / 384 / 512 measured
# slower)
DEC_ADAM_BLOCKS = 256
# share of W_dec's rows whose Adam update runs on the side stream beside the next step's G1; the rest (and
# b_dec) runs on the main stream after G1 with the whole chip.  Beside G1 the
# side launch gets one wave per SIMD (G1 holds the rest of the register file), which streams slowly once
# G1 has finished.  Since the bf16 update's instruction count was cut by about 40 % the side launch ends well
# before G1, so deferring rows no longer pays: 1.0 measured fastest of 0.92 / 0.96 / 1.0.
DEC_SIDE_ROWS = 1.0
# False: the decoder half's Adam runs on torch's stream right after the encoder half, with the whole chip (no side
# stream, nothing deferred) -- the alternative DESIGN.md section 3.3 measures against the overlap with G1
DEC_ADAM_BESIDE_G1 = True
SERIAL_DEC_BLOCKS = 0  # (0: the library's default grid for the serial form)


def clip_and_adam(ws, P, G, M, V, lr, beta1, beta2, eps, step, max_norm=1.0, side_stream=None, extra=None,
                  next_batch=None, master=None):
    """clip_grad_norm_ (from the squared-sum slabs of the backward) + Adam (see adam())."""
    emulate = clip_emulation(ws, len(ws.sq_off) - 1)
    if not ws.clip_ready:
        ops.clip_finalize(ws.sq, ws.sq_off, max_norm, emulate, ws.clip_out)
    ws.clip_ready = False
    adam(ws, P, G, M, V, lr, beta1, beta2, eps, step, side_stream, extra=extra, next_batch=next_batch, master=master)


def _adam_master(ws, P, G, M, V, master, hp, side_stream, clip_sums):
    """adam()'s launch with fp32 master weights (cc_adam_master_step): `master`, M and V are fp32 arenas, G the bf16
    gradients, and P, the bf16 arena the GEMMs read, receives the rounded masters.  One launch over the whole arena
    on torch's stream, then the next step's decoder norms (/ W_dec^T) from the rounded W_dec on the same stream;
    nothing is pending afterwards.  The side stream is not used: with the decoder half on it, ordered for its readers
    by an event as in adam()'s last branch, a snapshot taken after Trainer.synchronize() intermittently held the
    decoder half from before the update (DESIGN.md sections 3.16 and 3.7; the cause is not found).  No prep ride:
    the next forward preps."""
    if clip_sums is not None:
        raise ValueError("master weights take the step's own coefficient")
    ws.prep_token = None
    with _span("adam"):
        ops.adam_master_step(master.data, G.data, M.data, V.data, P.data, *hp)
    if side_stream is not None:  # (the Trainer's step: the standalone form leaves the norms to the next forward)
        norms_for_next(ws, P)


def adam(ws, P, G, M, V, lr, beta1, beta2, eps, step, side_stream=None, clip_sums=None, extra=None,
         next_batch=None, master=None):
    """Adam with the clip coefficient in ws.clip_out[0] -- or, clip_sums (sums [4], max_norm): formed in each
    launch from the per-parameter squared gradient sums (cc_adam_step_clip; the encoder-half launch also writes
    ws.clip_out), so no clip launch sits between the sums' all-reduce and Adam.  side_stream: the encoder half runs on torch's
    stream, then the decoder half (+ the next step's decoder norms / W_dec^T) on the side stream, so it
    overlaps the next step's prep / encoder GEMM (G1 reads only the encoder half); P.pending orders every
    later decoder-half use (forward() waits before G2; CrossCoder's accessors, FusedAdam.state and
    Trainer.synchronize() wait).  Without a side stream: one launch over the whole arena.
    extra ((p, g, m, v), fp32 flat tensors: a JumpReLU crosscoder's thresholds): one more cc_adam_step launch with the
    same coefficient and hyper-parameters, on torch's stream before anything else.
    next_batch ((x_in, factor, tag), with a side stream): the raw batch the next forward(ws, ..., prep_tag=tag) will most
    likely be handed, unchanged until then; where the shapes allow, its prep rides in the encoder half's launch
    (PREP_IN_ADAM) and that forward launches none.  A forward handed anything else runs its prep as always.
    master (an fp32 Arena, with fp32 M and V; a bf16 P): the master-weight update instead (_adam_master)."""
    P.wait_pending()  # (no deferred rows of an earlier step may read this step's coefficient)
    P.updates += 1
    coef = ws.clip_out[0:1]
    emulate = ws.dtype == torch.bfloat16
    if extra is not None:
        if clip_sums is not None:
            raise ValueError("extra parameters take the step's own coefficient")
        with _span("adam_theta"):
            ops.adam_step(*extra, coef, lr, beta1, beta2, eps, step)

    def step_(p, g, m, v, max_blocks=0, clip_out=None):
        if clip_sums is None:
            ops.adam_step(p, g, m, v, coef, lr, beta1, beta2, eps, step, max_blocks=max_blocks)
        else:
            ops.adam_step_clip(p, g, m, v, clip_sums[0], clip_sums[1], emulate, lr, beta1, beta2, eps, step,
                               max_blocks=max_blocks, clip_out=clip_out)

    if master is not None:
        _adam_master(ws, P, G, M, V, master, (coef, lr, beta1, beta2, eps, step), side_stream, clip_sums)
        return
    if side_stream is None:
        with _span("adam"):
            step_(P.data, G.data, M.data, V.data, clip_out=ws.clip_out)
        return
    dev = P.data.device
    enc = [A.enc_part() for A in (P, G, M, V)]
    ride = None
    if (PREP_IN_ADAM and next_batch is not None and clip_sums is None and enc[0].numel() % 8 == 0
            and tuple(next_batch[0].shape) == (ws.B, ws.n, ws.d) and next_batch[0].device == dev
            and ops.prep_job_ok(next_batch[0], next_batch[1], ws.dtype, ws.x_t)):
        ride = _prep_token(*next_batch)
    with _span("adam"):
        if ride is not None:
            # (into the second set of prep outputs, whose last readers -- the step before this one -- are long done)
            if ws.x_next is None:
                ws.x_next = tuple(torch.empty_like(t) for t in (ws.x, ws.x_t, ws.x_colpart))
            ops.adam_step_prep(*enc, coef, lr, beta1, beta2, eps, step,
                               ops.prep_job(next_batch[0], next_batch[1], ws.x_next[0], ws.x_next[2], ws.x_next[1]))
        else:
            step_(*enc, clip_out=ws.clip_out)
    ws.prep_token = ride
    if not DEC_ADAM_BESIDE_G1 and ws.W_dec_t is None and ws.norm_part is not None:
        # serial: the decoder half (+ the next step's norm partials) on this stream, the whole chip
        dec = [A.dec_part() for A in (P, G, M, V)]
        with _span("adam_dec"):
            ops.adam_dec_norms(*dec, ws.h, ws.K, lr, beta1, beta2, eps, step, ws.norm_part,
                               coef=coef if clip_sums is None else None, clip_sums=clip_sums, emulate=emulate,
                               max_blocks=SERIAL_DEC_BLOCKS)
        ws.norms_token = _norms_token(P)
        ws.norms_fin_pending = True
        return
    # both halves are HBM-bound: the decoder half starts after the encoder half (run together they only
    # share the bandwidth), i.e. beside the next step's prep / G1 on the main stream
    enc_done = _hip.DeviceEvent().record(torch.cuda.current_stream(dev))
    ws.fork_events[1] = enc_done
    with torch.cuda.stream(side_stream):
        enc_done.wait(side_stream)
        if ws.W_dec_t is None and ws.norm_part is not None:
            # the decoder norms' partials come out of the Adam launches themselves (no pass over W_dec of their
            # own).  The side stream updates the first hs rows of W_dec beside the next step's G1; the first
            # reader of the params (the next forward, after G1) launches the rest on its stream, waits for the
            # side part and forms the norms (P.pending_rest)
            K, nblk = ws.K, ws.K // 64
            hs = min(ws.h, int(ws.h * DEC_SIDE_ROWS) // 8 * 8)
            dec = [A.dec_part() for A in (P, G, M, V)]
            # (every row on the side stream: b_dec, the decoder half's trailing elements, goes along -- no norm
            # partials for them)
            side_bias = BDEC_IN_SIDE_ADAM and hs == ws.h
            side_part = dec if side_bias else [t[:hs * K] for t in dec]
            kw = dict(coef=coef if clip_sums is None else None, clip_sums=clip_sums, emulate=emulate)
            hp = (lr, beta1, beta2, eps, step)
            target = None
            if hs > 0:
                with _span("adam_dec"):
                    nb = ops.adam_dec_norms(*side_part, hs, K, *hp, ws.norm_part[:hs * nblk],
                                            max_blocks=DEC_ADAM_BLOCKS, done_ctr=ws.adam_done, **kw)
                ws.adam_done_target = (ws.adam_done_target + nb) & 0xFFFFFFFF
                target = ws.adam_done_target
            done = _hip.DeviceEvent().record(side_stream)

            def rest(kernel_wait=False):
                # the rows on the reader's stream, then it waits for the side stream's rows; the norm partials are
                # then complete, and the finaliser rides in the next G2 launch (decode_loss: G3 and the loss tail,
                # its first readers, run after G2) or runs before the first other reader (flush_norms).
                # kernel_wait (the reader is that G2 launch): G2 waits for the side stream's rows in its kernel
                # (returns the done counter and its target; P.pending keeps the event for other streams' readers)
                cur = torch.cuda.current_stream(dev)
                if not side_bias:
                    with _span("adam_dec_rest"):
                        if ws.h > hs:
                            ops.adam_dec_norms(*(t[hs * K:] for t in dec), ws.h - hs, K, *hp, ws.norm_part[hs * nblk:],
                                               **kw)
                        else:  # (every row on the side stream: b_dec only)
                            step_(*(t[hs * K:] for t in dec))
                ws.norms_fin_pending = True
                if kernel_wait and target is not None:
                    P.pending = done
                    return ws.adam_done, target
                done.wait(cur)
                return None

            ws.norms_token = _norms_token(P)
            P.pending_rest = rest
            P.pending = None
            return
        else:
            with _span("adam_dec"):
                step_(P.dec_part(), G.dec_part(), M.dec_part(), V.dec_part(), max_blocks=DEC_ADAM_BLOCKS)
            norms_for_next(ws, P)
            done = _hip.DeviceEvent().record(side_stream)
    P.pending = done
