"""Drop-in `CrossCoder` (reference: crosscoder.py:24-217) running on gfx950 HIP kernels.

Same constructor cfg, same parameter names / shapes / dtypes / strides, same state_dict and
checkpoint format, same `encode / decode / forward / get_losses / save / load` surface.
The parameters are views of one flat HBM arena (engine.Arena) so the fused Adam can update
all of them in one launch; `W_enc` keeps the reference's h-major strides (d, 1, n*d).
"""
import json
import pprint
import weakref
from collections import OrderedDict
from pathlib import Path
from typing import NamedTuple, Optional, Union

import torch
from torch import nn

from . import engine, ops

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SAVE_DIR = Path("./checkpoints")


class LossOutput(NamedTuple):
    l2_loss: torch.Tensor
    l1_loss: torch.Tensor
    l0_loss: torch.Tensor
    explained_variance: torch.Tensor
    explained_variance_A: torch.Tensor
    explained_variance_B: torch.Tensor


def reference_init(cfg, n_models=2):
    """Bit-exact restatement of the reference initialisation (crosscoder.py:31-62) on the CPU
    generator: seed, W_dec drawn twice (the second draw wins), per-(h, model) rows scaled to
    dec_init_norm, W_enc = rearranged clone (same values), zero biases."""
    dtype = DTYPES[cfg["enc_dtype"]]
    h, d = cfg["dict_size"], cfg["d_in"]
    torch.manual_seed(cfg["seed"])
    _ = torch.empty(n_models, d, h, dtype=dtype)  # W_enc placeholder (no RNG use)
    torch.nn.init.normal_(torch.empty(h, n_models, d, dtype=dtype))  # first draw, discarded
    W_dec = torch.nn.init.normal_(torch.empty(h, n_models, d, dtype=dtype))
    W_dec = W_dec / W_dec.norm(dim=-1, keepdim=True) * cfg["dec_init_norm"]
    return W_dec


def write_checkpoint(state_dict, cfg, save_dir=None, version=0):
    """crosscoder.py:132-146's two-file format: {save_dir}/{version}.pt (state_dict) + {version}_cfg.json,
    save_dir = ./checkpoints/version_N (next free N) when None.  Returns (save_dir, version + 1)."""
    if save_dir is None:
        SAVE_DIR.mkdir(parents=True, exist_ok=True)
        versions = [int(f.name.split("_")[1]) for f in SAVE_DIR.iterdir() if "version" in str(f)]
        save_dir = SAVE_DIR / f"version_{1 + max(versions) if versions else 0}"
        save_dir.mkdir(parents=True)
    torch.save(state_dict, save_dir / f"{version}.pt")
    with open(save_dir / f"{version}_cfg.json", "w") as f:
        json.dump(cfg, f)
    print(f"Saved as version {version} in {save_dir}")
    return save_dir, version + 1


ACTIVATIONS = ("relu", "topk", "batch_topk", "jumprelu")
TOPK_WEIGHTS = ("decoder_norm", "none")


def activation_of(cfg):
    """(activation, k) of a cfg (framework extension; the keys travel in the checkpoint's cfg json): "relu", the
    reference's and the default, or "topk" -- each row keeps its cfg["k"] largest positive pre-activations
    (ties: the smaller latent), the rest are zero -- which needs cfg["k"], an int in 1..dict_size; or "batch_topk"
    -- the batch keeps its rows * cfg["k"] best (row, latent) pairs, so k is the mean number kept per row -- with
    the optional keys of batch_topk_options; or "jumprelu" -- an activation is kept iff it exceeds its latent's
    learned threshold -- with the keys of jumprelu_options (no k)."""
    act = cfg.get("activation", "relu")
    if act not in ACTIVATIONS:
        raise ValueError(f"cfg['activation'] must be one of {ACTIVATIONS}, got {act!r}")
    if act == "relu":
        return act, None
    if act == "jumprelu":
        jumprelu_options(cfg)
        return act, None
    k = cfg.get("k")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= cfg["dict_size"]:
        raise ValueError(f"activation {act!r} needs cfg['k'], an int in 1..dict_size ({cfg['dict_size']}), got {k!r}")
    if act == "batch_topk":
        batch_topk_options(cfg)
    return act, k


def batch_topk_options(cfg):
    """(topk_weight, threshold_beta) of a "batch_topk" cfg: cfg["topk_weight"], "decoder_norm" (the default: a
    pair's score is its activation times the latent's summed per-model decoder norms, the weight of the L1 term) or
    "none" (the activation itself); cfg["threshold_beta"], a float in [0, 1), default 0.999: the decay of the
    running mean of the training batches' threshold scores that serves inference (CrossCoder.threshold)."""
    weight = cfg.get("topk_weight", "decoder_norm")
    if weight not in TOPK_WEIGHTS:
        raise ValueError(f"cfg['topk_weight'] must be one of {TOPK_WEIGHTS}, got {weight!r}")
    beta = cfg.get("threshold_beta", 0.999)
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0 <= beta < 1:
        raise ValueError(f"cfg['threshold_beta'] must be a float in [0, 1), got {beta!r}")
    return weight, float(beta)


def _finite_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and abs(v) != float("inf")


def jumprelu_options(cfg):
    """(l0_coeff, jump_bandwidth, jump_threshold_init) of a "jumprelu" cfg: cfg["l0_coeff"], required, a finite float
    >= 0: the weight of the L0 penalty (the mean number of kept activations per row) in the objective
    l2 + l1_coeff l1 + l0_coeff l0, warmed up like l1_coeff; cfg["jump_bandwidth"], a finite float > 0 (default 1e-3):
    the width eps of the straight-through estimators' window around each threshold; cfg["jump_threshold_init"], a
    finite float (default 1e-3): every latent's threshold at construction (<= 0: that latent starts as plain ReLU)."""
    if "l0_coeff" not in cfg:
        raise ValueError("activation 'jumprelu' needs cfg['l0_coeff'], a float >= 0: the weight of its L0 penalty")
    l0c = cfg["l0_coeff"]
    if not _finite_number(l0c) or l0c < 0:
        raise ValueError(f"cfg['l0_coeff'] must be a finite float >= 0, got {l0c!r}")
    eps = cfg.get("jump_bandwidth", 1e-3)
    if not _finite_number(eps) or not eps > 0 or not float(torch.tensor(eps, dtype=torch.float32)) > 0:
        raise ValueError(f"cfg['jump_bandwidth'] must be a finite float > 0 (in fp32), got {eps!r}")
    init = cfg.get("jump_threshold_init", 1e-3)
    if not _finite_number(init):
        raise ValueError(f"cfg['jump_threshold_init'] must be a finite float, got {init!r}")
    return float(l0c), float(eps), float(init)


def auxk_options(cfg, n_models=2):
    """(auxk_coeff, k_aux, dead_tokens) of a cfg, or None when the AuxK dead-latent loss is off (framework extension;
    the keys travel in the checkpoint's cfg json).  cfg["auxk_coeff"]: a float >= 0, absent or 0: off.  On, it needs
    activation "topk" or "batch_topk" and takes cfg["k_aux"], an int in 1..dict_size (default
    min(dict_size, max(1, n_models * d_in // 2))): how many dead latents per row reconstruct the residual; and
    cfg["dead_tokens"], an int >= 1 (default 10 000 000): a latent is dead once it has not fired for that many
    tokens."""
    coeff = cfg.get("auxk_coeff", 0)
    if isinstance(coeff, bool) or not isinstance(coeff, (int, float)) or not coeff >= 0 or coeff == float("inf"):
        raise ValueError(f"cfg['auxk_coeff'] must be a finite float >= 0, got {coeff!r}")
    if coeff == 0:
        return None
    if cfg.get("activation", "relu") == "relu":
        raise ValueError("cfg['auxk_coeff'] > 0 needs activation 'topk' or 'batch_topk': a ReLU crosscoder's latents "
                         "get gradient whenever they are positive")
    if cfg.get("activation", "relu") == "jumprelu":
        raise ValueError("cfg['auxk_coeff'] > 0 is not served with activation 'jumprelu': the aux rows would need a "
                         "threshold gradient of their own, and a JumpReLU latent is revived by its threshold falling; "
                         "use 'topk' or 'batch_topk'")
    h = cfg["dict_size"]
    k_aux = cfg.get("k_aux", min(h, max(1, n_models * cfg["d_in"] // 2)))
    if isinstance(k_aux, bool) or not isinstance(k_aux, int) or not 1 <= k_aux <= h:
        raise ValueError(f"cfg['k_aux'] must be an int in 1..dict_size ({h}), got {k_aux!r}")
    dead = cfg.get("dead_tokens", 10_000_000)
    if isinstance(dead, bool) or not isinstance(dead, int) or dead < 1:
        raise ValueError(f"cfg['dead_tokens'] must be an int >= 1, got {dead!r}")
    return float(coeff), k_aux, dead


def master_weights_of(cfg):
    """cfg["master_weights"] (framework extension; the key travels in the checkpoint's cfg json): a bool, absent or
    False: off.  True on a bf16 crosscoder: Trainer keeps fp32 master weights and fp32 Adam moments, and the bf16
    parameters are the masters rounded after every update.  On an fp32 crosscoder it changes
    nothing: the parameters are their own masters."""
    mw = cfg.get("master_weights", False)
    if not isinstance(mw, bool):
        raise ValueError(f"cfg['master_weights'] must be a bool, got {mw!r}")
    return mw


def sparse_step_of(cfg):
    """cfg["sparse_step"] (framework extension; the key travels in the checkpoint's cfg json): a bool, absent or False:
    off.  True needs activation "topk": Trainer.step then runs its decode and its whole backward on the k (value,
    latent) pairs per row instead of the masked dense activations.  It changes Trainer.step
    only: encode, decode, forward and get_losses are the dense code either way."""
    sp = cfg.get("sparse_step", False)
    if not isinstance(sp, bool):
        raise ValueError(f"cfg['sparse_step'] must be a bool, got {sp!r}")
    if sp and cfg.get("activation", "relu") != "topk":
        raise ValueError(f"cfg['sparse_step'] needs activation 'topk' (k pairs per row), got "
                         f"{cfg.get('activation', 'relu')!r}")
    return sp


def auxk_compact_of(cfg):
    """cfg["auxk_compact"] (framework extension; the key travels in the checkpoint's cfg json): a bool, absent or False:
    off.  True needs cfg["auxk_coeff"] > 0 and cfg["sparse_step"]: Trainer.step then serves the AuxK loss under the
    sparse step, running the aux GEMMs over the compacted dead set instead of the whole dictionary (DESIGN.md section
    3.22).  The dense TopK / BatchTopK step's AuxK is unchanged and does not take the key."""
    ac = cfg.get("auxk_compact", False)
    if not isinstance(ac, bool):
        raise ValueError(f"cfg['auxk_compact'] must be a bool, got {ac!r}")
    coeff = cfg.get("auxk_coeff", 0)
    if ac and not (isinstance(coeff, (int, float)) and not isinstance(coeff, bool) and coeff > 0):
        raise ValueError("cfg['auxk_compact'] needs cfg['auxk_coeff'] > 0: there is no aux loss to compact")
    if ac and not cfg.get("sparse_step", False):
        raise ValueError("cfg['auxk_compact'] needs cfg['sparse_step']: the compacted aux path is built for the sparse "
                         "step only")
    return ac


class CrossCoder(nn.Module):
    def __init__(self, cfg, n_models: Optional[int] = None, init_W_dec: Optional[torch.Tensor] = None):
        """init_W_dec (framework extension): start from this decoder ([h, n, d], W_enc = its rearranged
        copy, zero biases) instead of the seeded reference draw -- the latent-sharded trainer passes
        its slice of the full dictionary's reference init."""
        super().__init__()
        self.cfg = cfg
        d_hidden = cfg["dict_size"]
        self.activation, self.k = activation_of(cfg)
        d_in = cfg["d_in"]
        self.n_models = int(n_models if n_models is not None else cfg.get("n_models", 2))
        self.auxk = auxk_options(cfg, self.n_models)  # (auxk_coeff, k_aux, dead_tokens) or None: Trainer.step's
        master_weights_of(cfg)  # (validated here; Trainer's optimizer is what it switches)
        sparse_step_of(cfg)  # (validated here; Trainer.step is what it switches)
        auxk_compact_of(cfg)  # (likewise; after auxk_options and sparse_step_of, whose own errors come first)
        self.dtype = DTYPES[cfg["enc_dtype"]]
        if self.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("crosscoder_amd kernels support enc_dtype 'bf16' and 'fp32'")
        device = torch.device(cfg["device"])
        W_dec = reference_init(cfg, self.n_models) if init_W_dec is None else init_W_dec.to(self.dtype)
        # kernel dims: dict_size / d_in rounded up to multiples of 8 (zero padding latents / columns that
        # stay zero, engine.padded_dims); the parameters are the reference-shaped views
        self._hp, self._dp = engine.padded_dims(d_hidden, d_in)
        self._arena = engine.Arena(self._hp, self.n_models, self._dp, self.dtype, device, ref=(d_hidden, d_in))
        with torch.no_grad():
            self._arena.W_dec().copy_(W_dec)
            self._arena.W_enc().copy_(W_dec.permute(1, 2, 0))
        self._bind_params()
        if self.activation == "batch_topk":
            self.topk_weight, self.threshold_beta = batch_topk_options(cfg)
            # the inference threshold on the score: the running mean of the training batches' threshold scores
            # (Trainer.step); -1: unset.  Saved and loaded with the state dict (BatchTopK crosscoders only)
            self.register_buffer("threshold", torch.tensor(-1.0, dtype=torch.float32, device=device))
        if self.activation == "jumprelu":
            # one learned fp32 threshold per latent (JumpReLU crosscoders only: the other activations' state dicts keep
            # their keys); the kernels read the kernel-h buffer, whose padding latents never fire
            self.l0_coeff, self.jump_bandwidth, init = jumprelu_options(cfg)
            self._theta_buf = torch.zeros(self._hp, dtype=torch.float32, device=device)
            self._theta_buf[:d_hidden] = init
            self.jump_threshold = nn.Parameter(self._theta_buf[:d_hidden])
        self._thr_set = None  # (threshold's version when it was read as set): encode then skips the host read
        self._sel_w = None  # (key, tensor): the selection weights of the W_dec they were computed from
        self.d_hidden = d_hidden
        self.save_dir = None
        self.save_version = 0
        self._ws = None

    # ------------------------------------------------------------------ arena plumbing
    def _bind_params(self):
        v = self._arena.views()
        self.W_enc = nn.Parameter(v["W_enc"])
        self.W_dec = nn.Parameter(v["W_dec"])
        self.b_enc = nn.Parameter(v["b_enc"])
        self.b_dec = nn.Parameter(v["b_dec"])

    # The Trainer runs the decoder half of Adam on a side stream (engine.adam); every public way to
    # reach the parameters orders torch's current stream after it first (a stream wait, no host sync):
    # attribute access to W_dec / b_dec, parameters() / named_parameters(), state_dict(), .to() and
    # friends (_apply), the arena re-pack, and the optimizer's state.  The step itself reaches the
    # params through the arena only, so it keeps the overlap.
    _SIDE_UPDATED = ("W_dec", "b_dec")

    def _sync_pending(self):
        a = self.__dict__.get("_arena")
        if a is not None:
            a.wait_pending()

    def __getattr__(self, name):
        if name in CrossCoder._SIDE_UPDATED:
            self._sync_pending()
        return super().__getattr__(name)

    def named_parameters(self, *args, **kwargs):
        self._sync_pending()
        return super().named_parameters(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._sync_pending()
        return super()._apply(fn, *args, **kwargs)

    def _arena_ok(self):
        a = self._arena
        v = a.views()
        for name in ("W_enc", "W_dec", "b_enc", "b_dec"):
            p = self._parameters[name]
            if p.data_ptr() != v[name].data_ptr() or p.stride() != v[name].stride() or p.device != a.data.device:
                return False
        return True

    def arena(self):
        """The flat parameter arena; re-packs the params if something (e.g. .to()) replaced them."""
        if not self._arena_ok():
            self._arena.wait_pending()  # the old arena's decoder half may still be written
            prm = self._parameters
            dev = prm["W_dec"].device
            new = engine.Arena(self._hp, self.n_models, self._dp, self.dtype, dev, ref=(self.d_hidden, self.cfg["d_in"]))
            with torch.no_grad():
                for name, dst in new.views().items():
                    dst.copy_(prm[name].data)
            self._arena = new
            grads = {n: prm[n].grad for n in ("W_enc", "W_dec", "b_enc", "b_dec")}
            self._bind_params()
            for n, g in grads.items():
                self._parameters[n].grad = g
            self._ws = None
        return self._arena

    def params_written(self):
        """Tell the crosscoder that its parameters were written in a way torch's version counters do not show: by a
        kernel (fold_activation_scaling_factor and LatentResampler call this themselves), or in place through
        `param.data` / a raw pointer.  Orders torch's current stream after pending Adam work on the side stream
        (launching its deferred rows), and counts the write in Arena.updates, which everything carried from the
        parameters is keyed on: the decoder norms, norm partials and W_dec^T of every step workspace on the arena (the
        crosscoder's, a Trainer's sparse one, a ShardedTrainer's), BatchTopK's selection weights and, in master mode,
        the fp32 masters, which are re-seeded where they no longer round to their parameter.  The next forward
        re-derives all of it.  Call it after the write and before the next step, get_losses or encode; a writer on
        another stream orders itself after `arena().wait_pending()` first.  Returns the crosscoder."""
        a = self.arena()
        a.wait_pending()
        a.updates += 1
        return self

    def theta(self):
        """fp32 [kernel h] on the arena's device: the JumpReLU thresholds as the kernels read them, of which the
        parameter jump_threshold is the first dict_size; re-packed if something (e.g. .to()) replaced the parameter."""
        p, dev = self._parameters["jump_threshold"], self.arena().data.device
        if p.data_ptr() != self._theta_buf.data_ptr() or p.device != dev or p.dtype != torch.float32:
            buf = torch.zeros(self._hp, dtype=torch.float32, device=dev)
            buf[:self.d_hidden] = p.data.to(dev, torch.float32)
            grad = p.grad
            self._theta_buf = buf
            self.jump_threshold = nn.Parameter(buf[:self.d_hidden])
            self._parameters["jump_threshold"].grad = grad
        return self._theta_buf

    def _workspace(self, B, step=False):
        """The cached step workspace for batch size B.  A workspace that a get_losses() graph still
        needs for its backward (ws.busy) is never reused: the next call gets a fresh one, which is
        cached in its place (so a second get_losses() before the first backward cannot overwrite
        the first one's activations)."""
        a = self.arena()
        ws = self._ws
        if (ws is None or ws.B != B or ws.x.device != a.data.device
                or (ws.busy is not None and ws.busy() is not None)):
            ws = engine.StepWorkspace(B, self.n_models, self._dp, self._hp, self.dtype, a.data.device,
                                      topk=self.k if self.activation == "topk" else None,
                                      batch_topk=(self.k, self.topk_weight != "none")
                                      if self.activation == "batch_topk" else None,
                                      auxk=(self.auxk[1],) if self.auxk is not None else None,
                                      jumprelu=self.jump_bandwidth if self.activation == "jumprelu" else None)
            self._ws = ws
        return ws

    def _check_x(self, x):
        if x.dim() != 3 or x.shape[1] != self.n_models or x.shape[2] != self.cfg["d_in"]:
            raise ValueError(f"expected x of shape [batch, {self.n_models}, {self.cfg['d_in']}], got {tuple(x.shape)}")

    def pad_input(self, x):
        """x [batch, n, d_in] -> [batch, n, kernel d] (zero columns appended when d_in % 8 != 0)."""
        return x if self._dp == x.shape[-1] else torch.nn.functional.pad(x, (0, self._dp - x.shape[-1]))

    def _flat_x(self, x):
        self._check_x(x)
        x = self.pad_input(x).contiguous()
        if x.dtype == self.dtype:
            return x.view(x.shape[0], -1)
        return ops.prep_input(x, None, self.dtype)

    # ------------------------------------------------------------------ reference API
    def encode(self, x, apply_relu=True, use_threshold=None):
        """x [batch, n_models, d_model] -> acts [batch, d_hidden] (crosscoder.py:69-80).  use_threshold (BatchTopK
        crosscoders): None -- keep the pairs whose score reaches `threshold` if it is set (>= 0), else the rows * k
        best pairs of the rows given; True -- the threshold (ValueError while it is unset); False -- the rows * k
        best pairs."""
        a = self.arena()
        xf = self._flat_x(x)
        acts = torch.empty(xf.shape[0], self._hp, dtype=self.dtype, device=xf.device)
        ops.encode_fwd(xf, a.W_enc_hk, a.b_enc, acts, apply_relu)
        if apply_relu:
            self.activate_(acts, use_threshold)
        return acts[:, :self.d_hidden].contiguous() if self._hp != self.d_hidden else acts

    def activate_(self, acts, use_threshold=None):
        """The crosscoder's sparsifying activation on acts [rows, kernel h] = relu(pre), in place: nothing (ReLU), each
        row's k largest positive values (TopK; the padding latents are 0), the BatchTopK selection / threshold
        mask under selection_weights() (see encode), or the values above their latent's threshold (JumpReLU)."""
        if self.activation == "jumprelu":
            ops.jumprelu_mask(acts, self._hp, self.theta(), self.jump_bandwidth, out=acts)
        elif self.activation == "topk":
            ops.topk_rows(acts, self._hp, self.k, out=acts)
        elif self.activation == "batch_topk":
            if use_threshold is None:
                use_threshold = self._threshold_is_set()
            elif use_threshold and not self._threshold_is_set():
                raise ValueError("encode(use_threshold=True): the threshold is unset (-1); it is learned by Trainer.step "
                                 "or loaded with a checkpoint")
            w = self._selection_weights() if self.topk_weight != "none" else None
            if use_threshold:
                ops.threshold_mask(acts, self._hp, self.threshold.reshape(1), weight=w, out=acts)
            else:
                ops.batch_topk(acts, self._hp, acts.shape[0] * self.k, weight=w, out=acts)
        return acts

    def _threshold_is_set(self):
        """threshold >= 0.  Read on the host (a device synchronise) until it is seen set; a set threshold stays set
        -- Trainer.step only moves it between positive scores -- unless torch writes the buffer (its version counter
        changes: load_state_dict, fill_, .to()), which reads it again."""
        t = self.threshold
        key = (t.data_ptr(), t._version)
        if self._thr_set != key:
            if not float(t) >= 0:
                return False
            self._thr_set = key
        return True

    def _selection_weights(self):
        """fp32 [kernel h]: the summed per-model decoder norms (0 for the padding latents), from cc_dec_norms; kept
        while W_dec is the same storage, unwritten by torch (version counter) and by kernels (Arena.updates)."""
        a = self.arena()
        a.wait_pending()
        key = engine._norms_token(a)
        if self._sel_w is None or self._sel_w[0] != key:
            self._sel_w = (key, ops.dec_norms(a.W_dec_hk, self._hp, self.n_models, self._dp)[1])
        return self._sel_w[1]

    def selection_weights(self):
        """fp32 [dict_size]: the weights a BatchTopK crosscoder's encode multiplies the activations by to score them --
        sum_m ||W_dec[h, m]|| for topk_weight "decoder_norm", ones for "none".  The training step scores with ws.tn,
        the L1 term's norms, which the batch-major step (the only one BatchTopK runs) fills with the same kernel,
        cc_dec_norms: the same bits for the same W_dec."""
        if self.activation != "batch_topk":
            raise ValueError("selection_weights() serves activation 'batch_topk'")
        if self.topk_weight == "none":
            return torch.ones(self.d_hidden, dtype=torch.float32, device=self._arena.data.device)
        return self._selection_weights()[:self.d_hidden].clone()

    def batch_topk_info(self):
        """The last get_losses() / Trainer.step() selection of a BatchTopK crosscoder (synchronises): threshold (the
        smallest selected score), selected, ties (pairs at the threshold score that were admitted), eligible,
        row_count (int32 [batch]: every row's selected count)."""
        ws = self._ws
        if self.activation != "batch_topk" or ws is None:
            raise ValueError("batch_topk_info(): no BatchTopK forward has run")
        info = ws.bt_info.cpu()
        return {"threshold": info[0:1].view(torch.float32).item(), "selected": int(info[1]), "ties": int(info[2]),
                "eligible": int(info[3]), "row_count": ws.bt_row_count.clone()}

    ENCODE_ROWS = 4096  # rows encode_topk encodes per launch pair (its one activation buffer)

    def encode_topk(self, x, k=None):
        """x [rows, n_models, d_model] -> (values [rows, k], indices [rows, k] int32): each row's k largest positive
        activations of relu(x W_enc + b_enc) (ties: the smaller latent) in ascending latent index, padded with
        (0, -1) where fewer are positive -- the compact form of a wide dictionary's activations.  Framework
        extension; serves any crosscoder (k defaults to cfg["k"]); indices refer to the dict_size latents."""
        return self._encode_compact(x, k, own=False)

    def _encode_compact(self, x, k, own, use_threshold=None):
        """encode_topk (own=False: the k largest of relu(pre)) / encode_pairs (own=True: of the crosscoder's own
        activation): ENCODE_ROWS rows at a time through one activation buffer, cc_topk_rows writing only the pairs."""
        k = self.k if k is None else k
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= self.d_hidden:
            raise ValueError(f"k must be an int in 1..dict_size ({self.d_hidden}), got {k!r}")
        self._check_x(x)
        a = self.arena()
        rows, dev = x.shape[0], a.data.device
        vals = torch.empty(rows, k, dtype=self.dtype, device=dev)
        idx = torch.empty(rows, k, dtype=torch.int32, device=dev)
        buf = torch.empty(min(rows, self.ENCODE_ROWS), self._hp, dtype=self.dtype, device=dev)
        for r0 in range(0, rows, self.ENCODE_ROWS):
            r1 = min(rows, r0 + self.ENCODE_ROWS)
            acts = buf[:r1 - r0]
            ops.encode_fwd(self._flat_x(x[r0:r1]), a.W_enc_hk, a.b_enc, acts, True)
            if own:
                self.activate_(acts, use_threshold)
            ops.topk_rows(acts, self._hp, k, idx_out=idx[r0:r1], val_out=vals[r0:r1])
        return vals, idx

    def encode_pairs(self, x, k=None, use_threshold=None):
        """x [rows, n_models, d_model] -> (values [rows, k], indices [rows, k] int32): the crosscoder's OWN activations
        -- what encode(x, use_threshold=use_threshold) gives: ReLU, TopK, the BatchTopK selection / threshold mask,
        JumpReLU -- in encode_topk's compact form (ascending latent index, padded at the end with (0, -1)).  Exact where
        k >= the row's number of non-zero activations; a row with more keeps its k largest.  k defaults to cfg["k"]
        and is required for a crosscoder without one.  ENCODE_ROWS rows at a time: a BatchTopK crosscoder without a
        threshold selects among the rows of each such slice.  Framework extension; decode_pairs / pairs_sq_err take
        the pairs back to the residual stream without the dense [rows, dict_size] matrix."""
        return self._encode_compact(x, k, own=True, use_threshold=use_threshold)

    def _pairs(self, values, indices):
        """(values, indices) as cc_decode_pairs reads them: [rows, k] of the crosscoder's dtype and int32, contiguous
        (int64 indices are converted; one beyond int32 stays out of range)."""
        if values.dim() != 2 or indices.shape != values.shape or values.shape[1] < 1:
            raise ValueError(f"expected values and indices of one shape [rows, k >= 1], got {tuple(values.shape)} and "
                             f"{tuple(indices.shape)}")
        if indices.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"indices must be int32 or int64, got {indices.dtype}")
        if indices.dtype == torch.int64:
            indices = indices.clamp(min=-1, max=self.d_hidden).to(torch.int32)
        return values.to(self.dtype).contiguous(), indices.contiguous()

    def decode_pairs(self, values, indices, differentiable=False):
        """(values, indices) [rows, k] as encode_pairs / encode_topk give them -> [rows, n_models, d_model] incl. b_dec:
        the sparse counterpart of decode (cc_decode_pairs: k decoder rows gathered per token, an fp32 sum in slot
        order rounded once).  A slot whose index is outside [0, dict_size) -- the -1 padding -- adds nothing.
        differentiable=True: the same forward as one autograd node whose backward gives the gradients with respect to
        values (0 at such slots), W_dec and b_dec from gather kernels (cc_pairs_grad_values, cc_pairs_grad_decoder);
        no [rows, dict_size] matrix is formed in either direction."""
        if differentiable:
            vals, idx = self._pairs(values, indices)
            return _DecodePairsFn.apply(self, vals, idx, self.W_dec, self.b_dec)
        a = self.arena()
        a.wait_pending()
        vals, idx = self._pairs(values, indices)
        B = vals.shape[0]
        out = torch.empty(B, self.n_models * self._dp, dtype=self.dtype, device=vals.device)
        if B:
            ops.decode_pairs(vals, idx, a.W_dec_hk, a.b_dec_flat, self.n_models, self._dp, h=self.d_hidden, recon=out)
        out = out.view(B, self.n_models, self._dp)
        return out[:, :, :self.cfg["d_in"]].contiguous() if self._dp != self.cfg["d_in"] else out

    def pairs_sq_err(self, values, indices, x):
        """fp32 [rows, n_models]: per row and model, sum_d (decode_pairs(values, indices) - x)^2 of the rounded
        reconstruction (crosscoder.py:104's squared difference), from the same kernel pass: the reconstruction is
        never stored."""
        a = self.arena()
        a.wait_pending()
        vals, idx = self._pairs(values, indices)
        B = vals.shape[0]
        self._check_x(x)
        if x.shape[0] != B:
            raise ValueError(f"x has {x.shape[0]} rows, the pairs {B}")
        sq = torch.empty(B, self.n_models, dtype=torch.float32, device=vals.device)
        if B:
            ops.decode_pairs(vals, idx, a.W_dec_hk, a.b_dec_flat, self.n_models, self._dp, h=self.d_hidden,
                             x=self._flat_x(x), sq_err=sq)
        return sq

    def pairs_attribution(self, values, indices, g):
        """fp32 [rows, k, n_models]: per pair and model, value * <g[row, model], W_dec[latent, model]> -- the first-order
        effect of the pair on a metric whose gradient with respect to the reconstruction is g [rows, n_models, d_model]
        (cc_pairs_grad_values: k decoder rows gathered per token, the row of g read once).  +0 at a slot whose index
        is outside [0, dict_size)."""
        a = self.arena()
        a.wait_pending()
        vals, idx = self._pairs(values, indices)
        B, k = vals.shape
        self._check_x(g)
        if g.shape[0] != B:
            raise ValueError(f"g has {g.shape[0]} rows, the pairs {B}")
        if not B:
            return torch.empty(0, k, self.n_models, dtype=torch.float32, device=vals.device)
        return ops.pairs_grad_values(idx, a.W_dec_hk, self._flat_x(g.detach()), self.n_models, self._dp, val=vals.detach(),
                                     h=self.d_hidden)[0]

    def decode(self, acts):
        """acts [batch, d_hidden] -> [batch, n_models, d_model] incl. b_dec (crosscoder.py:82-89)."""
        a = self.arena()
        a.wait_pending()
        acts = acts.to(self.dtype)
        if self._hp != self.d_hidden:  # zero activations of the padding latents
            acts = torch.nn.functional.pad(acts, (0, self._hp - acts.shape[-1]))
        acts = acts.contiguous()
        B = acts.shape[0]
        out = torch.empty(B, self.n_models * self._dp, dtype=self.dtype, device=acts.device)
        ops.decode_fwd(acts, a.W_dec_hk, a.b_dec_flat, recon_t=out)
        out = out.view(B, self.n_models, self._dp)
        return out[:, :, :self.cfg["d_in"]].contiguous() if self._dp != self.cfg["d_in"] else out

    def forward(self, x):
        return self.decode(self.encode(x))

    def get_losses(self, x):
        """Same LossOutput as crosscoder.py:96-130; differentiable w.r.t. the four params
        (backward runs the fused HIP backward kernels).  A JumpReLU crosscoder's thresholds get no gradient here:
        Trainer.step is what trains them."""
        a = self.arena()
        return LossOutput(*_LossFn.apply(self, x, a.data, self.W_enc, self.W_dec, self.b_enc, self.b_dec))

    def state_dict(self, *args, **kwargs):
        # the decoder half may still be updating on the trainer's side stream
        if getattr(self, "_arena", None) is not None:
            self._arena.wait_pending()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, *args, **kwargs):
        # torch copies into self._parameters directly (no attribute access): the decoder half may still be updating on
        # the trainer's side stream, and its deferred rows would otherwise be applied after the load
        self._sync_pending()
        # a BatchTopK crosscoder takes the reference's four tensors as they are (e.g. a ReLU checkpoint to train on):
        # its threshold then stays what it is
        if self.activation == "batch_topk" and "threshold" not in state_dict:
            meta = getattr(state_dict, "_metadata", None)
            state_dict = OrderedDict(state_dict, threshold=self.threshold.detach().clone())
            if meta is not None:
                state_dict._metadata = meta
        # likewise a JumpReLU crosscoder: its thresholds then stay what they are
        if self.activation == "jumprelu" and "jump_threshold" not in state_dict:
            meta = getattr(state_dict, "_metadata", None)
            state_dict = OrderedDict(state_dict, jump_threshold=self.jump_threshold.detach().clone())
            if meta is not None:
                state_dict._metadata = meta
        return super().load_state_dict(state_dict, *args, **kwargs)

    # ------------------------------------------------------------------ checkpoints
    def create_save_dir(self):
        SAVE_DIR.mkdir(parents=True, exist_ok=True)
        versions = [int(f.name.split("_")[1]) for f in SAVE_DIR.iterdir() if "version" in str(f)]
        version = 1 + max(versions) if versions else 0
        self.save_dir = SAVE_DIR / f"version_{version}"
        self.save_dir.mkdir(parents=True)

    def save(self):
        if self.save_dir is None:
            self.create_save_dir()
        sd = self.reference_state_dict()
        if self.activation == "jumprelu":  # (the checkpoint carries the thresholds; reference_state_dict does not)
            sd["jump_threshold"] = self.jump_threshold.detach().clone()
        self.save_dir, self.save_version = write_checkpoint(sd, self.cfg, self.save_dir, self.save_version)

    def reference_state_dict(self):
        """state_dict() in the reference's own tensor layout: the views themselves, or -- when the kernel
        dims are padded -- compact copies with the reference strides (W_enc [n, d, h] strides (d, 1, n*d))."""
        sd = self.state_dict()
        if "jump_threshold" in sd:  # (a JumpReLU crosscoder's fifth parameter is not the reference's)
            sd = type(sd)((k, v) for k, v in sd.items() if k != "jump_threshold")
        if not self._arena.padded:
            return sd
        out = type(sd)()
        for k, v in sd.items():
            out[k] = v.permute(2, 0, 1).contiguous().permute(1, 2, 0) if k == "W_enc" else v.contiguous()
        return out

    def _load_checked(self, state_dict):
        self.load_state_dict(state_dict)
        self.arena()

    @classmethod
    def load(cls, version_dir, checkpoint_version):
        save_dir = Path("./checkpoints") / str(version_dir)
        cfg = json.load(open(save_dir / f"{checkpoint_version}_cfg.json", "r"))
        pprint.pprint(cfg)
        self = cls(cfg=cfg)
        self._load_checked(torch.load(save_dir / f"{checkpoint_version}.pt", map_location=cfg["device"],
                                      weights_only=True))
        return self

    @classmethod
    def load_from_path(cls, cfg_path, weights_path, device: Optional[Union[str, torch.device]] = None):
        """Offline form of `load_from_hf` (crosscoder.py:160-205): a local cfg.json +
        cc_weights.pt pair (no network in this framework)."""
        with open(cfg_path, "r") as f:
            cfg = json.load(f)
        if device is not None:
            cfg["device"] = str(device)
        inst = cls(cfg)
        inst._load_checked(torch.load(weights_path, map_location=cfg["device"], weights_only=True))
        return inst

    @classmethod
    def load_from_hf(cls, repo_id="ckkissane/crosscoder-gemma-2-2b-model-diff", path="blocks.14.hook_resid_pre",
                     device=None, local_dir=None):
        """The reference downloads from the Hub; here only an already-present local copy
        ({local_dir}/{path}/cfg.json + cc_weights.pt) is read."""
        if local_dir is None:
            raise RuntimeError("load_from_hf: no network; pass local_dir with {path}/cfg.json and cc_weights.pt")
        base = Path(local_dir) / path
        return cls.load_from_path(base / "cfg.json", base / "cc_weights.pt", device)


class _GraphToken:
    """Held by one get_losses() autograd node while its backward may still run; the workspace it used
    keeps a weak reference (engine.StepWorkspace.busy)."""


class _LossFn(torch.autograd.Function):
    """get_losses as one autograd node over the fused kernels."""

    @staticmethod
    def forward(ctx, cc, x, arena_data, W_enc, W_dec, b_enc, b_dec):
        cc._check_x(x)
        ws = cc._workspace(x.shape[0])
        a = cc.arena()
        engine.forward(ws, a, cc.pad_input(x).contiguous(), None,
                       theta=cc.theta() if cc.activation == "jumprelu" else None)
        s = ws.scalars
        dt = cc.dtype
        out = (s[0].clone(), s[1].to(dt, copy=True), s[2].clone(), ws.ev.clone(), ws.ev_a.to(dt, copy=True),
               ws.ev_b.to(dt, copy=True))
        ctx.cc = cc
        ctx.ws = ws
        if any(ctx.needs_input_grad[3:]):  # a graph whose backward will read ws
            ctx.token = _GraphToken()
            ws.busy = weakref.ref(ctx.token)  # freed with the graph, or cleared by backward
        ctx.mark_non_differentiable(out[2], out[3], out[4], out[5])
        return out

    @staticmethod
    def backward(ctx, g_l2, g_l1, *_):
        cc, ws = ctx.cc, ctx.ws
        a = cc.arena()
        w2 = 0.0 if g_l2 is None else float(g_l2)
        w1 = 0.0 if g_l1 is None else float(g_l1)
        if w2 != 1.0:  # g_recon was formed for d(l2)=1; re-form it for this upstream weight
            engine.loss_from_recon(ws, a, grad_scale=2.0 * w2 / ws.B)
        G = a.like()
        engine.backward(ws, a, G, l1_coeff=w1)
        ws.busy = None
        v = G.views()
        return None, None, None, v["W_enc"], v["W_dec"], v["b_enc"], v["b_dec"]


class _DecodePairsFn(torch.autograd.Function):
    """decode_pairs(..., differentiable=True) as one autograd node over the sparse decode and its gather backward."""

    @staticmethod
    def forward(ctx, cc, vals, idx, W_dec, b_dec):
        a = cc.arena()
        a.wait_pending()
        B = vals.shape[0]
        out = torch.empty(B, cc.n_models * cc._dp, dtype=cc.dtype, device=vals.device)
        if B:
            ops.decode_pairs(vals, idx, a.W_dec_hk, a.b_dec_flat, cc.n_models, cc._dp, h=cc.d_hidden, recon=out)
        ctx.cc = cc
        ctx.save_for_backward(vals, idx)
        out = out.view(B, cc.n_models, cc._dp)
        return out[:, :, :cc.cfg["d_in"]].contiguous() if cc._dp != cc.cfg["d_in"] else out

    @staticmethod
    def backward(ctx, g):
        cc = ctx.cc
        vals, idx = ctx.saved_tensors
        a = cc.arena()
        a.wait_pending()
        n, dp, h, d_in = cc.n_models, cc._dp, cc.d_hidden, cc.cfg["d_in"]
        B = vals.shape[0]
        gf = cc.pad_input(g).to(cc.dtype).contiguous().view(B, n * dp)
        g_vals = g_W = g_b = None
        if ctx.needs_input_grad[1]:
            g_vals = torch.zeros_like(vals)
            if B:  # (total: the models' sums in model order, rounded once to the values' dtype)
                g_vals = ops.pairs_grad_values(idx, a.W_dec_hk, gf, n, dp, h=h, want_dot=False, want_total=True)[1].to(vals.dtype)
        if ctx.needs_input_grad[3]:
            dW = torch.zeros(h, n * dp, dtype=cc.dtype, device=vals.device)
            if B:
                perm, seg = ops.pairs_by_latent(idx, h)
                ops.pairs_grad_decoder(perm, seg, vals, gf, n * dp, out=dW)
            g_W = dW.view(h, n, dp)[:, :, :d_in]
        if ctx.needs_input_grad[4]:
            g_b = gf.sum(0, dtype=torch.float32).to(cc.dtype).view(n, dp)[:, :d_in]
        return None, g_vals, None, g_W, g_b
