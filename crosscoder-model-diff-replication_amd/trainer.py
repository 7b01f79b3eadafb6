"""Drop-in `Trainer` (reference: trainer.py:7-82) whose `step()` is the fused HIP step.

`step()` returns the reference's 9-key loss dict (plus "auxk_loss" and "dead_latents" when cfg["auxk_coeff"] > 0:
the AuxK dead-latent loss of TopK / BatchTopK crosscoders; plus "l0_coeff" for a JumpReLU
crosscoder, whose "loss" includes l0_coeff * l0_loss and whose thresholds the step trains).  Per step it issues the fixed launch
sequence of engine.py and reads the 6 loss scalars once, from mapped host memory the loss-tail
kernel writes directly (the reference does 7 `.item()` syncs).  Adam state (exp_avg / exp_avg_sq, bf16 like the
reference's) lives in arenas mirroring the parameter arena, exposed through
`optimizer.state[param]` for inspection.  cfg["master_weights"] = True (bf16 crosscoders) keeps fp32 master weights and
fp32 moments instead, the bf16 parameters being the masters rounded after every update;
`Trainer.state_dict()` / `load_state_dict()` carry the optimizer's state across a restart in either mode.
cfg["resample_every"] = N re-seeds the dead latents after every N-th step (dead-latent resampling, DESIGN.md section
3.18; `Trainer.resample_dead_latents` is the same between steps of the caller's choosing).
cfg["sparse_step"] = True (TopK crosscoders, l1_coeff 0) runs the step's decode and backward on the k (value, latent)
pairs per row instead of the masked dense activations; `Trainer.sparse_step` says which ran.
cfg["auxk_compact"] = True serves the AuxK loss under the sparse step, its GEMMs over the compacted dead set alone
(DESIGN.md section 3.22).
"""
import torch
import tqdm

from . import _hip, engine
from .buffer import Buffer
from .crosscoder import CrossCoder, auxk_compact_of, master_weights_of, sparse_step_of
from .resample import LatentResampler

RESAMPLE_ROWS = 819200  # cfg["resample_rows"]'s default: the pool of "Towards Monosemanticity"'s neuron resampling


def resample_options(cfg):
    """(resample_every, resample_rows, resample_enc_scale) of a cfg (framework extension), or None when periodic
    dead-latent resampling is off.  cfg["resample_every"]: an int >= 0 of steps, absent or 0: off.  On, Trainer.step
    re-seeds the dead latents after every resample_every-th step before the LR decay starts (0.8 of the run), from a
    pool of cfg["resample_rows"] // batch_size batches (an int >= batch_size, default 819 200) that it draws with
    buffer.next() -- those batches are consumed: the steps that follow train on the ones after them -- and with
    cfg["resample_enc_scale"] (a float > 0, default 0.2) as LatentResampler's enc_scale."""
    every = cfg.get("resample_every", 0)
    if isinstance(every, bool) or not isinstance(every, int) or every < 0:
        raise ValueError(f"cfg['resample_every'] must be an int >= 0 (steps), got {every!r}")
    if every == 0:
        return None
    if cfg.get("activation", "relu") == "jumprelu":
        raise ValueError("cfg['resample_every'] is not served with activation 'jumprelu' (LatentResampler)")
    rows = cfg.get("resample_rows", max(RESAMPLE_ROWS, cfg["batch_size"]))
    if isinstance(rows, bool) or not isinstance(rows, int) or rows < cfg["batch_size"]:
        raise ValueError(f"cfg['resample_rows'] must be an int >= batch_size ({cfg['batch_size']}), got {rows!r}")
    scale = cfg.get("resample_enc_scale", 0.2)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not scale > 0 or scale == float("inf"):
        raise ValueError(f"cfg['resample_enc_scale'] must be a finite float > 0, got {scale!r}")
    return every, rows, float(scale)


def reference_loss(l2, l1, l1c, dtype):
    """The reference's logged "loss" (trainer.py:44,52): `l2_loss + l1_coeff * l1_loss` where l2 is an
    fp32 0-dim tensor and l1 one in the parameter dtype, so the product is rounded to that dtype
    first and the sum to fp32 (torch's type promotion), then `.item()`."""
    t = torch.tensor(l2, dtype=torch.float32) + l1c * torch.tensor(l1, dtype=dtype)
    return t.item()


def jumprelu_loss(loss, l0, l0c):
    """A JumpReLU step's logged "loss": reference_loss plus l0_coeff * l0_loss, l0 an fp32 0-dim tensor like l2."""
    return (torch.tensor(loss, dtype=torch.float32) + l0c * torch.tensor(l0, dtype=torch.float32)).item()


def rounded(v, dtype):
    """float(v) rounded to the parameter dtype (the reference's param-dtype loss tensors, crosscoder.py:115-126)."""
    return float(torch.tensor(v, dtype=dtype)) if dtype != torch.float32 else float(torch.tensor(v))


class FusedAdam:
    """State holder with torch.optim.Adam's observable surface (param_groups, state)."""

    def __init__(self, cc, lr, betas, eps=1e-8, master_weights=False):
        """master_weights (cfg["master_weights"]) on a bf16 crosscoder: `master`, an fp32 arena of the parameters, and
        fp32 moments; the bf16 parameters are the masters rounded after every update (cc_adam_master_step).  On an
        fp32 crosscoder the flag changes nothing."""
        a = cc.arena()
        self.cc = cc
        self.master_mode = bool(master_weights) and cc.dtype == torch.bfloat16
        state_dtype = torch.float32 if self.master_mode else None
        self.exp_avg = a.like(dtype=state_dtype)
        self.exp_avg_sq = a.like(dtype=state_dtype)
        self.grads = a.like()
        self.master = None
        self._master_token = None  # _arena_token of the bf16 arena when it last was the masters rounded
        if self.master_mode:
            self.master_for_update()
        # a JumpReLU crosscoder's thresholds: fp32 gradient and moments over the kernel h, in every mode
        self.theta_grad = self.theta_m = self.theta_v = None
        if cc.activation == "jumprelu":
            z = lambda: torch.zeros(cc._hp, dtype=torch.float32, device=a.data.device)  # noqa: E731
            self.theta_grad, self.theta_m, self.theta_v = z(), z(), z()
        self.param_groups = [{"lr": lr, "initial_lr": lr, "betas": betas, "eps": eps, "weight_decay": 0.0}]
        self.t = 0

    @staticmethod
    def _arena_token(a):
        # what the bf16 arena is keyed on (as engine._norms_token): its storage, the version counter every view of
        # it shares (any in-place write through torch bumps it; our Adam kernels do not) and the count of kernel
        # writes (Arena.updates: Adam's, fold_activation_scaling_factor's)
        return (a.data.data_ptr(), a.data._version, a.updates)

    def master_for_update(self):
        """The master arena for the next Adam launch (None outside master mode).  If the bf16 parameters were written
        since the last update (load_state_dict, fold_activation_scaling_factor, user code), the masters of the
        elements that no longer round to their parameter are re-seeded from it first; every other master keeps its
        extra bits, and the moments stay, as torch's would."""
        if not self.master_mode:
            return None
        a = self.cc.arena()
        tok = self._arena_token(a)
        if self._master_token != tok:
            a.wait_pending()  # the decoder half may still be updating on the side stream
            if (self.master is None or self.master.data.device != a.data.device
                    or self.master.data.shape != a.data.shape):
                self.master = a.like(dtype=torch.float32)
                self.master.data.copy_(a.data)
            else:
                keep = self.master.data.to(a.data.dtype) == a.data
                self.master.data.copy_(torch.where(keep, self.master.data, a.data.float()))
            self._master_token = tok
        return self.master

    def master_updated(self):
        """After the step's Adam launches: the bf16 arena is the masters rounded."""
        self._master_token = self._arena_token(self.cc.arena())

    @property
    def state(self):
        self.cc.arena().wait_pending()  # the decoder half may still be updating on the side stream
        m, v = self.exp_avg.views(), self.exp_avg_sq.views()
        w = self.master_for_update().views() if self.master_mode else None
        st = {}
        for name in ("W_enc", "W_dec", "b_enc", "b_dec"):
            p = getattr(self.cc, name)
            st[p] = {"step": torch.tensor(float(self.t)), "exp_avg": m[name], "exp_avg_sq": v[name]}
            if w is not None:
                st[p]["master"] = w[name]
        if self.theta_m is not None:
            h = self.cc.d_hidden
            st[self.cc.jump_threshold] = {"step": torch.tensor(float(self.t)), "exp_avg": self.theta_m[:h],
                                          "exp_avg_sq": self.theta_v[:h]}
        return st

    def zero_grad(self, set_to_none=True):
        pass  # grads are overwritten (never accumulated) by the backward kernels

    def state_dict(self):
        """What a restart needs beside CrossCoder.save(): the step count, both moments as flat arenas in their own
        dtype, in master mode the master arena, and a JumpReLU crosscoder's threshold moments (clones)."""
        self.cc.arena().wait_pending()
        sd = {"step": self.t, "master_weights": self.master_mode,
              "exp_avg": self.exp_avg.data.detach().clone(), "exp_avg_sq": self.exp_avg_sq.data.detach().clone()}
        if self.master_mode:
            sd["master"] = self.master_for_update().data.detach().clone()
        if self.theta_m is not None:
            sd["theta_exp_avg"] = self.theta_m.detach().clone()
            sd["theta_exp_avg_sq"] = self.theta_v.detach().clone()
        return sd

    def check_state_dict(self, sd):
        """ValueError unless `sd` is state_dict()'s output of an optimizer of the same mode, shapes and dtypes; writes
        nothing.  Returns the destination of every tensor entry."""
        if not isinstance(sd, dict) or not isinstance(sd.get("step"), int) or isinstance(sd.get("step"), bool) \
                or sd["step"] < 0:
            raise ValueError("FusedAdam.load_state_dict: not a FusedAdam state dict (no integer 'step' >= 0)")
        if bool(sd.get("master_weights", False)) != self.master_mode:
            raise ValueError(f"FusedAdam.load_state_dict: the state was saved with master_weights="
                             f"{bool(sd.get('master_weights', False))}, this optimizer runs with {self.master_mode}")
        want = {"exp_avg": self.exp_avg.data, "exp_avg_sq": self.exp_avg_sq.data}
        if self.master_mode:
            want["master"] = self.master_for_update().data
        if self.theta_m is not None:
            want["theta_exp_avg"], want["theta_exp_avg_sq"] = self.theta_m, self.theta_v
        extra = set(sd) - set(want) - {"step", "master_weights"}
        if extra:
            raise ValueError(f"FusedAdam.load_state_dict: unexpected entries {sorted(extra)}")
        for k, dst in want.items():
            t = sd.get(k)
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(dst.shape) or t.dtype != dst.dtype:
                got = (tuple(t.shape), t.dtype) if torch.is_tensor(t) else t
                raise ValueError(f"FusedAdam.load_state_dict: {k!r} must be a {dst.dtype} tensor of shape "
                                 f"{tuple(dst.shape)}, got {got}")
        return want

    def load_state_dict(self, sd):
        """Takes state_dict()'s output of an optimizer of the same mode, shapes and dtypes (ValueError otherwise;
        nothing is written then).  The masters of parameters that are not their rounding -- the crosscoder was
        loaded from something else -- are re-seeded from the parameters before the next update."""
        want = self.check_state_dict(sd)
        self.cc.arena().wait_pending()
        for k, dst in want.items():
            dst.copy_(sd[k])
        self.t = sd["step"]
        self._master_token = None  # (checked against the parameters before the next update)


class LambdaLRHost:
    """torch.optim.lr_scheduler.LambdaLR over one group, evaluated on the host."""

    def __init__(self, optimizer, lr_lambda):
        self.optimizer = optimizer
        self.lr_lambda = lr_lambda
        self.base_lr = optimizer.param_groups[0]["initial_lr"]
        self.last_epoch = 0
        optimizer.param_groups[0]["lr"] = self.base_lr * lr_lambda(0)
        self._last_lr = [optimizer.param_groups[0]["lr"]]

    def step(self):
        self.last_epoch += 1
        lr = self.base_lr * self.lr_lambda(self.last_epoch)
        self.optimizer.param_groups[0]["lr"] = lr
        self._last_lr = [lr]

    def get_last_lr(self):
        return list(self._last_lr)


class Trainer:
    def __init__(self, cfg, model_A=None, model_B=None, all_tokens=None, buffer=None, crosscoder=None, logger=None,
                 latent_stats=None):
        """latent_stats (framework extension): a LatentStats of this trainer's crosscoder; every step then folds
        its activations into it (one launch after the forward -- G1, G2 and the loss rows -- and before G3, on the same
        stream; row ids step * batch_size + b).  The step's own launches are
        the same with and without it; read `trainer.latent_stats.result()`, e.g. in `logger`.  bf16 crosscoders only:
        the fp32 step's streams are not shown to be independent of what else is launched."""
        self.cfg = cfg
        self.model_A = model_A
        self.model_B = model_B
        self.crosscoder = crosscoder if crosscoder is not None else CrossCoder(cfg)
        self.buffer = buffer if buffer is not None else Buffer(cfg, model_A, model_B, all_tokens)
        self.total_steps = cfg["num_tokens"] // cfg["batch_size"]
        # cfg["master_weights"] (bf16 crosscoders): fp32 master weights and fp32 Adam moments, DESIGN.md section 3.16
        self.optimizer = FusedAdam(self.crosscoder, cfg["lr"], (cfg["beta1"], cfg["beta2"]),
                                   master_weights=master_weights_of(cfg))
        self.scheduler = LambdaLRHost(self.optimizer, self.lr_lambda)
        self.step_counter = 0
        self.logger = logger
        if latent_stats is not None and latent_stats.cc is not self.crosscoder:
            raise ValueError("latent_stats must be built on this trainer's crosscoder")
        if latent_stats is not None and self.crosscoder.dtype != torch.bfloat16:
            raise ValueError("Trainer(latent_stats=...) serves enc_dtype 'bf16' only: a reader of the fp32 step's "
                             "decoder half is not reliably ordered after its side-stream Adam (DESIGN.md section 3.7); "
                             "call LatentStats.update on the batches instead")
        self.latent_stats = latent_stats
        self._mapped = None  # mapped host words the step's loss tail writes (allocated on the first step)
        self._seq = 0
        self._side = None  # stream of the decoder half's Adam (created on the first step)
        self._last_ws = None  # the last step's workspace (its G2 abort word, engine.check_step_abort)
        # the AuxK dead-latent loss (crosscoder.auxk_options): tokens since each latent fired (int64, kernel h, on the
        # device, allocated with the first use) and the number of dead latents under that state, which the host knows
        # without a sync: the step's dead update writes it to mapped host memory with the loss scalars
        self.auxk = self.crosscoder.auxk
        self._tsf = None
        self._dead_count = 0
        # periodic dead-latent resampling (resample_options); the pool is allocated with the first resample
        self.resample = resample_options(cfg)
        self._resampler = None
        # the sparse TopK step (crosscoder.sparse_step_of): what it does not serve is refused here, not run densely
        self.sparse_step = sparse_step_of(cfg)
        # the AuxK loss of the sparse step: the aux GEMMs on the compacted dead set
        self.auxk_compact = auxk_compact_of(cfg)
        self._sparse_ws = None  # its workspace, the Trainer's own: the crosscoder's serves get_losses' dense autograd
        if self.sparse_step:
            why = None
            if cfg["l1_coeff"] != 0:
                why = ("cfg['l1_coeff'] != 0: TopK replaces the L1 penalty, and the L1 term's dense dW_dec part is not "
                       "built for the sparse step")
            elif self.auxk is not None and not self.auxk_compact:
                why = ("cfg['auxk_coeff'] > 0: the AuxK loss on pairs is not built; cfg['auxk_compact'] = True serves "
                       "it with the aux GEMMs on the compacted dead set")
            elif self.resample is not None:
                why = "cfg['resample_every']: resampling under the sparse step is not built"
            elif latent_stats is not None:
                why = "latent_stats=...: the sparse step never writes the masked dense activations"
            if why is not None:
                raise ValueError(f"cfg['sparse_step'] is not served with {why}")

    def lr_lambda(self, step):
        if step < 0.8 * self.total_steps:
            return 1.0
        return 1.0 - (step - 0.8 * self.total_steps) / (0.2 * self.total_steps)

    def get_l1_coeff(self):
        if self.step_counter < 0.05 * self.total_steps:
            return self.cfg["l1_coeff"] * self.step_counter / (0.05 * self.total_steps)
        return self.cfg["l1_coeff"]

    def get_l0_coeff(self):
        """cfg["l0_coeff"] (JumpReLU crosscoders) on get_l1_coeff's warm-up schedule."""
        if self.step_counter < 0.05 * self.total_steps:
            return self.cfg["l0_coeff"] * self.step_counter / (0.05 * self.total_steps)
        return self.cfg["l0_coeff"]

    def _since_fired(self):
        if self._tsf is None:
            cc = self.crosscoder
            self._tsf = torch.zeros(cc._hp, dtype=torch.int64, device=cc.arena().data.device)
        return self._tsf

    @property
    def tokens_since_fired(self):
        """int64 [dict_size] on the device (AuxK trainers): tokens since each latent last fired; a latent is dead
        for the next step iff its entry is >= cfg["dead_tokens"].  Settable with a tensor of the same shape (tests,
        resuming): the setter reads the new dead count back once."""
        if self.auxk is None:
            raise ValueError("tokens_since_fired: cfg['auxk_coeff'] is 0 or absent")
        return self._since_fired()[:self.crosscoder.d_hidden]

    @tokens_since_fired.setter
    def tokens_since_fired(self, value):
        cur = self.tokens_since_fired
        value = self._checked_since_fired(value)
        cur.copy_(value.to(cur.device, torch.int64))
        self._dead_count = int((cur >= self.auxk[2]).sum())

    def _checked_since_fired(self, value):
        # what the tokens_since_fired setter accepts, as a tensor (ValueError otherwise; nothing is written)
        if self.auxk is None:
            raise ValueError("tokens_since_fired: cfg['auxk_coeff'] is 0 or absent")
        shape = (self.crosscoder.d_hidden,)
        value = torch.as_tensor(value)
        if (tuple(value.shape) != shape or value.dtype.is_floating_point or value.dtype.is_complex
                or bool((value < 0).any())):
            raise ValueError(f"tokens_since_fired takes a non-negative integer tensor of shape {shape}")
        return value

    def auxk_state(self):
        """The last step's AuxK state (synchronises): aux_acts ([batch, dict_size], a view of the step's aux
        activations; zeros when the step issued no aux launches), dead (bool [dict_size], the dead set the step
        used), den, auxk_loss and dead_latents (the dead count after the step).  The sparse step (cfg["auxk_compact"])
        scatters aux_acts from its compact form and adds dead_ids (int64, the dead latents in the compact order) and
        compact_count (the dead count cc_dead_compact found on the device: the host's, which sized the step)."""
        ws = self._last_ws
        if self.auxk is None or ws is None:
            raise ValueError("auxk_state(): no AuxK step has run")
        torch.cuda.synchronize(ws.x.device)
        hr = self.crosscoder.d_hidden
        sc = ws.auxk_scalars.cpu()
        active = ws.aux_active
        if ws.sparse:
            # the compact form scattered to [batch, dict_size] (plain torch: not the hot path); dead_ids: the dead set
            # in the compact order, ascending
            aux = torch.zeros(ws.B, ws.h, dtype=ws.dtype, device=ws.x.device)
            ids = torch.zeros(0, dtype=torch.int64, device=ws.x.device)
            if active:
                ids = ws.ids[:min(ws.aux_D, ws.aux_Dp)].long()
                aux[:, ids] = ws.aux_c[:, :ids.numel()]
            return {"aux_acts": aux[:, :hr], "dead": ws.was_dead[:hr].bool(),
                    "row_count": (aux > 0).sum(1, dtype=torch.int32) if active else None,
                    "den": float(sc[1]) if active else 0.0, "auxk_loss": float(sc[0]) if active else 0.0,
                    "dead_latents": int(ws.dead_count), "dead_ids": ids,
                    "compact_count": int(ws.aux_count) if active else 0}
        return {"aux_acts": ws.aux_acts[:, :hr] if active else torch.zeros_like(ws.aux_acts[:, :hr]),
                "dead": ws.was_dead[:hr].bool(), "row_count": ws.aux_row_count if active else None,
                "den": float(sc[1]) if active else 0.0, "auxk_loss": float(sc[0]) if active else 0.0,
                "dead_latents": int(ws.dead_count)}

    def _launch_step(self, host, seq):
        """The step's launches; the loss tail writes the scalars to `host` (a _hip.MappedHostBuffer), then `seq`:
        the host waits for that word, not for a stream.  Only step() launches a step, and it checks the step's abort
        word before the next one is launched (_check_abort): a timed-out G2 aborts exactly one step, whose rollback
        of the optimizer's step count and LR schedule happens in that same step()."""
        cc = self.crosscoder
        raw, factor = self.buffer.next_raw()
        raw = cc.pad_input(raw)  # (zero columns only when d_in % 8 != 0)
        normalize = getattr(self.buffer, "normalize", True)
        # the buffer's refresh count tags the batch for engine.PREP_IN_ADAM: the last step's Adam launch may have
        # prepped exactly these rows
        tag = getattr(self.buffer, "refresh_count", 0)
        P = cc.arena()
        opt = self.optimizer
        side = self._side_stream()
        if self.sparse_step:
            ws, aux_on = self._launch_sparse_step(raw, factor if normalize else None, tag, P, side, host, seq)
            return self._launch_adam(ws, P, side, normalize, self.get_l1_coeff(), None, aux_on)
        ws = cc._workspace(raw.shape[0], step=True)
        # prep, G1, G2 + the loss rows (one pass where decode_loss_t serves the shape)
        # (BatchTopK: the selection's last launch folds the step's threshold score T into the crosscoder's inference
        # threshold -- T at the first step, then beta * threshold + (1 - beta) * T -- on the device, in stream order)
        # (AuxK: the dead set of this step is the state the last step's dead update left, whose count the host
        # already holds -- none dead: no aux launch is issued and the backward is the plain one)
        aux_on = self.auxk is not None and self._dead_count > 0
        engine.forward(ws, P, raw, factor if normalize else None, finalize=False, prep_tag=tag,
                       bt_threshold=(cc.threshold, cc.threshold_beta) if ws.batch_topk is not None else None,
                       aux=(self._since_fired(), self.auxk[2]) if aux_on else None,
                       theta=cc.theta() if ws.jumprelu is not None else None)
        if self.latent_stats is not None:  # (after G2 and the loss rows, before G3; acts is only read from G1 on: this stream's order suffices)
            self.latent_stats.update_from_acts(ws.acts, row0=self.step_counter * self.cfg["batch_size"])
        # the loss scalars: into mapped host memory from the G3 launch (or, where G3 cannot carry the tail, from a
        # launch on the side stream beside G3)
        if self.auxk is not None:
            # on this stream before the event the loss tail waits for: its sequence word publishes words 9 and 10 too
            engine.auxk_forward(ws, P, self._since_fired(), cc.d_hidden, self.auxk[2], self.auxk[0], aux_on, host=host)
        engine.loss_finalize_with_g3(ws, side, host=host, seq=seq)
        l1c = self.get_l1_coeff()
        # clip_grad_norm_(max_norm=1.0), trainer.py:46
        l0c = None
        if ws.jumprelu is not None:
            # JumpReLU: the objective gains l0_coeff * l0, and the thresholds their gradient, their share of the clip
            # norm and (below) their Adam launch
            l0c = self.get_l0_coeff()
            engine.backward(ws, P, opt.grads, l1c, clip=1.0, l0_coeff=l0c, theta_grad=opt.theta_grad)
        elif aux_on:
            engine.backward_auxk(ws, P, opt.grads, l1c, clip=1.0)
        else:
            engine.backward(ws, P, opt.grads, l1c, clip=1.0)
        self._launch_adam(ws, P, side, normalize, l1c, l0c, aux_on)

    def _launch_adam(self, ws, P, side, normalize, l1c, l0c, aux_on):
        """The end of every step's launches: clip_grad_norm_'s coefficient (where the backward did not leave it) and
        Adam, then the step's bookkeeping."""
        cc, opt = self.crosscoder, self.optimizer
        g = opt.param_groups[0]
        opt.t += 1
        b1, b2 = g["betas"]
        # the batch the next step will most likely train on (a buffer that can say, no column padding): its prep
        # rides in this step's encoder-half Adam launch; a next step handed anything else preps as always
        # (master weights: the fp32 update carries no prep, and the next forward preps as always)
        master = opt.master_for_update()
        peek = getattr(self.buffer, "peek_raw", None) if engine.PREP_IN_ADAM and master is None else None
        nxt = peek() if peek is not None and cc._dp == cc.cfg["d_in"] else None
        if nxt is not None:
            nxt = (nxt[0], nxt[1] if normalize else None, getattr(self.buffer, "refresh_count", 0))
        engine.clip_and_adam(ws, P, opt.grads, opt.exp_avg, opt.exp_avg_sq, g["lr"], b1, b2, g["eps"], opt.t,
                             side_stream=side, next_batch=nxt, master=master,
                             extra=(ws.theta, opt.theta_grad, opt.theta_m, opt.theta_v) if l0c is not None else None)
        if master is not None:
            opt.master_updated()
        self.scheduler.step()
        self._last_l1c = l1c
        self._last_l0c = l0c
        self._last_ws = ws
        self._last_aux_on = aux_on

    def _sparse_workspace(self, B, P):
        cc, ws = self.crosscoder, self._sparse_ws
        if ws is None or ws.B != B or ws.x.device != P.data.device:
            ws = self._sparse_ws = engine.StepWorkspace(B, cc.n_models, cc._dp, cc._hp, cc.dtype, P.data.device,
                                                        topk=cc.k, sparse=True,
                                                        auxk=(self.auxk[1],) if self.auxk is not None else None)
        return ws

    def _launch_sparse_step(self, raw, factor, tag, P, side, host, seq):
        """_launch_step's forward and backward for cfg["sparse_step"] (engine.forward_sparse / backward_sparse): no launch
        of it waits in its kernel, so the step has no abort word, and the loss tail runs beside d_acts on the side
        stream.  With cfg["auxk_compact"]: the dead update after the loss rows and, while the host's dead count is not
        0, the aux problem on the compacted dead set; the loss tail is forked after both, so
        its sequence word publishes words 9 and 10 too.  -> the workspace and whether the aux launches ran, for
        _launch_adam."""
        ws = self._sparse_workspace(raw.shape[0], P)
        aux_on = self.auxk is not None and self._dead_count > 0
        aux = None
        if aux_on:
            # (the capacity follows the dead count the host already holds: an allocation between steps, no sync)
            ws.aux_reserve(self._dead_count)
            aux = (self._since_fired(), self.crosscoder.d_hidden, self.auxk[2], self._dead_count)
        engine.forward_sparse(ws, P, raw, factor, prep_tag=tag, aux=aux)
        if self.auxk is not None:
            engine.auxk_forward_sparse(ws, P, self._since_fired(), self.crosscoder.d_hidden, self.auxk[2], self.auxk[0],
                                       aux_on, host=host)
        engine.loss_finalize_beside(ws, side, host=host, seq=seq)
        engine.backward_sparse(ws, P, self.optimizer.grads, aux=aux_on)
        return ws, aux_on

    def _side_stream(self):
        # the decoder half of Adam (+ the next step's decoder norms / W_dec^T) runs here, beside the
        # next step's prep / encoder GEMM (engine.adam)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.crosscoder.arena().data.device)
        return self._side

    def synchronize(self):
        """Order torch's current stream after every launch of the last step (the decoder half of
        Adam may still run on the side stream, and its last rows are deferred to the next reader, which
        launches them; CrossCoder's accessors and optimizer.state do this by themselves)."""
        self.crosscoder.arena().wait_pending()
        self._check_abort()

    def _check_abort(self):
        """Raise engine.STEP_ABORTED_MSG if the last step's G2 timed out waiting for the side-stream Adam; its
        launches applied no update, so the optimizer's step count and the LR schedule are rolled back."""
        try:
            engine.check_step_abort(self._last_ws)
        except RuntimeError:
            self.optimizer.t -= 1
            self.scheduler.last_epoch -= 1
            lr = self.scheduler.base_lr * self.lr_lambda(self.scheduler.last_epoch)
            self.optimizer.param_groups[0]["lr"] = lr
            self.scheduler._last_lr = [lr]
            raise

    def step(self):
        if self._mapped is None:
            self._mapped = _hip.MappedHostBuffer(16)
        self._seq = (self._seq + 1) & 0xFFFFFFFF or 1
        self._launch_step(self._mapped, self._seq)
        self._mapped.wait(8, self._seq)
        self._check_abort()  # (G2 timed out: raise in THIS step; its Adam launches applied nothing)
        s = [float(v) for v in self._mapped.f32[:6]]
        l1c = self._last_l1c
        dt = self.crosscoder.dtype
        l2, l1, l0 = s[0], rounded(s[1], dt), s[2]
        loss_dict = {
            "loss": reference_loss(l2, l1, l1c, dt),
            "l2_loss": l2,
            "l1_loss": l1,
            "l0_loss": l0,
            "l1_coeff": l1c,
            "lr": self.scheduler.get_last_lr()[0],
            "explained_variance": s[3],
            "explained_variance_A": rounded(s[4], dt),
            "explained_variance_B": rounded(s[5], dt),
        }
        if self.auxk is not None:
            auxk_loss = float(self._mapped.f32[9]) if self._last_aux_on else 0.0
            self._dead_count = int(self._mapped.u32[10])
            loss_dict["loss"] = loss_dict["loss"] + self.auxk[0] * auxk_loss
            loss_dict["auxk_loss"] = auxk_loss
            loss_dict["dead_latents"] = self._dead_count
        if self._last_l0c is not None:
            l0c = self._last_l0c
            loss_dict["loss"] = jumprelu_loss(loss_dict["loss"], l0, l0c)
            loss_dict["l0_coeff"] = l0c
        self.step_counter += 1
        if (self.resample is not None and self.step_counter % self.resample[0] == 0
                and self.step_counter < 0.8 * self.total_steps):
            loss_dict["resampled"] = self._resample_from_buffer()
        return loss_dict

    def _resample_from_buffer(self):
        """cfg["resample_every"]'s resample: a pool of resample_rows // batch_size batches drawn with buffer.next()
        (consumed: the next step trains on the batch after them), the latents that fired on none of them re-seeded
        with uniforms from a generator seeded with cfg["seed"] and the step.  -> the number re-seeded."""
        _, rows, enc_scale = self.resample
        B = self.cfg["batch_size"]
        rs = self._resampler
        if rs is None or rs.cc.arena().data.device != rs._x.device:
            rs = self._resampler = LatentResampler(self.crosscoder, rows // B * B, enc_scale=enc_scale,
                                                   seed=self.cfg["seed"])
        rs.reset()
        self.synchronize()
        for _ in range(rows // B):
            rs.add(self.buffer.next())
        J = int(rs.dead().sum())
        gen = torch.Generator(device="cpu").manual_seed((self.cfg["seed"] * 1000003 + self.step_counter) % (1 << 63))
        u = torch.rand(J, dtype=torch.float64, generator=gen)
        return self.resample_dead_latents(rs, u=u)["resampled"]

    def resample_dead_latents(self, resampler, dead=None, u=None):
        """Re-seed dead latents between two steps (LatentResampler.apply with this trainer's optimizer): orders
        torch's current stream after the last step's launches on both of its streams, applies `resampler` (built on
        this trainer's crosscoder and filled by the caller; dead, u: apply's; its CrossCoder.params_written() drops what
        the last step's workspace carries of the old decoder), and -- AuxK trainers -- zeroes tokens_since_fired of the
        re-seeded latents and refreshes the dead count.  Returns apply's dict."""
        if resampler.cc is not self.crosscoder:
            raise ValueError("resampler must be built on this trainer's crosscoder")
        self.synchronize()
        dev = self.crosscoder.arena().data.device
        if self._side is not None:
            torch.cuda.current_stream(dev).wait_stream(self._side)
        out = resampler.apply(self.optimizer, dead=dead, u=u)
        # (what the last step's workspace carries of the old decoder is keyed on Arena.updates, which apply counted up)
        if out["resampled"]:
            if self.auxk is not None:
                tsf = self._since_fired()
                tsf[out["latents"][out["written"]]] = 0
                self._dead_count = int((self.tokens_since_fired >= self.auxk[2]).sum())
        return out

    def log(self, loss_dict):
        if self.logger is not None:
            self.logger(loss_dict, self.step_counter)
        print(loss_dict)

    def save(self):
        self.synchronize()
        self.crosscoder.save()

    def state_dict(self):
        """The trainer's own state, for resuming beside CrossCoder.save() (which keeps the parameters and a BatchTopK
        threshold, format unchanged): the optimizer's state dict, step_counter, the scheduler's last_epoch and, for
        AuxK trainers, tokens_since_fired.  Synchronises with the last step's launches."""
        self.synchronize()
        sd = {"optimizer": self.optimizer.state_dict(), "step_counter": self.step_counter,
              "last_epoch": self.scheduler.last_epoch}
        if self.auxk is not None:
            sd["tokens_since_fired"] = self.tokens_since_fired.detach().clone()
        return sd

    def load_state_dict(self, sd):
        """Takes state_dict()'s output of a trainer of the same cfg (ValueError on a mode, shape or dtype mismatch,
        raised before anything is written: every entry is checked first).  The buffer's position is the caller's to
        restore."""
        keys = {"optimizer", "step_counter", "last_epoch"} | ({"tokens_since_fired"} if self.auxk is not None else set())
        if not isinstance(sd, dict) or set(sd) != keys:
            raise ValueError(f"Trainer.load_state_dict: expected the entries {sorted(keys)}, got "
                             f"{sorted(sd) if isinstance(sd, dict) else type(sd).__name__}")
        for k in ("step_counter", "last_epoch"):
            if isinstance(sd[k], bool) or not isinstance(sd[k], int) or sd[k] < 0:
                raise ValueError(f"Trainer.load_state_dict: {k!r} must be an int >= 0, got {sd[k]!r}")
        self.optimizer.check_state_dict(sd["optimizer"])
        if self.auxk is not None:
            self._checked_since_fired(sd["tokens_since_fired"])
        self.synchronize()
        self.optimizer.load_state_dict(sd["optimizer"])
        if self.auxk is not None:
            self.tokens_since_fired = sd["tokens_since_fired"]
        self.step_counter = sd["step_counter"]
        self.scheduler.last_epoch = sd["last_epoch"]
        lr = self.scheduler.base_lr * self.lr_lambda(self.scheduler.last_epoch)  # (as _check_abort re-derives it)
        self.optimizer.param_groups[0]["lr"] = lr
        self.scheduler._last_lr = [lr]

    def train(self):
        self.step_counter = 0
        try:
            for i in tqdm.trange(self.total_steps):
                loss_dict = self.step()
                if i % self.cfg["log_every"] == 0:
                    self.log(loss_dict)
                if (i + 1) % self.cfg["save_every"] == 0:
                    self.save()
        finally:
            self.save()
