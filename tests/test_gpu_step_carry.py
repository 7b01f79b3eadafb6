"""What a training step hands to the next one through host-side state, across a write of the parameters between two
steps: the workspace's decoder norms, norm partials pending their finaliser and W_dec^T
(keyed by engine._norms_token), the prepped next batch, the deferred decoder-half Adam rows, the fp32 masters' token
and BatchTopK's selection weights.

A scenario is one write under one configuration.  Trainer A runs two steps (past the l1 warm-up, so stale norms reach
the gradients), the write is applied, A runs a third step.  The reference is a twin with no carried state, built after
the write through public API only: a fresh CrossCoder and Trainer of the same cfg, loaded from A's state dicts, its
buffer at A's position, one step.  Loss dict, parameter arena, both moments and (master mode) the masters must be equal
bit for bit; every configuration also runs with no write (the control).  Independently of any second kernel run, the
step's l1_loss is compared with an fp64 sum over the step's own activations and the decoder norms of the parameters as
written (rel 1e-2, the l1 line of test_gpu_configs.py); every decoder write moves every latent's summed norm by a
factor >= 1.5, so a stale carry is off by a third or more."""
import math

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import engine, ops

pytestmark = pytest.mark.gpu

# name -> (B, d, h, enc_dtype, cfg keys, engine flags).  The smallest shapes at which each carry path exists:
CONFIGS = {
    # the fused G2 (cc_decode_loss, d % 64 == 0) with the product's flags: norm partials out of the side-stream Adam,
    # their finaliser in the next G2 launch
    "bf16-fused": (256, 64, 512, "bf16", {}, {}),
    # transposed operands, not fused: W_dec^T and the norms from one pass on the side stream (no partials at these dims)
    "bf16-transposed": (96, 40, 200, "bf16", {}, {}),
    "bf16-padded": (96, 36, 203, "bf16", {}, {}),  # padded kernel dims
    "fp32": (64, 32, 256, "fp32", {}, {}),  # norms_for_next on the side stream, no partials
    # the serial form: the partials are pending their finaliser right after Adam
    "bf16-serial": (256, 64, 512, "bf16", {}, {"DEC_ADAM_BESIDE_G1": False}),
    "bf16-split": (256, 64, 512, "bf16", {}, {"DEC_SIDE_ROWS": 0.5}),  # half the rows deferred to the first reader
    "bf16-master": (256, 64, 512, "bf16", {"master_weights": True}, {}),
    # the carried tn decides the selection; CrossCoder._sel_w serves encode
    "batch-topk": (256, 64, 512, "bf16", {"activation": "batch_topk", "k": 16}, {}),
    # the sparse TopK step (the Trainer's own workspace): it carries the decoder norms for its l1_loss (norms_for_next)
    "sparse-topk": (256, 64, 512, "bf16", {"activation": "topk", "k": 8, "sparse_step": True, "l1_coeff": 0}, {}),
}
F = (0.5, 0.25)    # per-model factors of the in-place writes: the summed norm falls to between 1/4 and 1/2
F2 = (0.25, 0.5)   # of copy_ and the .data writes
FOLD = (0.25, 0.5)  # fold_activation_scaling_factor: W_dec[:, m] /= s_m, the summed norm grows 2 to 4 times


def cfg_of(name):
    B, d, h, dtype, extra, _ = CONFIGS[name]
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 1e-3, "num_tokens": B * 100, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": dtype, "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    cfg.update(extra)
    return cfg


def trainer_of(cfg):
    return ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=4 * cfg["batch_size"], seed=3),
                      crosscoder=ca.CrossCoder(cfg))


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def per_model(cc, f):
    return torch.tensor(f, dtype=cc.dtype, device=cc.arena().data.device)[None, :, None]


def tn64(W_dec):
    """fp64 [dict_size]: sum over the models of ||W_dec[h, m]|| (crosscoder.py:123-125)."""
    return W_dec.detach().double().norm(dim=-1).sum(-1)


def batch_of(tr, rows=None):
    buf = tr.buffer
    x = buf.buffer[:rows or tr.cfg["batch_size"]].float() * buf.normalisation_factor.float()[None, :, None]
    return x


# ---------------------------------------------------------------- the writes: fn(A) -> expected W_dec or None
def w_none(A):
    return None


def w_load_state_dict(A, held=None):
    """The roll-back-in-process sequence.  held: state dicts taken before the last step (the load then follows step()
    at once: torch copies into the parameters without reading them through the crosscoder)."""
    cc = A.crosscoder
    if held is None:
        sd = {k: v.detach().clone() for k, v in cc.state_dict().items()}
        sd["W_dec"] = sd["W_dec"] * per_model(cc, F)
        tr_sd = None
    else:
        sd, tr_sd = held
    cc.load_state_dict(sd)
    A.load_state_dict(tr_sd if tr_sd is not None else A.state_dict())
    for k, v in sd.items():  # (the load is what the crosscoder holds: no deferred Adam rows were applied on top of it)
        assert torch.equal(bits(getattr(cc, k).detach().contiguous()), bits(v.contiguous())), k
    return sd["W_dec"]


def w_mul(A):
    cc = A.crosscoder
    with torch.no_grad():
        want = cc.W_dec.detach() * per_model(cc, F)
        cc.W_dec.mul_(per_model(cc, F))
    return want


def w_copy(A):
    cc = A.crosscoder
    with torch.no_grad():
        new = (cc.W_dec.detach() * per_model(cc, F2)).clone()
        cc.W_dec.copy_(new)
    return new


def w_fold(A):
    ca.fold_activation_scaling_factor(A.crosscoder, *FOLD)
    return None


def w_fold_enc(A):
    cc = A.crosscoder
    want = cc.W_dec.detach().clone()
    ca.fold_activation_scaling_factor(cc, *FOLD, fold_decoder=False)
    return want


def w_data_assign(A):
    cc = A.crosscoder
    new = (cc.W_dec.detach() * per_model(cc, F2)).contiguous().clone()
    cc.W_dec.data = new  # (an assignment: the arena re-packs)
    return new


def w_data_mul(A):
    cc = A.crosscoder
    want = cc.W_dec.detach() * per_model(cc, F2)
    cc.W_dec.data.mul_(per_model(cc, F2))  # (bumps no counter)
    cc.params_written()
    return want


def w_b_dec(A):
    cc = A.crosscoder
    with torch.no_grad():
        cc.b_dec.add_(0.125)
    return None


def w_W_enc(A):
    cc = A.crosscoder
    with torch.no_grad():
        cc.W_enc.mul_(0.5)
    return None


WRITES = {"none": w_none, "load_state_dict": w_load_state_dict, "mul_": w_mul, "copy_": w_copy, "fold": w_fold,
          "fold_enc": w_fold_enc, "data_assign": w_data_assign, "data_mul_params_written": w_data_mul,
          "b_dec": w_b_dec, "W_enc": w_W_enc}
KEEPS_NORMS = ("none", "fold_enc", "b_dec", "W_enc")  # the decoder norms are those before the write

# ops wrappers that launch kernels: the step's, and the ones that derive something from W_dec
DERIVES = ("dec_norms", "transpose", "transpose_dec_norms", "dec_norms_finalize")
LAUNCHERS = DERIVES + (
    "prep_input", "reduce_rows", "encode_fwd", "encode_fwd_t", "decode_fwd", "decode_partial", "decode_partial_jobs",
    "decode_partial_t", "decode_loss_t", "decode_loss", "loss_fwd_bwd", "loss_finalize", "loss_tail", "grad_tail",
    "grad_tail_sums", "segment_sums", "dacts_bwd", "dacts_bwd_t", "adam_dec_norms", "adam_dec_transposed", "wgrad_dec",
    "wgrad_enc", "wgrad_both", "wgrad_both_t", "wgrad_both_clip_t", "wgrad_both_sums_t", "clip_finalize", "adam_step",
    "adam_master_step", "adam_step_prep", "adam_step_clip", "topk_rows", "batch_topk", "pairs_group",
    "decode_pairs_partial", "pairs_grad_values", "pairs_wgrad")
# one undisturbed steady-state step of the product path (bf16-fused): the prep rides in the encoder-half Adam, the norm
# finaliser in G2, the loss tail in G3, the grad tail in G4G5 -- six launches, none of them a pass over W_dec
PRODUCT_STEP = ["encode_fwd_t", "decode_loss", "dacts_bwd_t", "wgrad_both_clip_t", "adam_step_prep", "adam_dec_norms"]


def record_launches(monkeypatch):
    """-> the list that every launching ops wrapper appends (name, the riders it was handed) to."""
    log = []
    for name in LAUNCHERS:
        orig = getattr(ops, name)

        def wrapper(*a, _orig=orig, _name=name, **k):
            log.append((_name, {r for r in ("norm_fin", "wait", "pre", "tail") if k.get(r) is not None}))
            return _orig(*a, **k)

        monkeypatch.setattr(ops, name, wrapper)
    return log


def snapshot(tr):
    """Clones of the parameter arena, both moments and (master mode) the masters, after the step's launches."""
    tr.synchronize()
    o, a = tr.optimizer, tr.crosscoder.arena()
    out = {"params": a.data, "exp_avg": o.exp_avg.data, "exp_avg_sq": o.exp_avg_sq.data}
    if o.master_mode:
        out["master"] = o.master_for_update().data
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def l1_fp64(ws, tn, h):
    """(acts.double() @ tn64).mean() of the step's own activations (the sparse step's are its pairs)."""
    if ws.sparse:
        idx = ws.pair_idx.long()
        ok = (idx >= 0) & (idx < h)
        return (ws.pair_val.double() * tn[idx.clamp(0, h - 1)] * ok).sum(1).mean().item()
    return (ws.acts[:, :h].double() @ tn).mean().item()


def run_scenario(monkeypatch, config, write, timing="at_once", between=None):
    """-> nothing; asserts.  timing: "at_once" (the write follows step(): the decoder-half Adam is still pending on
    the side stream) or "after_read" (a read of the parameters came first: the deferred rows ran and, on the partial
    path, the norm partials are pending their finaliser).  between: "get_losses" / "get_losses_other_B": a forward on
    the crosscoder's workspace between the write and the step."""
    B, d, h, _, _, flags = CONFIGS[config]
    for k, v in flags.items():
        monkeypatch.setattr(engine, k, v)
    cfg = cfg_of(config)
    A = trainer_of(cfg)
    cc = A.crosscoder
    A.step_counter = 10  # past the l1 warm-up (5 steps), before the lr decay
    A.step()
    held = None
    if write == "load_state_dict" and timing == "at_once":
        sd = {k: v.detach().clone() for k, v in cc.state_dict().items()}
        sd["W_dec"] = sd["W_dec"] * per_model(cc, F)
        held = (sd, A.state_dict())
    A.step()
    assert A.get_l1_coeff() == cfg["l1_coeff"]
    ws, a = A._last_ws, cc.arena()
    # not vacuous: the step left a carry for the next one
    assert ws.norms_token is not None and ws.norms_token == engine._norms_token(a)
    # the norm partials come out of the Adam launches only where the workspace keeps no W_dec^T and the bf16 update
    # runs (master mode's one launch writes none: its norms are derived right after it, norms_for_next)
    partials = ws.W_dec_t is None and ws.norm_part is not None and not A.optimizer.master_mode
    if partials:
        assert a.pending_rest is not None or ws.norms_fin_pending
    else:
        assert a.pending is not None or A.optimizer.master_mode  # (master mode: everything on torch's stream)
    x = batch_of(A)
    if timing == "after_read":
        if cc.activation == "batch_topk":
            cc.encode(x)  # (a read that also fills the cached selection weights)
            assert cc._sel_w is not None
        else:
            cc.W_dec
        assert a.pending is None and a.pending_rest is None
        assert ws.norms_fin_pending == partials
    tn_before = None
    if timing == "after_read":
        tn_before = tn64(cc.W_dec)
    elif write != "none":
        # (no read through the crosscoder before the write, which would order after the side stream: the arena as it
        # is once the device is idle; rows whose Adam is still deferred are one update behind, 1e-3 of their norm)
        torch.cuda.synchronize()
        tn_before = tn64(a.W_dec().clone())

    want = WRITES[write](A, held) if held is not None else WRITES[write](A)
    W_written = cc.W_dec.detach().clone()  # the post-write parameters, before the step's Adam
    if want is not None:
        assert torch.equal(bits(W_written.contiguous()), bits(want.contiguous()))
    tn = tn64(W_written)
    ratio = tn / tn_before if tn_before is not None else torch.ones_like(tn)
    if write in KEEPS_NORMS:
        assert bool(((ratio - 1).abs() <= 0.01).all())
    else:  # a stale carry is off by a third or more
        assert bool((torch.maximum(ratio, 1 / ratio) >= 1.5).all()), (ratio.min().item(), ratio.max().item())

    # the twin: public API only, after the write
    T = trainer_of(cfg)
    T.crosscoder.load_state_dict({k: v.detach().clone() for k, v in cc.state_dict().items()})
    T.load_state_dict(A.state_dict())
    T.buffer.buffer_pointer = A.buffer.buffer_pointer

    if between is not None:
        xb = x if between == "get_losses" else x[:B // 2]
        with torch.no_grad():
            lo = cc.get_losses(xb)
        got, ref = lo.l1_loss.item(), l1_fp64(cc._ws, tn, h)
        print(f"{config} {write} {between}: get_losses l1 {got} fp64 {ref}")
        assert math.isclose(got, ref, rel_tol=1e-2), (got, ref)
    if cc.activation == "batch_topk":
        assert torch.equal(bits(cc.encode(x)), bits(T.crosscoder.encode(x)))

    if write == "none":
        with monkeypatch.context() as m:
            log = record_launches(m)
            la = A.step()
        derived = [name for name, _ in log if name in DERIVES]
        # with the carry the step derives nothing on the partial path (the finaliser rides in G2); elsewhere exactly
        # the pass that follows its Adam (norms_for_next: the norms, and W_dec^T where the workspace keeps one)
        after_adam = 2 if ws.W_dec_t is not None and ws.norm_part is None else 1
        # (a get_losses in between consumed the carry: the step then derives the norms once itself)
        assert len(derived) == (0 if partials else after_adam) + (between is not None), log
    else:
        la = A.step()
    ref = l1_fp64(A._last_ws, tn, h)
    print(f"{config} {write} {timing}: l1_loss {la['l1_loss']} fp64 {ref} (norm ratio {ratio.min().item():.3f}.."
          f"{ratio.max().item():.3f})")
    assert math.isclose(la["l1_loss"], ref, rel_tol=1e-2), (la["l1_loss"], ref)
    lt = T.step()
    assert la == lt, (la, lt)
    sa, st = snapshot(A), snapshot(T)
    assert sa.keys() == st.keys()
    for k in sa:
        assert torch.equal(bits(sa[k]), bits(st[k])), (k, int((bits(sa[k]) != bits(st[k])).sum()))
    assert all(math.isfinite(v) for v in la.values())


def test_undisturbed_step_launches(gpu, monkeypatch):
    """The third of three steps with nothing in between, on the product path: the six launches of the steady state,
    G2 carrying the norm finaliser and waiting in its kernel for the side-stream Adam (the carry's token matched), and
    no pass over W_dec of its own."""
    A = trainer_of(cfg_of("bf16-fused"))
    A.step()
    A.step()
    log = record_launches(monkeypatch)
    A.step()
    assert [name for name, _ in log] == PRODUCT_STEP, log
    riders = dict(log)
    assert riders["decode_loss"] == {"norm_fin", "wait", "pre"}, riders
    assert riders["dacts_bwd_t"] == {"tail"}, riders
    A.synchronize()


@pytest.mark.parametrize("config", list(CONFIGS))
def test_control_no_write(gpu, monkeypatch, config):
    """No write: the carry is used (no derivation launch beyond the step's own) and the twin, which derives everything
    from the parameters, gives the same bits."""
    run_scenario(monkeypatch, config, "none")


DECODER_WRITES = ("load_state_dict", "mul_", "copy_", "fold", "data_assign", "data_mul_params_written")


@pytest.mark.parametrize("timing", ["at_once", "after_read"])
@pytest.mark.parametrize("write", DECODER_WRITES + ("fold_enc", "b_dec", "W_enc"))
def test_write_between_steps_product_path(gpu, monkeypatch, write, timing):
    """Every write on the product path, right after step() and after a read of the parameters."""
    run_scenario(monkeypatch, "bf16-fused", write, timing)


@pytest.mark.parametrize("write", ["load_state_dict", "mul_", "fold"])
@pytest.mark.parametrize("config", [c for c in CONFIGS if c != "bf16-fused"])
def test_write_between_steps(gpu, monkeypatch, config, write):
    """The torch writes and the kernel write under every other configuration, after a read of the parameters (the
    state in which partials pend their finaliser; BatchTopK: in which the selection weights are cached)."""
    run_scenario(monkeypatch, config, write, "after_read")


@pytest.mark.parametrize("write", ["mul_", "fold"])
@pytest.mark.parametrize("config", ["bf16-serial", "bf16-split", "batch-topk", "sparse-topk"])
def test_write_right_after_the_step(gpu, monkeypatch, config, write):
    """The same right after step(), where Adam rows are deferred (split), the partials pend from Adam itself (serial)
    or another workspace than the crosscoder's carries the norms (sparse)."""
    run_scenario(monkeypatch, config, write, "at_once")


@pytest.mark.parametrize("between", ["get_losses", "get_losses_other_B"])
@pytest.mark.parametrize("write,timing", [("mul_", "after_read"), ("fold", "at_once"), ("none", "at_once")])
def test_get_losses_between_write_and_step(gpu, monkeypatch, write, timing, between):
    """A get_losses() under no_grad between the write and the step: on the step's workspace, and with another batch
    size, which replaces the workspace while Arena.pending_rest still refers to the old one."""
    run_scenario(monkeypatch, "bf16-fused", write, timing, between)
