"""The token logic of what a step carries to the next one, driven on the host: the real
engine.adam, engine.forward, Arena.wait_pending, CrossCoder accessors, params_written and the scaling-factor fold over
CPU tensors, with every kernel launch replaced by a recorder and the streams and events by stand-ins.  Every sequence
of up to five events out of adam / read / write (torch, kernel, .data + params_written) / forward is enumerated: a
forward re-derives the decoder norms exactly when no Adam launch left them or the parameters were written since, it
never finalises norm partials over norms it re-derived, and with a valid carry it derives nothing."""
import contextlib
import itertools

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _hip, engine, ops

STUBBED = ("prep_input", "reduce_rows", "dec_norms", "encode_fwd", "encode_fwd_t", "colsum_job", "decode_partial_jobs",
           "decode_partial_t", "decode_loss", "loss_fwd_bwd", "transpose", "transpose_dec_norms", "dec_norms_finalize",
           "adam_dec_norms", "adam_step", "adam_step_prep", "adam_step_clip", "prep_job", "prep_job_ok", "fold_scaling")
DERIVES = ("dec_norms", "transpose", "transpose_dec_norms")
EVENTS = ("adam", "read", "write_torch", "write_kernel", "write_data", "forward")
# (B, d, h, dtype, forward's loss=, engine flags): the fused G2, the latent-sharded step's G2 (decode_partial_jobs
# carries the finaliser), the serial decoder-half Adam, and a workspace without partials (norms_for_next)
FORMS = {"fused": (256, 64, 512, "bf16", True, {}), "partial_jobs": (256, 64, 512, "bf16", False, {}),
         "serial": (256, 64, 512, "bf16", True, {"DEC_ADAM_BESIDE_G1": False}),
         "split": (256, 64, 512, "bf16", True, {"DEC_SIDE_ROWS": 0.5}),
         "no_partials": (64, 32, 256, "fp32", True, {})}


class _Event:
    def record(self, stream=None):
        return self

    def wait(self, stream=None):
        pass


@pytest.fixture
def host_engine(monkeypatch):
    """-> the log every stubbed launch appends (name, norm_fin given) to."""
    log = []
    for name in STUBBED:
        def stub(*a, _name=name, **k):
            log.append((_name, k.get("norm_fin") is not None))
            return 1
        monkeypatch.setattr(ops, name, stub)
    monkeypatch.setattr(_hip, "DeviceEvent", _Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: "main")
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(engine, "_wait_err", lambda ws: 0)
    return log


def make(form):
    B, d, h, dtype, _, _ = FORMS[form]
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 1e-3, "num_tokens": B * 100, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": dtype, "device": "cpu",
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    cc = ca.CrossCoder(cfg)
    P = cc.arena()
    ws = engine.StepWorkspace(B, 2, d, h, cc.dtype, "cpu")
    x = torch.zeros(B, 2, d, dtype=cc.dtype)
    return cc, P, ws, x


def run(log, form, seq):
    """Drives `seq` and checks every forward against the model: carry = an Adam launch left the norms and neither a
    forward consumed them nor a write came since."""
    cc, P, ws, x = make(form)
    loss = FORMS[form][4]
    partials = ws.W_dec_t is None and ws.norm_part is not None
    G, M, V = P.like(), P.like(), P.like()
    carry = False
    for i, ev in enumerate(seq):
        del log[:]
        if ev == "adam":
            engine.adam(ws, P, G, M, V, 1e-3, 0.9, 0.999, 1e-8, 1, side_stream="side")
            carry = True
        elif ev == "read":
            cc.W_dec
            assert P.pending is None and P.pending_rest is None
        elif ev == "write_torch":
            with torch.no_grad():
                cc.W_dec.mul_(1.0)
            carry = False
        elif ev == "write_kernel":
            ca.fold_activation_scaling_factor(cc, 0.25, 0.5)
            assert ("fold_scaling", False) in log
            carry = False
        elif ev == "write_data":
            cc.W_dec.data.mul_(1.0)
            cc.params_written()
            carry = False
        else:
            engine.forward(ws, P, x, None, loss=loss, finalize=False)
            names = [n for n, _ in log]
            derived = [n for n in names if n in DERIVES]
            finalised = ("dec_norms_finalize" in names) or any(nf for _, nf in log)
            where = (form, seq, i, log)
            assert bool(derived) == (not carry), where
            assert finalised == (carry and partials), where
            assert not ws.norms_fin_pending and ws.norms_token is None, where
            assert P.pending is None or P.pending_ordered == "main", where
            assert P.pending_rest is None, where
            carry = False


@pytest.mark.parametrize("form", list(FORMS))
def test_every_sequence_of_adam_read_write_forward(host_engine, monkeypatch, form):
    for k, v in FORMS[form][5].items():
        monkeypatch.setattr(engine, k, v)
    n = 0
    for length in range(1, 5):
        for seq in itertools.product(EVENTS, repeat=length):
            if seq[-1] != "forward":
                continue
            run(host_engine, form, seq)
            n += 1
    assert n == 1 + 6 + 36 + 216


def test_another_workspace_on_the_arena(host_engine):
    """Two workspaces on one arena (the crosscoder's and a Trainer's own, as the sparse step's): the Adam of one leaves
    its carry there, a forward on the other derives its own norms and leaves the first's carry alone; a kernel write
    invalidates both."""
    cc, P, ws, x = make("fused")
    other = engine.StepWorkspace(256, 2, 64, 512, cc.dtype, "cpu")
    G, M, V = P.like(), P.like(), P.like()
    engine.adam(ws, P, G, M, V, 1e-3, 0.9, 0.999, 1e-8, 1, side_stream="side")
    del host_engine[:]
    engine.forward(other, P, x, None, finalize=False)
    assert ("dec_norms", False) in host_engine and not any(nf for _, nf in host_engine)
    assert ws.norms_token == engine._norms_token(P) and ws.norms_fin_pending  # (the wait ran the deferred rows)
    ca.fold_activation_scaling_factor(cc, 0.25, 0.5)
    for w in (ws, other):
        del host_engine[:]
        engine.forward(w, P, x, None, finalize=False)
        assert ("dec_norms", False) in host_engine and not any(nf for _, nf in host_engine), w is ws
        assert "dec_norms_finalize" not in [n for n, _ in host_engine]


def test_a_repacked_arena_never_matches_an_old_token(host_engine):
    """cc.W_dec.data = new re-packs the arena: the token of a workspace on the old one does not match the new arena,
    whatever address it got."""
    cc, P, ws, x = make("fused")
    tok = engine._norms_token(P)
    cc.W_dec.data = cc.W_dec.data.clone()
    P2 = cc.arena()
    assert P2 is not P and engine._norms_token(P2) != tok
    P2.data = P.data  # (the worst case: the same storage, version and update count)
    P2.W_dec_hk = P.W_dec_hk
    assert engine._norms_token(P2) != tok
