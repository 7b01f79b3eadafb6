"""Master weights (cfg["master_weights"]), the parts that need no GPU: the cfg key and its refusals, what the fp32
masters buy over bf16 Adam state (the two findings of DESIGN.md section 3.16, reproduced with torch on the CPU), the
optimizer's state on a CPU crosscoder (dtypes, the "master" entry, re-seeding after a torch write), the state dicts'
structure and their refusals, and the C ABI's declaration."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, sharded
from crosscoder_amd.crosscoder import master_weights_of
from crosscoder_amd.trainer import FusedAdam
from tests._master_adam_ref import MasterAdamRef, bf16_adam_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg_of(**kw):
    cfg = {"seed": 49, "batch_size": 64, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 6400, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": 100, "seq_len": 1024, "enc_dtype": "bf16", "device": "cpu",
           "dec_init_norm": 0.08, "d_in": 30, "log_every": 100, "save_every": 30000}
    cfg.update(kw)
    return cfg


def trainer_of(cfg):
    return ca.Trainer(cfg, buffer=object(), crosscoder=ca.CrossCoder(cfg))


# ----------------------------------------------------------------------------- cfg
def test_cfg_key():
    assert master_weights_of(cfg_of()) is False
    assert master_weights_of(cfg_of(master_weights=False)) is False
    assert master_weights_of(cfg_of(master_weights=True)) is True


@pytest.mark.parametrize("bad", [1, 0, "true", None, 1.0])
def test_cfg_validation(bad):
    with pytest.raises(ValueError, match="master_weights"):
        master_weights_of(cfg_of(master_weights=bad))
    with pytest.raises(ValueError, match="master_weights"):
        ca.CrossCoder(cfg_of(master_weights=bad))


def test_sharded_trainer_refuses():
    with pytest.raises(ValueError, match="master_weights"):
        sharded.ShardedTrainer(cfg_of(master_weights=True), buffer=None)
    with pytest.raises(ValueError, match="master_weights"):  # (a crosscoder built with the key handed in)
        sharded.ShardedTrainer(cfg_of(), buffer=None, crosscoder=ca.CrossCoder(cfg_of(master_weights=True)))


def test_modes_and_dtypes():
    tr = trainer_of(cfg_of(master_weights=True))
    opt, cc = tr.optimizer, tr.crosscoder
    assert opt.master_mode and opt.master.data.dtype == torch.float32
    assert opt.exp_avg.data.dtype == opt.exp_avg_sq.data.dtype == torch.float32
    assert opt.grads.data.dtype == torch.bfloat16
    for name in ("W_enc", "W_dec", "b_enc", "b_dec"):
        p = getattr(cc, name)
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq", "master"}
        for k in ("exp_avg", "exp_avg_sq", "master"):
            assert st[k].dtype == torch.float32 and st[k].shape == p.shape, (name, k)
        assert torch.equal(st["master"], p.detach().float())  # seeded as float(bf16 params)
    # dict_size 100 / d_in 30 are padded to 104 / 32: the padding is zero in the masters
    a, m = cc.arena(), opt.master
    assert a.padded and m.numel == a.numel
    assert float(m.W_dec_hk[100:].abs().sum()) == 0 and float(m.W_dec_hk.view(104, 2, 32)[:, :, 30:].abs().sum()) == 0
    # default mode: as before
    for cfg in (cfg_of(), cfg_of(master_weights=False)):
        opt = trainer_of(cfg).optimizer
        assert not opt.master_mode and opt.master is None and opt.master_for_update() is None
        assert opt.exp_avg.data.dtype == torch.bfloat16
        assert set(opt.state[opt.cc.W_dec]) == {"step", "exp_avg", "exp_avg_sq"}
    # an fp32 crosscoder: the parameters are their own masters
    opt = trainer_of(cfg_of(master_weights=True, enc_dtype="fp32")).optimizer
    assert not opt.master_mode and opt.master is None and opt.exp_avg.data.dtype == torch.float32
    assert set(opt.state[opt.cc.W_dec]) == {"step", "exp_avg", "exp_avg_sq"}


def test_torch_writes_reseed_only_what_changed():
    tr = trainer_of(cfg_of(master_weights=True))
    opt, cc = tr.optimizer, tr.crosscoder
    a = cc.arena()
    # masters with extra bits that still round to the parameters (as after an update)
    opt.master.data.mul_(1 + 2 ** -12)
    opt.master_updated()
    assert torch.equal(opt.master.data.to(torch.bfloat16), a.data)
    before = opt.master.data.clone()
    assert opt.master_for_update() is opt.master and torch.equal(opt.master.data, before)  # nothing written: kept
    with torch.no_grad():
        cc.W_dec[3:5].mul_(2)
        cc.b_enc[:7] = 0.25
    m = opt.master_for_update().views()
    assert torch.equal(m["W_dec"][3:5], cc.W_dec[3:5].detach().float())
    assert torch.equal(m["b_enc"][:7], torch.full((7,), 0.25))
    changed = opt.master.data != before
    assert int(changed.sum()) == 2 * 2 * 30 + 7  # (W_dec is never exactly 0 here; the padding columns stay 0)
    assert opt._master_token == FusedAdam._arena_token(a)
    # load_state_dict writes every parameter: the same values keep their masters
    kept = opt.master.data.clone()
    cc.load_state_dict(cc.state_dict())
    assert torch.equal(opt.master_for_update().data, kept)


# ----------------------------------------------------------------------------- what the masters are for
def test_large_parameter_moves_only_with_masters():
    """A parameter at 0.1 under 200 steps of same-sign gradient at lr 5e-5: half a bf16 ulp of 0.1 (2^-12 =
    2.4e-4) exceeds every step, so the bf16 parameter never moves; the fp32 master does, by about 200 lr, and its
    bf16 copy changes with it."""
    n = 1000
    g = (torch.rand(n, generator=torch.Generator().manual_seed(0)) * 1e-3 + 1e-4).to(torch.bfloat16)
    p = torch.full((n,), 0.1).to(torch.bfloat16)
    p0 = p.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ref = MasterAdamRef(p0.float())
    for t in range(1, 201):
        bf16_adam_step(p, g, m, v, t)
        p16 = ref.step(g)
    assert int((p != p0).sum()) == 0
    moved = ref.p32.detach() - p0.float()
    assert bool((moved < -6e-3).all()) and bool((moved > -1.1e-2).all()), (moved.min(), moved.max())
    assert bool((p16 != p0).all())
    assert torch.equal(p16, ref.p32.detach().to(torch.bfloat16))


def test_second_moment_decays_only_in_fp32():
    """The gradient scale drops 100x at step 100.  bf16 v = R(v * 0.999) returns v (1e-3 relative is under half an
    ulp), so v never decays: at step 2000 it still reads about its early value, while the fp32 v has decayed by
    e^-1.9 and keeps decaying."""
    n = 256
    gen = torch.Generator().manual_seed(1)
    p = torch.zeros(n, dtype=torch.bfloat16)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ref = MasterAdamRef(p.float())
    v_at = {}
    for t in range(1, 2001):
        scale = 1.0 if t <= 100 else 0.01
        g = (torch.randn(n, generator=gen) * scale).to(torch.bfloat16)
        bf16_adam_step(p, g, m, v, t)
        ref.step(g)
        if t in (100, 2000):
            v_at[t] = (v.float().mean().item(), ref.exp_avg_sq.mean().item())
    (b100, f100), (b2000, f2000) = v_at[100], v_at[2000]
    assert abs(b100 - f100) < 0.3 * f100  # both have seen the same 100 large gradients
    assert b2000 >= 0.95 * b100  # bf16: a ratchet
    assert f2000 < 0.2 * f100  # fp32: 0.999^1900 = 0.149 of it, plus the small gradients' 1e-4
    # every bf16 value is a fixed point of the decay multiply
    x = torch.rand(100000, generator=gen).to(torch.bfloat16) + 2.0 ** -20
    assert torch.equal(x * 0.999, x)


# ----------------------------------------------------------------------------- state dicts
def test_state_dict_structure():
    tr = trainer_of(cfg_of(master_weights=True))
    sd = tr.state_dict()
    assert set(sd) == {"optimizer", "step_counter", "last_epoch"}
    o = sd["optimizer"]
    assert set(o) == {"step", "master_weights", "exp_avg", "exp_avg_sq", "master"} and o["master_weights"] is True
    n = tr.crosscoder.arena().numel
    for k in ("exp_avg", "exp_avg_sq", "master"):
        assert o[k].dtype == torch.float32 and o[k].shape == (n,)
    assert o["master"].data_ptr() != tr.optimizer.master.data.data_ptr()  # clones
    o = trainer_of(cfg_of()).state_dict()["optimizer"]
    assert set(o) == {"step", "master_weights", "exp_avg", "exp_avg_sq"} and o["exp_avg"].dtype == torch.bfloat16
    o = trainer_of(cfg_of(activation="jumprelu", l0_coeff=0.5)).state_dict()["optimizer"]
    assert {"theta_exp_avg", "theta_exp_avg_sq"} <= set(o) and o["theta_exp_avg"].dtype == torch.float32
    sd = trainer_of(cfg_of(activation="topk", k=8, auxk_coeff=0.03)).state_dict()
    assert sd["tokens_since_fired"].dtype == torch.int64 and sd["tokens_since_fired"].shape == (100,)


def test_state_dict_round_trip_on_the_host():
    cfg = cfg_of(master_weights=True, activation="topk", k=8, auxk_coeff=0.03, dead_tokens=128)
    a = trainer_of(cfg)
    gen = torch.Generator().manual_seed(5)
    for t in (a.optimizer.exp_avg.data, a.optimizer.exp_avg_sq.data):
        t.copy_(torch.rand(t.shape, generator=gen))
    a.optimizer.master.data.mul_(1 + 2 ** -12)
    a.optimizer.t = 85
    a.step_counter = 85
    for _ in range(85):
        a.scheduler.step()
    a.tokens_since_fired = torch.arange(100) * 2
    sd = a.state_dict()
    b = trainer_of(cfg)
    b.crosscoder.load_state_dict(a.crosscoder.state_dict())
    b.load_state_dict(sd)
    assert b.optimizer.t == 85 and b.step_counter == 85 and b.scheduler.last_epoch == 85
    assert b.optimizer.param_groups[0]["lr"] == a.optimizer.param_groups[0]["lr"] < cfg["lr"]  # (the decay branch)
    assert b.scheduler.get_last_lr() == a.scheduler.get_last_lr()
    assert torch.equal(b.tokens_since_fired, a.tokens_since_fired) and b._dead_count == a._dead_count == 36
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(b.optimizer, k).data, getattr(a.optimizer, k).data)
    # the masters keep their extra bits: the loaded parameters are their rounding
    assert torch.equal(b.optimizer.master_for_update().data, a.optimizer.master.data)


def test_state_dict_mismatches_raise():
    master, default = trainer_of(cfg_of(master_weights=True)), trainer_of(cfg_of())
    with pytest.raises(ValueError, match="master_weights"):
        default.load_state_dict(master.state_dict())
    with pytest.raises(ValueError, match="master_weights"):
        master.load_state_dict(default.state_dict())
    with pytest.raises(ValueError, match="shape"):  # another dictionary size
        master.load_state_dict(trainer_of(cfg_of(master_weights=True, dict_size=96)).state_dict())
    with pytest.raises(ValueError, match="float32"):  # an fp32 crosscoder's moments into a bf16 one's
        default.load_state_dict(trainer_of(cfg_of(enc_dtype="fp32")).state_dict())
    sd = master.state_dict()
    del sd["optimizer"]["master"]
    with pytest.raises(ValueError, match="master"):
        master.load_state_dict(sd)
    with pytest.raises(ValueError, match="tokens_since_fired"):  # AuxK state into a trainer without it
        default.load_state_dict(trainer_of(cfg_of(activation="topk", k=8, auxk_coeff=0.03)).state_dict())
    with pytest.raises(ValueError, match="theta"):  # a JumpReLU trainer's threshold moments
        default.load_state_dict(trainer_of(cfg_of(activation="jumprelu", l0_coeff=0.5)).state_dict())
    with pytest.raises(ValueError, match="step_counter"):
        default.load_state_dict(dict(default.state_dict(), step_counter=-1))
    with pytest.raises(ValueError):
        default.load_state_dict({"step": 3})
    # nothing was written by the refused loads
    assert default.optimizer.t == 0 and float(default.optimizer.exp_avg.data.abs().sum()) == 0


@pytest.mark.parametrize("bad", ["negative", "shape", "float"])
def test_bad_tokens_since_fired_is_refused_before_the_optimizer_is_loaded(bad):
    """Every entry is checked before the first is written: a good optimizer state beside a tokens_since_fired the
    setter refuses leaves moments, masters, step counts and the lr as they were."""
    cfg = cfg_of(master_weights=True, activation="topk", k=8, auxk_coeff=0.03, dead_tokens=128)
    src, dst = trainer_of(cfg), trainer_of(cfg)
    for t in (src.optimizer.exp_avg.data, src.optimizer.exp_avg_sq.data):
        t.fill_(0.25)
    src.optimizer.master.data.mul_(1 + 2 ** -12)
    src.optimizer.t = src.step_counter = 7
    for _ in range(7):
        src.scheduler.step()
    sd = src.state_dict()
    sd["tokens_since_fired"] = {"negative": torch.full((100,), -1), "shape": torch.zeros(99, dtype=torch.int64),
                                "float": torch.zeros(100)}[bad]
    o = dst.optimizer
    before = [t.clone() for t in (o.exp_avg.data, o.exp_avg_sq.data, o.master.data, dst.tokens_since_fired)]
    lr = o.param_groups[0]["lr"]
    with pytest.raises(ValueError, match="tokens_since_fired"):
        dst.load_state_dict(sd)
    after = (o.exp_avg.data, o.exp_avg_sq.data, o.master.data, dst.tokens_since_fired)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert o.t == 0 and dst.step_counter == 0 and dst.scheduler.last_epoch == 0 and o.param_groups[0]["lr"] == lr


# ----------------------------------------------------------------------------- the C ABI
def test_entry_point_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    assert re.search(r"\bint\s+cc_adam_master_step\s*\(", header)
    lib = _lib.load()
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "cc_adam_master_step" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert len(_lib.SIGNATURES["cc_adam_master_step"][1]) == 14
    # argument checks happen before any launch: null pointers, empty, step 0, misaligned
    f = lib.cc_adam_master_step
    ok = 4096
    assert f(None, ok, ok, ok, ok, 8, None, 1e-3, 0.9, 0.999, 1e-8, 1, 0, None) != 0
    assert f(ok, ok, ok, ok, None, 8, None, 1e-3, 0.9, 0.999, 1e-8, 1, 0, None) != 0
    assert f(ok, ok, ok, ok, ok, 0, None, 1e-3, 0.9, 0.999, 1e-8, 1, 0, None) != 0
    assert f(ok, ok, ok, ok, ok, 8, None, 1e-3, 0.9, 0.999, 1e-8, 0, 0, None) != 0
    assert f(ok, ok + 2, ok, ok, ok, 8, None, 1e-3, 0.9, 0.999, 1e-8, 1, 0, None) != 0
    assert f(ok, ok, ok, ok, ok + 8, 8, None, 1e-3, 0.9, 0.999, 1e-8, 1, 0, None) != 0
