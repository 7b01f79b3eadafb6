"""CPU: AuxK under the sparse TopK step -- cfg["auxk_compact"] and the Trainer's rules, the key
in the checkpoint's cfg json, the three entry points declared, exported and typed, and their argument checks in the
stated order before any launch."""
import ctypes
import os
import re

import pytest

import crosscoder_amd as ca
from crosscoder_amd import _lib, crosscoder, engine, ops
from crosscoder_amd.sharded import ShardedTrainer
from tests.test_cpu_host import _cfg, _dynamic_exports
from tests.test_pairs_grad_host import FAKE, caller
from tests.test_sparse_step_host import _NoBuffer, sparse_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DTYPE, SHAPE, ALIGN, TOO_LARGE = 0, 1, 2, 3, 4, 5
NAMES = {"cc_dead_compact": 9, "cc_compact_gather": 14, "cc_pairs_wgrad_add": 31}


def aux_cfg(**kw):
    return sparse_cfg(**dict(dict(auxk_coeff=0.03125, auxk_compact=True), **kw))


# ---------------------------------------------------------------- the cfg key and the Trainer
def test_auxk_compact_of():
    assert crosscoder.auxk_compact_of(_cfg()) is False
    assert crosscoder.auxk_compact_of(sparse_cfg()) is False
    assert crosscoder.auxk_compact_of(sparse_cfg(auxk_coeff=0.03125, auxk_compact=False)) is False
    assert crosscoder.auxk_compact_of(aux_cfg()) is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="auxk_compact"):
            crosscoder.auxk_compact_of(aux_cfg(auxk_compact=bad))
        with pytest.raises(ValueError, match="auxk_compact"):
            ca.CrossCoder(aux_cfg(auxk_compact=bad))
    # the key without its partners
    for coeff in ({}, {"auxk_coeff": 0}, {"auxk_coeff": 0.0}):
        cfg = dict(sparse_cfg(auxk_compact=True), **coeff)
        with pytest.raises(ValueError, match="auxk_coeff"):
            crosscoder.auxk_compact_of(cfg)
        with pytest.raises(ValueError, match="auxk_coeff"):
            ca.CrossCoder(cfg)
    dense = {k: v for k, v in aux_cfg().items() if k != "sparse_step"}
    for cfg in (dense, dict(dense, sparse_step=False)):
        with pytest.raises(ValueError, match="built for the sparse step only"):
            crosscoder.auxk_compact_of(cfg)
        with pytest.raises(ValueError, match="built for the sparse step only"):
            ca.CrossCoder(cfg)


def test_trainer_serves_the_combination_only_with_the_key():
    def trainer(cfg, **kw):
        return ca.Trainer(cfg, buffer=_NoBuffer(), crosscoder=ca.CrossCoder(cfg), **kw)

    # the old refusal stands, and now names the key
    with pytest.raises(ValueError, match="auxk_coeff") as e:
        trainer(sparse_cfg(auxk_coeff=0.03125))
    assert "auxk_compact" in str(e.value)
    with pytest.raises(ValueError, match="auxk_coeff"):
        trainer(sparse_cfg(auxk_coeff=0.03125, auxk_compact=False))
    tr = trainer(aux_cfg())
    assert tr.sparse_step is True and tr.auxk_compact is True and tr.auxk == (0.03125, tr.auxk[1], 10_000_000)
    assert trainer(aux_cfg(master_weights=True)).auxk_compact is True
    assert trainer(sparse_cfg()).auxk_compact is False
    # what the sparse step refuses stays refused
    with pytest.raises(ValueError, match="resample_every"):
        trainer(aux_cfg(resample_every=10))
    with pytest.raises(ValueError, match="l1_coeff"):
        trainer(aux_cfg(l1_coeff=2.0))
    cfg = aux_cfg()
    cc = ca.CrossCoder(cfg)
    with pytest.raises(ValueError, match="latent_stats"):
        ca.Trainer(cfg, buffer=_NoBuffer(), crosscoder=cc, latent_stats=ca.LatentStats(cc, k=4))
    # the latent-sharded trainer keeps refusing AuxK
    with pytest.raises(ValueError, match="topk"):
        ShardedTrainer(aux_cfg(), buffer=_NoBuffer())
    with pytest.raises(ValueError, match="auxk_coeff"):   # (whatever the activation says)
        ShardedTrainer(dict(_cfg(), auxk_coeff=0.03125, auxk_compact=True, sparse_step=True), buffer=_NoBuffer())


def test_cfg_key_travels_in_the_checkpoint(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cc = ca.CrossCoder(aux_cfg(k_aux=16, dead_tokens=4096))
    cc.save()
    loaded = ca.CrossCoder.load("version_0", 0)
    assert loaded.cfg["auxk_compact"] is True and loaded.cfg["sparse_step"] is True
    assert loaded.auxk == (0.03125, 16, 4096)
    assert ca.Trainer(loaded.cfg, buffer=_NoBuffer(), crosscoder=loaded).auxk_compact is True


def test_padding_and_capacity_rules():
    g = engine.AUX_GRANULE
    assert g >= 8 and g % 8 == 0
    assert engine.aux_pad(1) == g and engine.aux_pad(g) == g and engine.aux_pad(g + 1) == 2 * g
    assert engine.aux_pad(0) == g     # (never a GEMM of extent 0)
    assert engine.AUX_CAP_FRACTION >= 1


# ---------------------------------------------------------------- the entry points
def test_public_names_exist():
    for name in ("dead_compact", "compact_gather", "pairs_wgrad_add"):
        assert callable(getattr(ops, name))
    assert callable(engine.auxk_forward_sparse) and callable(crosscoder.auxk_compact_of)


def test_entry_points_are_declared_exported_and_typed():
    raw = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert name in _dynamic_exports(_lib.LIB_PATH)
        assert name in _dynamic_exports(_lib.DEBUG_LIB_PATH)
    # cc_pairs_wgrad_add is cc_pairs_wgrad's signature, the addends before the stream
    assert _lib.SIGNATURES["cc_pairs_wgrad_add"][1][:23] == _lib.SIGNATURES["cc_pairs_wgrad"][1][:23]


def test_dead_compact_checks_run_in_order_before_any_launch():
    good = dict(since_fired=FAKE, h=208, h_real=200, dead_after=1000, ids=FAKE + 4096, d_pad=16, slot=FAKE + 8192,
                count=FAKE + 12288, stream=0)
    call = caller("cc_dead_compact", list(good), good)
    for bad in (dict(h=0), dict(h_real=-1), dict(h_real=209), dict(d_pad=0), dict(d_pad=12), dict(d_pad=-8)):
        assert call(**bad) == SHAPE, bad
    assert call(h=0, ids=0) == SHAPE
    for name in ("since_fired", "ids", "slot", "count"):
        assert call(**{name: 0}) == NULL, name
    assert call(ids=0, h=1 << 18, h_real=0) == NULL
    assert call(h=(1 << 17) + 8) == TOO_LARGE and call(d_pad=(1 << 17) + 8) == TOO_LARGE
    assert call(h=1 << 18, ids=FAKE + 2) == TOO_LARGE
    assert call(since_fired=FAKE + 4) == ALIGN
    for name in ("ids", "slot", "count"):
        assert call(**{name: good[name] + 2}) == ALIGN, name


def test_compact_gather_checks_run_in_order_before_any_launch():
    names = ("ids", "d_pad", "h", "W", "ldw", "K", "Wc", "ldc", "acts", "lda", "B", "acts_c", "dtype", "stream")
    good = dict(ids=FAKE, d_pad=16, h=200, W=FAKE + 4096, ldw=80, K=80, Wc=FAKE + 8192, ldc=80, acts=FAKE + 12288,
                lda=208, B=40, acts_c=FAKE + 16384, dtype=1, stream=0)
    call = caller("cc_compact_gather", list(names), good)
    for bad in (dict(d_pad=0), dict(d_pad=12), dict(h=0), dict(K=0), dict(K=4), dict(K=84, ldw=88, ldc=88), dict(ldw=72),
                dict(ldc=79), dict(B=0), dict(lda=199)):
        assert call(**bad) == SHAPE, bad
    assert call(d_pad=0, ids=0, dtype=7) == SHAPE
    # a group left out takes no shape of its own
    assert call(W=0, Wc=0, K=0, ids=0) == NULL and call(acts=0, acts_c=0, B=0, ids=0) == NULL
    for bad in (dict(ids=0), dict(W=0), dict(Wc=0), dict(acts=0), dict(acts_c=0), dict(W=0, Wc=0, acts=0, acts_c=0),
                dict(Wc=good["W"]), dict(acts_c=good["acts"])):
        assert call(**bad) == NULL, bad
    assert call(ids=0, dtype=7) == NULL
    assert call(dtype=0) == DTYPE and call(dtype=3) == DTYPE
    assert call(dtype=7, h=1 << 31, lda=1 << 31) == DTYPE
    for bad in (dict(h=1 << 31, lda=1 << 31), dict(d_pad=(1 << 17) + 8), dict(K=1 << 31, ldw=1 << 31, ldc=1 << 31),
                dict(B=(1 << 20) + 1)):
        assert call(**bad) == TOO_LARGE, bad
    assert call(ids=FAKE + 2) == ALIGN
    for name in ("W", "Wc", "acts_c"):
        assert call(**{name: good[name] + 8}) == ALIGN, name
    assert call(acts=good["acts"] + 1) == ALIGN and call(acts=good["acts"] + 2, dtype=2) == ALIGN
    assert call(ldw=84) == ALIGN and call(ldc=84) == ALIGN and call(ldw=82, dtype=2) == ALIGN


def test_pairs_wgrad_add_checks_run_in_order_before_any_launch():
    names = ("perm", "P", "seg", "h", "val", "g_pre", "B", "k", "g_recon", "ldg", "x", "ldx", "K", "dtype", "dW_dec",
             "ld_dec", "dW_enc", "ld_enc", "db_enc", "sq_dec", "sq_enc", "sq_b_enc", "ws", "slot", "d_pad", "aWd", "lda_d",
             "aWe", "lda_e", "ab", "stream")
    base = ("perm", "seg", "val", "g_pre", "g_recon", "x", "dW_dec", "dW_enc", "db_enc", "sq_dec", "sq_enc", "sq_b_enc", "ws")
    addends = ("slot", "aWd", "aWe", "ab")
    good = dict(P=300, h=64, B=40, k=8, ldg=80, ldx=80, K=80, dtype=1, ld_dec=80, ld_enc=80, d_pad=16, lda_d=80, lda_e=80,
                stream=0)
    good.update({n: FAKE + 4096 * i for i, n in enumerate(base + addends)})
    call = caller("cc_pairs_wgrad_add", list(names), good)
    # cc_pairs_wgrad's own checks, in its order
    for bad in (dict(B=0), dict(k=0), dict(h=0), dict(P=-1), dict(K=0), dict(K=4), dict(K=84), dict(ldg=72), dict(ldx=72),
                dict(ld_dec=79), dict(ld_enc=72), dict(d_pad=0), dict(d_pad=-8), dict(lda_d=72), dict(lda_e=79)):
        assert call(**bad) == SHAPE, bad
    assert call(B=0, seg=0, dtype=7) == SHAPE
    for name in base + addends:
        assert call(**{name: 0}) == NULL, name
    assert call(slot=0, aWd=0, aWe=0) == NULL       # some addends without the others
    assert call(seg=0, dtype=7, k=(1 << 17) + 1) == NULL
    assert call(dtype=0) == DTYPE and call(dtype=3) == DTYPE
    for bad in (dict(h=1 << 31), dict(k=(1 << 17) + 1), dict(B=1 << 28), dict(P=1 << 31), dict(d_pad=1 << 31)):
        assert call(**bad) == TOO_LARGE, bad
    for name in ("g_recon", "x", "dW_dec", "dW_enc", "ws", "aWd", "aWe"):
        assert call(**{name: good[name] + 8}) == ALIGN, name
    for name in ("ldg", "ldx", "ld_dec", "ld_enc", "lda_d", "lda_e"):
        assert call(**{name: 84}) == ALIGN, name
        assert call(**{name: 82}, dtype=2) == ALIGN, name
    assert call(seg=good["seg"] + 4) == ALIGN
    for name in ("perm", "g_pre", "sq_dec", "sq_enc", "sq_b_enc", "slot"):
        assert call(**{name: good[name] + 2}) == ALIGN, name
    for name in ("val", "db_enc", "ab"):
        assert call(**{name: good[name] + 1}) == ALIGN, name
        assert call(**{name: good[name] + 2}, dtype=2) == ALIGN, name
    # without any addend it is cc_pairs_wgrad: its shape rules for them do not apply, and a later check still answers
    none = dict(slot=0, aWd=0, aWe=0, ab=0)
    assert call(**none, d_pad=0, lda_d=0, lda_e=0, x=good["x"] + 8) == ALIGN
