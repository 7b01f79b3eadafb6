"""CPU: the sparse TopK step -- its entry points are declared, exported and typed, validate their arguments in the stated
order before any launch, cfg["sparse_step"] and the Trainer's refusals raise, and the CPU restatements the GPU tests
compare with (tests/_sparse_step_ref.py) agree with ops.pairs_by_latent, with a plain loop and, on a dyadic case where
every sum is exact, with fp64."""
import ctypes
import os
import re
from fractions import Fraction

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, crosscoder, ops
from tests import _pairs_grad_ref as pref
from tests import _sparse_step_ref as ref
from tests.test_cpu_host import _cfg, _dynamic_exports
from tests.test_pairs_grad_host import FAKE, caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DTYPE, SHAPE, ALIGN, TOO_LARGE = 0, 1, 2, 3, 4, 5
NAMES = {"cc_pairs_group_ws_bytes": 3, "cc_pairs_group": 8, "cc_decode_pairs_partial": 12, "cc_pairs_wgrad_ws_floats": 2,
         "cc_pairs_wgrad_parts": 1, "cc_pairs_wgrad": 24}
SIZES = ("cc_pairs_group_ws_bytes", "cc_pairs_wgrad_ws_floats", "cc_pairs_wgrad_parts")


def test_public_names_exist():
    for name in ("pairs_group", "pairs_group_ws_bytes", "decode_pairs_partial", "pairs_wgrad", "pairs_wgrad_ws_floats",
                 "pairs_wgrad_parts"):
        assert callable(getattr(ops, name))
    assert callable(crosscoder.sparse_step_of)
    from crosscoder_amd import engine
    assert callable(engine.forward_sparse) and callable(engine.backward_sparse)


def test_entry_points_are_declared_exported_and_typed():
    raw = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\bint(64_t)?\s+%s\s*\(" % name, txt), name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int64 if name in SIZES else ctypes.c_int) and len(args) == nargs
        assert name in _dynamic_exports(_lib.LIB_PATH)
        assert name in _dynamic_exports(_lib.DEBUG_LIB_PATH)
    lib = _lib.load()
    L = ops.PAIRS_GRAD_SPLIT
    ws = lib.cc_pairs_wgrad_ws_floats
    assert ws(L - 1, 80) == 0 and ws(L, 80) == 168 and ws(5 * L + 3, 4608) == 5 * (2 * 4608 + 8) and ws(0, 80) == 0
    parts = lib.cc_pairs_wgrad_parts
    assert parts(0) == 0 and parts(200) == 200 and parts(1 << 17) == 1 << 16
    assert ref.wgrad_parts(200) == 200 and ref.wgrad_parts(1 << 17) == 1 << 16
    gb = lib.cc_pairs_group_ws_bytes
    # cells h * ceil(B / 256), one sum per 4096 cells, one word per slot; rounded up to 16 bytes
    assert gb(300, 8, 128) == (4 * (128 * 2 + 1 + 2400) + 15) // 16 * 16
    assert gb(4096, 32, 1 << 17) == 4 * ((1 << 21) + 512 + 4096 * 32)
    assert gb(0, 8, 128) == 0 and gb(4, 0, 8) == 0 and gb(4, 8, 0) == 0 and gb(1 << 28, 8, 8) == 0
    assert gb(1 << 20, 1, 1 << 17) == 0          # 2^29 cells


def test_pairs_group_checks_run_in_order_before_any_launch():
    good = dict(idx=FAKE, B=40, k=8, h=64, perm=FAKE + 4096, seg=FAKE + 8192, ws=FAKE + 12288, stream=0)
    call = caller("cc_pairs_group", list(good), good)
    for bad in (dict(B=0), dict(k=0), dict(h=0), dict(B=-1)):
        assert call(**bad) == SHAPE, bad
    assert call(B=0, idx=0) == SHAPE
    for bad in (dict(idx=0), dict(perm=0), dict(seg=0), dict(ws=0)):
        assert call(**bad) == NULL, bad
    assert call(idx=0, h=1 << 31) == NULL
    for bad in (dict(h=1 << 31), dict(k=(1 << 17) + 1), dict(B=1 << 28), dict(B=1 << 20, k=1, h=1 << 17)):
        assert call(**bad) == TOO_LARGE, bad
    assert call(h=1 << 31, ws=FAKE + 8) == TOO_LARGE
    assert call(ws=good["ws"] + 8) == ALIGN
    assert call(seg=good["seg"] + 4) == ALIGN
    for name in ("idx", "perm"):
        assert call(**{name: good[name] + 2}) == ALIGN, name


def test_decode_pairs_partial_checks_run_in_order_before_any_launch():
    good = dict(val=FAKE, idx=FAKE + 4096, B=4, k=8, W_dec=FAKE + 8192, ldw=80, h=64, K=80, dtype=1, recon=FAKE + 12288,
                ldr=80, stream=0)
    call = caller("cc_decode_pairs_partial", list(good), good)
    for bad in (dict(B=0), dict(k=0), dict(h=0), dict(K=0), dict(K=4), dict(K=84, ldw=88, ldr=88), dict(ldw=72),
                dict(ldr=79)):
        assert call(**bad) == SHAPE, bad
    assert call(B=0, val=0, dtype=7) == SHAPE
    for bad in (dict(val=0), dict(idx=0), dict(W_dec=0), dict(recon=0)):
        assert call(**bad) == NULL, bad
    assert call(val=0, dtype=7) == NULL
    assert call(dtype=0) == DTYPE and call(dtype=3) == DTYPE
    assert call(dtype=7, h=1 << 31) == DTYPE
    for bad in (dict(h=1 << 31), dict(k=(1 << 17) + 1), dict(K=1 << 31, ldw=1 << 31, ldr=1 << 31)):
        assert call(**bad) == TOO_LARGE, bad
    for name in ("W_dec", "recon"):
        assert call(**{name: good[name] + 8}) == ALIGN, name
    assert call(ldw=84) == ALIGN and call(ldw=82, dtype=2) == ALIGN
    assert call(ldr=82) == ALIGN                                        # fp32 rows: 328 bytes
    assert call(idx=good["idx"] + 2) == ALIGN
    assert call(val=good["val"] + 1) == ALIGN and call(val=good["val"] + 2, dtype=2) == ALIGN


def test_pairs_wgrad_checks_run_in_order_before_any_launch():
    names = ("perm", "P", "seg", "h", "val", "g_pre", "B", "k", "g_recon", "ldg", "x", "ldx", "K", "dtype", "dW_dec",
             "ld_dec", "dW_enc", "ld_enc", "db_enc", "sq_dec", "sq_enc", "sq_b_enc", "ws", "stream")
    ptrs = [n for n in names if n in ("perm", "seg", "val", "g_pre", "g_recon", "x", "dW_dec", "dW_enc", "db_enc", "sq_dec",
                                      "sq_enc", "sq_b_enc", "ws")]
    good = dict(P=300, h=64, B=40, k=8, ldg=80, ldx=80, K=80, dtype=1, ld_dec=80, ld_enc=80, stream=0)
    good.update({n: FAKE + 4096 * i for i, n in enumerate(ptrs)})
    call = caller("cc_pairs_wgrad", list(names), good)
    for bad in (dict(B=0), dict(k=0), dict(h=0), dict(P=-1), dict(K=0), dict(K=4), dict(K=84), dict(ldg=72), dict(ldx=72),
                dict(ld_dec=79), dict(ld_enc=72)):
        assert call(**bad) == SHAPE, bad
    assert call(B=0, seg=0, dtype=7) == SHAPE
    for name in ptrs:
        assert call(**{name: 0}) == NULL, name
    assert call(seg=0, dtype=7, k=(1 << 17) + 1) == NULL
    assert call(dtype=0) == DTYPE and call(dtype=3) == DTYPE
    assert call(dtype=7, h=1 << 31) == DTYPE
    for bad in (dict(h=1 << 31), dict(k=(1 << 17) + 1), dict(B=1 << 28), dict(P=1 << 31),
                dict(K=1 << 31, ldg=1 << 31, ldx=1 << 31, ld_dec=1 << 31, ld_enc=1 << 31)):
        assert call(**bad) == TOO_LARGE, bad
    assert call(h=1 << 31, x=good["x"] + 8) == TOO_LARGE
    for name in ("g_recon", "x", "dW_dec", "dW_enc", "ws"):
        assert call(**{name: good[name] + 8}) == ALIGN, name
    for name in ("ldg", "ldx", "ld_dec", "ld_enc"):
        assert call(**{name: 84}) == ALIGN, name
        assert call(**{name: 82}, dtype=2) == ALIGN, name
    assert call(seg=good["seg"] + 4) == ALIGN
    for name in ("perm", "g_pre", "sq_dec", "sq_enc", "sq_b_enc"):
        assert call(**{name: good[name] + 2}) == ALIGN, name
    for name in ("val", "db_enc"):
        assert call(**{name: good[name] + 1}) == ALIGN, name
        assert call(**{name: good[name] + 2}, dtype=2) == ALIGN, name
    # perm may be missing with P = 0 and ws below one full piece: these fail later
    assert call(perm=0, P=0, ws=0, x=good["x"] + 8) == ALIGN
    assert call(P=ops.PAIRS_GRAD_SPLIT - 1, ws=0, x=good["x"] + 8) == ALIGN


def test_topk_rows_takes_pairs_and_slabs_without_a_dense_output():
    """The sparse step's call of cc_topk_rows: pairs and both slabs, no dense output -- it passes every check (the
    misaligned activations are reported last, so everything before them was accepted)."""
    sig = _lib.SIGNATURES["cc_topk_rows"][1]
    args = dict(acts=FAKE + 8, ld=64, B=4, h=64, dtype=1, k=8, acts_out=0, idx_out=FAKE + 4096, val_out=FAKE + 8192,
                colsum_part=FAKE + 12288, l0_part=FAKE + 16384, stream=0)
    vals = [ctypes.c_void_p(v) if t is ctypes.c_void_p else v for v, t in zip(args.values(), sig)]
    assert _lib.load().cc_topk_rows(*vals) == ALIGN


# ---------------------------------------------------------------- cfg["sparse_step"] and the Trainer's refusals
def sparse_cfg(**kw):
    cfg = dict(_cfg(), activation="topk", k=8, l1_coeff=0.0, sparse_step=True)
    cfg.update(kw)
    return cfg


def test_sparse_step_of():
    assert crosscoder.sparse_step_of(_cfg()) is False
    assert crosscoder.sparse_step_of(dict(_cfg(), sparse_step=False)) is False
    assert crosscoder.sparse_step_of(dict(_cfg(), activation="batch_topk", k=4, sparse_step=False)) is False
    assert crosscoder.sparse_step_of(sparse_cfg()) is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="sparse_step"):
            crosscoder.sparse_step_of(sparse_cfg(sparse_step=bad))
    for act in ({}, {"activation": "relu"}, {"activation": "batch_topk", "k": 4},
                {"activation": "jumprelu", "l0_coeff": 0.1}):
        cfg = {k: v for k, v in sparse_cfg().items() if k not in ("activation", "k")}
        cfg.update(act)
        with pytest.raises(ValueError, match="topk"):
            crosscoder.sparse_step_of(cfg)
        with pytest.raises(ValueError, match="topk"):
            ca.CrossCoder(cfg)
    with pytest.raises(ValueError, match="sparse_step"):
        ca.CrossCoder(sparse_cfg(sparse_step=1))


class _NoBuffer:
    pass


def test_trainer_refusals_name_their_reason():
    def trainer(cfg, **kw):
        return ca.Trainer(cfg, buffer=_NoBuffer(), crosscoder=ca.CrossCoder(cfg), **kw)

    tr = trainer(sparse_cfg())
    assert tr.sparse_step is True
    assert trainer(sparse_cfg(master_weights=True)).sparse_step is True
    dense = {k: v for k, v in sparse_cfg().items() if k != "sparse_step"}
    assert trainer(dense).sparse_step is False and trainer(dict(dense, l1_coeff=2.0)).sparse_step is False
    with pytest.raises(ValueError, match="l1_coeff"):
        trainer(sparse_cfg(l1_coeff=2.0))
    with pytest.raises(ValueError, match="auxk_coeff"):
        trainer(sparse_cfg(auxk_coeff=0.03125))
    with pytest.raises(ValueError, match="resample_every"):
        trainer(sparse_cfg(resample_every=10))
    cfg = sparse_cfg()
    cc = ca.CrossCoder(cfg)
    with pytest.raises(ValueError, match="latent_stats"):
        ca.Trainer(cfg, buffer=_NoBuffer(), crosscoder=cc, latent_stats=ca.LatentStats(cc, k=4))


def test_cfg_key_travels_in_the_checkpoint(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cc = ca.CrossCoder(sparse_cfg())
    cc.save()
    loaded = ca.CrossCoder.load("version_0", 0)
    assert loaded.cfg["sparse_step"] is True and loaded.activation == "topk" and loaded.k == 8


# ---------------------------------------------------------------- the restatements
def test_fma32_is_correctly_rounded():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(2000, generator=g), torch.randn(2000, generator=g)
    c = -(a * b) + torch.randn(2000, generator=g) * 1e-7          # heavy cancellation: the product's low bits decide
    c[:500] = torch.randn(500, generator=g)
    got = ref.fma32(a, b, c)
    for i in range(0, 2000, 7):
        exact = Fraction(a[i].item()) * Fraction(b[i].item()) + Fraction(c[i].item())
        r = got[i].item()
        lo, hi = torch.nextafter(got[i], torch.tensor(-float("inf"))).item(), torch.nextafter(got[i], torch.tensor(float("inf"))).item()
        assert abs(Fraction(r) - exact) <= min(abs(Fraction(lo) - exact), abs(Fraction(hi) - exact)), i
    # a tie between two fp32 neighbours that a double rounding through fp64 gets wrong without the odd step
    one, u = torch.tensor(1.0), torch.tensor(2.0 ** -24)
    assert ref.fma32(one + 2 * u, one, u + u * 2.0 ** -30).item() == 1.0 + 4 * 2.0 ** -24


HAND = torch.tensor([[5, -1, 5, 9], [200, 5, 0, 5], [-7, 9, 9, 9], [0, 63, 64, -2 ** 31], [5, 5, 5, 5]], dtype=torch.int32)


@pytest.mark.parametrize("case", ["hand", "k1", "blocks", "random"])
def test_grouping_restatement_agrees_with_pairs_by_latent(case):
    g = torch.Generator().manual_seed(11)
    if case == "hand":
        idx, h = HAND, 64
    elif case == "k1":
        idx, h = torch.randint(-2, 12, (37, 1), generator=g, dtype=torch.int32), 10
    elif case == "blocks":  # three row blocks; latent 2 in every row, twice in some
        idx, h = torch.randint(0, 40, (600, 4), generator=g, dtype=torch.int32), 40
        idx[:, 1] = 2
        idx[::7, 3] = 2
    else:
        idx, h = torch.randint(-3, 300, (300, 8), generator=g, dtype=torch.int32), 256
    perm, seg = ops.pairs_by_latent(idx, h)
    lp, ls = pref.by_latent_loop(idx, h)
    assert seg.tolist() == ls and perm[:ls[-1]].tolist() == lp
    for shuffle in (0, 1):
        gp, gs = ref.group_cells(idx, h, shuffle_seed=shuffle)
        assert torch.equal(gs, seg) and torch.equal(gp[:ls[-1]], perm[:ls[-1]])
        assert bool((gp >= 0).all()) and bool((gp < idx.numel()).all())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_restatements_are_exact_on_a_dyadic_case(dt):
    """Small integers times 2^-3 everywhere: every product and partial sum is exact in fp32 and the results are bf16
    values, so each restatement equals fp64 bit for bit, whatever its order."""
    B, n, d, h, k = 300, 2, 16, 40, 4
    K = n * d
    g = torch.Generator().manual_seed(23)
    q = lambda *s: (torch.randint(-4, 5, s, generator=g).float() / 8).to(dt)  # noqa: E731
    W, gr, x, val = q(h, K), q(B, K), q(B, K), q(B, k)
    gpre = q(B, k).float()
    idx = torch.randint(-1, h - 8, (B, k), generator=g, dtype=torch.int32)      # -1 padding; latents h-9 .. h-1 never occur
    idx[:, 0] = 5                                                               # 300 entries: two full pieces and a rest
    perm, seg = ops.pairs_by_latent(idx, h)
    assert int(seg[6] - seg[5]) >= B > 2 * ref.SPLIT
    # the partial decode
    assert torch.equal(ref.decode_partial_f32(val, idx, W, h, K).double(), ref.decode_partial_f64(val, idx, W, h, K))
    # both weight gradients and db_enc against a dense fp64 contraction
    ok = (idx >= 0) & (idx < h)
    z = torch.zeros((), dtype=torch.float64)

    def dense(coef):
        a = torch.zeros(B, h, dtype=torch.float64)
        return a.scatter_add_(1, idx.long().clamp(0, h - 1), torch.where(ok, coef.double(), z))

    dW_dec = ref.lists_f32(perm, seg, val, gr, K)
    dW_enc = ref.lists_f32(perm, seg, gpre, x, K)
    db = ref.lists_sum_f32(perm, seg, gpre)
    assert torch.equal(dW_dec.double(), dense(val).t() @ gr.double())
    assert torch.equal(dW_enc.double(), dense(gpre).t() @ x.double())
    assert torch.equal(db.double(), dense(gpre).sum(0))
    assert bool((dW_dec[h - 8:] == 0).all()) and bool((db[h - 8:] == 0).all())
    # for bf16 operands lists_f32 is the parent's restatement of cc_pairs_grad_decoder
    if dt == torch.bfloat16:
        assert torch.equal(dW_dec, pref.decoder_f32(perm, seg, val, gr, K))
    # the squared sums: the stored values are multiples of 2^-6 below 2^7, their squares and sums exact
    for stored in (dW_dec.to(dt), db.to(dt)):
        part = ref.sq_partials(stored)
        assert part.shape == (h,)
        want = stored.double().pow(2).sum(-1) if stored.dim() == 2 else stored.double().pow(2)
        assert torch.equal(part.double(), want)
    assert ref.sq_chain_depth(h, K) == 18 and ref.sq_chain_depth(1 << 17, 4608) == 8 * 3 * 2 + 10


def test_skewed_case_meets_its_three_conditions():
    c = ref.make_case(300, 2, 32, 128, 8, torch.bfloat16, skew=True)
    ref.assert_skewed(c["idx"], 128, 8)
