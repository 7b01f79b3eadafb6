"""CPU: the sparse decode's public surface (cc_decode_pairs, ops.decode_pairs, CrossCoder.encode_pairs / decode_pairs /
pairs_sq_err, LatentAblation) exists and validates its arguments before any launch, and the CPU restatements the GPU
tests compare with (tests/_decode_pairs_ref.py) agree with each other within their derived bound."""
import ctypes
import os
import re

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, ops
from tests import _decode_pairs_ref as ref
from tests.test_cpu_host import _cfg, _dynamic_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DTYPE, SHAPE, ALIGN, TOO_LARGE = 0, 1, 2, 3, 4, 5


def test_public_names_exist():
    assert callable(ca.LatentAblation)
    for name in ("encode_pairs", "decode_pairs", "pairs_sq_err"):
        assert callable(getattr(ca.CrossCoder, name))
    assert callable(ops.decode_pairs)


def test_entry_point_is_declared_exported_and_typed():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+cc_decode_pairs\s*\(", txt)
    res, args = _lib.SIGNATURES["cc_decode_pairs"]
    assert res is ctypes.c_int and len(args) == 17
    assert "cc_decode_pairs" in _dynamic_exports(_lib.LIB_PATH)
    assert "cc_decode_pairs" in _dynamic_exports(_lib.DEBUG_LIB_PATH)


FAKE = 1 << 20  # a 16-byte aligned address that is never dereferenced: every call below fails a check first
GOOD = dict(val=FAKE, idx=FAKE + 4096, B=4, k=8, W_dec=FAKE + 8192, ldw=80, h=64, b_dec=FAKE + 12288, n=2, d=40, dtype=1,
            recon=FAKE + 16384, ldr=80, x=FAKE + 20480, ldx=80, sq_err=FAKE + 24576, stream=0)


def call(**kw):
    a = dict(GOOD, **kw)
    assert a != GOOD, "a call with valid arguments would launch"
    p = lambda v: ctypes.c_void_p(v)  # noqa: E731
    return _lib.load().cc_decode_pairs(p(a["val"]), p(a["idx"]), a["B"], a["k"], p(a["W_dec"]), a["ldw"], a["h"],
                                       p(a["b_dec"]), a["n"], a["d"], a["dtype"], p(a["recon"]), a["ldr"], p(a["x"]),
                                       a["ldx"], p(a["sq_err"]), p(a["stream"]))


def test_c_abi_checks_run_in_order_before_any_launch():
    # 1. shape
    for bad in (dict(B=0), dict(k=0), dict(h=0), dict(n=0), dict(d=0), dict(d=4), dict(d=12), dict(d=44), dict(ldw=79),
                dict(ldr=72), dict(ldx=79), dict(n=1 << 62, d=8)):
        assert call(**bad) == SHAPE, bad
    assert call(ldr=0, recon=0, ldw=72) == SHAPE          # (ldw is checked with or without recon)
    # ... a pitch is only checked for an operand that is given: these fall through to the pointer checks
    assert call(recon=0, ldr=0, val=0) == NULL
    assert call(x=0, ldx=0, sq_err=0, val=0) == NULL
    # ... and shape comes first
    assert call(B=0, val=0, dtype=7) == SHAPE
    # 2. null
    for bad in (dict(val=0), dict(idx=0), dict(W_dec=0), dict(b_dec=0), dict(recon=0, x=0, sq_err=0), dict(x=0),
                dict(sq_err=0), dict(recon=GOOD["x"])):
        assert call(**bad) == NULL, bad
    assert call(val=0, dtype=7, k=(1 << 17) + 1) == NULL
    # 3. dtype
    assert call(dtype=0) == DTYPE and call(dtype=3) == DTYPE
    assert call(dtype=7, k=(1 << 17) + 1, W_dec=FAKE + 2) == DTYPE
    # 4. too large
    assert call(h=1 << 31) == TOO_LARGE
    assert call(k=(1 << 17) + 1) == TOO_LARGE
    assert call(k=(1 << 17) + 1, W_dec=FAKE + 2) == TOO_LARGE
    # 5. alignment: 16 bytes for W_dec, b_dec, x, recon and their pitches; 4 for idx and sq_err; val its element
    for name in ("W_dec", "b_dec", "x", "recon"):
        assert call(**{name: GOOD[name] + 8}) == ALIGN, name
    for name in ("ldw", "ldr", "ldx"):
        assert call(**{name: 84}) == ALIGN, name               # bf16: 168 bytes
        assert call(**{name: 82}, dtype=2) == ALIGN, name      # fp32: 328 bytes
    for name in ("idx", "sq_err"):
        assert call(**{name: GOOD[name] + 2}) == ALIGN, name
    assert call(val=FAKE + 1) == ALIGN
    assert call(val=FAKE + 2, dtype=2) == ALIGN


def cpu_operands(rows=4, n=2, d=40, h=64, k=8, dtype=torch.bfloat16):
    c = ref.make_case(rows, n, d, h, k, dtype)
    return c["val"], c["idx"], c["W"], c["b"], c["x"]


def test_ops_wrapper_validates_then_refuses_cpu_tensors():
    val, idx, W, b, x = cpu_operands()
    n, d = 2, 40
    with pytest.raises(ValueError, match="int32"):
        ops.decode_pairs(val, idx.long(), W, b, n, d)
    with pytest.raises(ValueError, match="bf16 or fp32"):
        ops.decode_pairs(val.half(), idx, W, b, n, d)
    with pytest.raises(ValueError, match="rows >= 1, k >= 1"):
        ops.decode_pairs(val, idx[:, :4], W, b, n, d)
    with pytest.raises(ValueError, match="contiguous"):
        ops.decode_pairs(val.t().contiguous().t(), idx, W, b, n, d)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.decode_pairs(val, idx, W, b, 4, 20)
    with pytest.raises(ValueError, match="W_dec must be"):
        ops.decode_pairs(val, idx, W[:, :72], b, n, d)
    with pytest.raises(ValueError, match="W_dec must be"):
        ops.decode_pairs(val, idx, W.float(), b, n, d)
    with pytest.raises(ValueError, match="h must be"):
        ops.decode_pairs(val, idx, W, b, n, d, h=65)
    with pytest.raises(ValueError, match="b_dec"):
        ops.decode_pairs(val, idx, W, b[:72], n, d)
    with pytest.raises(ValueError, match="sq_err needs x"):
        ops.decode_pairs(val, idx, W, b, n, d, sq_err=torch.empty(4, 2))
    with pytest.raises(ValueError, match="sq_err"):
        ops.decode_pairs(val, idx, W, b, n, d, x=x, sq_err=torch.empty(4, 3))
    with pytest.raises(ValueError, match="recon must be"):
        ops.decode_pairs(val, idx, W, b, n, d, recon=torch.empty(3, 80, dtype=val.dtype))
    with pytest.raises(ValueError, match="x must be"):
        ops.decode_pairs(val, idx, W, b, n, d, x=x.float())
    # valid arguments: no CPU fallback
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.decode_pairs(val, idx, W, b, n, d)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.decode_pairs(val, idx, W, b, n, d, h=32, x=x)


def test_crosscoder_methods_validate():
    cc = ca.CrossCoder(_cfg("bf16", h=256, d=32))            # ReLU: no cfg["k"]
    x = torch.zeros(4, 2, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="k must be"):
        cc.encode_pairs(x)
    with pytest.raises(ValueError, match="k must be"):
        cc.encode_pairs(x, k=257)
    with pytest.raises(ValueError, match="expected x"):
        cc.encode_pairs(x[:, :1], k=4)
    v, i = torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="one shape"):
        cc.decode_pairs(v, i[:, :4])
    with pytest.raises(ValueError, match="int32 or int64"):
        cc.decode_pairs(v, i.float())
    with pytest.raises(ValueError, match="rows"):
        cc.pairs_sq_err(v, i, x[:3])
    with pytest.raises(RuntimeError, match="ROCm"):
        cc.decode_pairs(v, i)
    with pytest.raises(RuntimeError, match="ROCm"):
        cc.pairs_sq_err(v, i.int(), x)
    # int64 indices beyond int32 stay out of range instead of wrapping into it
    vals, idx = cc._pairs(v, torch.tensor([[(1 << 32) + 5, -(1 << 40), 5, -1, 255, 256, 0, 1]] * 4))
    assert idx.dtype == torch.int32 and vals.dtype == torch.bfloat16
    assert idx[0].tolist() == [256, -1, 5, -1, 255, 256, 0, 1]


def test_latent_ablation_constructor_validates():
    relu = ca.CrossCoder(_cfg("bf16", h=256, d=32))
    with pytest.raises(ValueError, match="k must be"):
        ca.LatentAblation(relu, {})                          # a ReLU crosscoder has no k of its own
    with pytest.raises(ValueError, match="k must be"):
        ca.LatentAblation(relu, {}, k=0)
    with pytest.raises(ValueError, match="shape"):
        ca.LatentAblation(relu, {"a": torch.zeros(255, dtype=torch.bool)}, k=8)
    with pytest.raises(ValueError, match="bool mask or int32 / int64"):
        ca.LatentAblation(relu, {"a": torch.zeros(3)}, k=8)
    with pytest.raises(ValueError, match="0..255"):
        ca.LatentAblation(relu, {"a": torch.tensor([0, 256])}, k=8)
    with pytest.raises(ValueError, match="0..255"):
        ca.LatentAblation(relu, {"a": torch.tensor([-1])}, k=8)
    with pytest.raises(ValueError, match="name"):
        ca.LatentAblation(relu, {"baseline": torch.tensor([1])}, k=8)
    with pytest.raises(ValueError, match="dict"):
        ca.LatentAblation(relu, [torch.tensor([1])], k=8)
    ab = ca.LatentAblation(relu, {"mask": torch.arange(256) % 2 == 0, "idx": torch.tensor([3, 5, 3]),
                                  "none": torch.zeros(0, dtype=torch.int64)}, k=8)
    assert ab.k == 8 and ab.names == ["mask", "idx", "none"]
    assert [int(m.sum()) for m in ab._masks] == [128, 2, 0]
    with pytest.raises(ValueError, match="no rows"):
        ab.result()
    topk = ca.CrossCoder(dict(_cfg("bf16", h=256, d=32), activation="topk", k=16))
    assert ca.LatentAblation(topk, {}).k == 16               # k defaults to cfg["k"]


REF_SHAPES = [(1, 1, 8, 8, 1), (3, 2, 40, 200, 5), (5, 3, 696, 64, 9), (4, 2, 40, 16, 16), (33, 4, 64, 256, 32)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", REF_SHAPES, ids=lambda s: "r%d_n%d_d%d_h%d_k%d" % s)
def test_references_agree(shape, dtype):
    """The fp32 slot-order loop against the fp64 chain and against a dense fp64 acts @ W_dec + b_dec of the scattered
    pairs, within (k + 1) 2^-23 S, with indices >= h among the slots (skipped like the negative ones)."""
    rows, n, d, h, k = shape
    c = ref.make_case(rows, n, d, h, k, dtype)
    val, idx, W, b = c["val"], c["idx"].clone(), c["W"], c["b"]
    if k >= 2:
        idx[0, k - 1] = h                  # the first index out of range above
        if rows > 1:
            idx[1, 0] = 2 ** 31 - 1
    got = ref.decode_f32(val, idx, W, b, h)
    acc = ref.decode_f32(val, idx, W, b, h, rounded=False)
    assert torch.equal(got, acc.to(dtype))
    exact, S = ref.decode_f64(val, idx, W, b, h)
    tol = ref.chain_tol(k, S)
    assert ((acc.double() - exact).abs() <= tol).all()
    dense = ref.dense_f64(val, idx, W, b, h)
    assert ((dense - exact).abs() <= tol).all()   # (fp64 against fp64: the order of the sum only)
    assert ((acc.double() - dense).abs() <= tol).all()
    # a row with no valid slot is b_dec's bits; a narrower h skips what lies beyond it
    if rows >= 2:
        assert torch.equal(got[rows - 1], b)
    half = ref.decode_f32(val, idx, W, b, max(1, h // 2))
    keep = idx.clone()
    keep[keep >= max(1, h // 2)] = -1
    assert torch.equal(half, ref.decode_f32(val, keep, W, b, h))
    sq = ref.sq_err_f64(got, c["x"], n, d)
    assert sq.shape == (rows, n) and (sq > 0).all()
