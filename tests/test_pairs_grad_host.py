"""CPU: the sparse decode's backward -- its public surface exists, the three entry points validate their arguments in the
stated order before any launch, ops.pairs_by_latent agrees with a plain loop, and the CPU restatements the GPU tests
compare with (tests/_pairs_grad_ref.py) agree with a dense fp64 autograd."""
import ctypes
import os
import re

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, attribution, ops
from tests import _decode_pairs_ref as dref
from tests import _pairs_grad_ref as ref
from tests.test_cpu_host import _cfg, _dynamic_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DTYPE, SHAPE, ALIGN, TOO_LARGE = 0, 1, 2, 3, 4, 5
NAMES = {"cc_pairs_grad_values": 15, "cc_pairs_grad_decoder_ws_floats": 2, "cc_pairs_grad_decoder": 15,
         "cc_pairs_latent_sums": 12}


def test_public_names_exist():
    assert callable(ca.LatentAttribution)
    assert callable(ca.CrossCoder.pairs_attribution)
    for name in ("pairs_by_latent", "pairs_grad_values", "pairs_grad_decoder", "pairs_latent_sums"):
        assert callable(getattr(ops, name))


def test_entry_points_are_declared_exported_and_typed():
    raw = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define\s+CC_PAIRS_GRAD_SPLIT\s+%d\b" % ops.PAIRS_GRAD_SPLIT, txt)
    assert ref.SPLIT == ops.PAIRS_GRAD_SPLIT
    for name, nargs in NAMES.items():
        assert re.search(r"\bint(64_t)?\s+%s\s*\(" % name, txt), name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int64 if name.endswith("ws_floats") else ctypes.c_int) and len(args) == nargs
        assert name in _dynamic_exports(_lib.LIB_PATH)
        assert name in _dynamic_exports(_lib.DEBUG_LIB_PATH)
    L = ops.PAIRS_GRAD_SPLIT
    ws = _lib.load().cc_pairs_grad_decoder_ws_floats
    assert ws(L - 1, 80) == 0 and ws(L, 80) == 80 and ws(5 * L + 3, 4608) == 5 * 4608 and ws(0, 80) == 0


FAKE = 1 << 20  # a 16-byte aligned address that is never dereferenced: every call below fails a check first


def caller(fn, order, good):
    def call(**kw):
        a = dict(good, **kw)
        assert a != good, "a call with valid arguments would launch"
        args = [ctypes.c_void_p(a[name]) if t is ctypes.c_void_p else a[name]
                for name, t in zip(order, _lib.SIGNATURES[fn][1])]
        return getattr(_lib.load(), fn)(*args)
    return call


def test_grad_values_checks_run_in_order_before_any_launch():
    good = dict(idx=FAKE, val=FAKE + 4096, B=4, k=8, W_dec=FAKE + 8192, ldw=80, h=64, g=FAKE + 12288, ldg=80, n=2, d=40,
                dtype=1, dot=FAKE + 16384, total=FAKE + 20480, stream=0)
    call = caller("cc_pairs_grad_values", list(good), good)
    for bad in (dict(B=0), dict(k=0), dict(h=0), dict(n=0), dict(d=0), dict(d=4), dict(d=12), dict(d=44), dict(ldw=79),
                dict(ldg=72), dict(n=1 << 62, d=8)):
        assert call(**bad) == SHAPE, bad
    assert call(B=0, idx=0, dtype=7) == SHAPE
    for bad in (dict(idx=0), dict(W_dec=0), dict(g=0), dict(dot=0, total=0)):
        assert call(**bad) == NULL, bad
    assert call(idx=0, dtype=7, k=(1 << 17) + 1) == NULL
    assert call(dtype=0) == DTYPE and call(dtype=3) == DTYPE
    assert call(dtype=7, k=(1 << 17) + 1, W_dec=FAKE + 2) == DTYPE
    assert call(h=1 << 31) == TOO_LARGE
    assert call(k=(1 << 17) + 1) == TOO_LARGE
    assert call(k=(1 << 17) + 1, W_dec=FAKE + 2) == TOO_LARGE
    for name in ("W_dec", "g"):
        assert call(**{name: good[name] + 8}) == ALIGN, name
    for name in ("ldw", "ldg"):
        assert call(**{name: 84}) == ALIGN, name               # bf16: 168 bytes
        assert call(**{name: 82}, dtype=2) == ALIGN, name      # fp32: 328 bytes
    for name in ("idx", "dot", "total"):
        assert call(**{name: good[name] + 2}) == ALIGN, name
    assert call(val=good["val"] + 1) == ALIGN
    assert call(val=good["val"] + 2, dtype=2) == ALIGN
    # val and one of the outputs are optional: these pass the pointer checks and fail later
    assert call(val=0, dot=0, W_dec=FAKE + 8) == ALIGN
    assert call(total=0, g=FAKE + 8) == ALIGN


def test_grad_decoder_checks_run_in_order_before_any_launch():
    good = dict(perm=FAKE, P=300, seg=FAKE + 4096, h=64, val=FAKE + 8192, B=40, k=8, g=FAKE + 12288, ldg=80, K=80,
                dtype=1, dW=FAKE + 16384, ldo=80, ws=FAKE + 20480, stream=0)
    call = caller("cc_pairs_grad_decoder", list(good), good)
    for bad in (dict(B=0), dict(k=0), dict(h=0), dict(P=-1), dict(K=0), dict(K=4), dict(K=84), dict(ldg=72), dict(ldo=79)):
        assert call(**bad) == SHAPE, bad
    assert call(B=0, seg=0, dtype=7) == SHAPE
    for bad in (dict(perm=0), dict(seg=0), dict(val=0), dict(g=0), dict(dW=0), dict(ws=0)):
        assert call(**bad) == NULL, bad
    assert call(seg=0, dtype=7, k=(1 << 17) + 1) == NULL
    assert call(dtype=0) == DTYPE and call(dtype=3) == DTYPE
    assert call(dtype=7, h=1 << 31) == DTYPE
    for bad in (dict(h=1 << 31), dict(k=(1 << 17) + 1), dict(B=1 << 28), dict(P=1 << 31),
                dict(K=1 << 31, ldg=1 << 31, ldo=1 << 31)):
        assert call(**bad) == TOO_LARGE, bad
    assert call(h=1 << 31, g=FAKE + 8) == TOO_LARGE
    for name in ("g", "dW", "ws"):
        assert call(**{name: good[name] + 8}) == ALIGN, name
    for name in ("ldg", "ldo"):
        assert call(**{name: 84}) == ALIGN, name
        assert call(**{name: 82}, dtype=2) == ALIGN, name
    assert call(seg=good["seg"] + 4) == ALIGN
    assert call(perm=FAKE + 2) == ALIGN
    assert call(val=good["val"] + 1) == ALIGN
    assert call(val=good["val"] + 2, dtype=2) == ALIGN
    # perm may be missing with P = 0 and ws below one full piece: these fail later
    assert call(perm=0, P=0, ws=0, g=FAKE + 8) == ALIGN
    assert call(P=ops.PAIRS_GRAD_SPLIT - 1, ws=0, g=FAKE + 8) == ALIGN


def test_latent_sums_checks_run_in_order_before_any_launch():
    good = dict(a=FAKE, B=40, k=8, n=2, perm=FAKE + 4096, P=300, seg=FAKE + 8192, h=64, sum=FAKE + 12288,
                abs_sum=FAKE + 16384, count=FAKE + 20480, stream=0)
    call = caller("cc_pairs_latent_sums", list(good), good)
    for bad in (dict(B=0), dict(k=0), dict(h=0), dict(n=0), dict(P=-1)):
        assert call(**bad) == SHAPE, bad
    assert call(B=0, a=0) == SHAPE
    for bad in (dict(a=0), dict(perm=0), dict(seg=0), dict(sum=0), dict(abs_sum=0), dict(count=0)):
        assert call(**bad) == NULL, bad
    assert call(a=0, h=1 << 31) == NULL
    for bad in (dict(h=1 << 31), dict(k=(1 << 17) + 1), dict(B=1 << 28), dict(P=1 << 31), dict(n=1 << 31)):
        assert call(**bad) == TOO_LARGE, bad
    assert call(h=1 << 31, seg=FAKE + 4) == TOO_LARGE
    for name in ("seg", "sum", "abs_sum", "count"):
        assert call(**{name: good[name] + 4}) == ALIGN, name
    for name in ("a", "perm"):
        assert call(**{name: good[name] + 2}) == ALIGN, name
    assert call(perm=0, P=0, a=FAKE + 2) == ALIGN


BY_LATENT = [(1, 1, 8, 8, 1), (3, 2, 40, 200, 5), (33, 4, 64, 256, 32), (4, 2, 40, 16, 16), (300, 1, 8, 16, 2)]


@pytest.mark.parametrize("shape", BY_LATENT, ids=lambda s: "r%d_n%d_d%d_h%d_k%d" % s)
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_pairs_by_latent_against_a_loop(shape, dtype):
    """-1 padding, other negative values, indices >= h and duplicates within a row among the slots"""
    rows, n, d, h, k = shape
    idx = dref.make_case(rows, n, d, h, k, torch.float32)["idx"].clone()
    if k >= 2:
        idx[0, k - 1] = h                  # the first index out of range above
        if rows > 1:
            idx[1, 0] = 2 ** 31 - 1
    if rows >= 3:
        idx[:, 0] = 3 % h                  # one latent in every row
    perm, seg = ops.pairs_by_latent(idx.to(dtype), h)
    want_perm, want_seg = ref.by_latent_loop(idx, h)
    assert perm.dtype == torch.int32 and seg.dtype == torch.int64
    assert tuple(perm.shape) == (rows * k,) and tuple(seg.shape) == (h + 1,)
    assert seg.tolist() == want_seg
    assert perm[:want_seg[-1]].tolist() == want_perm
    # the rest: the invalid slots in slot order, in no segment
    flat = idx.reshape(-1)
    assert perm[want_seg[-1]:].tolist() == torch.nonzero((flat < 0) | (flat >= h)).flatten().tolist()
    again = ops.pairs_by_latent(idx.to(dtype), h)
    assert torch.equal(again[0], perm) and torch.equal(again[1], seg)


REF_SHAPES = [(1, 1, 8, 8, 1), (3, 2, 40, 200, 5), (5, 3, 696, 64, 9), (4, 2, 40, 16, 16), (33, 4, 64, 256, 32),
              (300, 1, 8, 16, 2)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", REF_SHAPES, ids=lambda s: "r%d_n%d_d%d_h%d_k%d" % s)
def test_restatements_against_dense_autograd(shape, dtype):
    """values_f64, decoder_f32 (with the split: 300 rows of one latent) and decoder_f64 against the fp64 autograd of
    scatter -> acts @ W_dec + b_dec, with indices >= h among the slots."""
    rows, n, d, h, k = shape
    K = n * d
    c = dref.make_case(rows, n, d, h, k, dtype)
    val, idx, W, b, g = c["val"], c["idx"].clone(), c["W"], c["b"], c["x"]
    if k >= 2:
        idx[0, k - 1] = h
    if rows >= 300:
        idx[:, 0] = 5                      # longer than 2 L
    recon, d_val, d_W, d_b = ref.dense_autograd(val, idx, W, b, g, h)
    chain, S_chain = dref.decode_f64(val, idx, W, b, h)
    assert ((recon - chain).abs() <= dref.chain_tol(k, S_chain)).all()
    dot, M = ref.values_f64(idx, W, g, n, d, h)
    assert ((dot.sum(-1) - d_val).abs() <= ref.values_tol(K, M.sum(-1))).all()
    assert (d_val[(idx < 0) | (idx >= h)] == 0).all()
    dot_v, M_v = ref.values_f64(idx, W, g, n, d, h, val=val)
    assert torch.equal(dot_v, dot * val.double().unsqueeze(-1))
    perm, seg = ref.by_latent_loop(idx, h)
    exact, S, length = ref.decoder_f64(perm, seg, val, g, K)
    assert ((exact - d_W).abs() <= ref.decoder_tol(length, S)).all()
    acc = ref.decoder_f32(perm, seg, val, g, K)
    assert ((acc.double() - exact).abs() <= ref.decoder_tol(length, S)).all()
    assert rows < 300 or int(length.max()) > 2 * ref.SPLIT
    assert (acc[length == 0] == 0).all()
    assert ((d_b - g.double().sum(0)).abs() <= 1e-12 * g.double().abs().sum(0)).all()
    # bad perm entries and seg values are skipped / clamped by the restatement like by the kernel
    bad_perm = list(perm) + [-1, rows * k]
    bad_seg = list(seg[:-1]) + [len(bad_perm) + 7]
    acc2 = ref.decoder_f32(bad_perm, bad_seg, val, g, K)
    assert torch.equal(acc2[:-1], acc[:-1])


def test_latent_sums_restatement():
    rows, n, d, h, k = 33, 4, 64, 256, 32
    idx = dref.make_case(rows, n, d, h, k, torch.float32)["idx"]
    a = torch.randn(rows, k, n, generator=torch.Generator().manual_seed(3))
    perm, seg = ref.by_latent_loop(idx, h)
    s, sa, cnt = torch.zeros(h, n, dtype=torch.float64), torch.zeros(h, n, dtype=torch.float64), torch.zeros(h, dtype=torch.int64)
    ref.latent_sums_f64(a, perm, seg, s, sa, cnt)
    i = idx.reshape(-1).long()
    ok = i >= 0
    want = torch.zeros(h, n, dtype=torch.float64).index_add_(0, i[ok], a.reshape(-1, n)[ok].double())
    assert ((s - want).abs() <= 1e-12).all() and (sa >= s.abs()).all()
    assert cnt.tolist() == torch.bincount(i[ok], minlength=h).tolist()


def test_ops_wrappers_validate_then_refuse_cpu_tensors():
    c = dref.make_case(4, 2, 40, 64, 8, torch.bfloat16)
    val, idx, W, g = c["val"], c["idx"], c["W"], c["x"]
    n, d = 2, 40
    with pytest.raises(ValueError, match="int32"):
        ops.pairs_grad_values(idx.long(), W, g, n, d)
    with pytest.raises(ValueError, match="rows >= 1, k >= 1"):
        ops.pairs_grad_values(idx, W, g, n, d, val=val[:, :4])
    with pytest.raises(ValueError, match="contiguous"):
        ops.pairs_grad_values(idx.t().contiguous().t(), W, g, n, d)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.pairs_grad_values(idx, W, g, 4, 20)
    with pytest.raises(ValueError, match="g must be"):
        ops.pairs_grad_values(idx, W, g[:3], n, d)
    with pytest.raises(ValueError, match="W_dec must be"):
        ops.pairs_grad_values(idx, W.float(), g, n, d)
    with pytest.raises(ValueError, match="val must have"):
        ops.pairs_grad_values(idx, W, g, n, d, val=val.float())
    with pytest.raises(ValueError, match="h must be"):
        ops.pairs_grad_values(idx, W, g, n, d, h=65)
    with pytest.raises(ValueError, match="dot"):
        ops.pairs_grad_values(idx, W, g, n, d, dot=torch.empty(4, 8, 3))
    with pytest.raises(ValueError, match="total"):
        ops.pairs_grad_values(idx, W, g, n, d, total=torch.empty(4, 7))
    with pytest.raises(ValueError, match="at least one"):
        ops.pairs_grad_values(idx, W, g, n, d, want_dot=False)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.pairs_grad_values(idx, W, g, n, d, val=val)
    perm, seg = ops.pairs_by_latent(idx, 64)
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.pairs_by_latent(idx.float(), 64)
    with pytest.raises(ValueError, match="h must be"):
        ops.pairs_by_latent(idx, 0)
    with pytest.raises(ValueError, match="val must be"):
        ops.pairs_grad_decoder(perm, seg, val.half(), g, 80)
    with pytest.raises(ValueError, match="perm must be"):
        ops.pairs_grad_decoder(perm.long(), seg, val, g, 80)
    with pytest.raises(ValueError, match="seg must be"):
        ops.pairs_grad_decoder(perm, seg.int(), val, g, 80)
    with pytest.raises(ValueError, match="K must be"):
        ops.pairs_grad_decoder(perm, seg, val, g, 84)
    with pytest.raises(ValueError, match="g must be"):
        ops.pairs_grad_decoder(perm, seg, val, g.float(), 80)
    with pytest.raises(ValueError, match="out must be"):
        ops.pairs_grad_decoder(perm, seg, val, g, 80, out=torch.empty(63, 80, dtype=val.dtype))
    with pytest.raises(ValueError, match="ws must be"):
        ops.pairs_grad_decoder(torch.zeros(256, dtype=torch.int32), seg, val, g, 80, ws=torch.empty(80))
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.pairs_grad_decoder(perm, seg, val, g, 80)
    a = torch.zeros(4, 8, 2)
    s, sa, cnt = torch.zeros(64, 2, dtype=torch.float64), torch.zeros(64, 2, dtype=torch.float64), torch.zeros(64, dtype=torch.int64)
    with pytest.raises(ValueError, match="a must be"):
        ops.pairs_latent_sums(a.double(), perm, seg, s, sa, cnt)
    with pytest.raises(ValueError, match="abs_sum"):
        ops.pairs_latent_sums(a, perm, seg, s, sa.float(), cnt)
    with pytest.raises(ValueError, match="count"):
        ops.pairs_latent_sums(a, perm, seg, s, sa, cnt[:63])
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.pairs_latent_sums(a, perm, seg, s, sa, cnt)


def test_crosscoder_methods_validate():
    cc = ca.CrossCoder(_cfg("bf16", h=256, d=32))
    v, i = torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.int64)
    g = torch.zeros(4, 2, 32, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="one shape"):
        cc.pairs_attribution(v, i[:, :4], g)
    with pytest.raises(ValueError, match="expected x"):
        cc.pairs_attribution(v, i, g[:, :1])
    with pytest.raises(ValueError, match="rows"):
        cc.pairs_attribution(v, i, g[:3])
    with pytest.raises(RuntimeError, match="ROCm"):
        cc.pairs_attribution(v, i, g)
    with pytest.raises(ValueError, match="one shape"):
        cc.decode_pairs(v, i[:, :4], differentiable=True)
    with pytest.raises(RuntimeError, match="ROCm"):
        cc.decode_pairs(v, i, differentiable=True)


class _Stub:
    """what LatentAttribution's constructor, result() and top() read of a crosscoder"""
    d_hidden, n_models, k = 6, 2, 3

    class _A:
        data = torch.zeros(1)

    def arena(self):
        return self._A()


def test_latent_attribution_group_arithmetic_on_a_stub():
    stub = _Stub()
    with pytest.raises(ValueError, match="k must be"):
        ca.LatentAttribution(stub, k=7)
    with pytest.raises(ValueError, match="name"):
        ca.LatentAttribution(stub, groups={"mean": torch.tensor([1])})
    with pytest.raises(ValueError, match="0..5"):
        ca.LatentAttribution(stub, groups={"a": torch.tensor([6])})
    with pytest.raises(ValueError, match="dict"):
        ca.LatentAttribution(stub, groups=[torch.tensor([1])])
    at = ca.LatentAttribution(stub, groups={"odd": torch.arange(6) % 2 == 1, "two": torch.tensor([4, 0, 4]),
                                            "none": torch.zeros(0, dtype=torch.int64)})
    assert at.k == 3 and at.names == ["odd", "two", "none"]
    with pytest.raises(ValueError, match="no rows"):
        at.result()
    at._sum.copy_(torch.tensor([[1., -2.], [3., 4.], [-5., 6.], [7., -8.], [9., 10.], [-11., 12.]], dtype=torch.float64))
    at._abs.copy_(at._sum.abs())
    at._count.copy_(torch.tensor([1, 2, 0, 4, 5, 6]))
    at._full += 3
    at.rows = 4
    r = at.result()
    assert r["rows"] == 4 and r["full_rows"] == 3 and r["count"].tolist() == [1, 2, 0, 4, 5, 6]
    assert torch.equal(r["mean"], at._sum / 4) and torch.equal(r["mean_abs"], at._sum.abs() / 4)
    assert r["odd"]["attribution"].tolist() == [3. + 7. - 11., 4. - 8. + 12.]
    assert r["two"]["attribution"].tolist() == [1. + 9., -2. + 10.]
    assert r["none"]["attribution"].tolist() == [0., 0.]
    assert attribution.group_sums(at._sum, []).shape == (0, 2)
    lat, s = at.top(2)                      # |sum over models|: 19 (latent 4), 7 (latent 1), ...
    assert lat.tolist() == [4, 1] and s.tolist() == [19., 7.]
    lat, s = at.top(3, model=1)
    assert lat.tolist() == [5, 4, 3] and s.tolist() == [12., 10., -8.]
    with pytest.raises(ValueError, match="n must be"):
        at.top(0)
    with pytest.raises(ValueError, match="model must be"):
        at.top(1, model=2)
