"""The sparse decode's backward on the GPU: cc_pairs_grad_values, cc_pairs_grad_decoder and cc_pairs_latent_sums against
their CPU restatements (tests/_pairs_grad_ref.py, where the bounds are derived), and CrossCoder.decode_pairs(...,
differentiable=True), pairs_attribution and LatentAttribution through the model.

The operands are the sparse decode's own cases (tests/_decode_pairs_ref.make_case: duplicates, padding at the end,
negative indices in the middle, rows without a valid slot); x serves as g.  No test feeds the device an index >= h or a
bad perm: those sides of the compares are covered on the CPU restatements (tests/test_pairs_grad_host.py)."""
import functools

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops
from tests import _decode_pairs_ref as dref
from tests import _pairs_grad_ref as ref

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
# the one rounding of an fp32 result to the dtype, relative: bf16 keeps 8 significant bits, so half an ulp is 2^-8
RND = {"bf16": 2.0 ** -8, "fp32": 0.0}

# (rows, n, d, h, k): the sparse decode's shapes
SHAPES = [(1, 1, 8, 8, 1), (3, 2, 40, 200, 5), (257, 4, 64, 256, 32), (5, 3, 696, 64, 9), (64, 2, 2304, 128, 33),
          (4, 2, 40, 16, 16), (2051, 1, 8, 16, 2), (3, 2, 1032, 512, 300)]
LONG_ROW = (2, 1, 8200, 8, 3)     # K beyond the 8192 columns of g that cc_pairs_grad_values stages in LDS
DENSE = (300, 2, 40, 64, 4)       # one latent in every row (300 > 2 L pairs: the split and its ordered merge) and latents
#                                   that never occur
PITCH_SHAPES = [SHAPES[1], SHAPES[3]]


def sid(s):
    return "r%d_n%d_d%d_h%d_k%d" % s


@functools.lru_cache(maxsize=None)
def case(shape, dt):
    """The shared case of a shape: CPU operands and references (computed once, never written)."""
    rows, n, d, h, k = shape
    c = dref.make_case(rows, n, d, h, k, DT[dt])
    c["g"] = c["x"]
    if shape == DENSE:
        idx = c["idx"]
        idx[idx >= 0] %= 40                # latents 40 .. 63 never occur
        idx[:, 0] = 5
    c["dot"], c["M"] = ref.values_f64(c["idx"], c["W"], c["g"], n, d, h)
    return c


@functools.lru_cache(maxsize=None)
def decoder_case(shape, dt):
    rows, n, d, h, k = shape
    c = dict(case(shape, dt))
    perm, seg = ref.by_latent_loop(c["idx"], h)
    c["perm"], c["seg"] = perm, seg
    c["exact"], c["S"], c["len"] = ref.decoder_f64(perm, seg, c["val"], c["g"], n * d)
    if dt == "bf16":
        c["bits"] = ref.decoder_f32(perm, seg, c["val"], c["g"], n * d).to(torch.bfloat16)
    return c


def on_gpu(c, *names):
    return [c[name].cuda() for name in names]


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def model_order_sum(dot):
    t = torch.zeros(dot.shape[:-1], dtype=torch.float32)
    for m in range(dot.shape[-1]):
        t = t + dot[..., m]
    return t


# ---------------------------------------------------------------- cc_pairs_grad_values
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES + [LONG_ROW], ids=sid)
def test_values_against_fp64(shape, dt):
    rows, n, d, h, k = shape
    c = case(shape, dt)
    val, idx, W, g = on_gpu(c, "val", "idx", "W", "g")
    dot, total = ops.pairs_grad_values(idx, W, g, n, d, want_total=True)
    assert dot.dtype == total.dtype == torch.float32 and tuple(dot.shape) == (rows, k, n) and tuple(total.shape) == (rows, k)
    dot_c, total_c = dot.cpu(), total.cpu()
    err, tol = (dot_c.double() - c["dot"]).abs(), ref.values_tol(d, c["M"])
    print("max |dot - fp64| / bound:", float((err / tol.clamp(min=1e-300)).max()))
    assert (err <= tol).all()
    err, tol = (total_c.double() - c["dot"].sum(-1)).abs(), ref.values_tol(n * d, c["M"].sum(-1))
    print("max |total - fp64| / bound:", float((err / tol.clamp(min=1e-300)).max()))
    assert (err <= tol).all()
    assert torch.equal(bits(total_c), bits(model_order_sum(dot_c)))     # the models' sums in model order
    invalid = c["idx"] < 0
    assert rows < 2 or invalid.any()
    assert (bits(dot_c)[invalid] == 0).all() and (bits(total_c)[invalid] == 0).all()   # +0
    # with val: one fp32 multiplication of the same sums
    dot_v, total_v = ops.pairs_grad_values(idx, W, g, n, d, val=val, want_total=True)
    want = torch.where(invalid.unsqueeze(-1), torch.zeros(()), c["val"].float().unsqueeze(-1) * dot_c)
    assert torch.equal(bits(dot_v.cpu()), bits(want))
    assert torch.equal(bits(total_v.cpu()), bits(model_order_sum(dot_v.cpu())))
    # each output alone, and a second call: the same bits
    only_dot, none = ops.pairs_grad_values(idx, W, g, n, d)
    assert none is None and torch.equal(bits(only_dot), bits(dot))
    none, only_total = ops.pairs_grad_values(idx, W, g, n, d, want_dot=False, want_total=True)
    assert none is None and torch.equal(bits(only_total), bits(total))
    again = ops.pairs_grad_values(idx, W, g, n, d, val=val, want_total=True)
    assert torch.equal(bits(again[0]), bits(dot_v)) and torch.equal(bits(again[1]), bits(total_v))
    # a narrower h drops the latents beyond it
    if h >= 2:
        keep = c["idx"].clone()
        keep[keep >= h // 2] = -1
        a = ops.pairs_grad_values(idx, W, g, n, d, h=h // 2)[0]
        b = ops.pairs_grad_values(keep.cuda(), W, g, n, d)[0]
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], LONG_ROW], ids=sid)
def test_values_dyadic_case_is_exact(shape, dt):
    """g and W_dec small integers times 2^-3: every product and partial sum is exact in fp32, so any order gives fp64's
    value"""
    rows, n, d, h, k = shape
    gen = torch.Generator().manual_seed(17)
    W = (torch.randint(-8, 9, (h, n * d), generator=gen).float() / 8).to(DT[dt])
    g = (torch.randint(-8, 9, (rows, n * d), generator=gen).float() / 8).to(DT[dt])
    idx = case(shape, dt)["idx"]
    exact, _ = ref.values_f64(idx, W, g, n, d, h)
    dot, total = ops.pairs_grad_values(idx.cuda(), W.cuda(), g.cuda(), n, d, want_total=True)
    assert torch.equal(dot.cpu().double(), exact) and torch.equal(total.cpu().double(), exact.sum(-1))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", PITCH_SHAPES, ids=sid)
def test_values_pitches_and_what_stays_untouched(shape, dt):
    rows, n, d, h, k = shape
    K = n * d
    c = case(shape, dt)
    val, idx, W, g = on_gpu(c, "val", "idx", "W", "g")
    want = ops.pairs_grad_values(idx, W, g, n, d, val=val, want_total=True)
    CAN = 1234.0
    Ww = torch.full((h, K + 24), CAN, dtype=DT[dt], device="cuda")
    Ww[:, 8:8 + K] = W
    gw = torch.full((rows, K + 16), CAN, dtype=DT[dt], device="cuda")
    gw[:, 16:] = g
    dot = torch.full((rows + 2, k, n), CAN, dtype=torch.float32, device="cuda")
    total = torch.full((rows + 2, k), CAN, dtype=torch.float32, device="cuda")
    got = ops.pairs_grad_values(idx, Ww[:, 8:8 + K], gw[:, 16:], n, d, val=val, dot=dot[:rows], total=total[:rows])
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
    assert (dot[rows:] == CAN).all() and (total[rows:] == CAN).all()
    assert (Ww[:, :8] == CAN).all() and (Ww[:, 8 + K:] == CAN).all() and (gw[:, :16] == CAN).all()


# ---------------------------------------------------------------- cc_pairs_grad_decoder
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES + [DENSE], ids=sid)
def test_decoder_against_cpu(shape, dt):
    rows, n, d, h, k = shape
    K = n * d
    c = decoder_case(shape, dt)
    val, idx, g = on_gpu(c, "val", "idx", "g")
    perm, seg = ops.pairs_by_latent(idx, h)
    assert seg.cpu().tolist() == c["seg"] and perm[:c["seg"][-1]].cpu().tolist() == c["perm"]
    dW = ops.pairs_grad_decoder(perm, seg, val, g, K)
    assert dW.dtype == DT[dt] and tuple(dW.shape) == (h, K)
    got = dW.cpu()
    if dt == "bf16":
        assert torch.equal(bits(got), bits(c["bits"]))
    else:
        err, tol = (got.double() - c["exact"]).abs(), ref.decoder_tol(c["len"], c["S"])
        print("max |dW - fp64| / bound:", float((err / tol.clamp(min=1e-300)).max()))
        assert (err <= tol).all()
    empty = c["len"] == 0
    assert empty.any() or (shape != DENSE and h <= rows * k)
    assert (bits(got)[empty] == 0).all()                                # a latent without pairs: a row of +0
    if shape == DENSE:
        assert int(c["len"][5]) >= rows > 2 * ref.SPLIT
    assert torch.equal(bits(ops.pairs_grad_decoder(perm, seg, val, g, K)), bits(dW))   # two calls
    # the compact perm (the valid pairs alone) gives the same rows
    short = perm[:c["seg"][-1]].contiguous()
    assert torch.equal(bits(ops.pairs_grad_decoder(short, seg, val, g, K)), bits(dW))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", PITCH_SHAPES + [DENSE], ids=sid)
def test_decoder_pitches_and_what_stays_untouched(shape, dt):
    rows, n, d, h, k = shape
    K = n * d
    c = decoder_case(shape, dt)
    val, idx, g = on_gpu(c, "val", "idx", "g")
    perm, seg = ops.pairs_by_latent(idx, h)
    want = ops.pairs_grad_decoder(perm, seg, val, g, K)
    CAN = 1234.0
    gw = torch.full((rows, K + 16), CAN, dtype=DT[dt], device="cuda")
    gw[:, 16:] = g
    ow = torch.full((h + 2, K + 40), CAN, dtype=DT[dt], device="cuda")
    ws = torch.full((ops.pairs_grad_decoder_ws_floats(rows * k, K) + 64,), CAN, dtype=torch.float32, device="cuda")
    got = ops.pairs_grad_decoder(perm, seg, val, gw[:, 16:], K, out=ow[:h, 32:32 + K], ws=ws)
    assert torch.equal(bits(got), bits(want))
    assert (ow[:, :32] == CAN).all() and (ow[:, 32 + K:] == CAN).all() and (ow[h:] == CAN).all()
    assert (ws[-64:] == CAN).all() and (gw[:, :16] == CAN).all()


# ---------------------------------------------------------------- cc_pairs_latent_sums
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], DENSE], ids=sid)
def test_latent_sums_over_two_updates(shape):
    rows, n, d, h, k = shape
    c = decoder_case(shape, "fp32")
    idx = c["idx"].cuda()
    perm, seg = ops.pairs_by_latent(idx, h)
    gen = torch.Generator().manual_seed(23)
    s, sa = (torch.zeros(h, n, dtype=torch.float64, device="cuda") for _ in range(2))
    cnt = torch.zeros(h, dtype=torch.int64, device="cuda")
    s_c, sa_c, cnt_c = s.cpu(), sa.cpu(), cnt.cpu()
    for _ in range(2):
        a = torch.randn(rows, k, n, generator=gen) * 10.0 ** torch.randint(-3, 4, (rows, k, 1), generator=gen)
        ops.pairs_latent_sums(a.cuda(), perm, seg, s, sa, cnt)
        ref.latent_sums_f64(a, c["perm"], c["seg"], s_c, sa_c, cnt_c)
    assert torch.equal(bits(s.cpu()), bits(s_c)) and torch.equal(bits(sa.cpu()), bits(sa_c))
    assert torch.equal(cnt.cpu(), cnt_c) and int(cnt_c.sum()) == 2 * c["seg"][-1]


# ---------------------------------------------------------------- through the model
MODEL_ROWS, MODEL_D, MODEL_H = 96, 36, 200  # d_in 36: the kernels run on d = 40; 200 = kernel h
ACTIVATIONS = {"relu": ({}, 100),                                  # 75..124 active latents per row: some rows are full
               "topk": ({"activation": "topk", "k": 12}, 16)}      # padding at the end of every row


def model(dt, extra, b_dec=True):
    cfg = {"seed": 49, "batch_size": MODEL_ROWS, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 640, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": MODEL_H, "seq_len": 1024, "enc_dtype": dt, "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": MODEL_D, "log_every": 100, "save_every": 30000}
    cc = ca.CrossCoder(dict(cfg, **extra))
    if b_dec:
        with torch.no_grad():  # (a non-zero b_dec: the init's is zero)
            cc.b_dec.copy_(torch.randn(2, MODEL_D, generator=torch.Generator().manual_seed(11)).to(DT[dt]))
    return cc


def model_x(dt, rows=MODEL_ROWS, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, 2, MODEL_D, generator=g).to(DT[dt]).cuda()


def arena_operands(cc):
    a = cc.arena()
    a.wait_pending()
    return a.W_dec_hk.cpu(), a.b_dec_flat.cpu()


def pad_flat(t, dp):
    """[rows, 2, MODEL_D] -> [rows, 2 dp] with zero padding columns, on the CPU"""
    return torch.nn.functional.pad(t.cpu(), (0, dp - MODEL_D)).reshape(t.shape[0], -1)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("activation", list(ACTIVATIONS))
def test_differentiable_decode_pairs(activation, dt):
    extra, k = ACTIVATIONS[activation]
    cc = model(dt, extra)
    x, G = model_x(dt), model_x(dt, seed=8)
    vals, idx = cc.encode_pairs(x, k)
    plain = cc.decode_pairs(vals, idx)
    assert plain.grad_fn is None and not plain.requires_grad
    v = vals.clone().requires_grad_(True)
    out = cc.decode_pairs(v, idx, differentiable=True)
    assert out.grad_fn is not None and torch.equal(bits(out.detach()), bits(plain))
    for p in (cc.W_dec, cc.b_dec, cc.W_enc, cc.b_enc):
        p.grad = None
    (out * G).sum().backward()
    assert cc.W_enc.grad is None and cc.b_enc.grad is None
    assert tuple(v.grad.shape) == tuple(vals.shape) and v.grad.dtype == DT[dt]
    assert tuple(cc.W_dec.grad.shape) == (MODEL_H, 2, MODEL_D) and tuple(cc.b_dec.grad.shape) == (2, MODEL_D)
    # the fp64 autograd of the dense restatement on the arena's own operands (kernel dims: d = 40)
    W, b = arena_operands(cc)
    dp = W.shape[1] // 2
    v_c, i_c, g_c = vals.cpu(), idx.cpu(), pad_flat(G, dp)
    _, d_val, d_W, d_b = ref.dense_autograd(v_c, i_c, W, b, g_c, MODEL_H)
    dot, M = ref.values_f64(i_c, W, g_c, 2, dp, MODEL_H)
    r = RND[dt]
    invalid = i_c < 0
    assert invalid.any() and (bits(v.grad.cpu())[invalid] == 0).all()   # 0 at padding
    tol = ref.values_tol(2 * dp, M.sum(-1))
    err = (v.grad.cpu().double() - d_val).abs()
    print("d values: max err / bound:", float((err / (tol + r * (d_val.abs() + tol)).clamp(min=1e-300)).max()))
    assert (err <= tol + r * (d_val.abs() + tol)).all()
    perm, seg = ref.by_latent_loop(i_c, MODEL_H)
    _, S, length = ref.decoder_f64(perm, seg, v_c, g_c, 2 * dp)
    crop = lambda t: t.view(-1, 2, dp)[:, :, :MODEL_D]  # noqa: E731
    tol = crop(ref.decoder_tol(length, S))
    err = (cc.W_dec.grad.cpu().double() - crop(d_W)).abs()
    print("d W_dec: max err / bound:", float((err / (tol + r * (crop(d_W).abs() + tol)).clamp(min=1e-300)).max()))
    assert (err <= tol + r * (crop(d_W).abs() + tol)).all()
    # b_dec: a column sum of MODEL_ROWS terms in fp32, any order
    tol = crop(((MODEL_ROWS + 1) * ref.EPS32 * g_c.double().abs().sum(0)).unsqueeze(0))[0]
    err = (cc.b_dec.grad.cpu().double() - crop(d_b.unsqueeze(0))[0]).abs()
    assert (err <= tol + r * (crop(d_b.unsqueeze(0))[0].abs() + tol)).all()
    # only what is asked for: values alone
    v2 = vals.clone().requires_grad_(True)
    with torch.no_grad():
        assert cc.decode_pairs(v2, idx, differentiable=True).grad_fn is None
    for p in (cc.W_dec, cc.b_dec):
        p.grad = None


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("activation", list(ACTIVATIONS))
def test_latent_attribution(activation, dt):
    """Two batches, two groups (one empty); every entry against an fp64 restatement from the same pairs, and a second
    run over the same stream bit for bit."""
    extra, k = ACTIVATIONS[activation]
    cc = model(dt, extra)
    even = torch.arange(MODEL_H) % 2 == 0
    groups = {"even": even, "nothing": torch.zeros(0, dtype=torch.int64)}
    batches = [(model_x(dt, 96, seed=5), model_x(dt, 96, seed=8)), (model_x(dt, 40, seed=6), model_x(dt, 40, seed=9))]
    runs = []
    for _ in range(2):
        at = ca.LatentAttribution(cc, k=k, groups=groups)
        for x, g in batches:
            at.update(x, g)
        runs.append(at.result())
    res, res2 = runs
    for key in ("mean", "mean_abs"):
        assert torch.equal(bits(res[key]), bits(res2[key]))
    assert torch.equal(res["count"], res2["count"]) and torch.equal(bits(res["even"]["attribution"]),
                                                                    bits(res2["even"]["attribution"]))
    W, _ = arena_operands(cc)
    dp = W.shape[1] // 2
    s64, a64, tol = (torch.zeros(MODEL_H, 2, dtype=torch.float64) for _ in range(3))
    cnt, full = torch.zeros(MODEL_H, dtype=torch.int64), 0
    for x, g in batches:
        vals, idx = cc.encode_pairs(x, k)
        full += int((idx[:, -1] >= 0).sum())
        i_c = idx.cpu()
        att, M = ref.values_f64(i_c, W, pad_flat(g, dp), 2, dp, MODEL_H, val=vals.cpu())
        ok = i_c >= 0
        lat = i_c[ok].long()
        s64.index_add_(0, lat, att[ok])
        a64.index_add_(0, lat, att[ok].abs())
        tol.index_add_(0, lat, ref.values_tol(dp + 1, M[ok]))   # (d + 1: the multiplication by the value)
        cnt += torch.bincount(lat, minlength=MODEL_H)
    assert res["rows"] == 136 and res["full_rows"] == full and torch.equal(res["count"], cnt)
    assert activation != "relu" or 0 < full < 136
    print("mean: max err / bound:", float(((res["mean"] * 136 - s64).abs() / tol.clamp(min=1e-300)).max()))
    assert ((res["mean"] * 136 - s64).abs() <= tol + 1e-12 * a64).all()
    assert ((res["mean_abs"] * 136 - a64).abs() <= tol + 1e-12 * a64).all()
    assert ((res["even"]["attribution"] - s64[even].sum(0)).abs() <= tol[even].sum(0) + 1e-12 * a64.sum(0)).all()
    assert (res["nothing"]["attribution"] == 0).all()
    lat, s = at.top(5, model=1)
    want = torch.sort((res["mean"][:, 1] * 136).abs(), descending=True, stable=True).indices[:5]
    assert lat.tolist() == want.tolist() and s.dtype == torch.float64


@pytest.mark.parametrize("activation", list(ACTIVATIONS))
def test_attribution_identity_with_decode_pairs(activation):
    """fp32, b_dec = 0 (the init's): <g, decode_pairs(v) - decode_pairs(v with G zeroed)> per row equals the summed
    attribution of G's slots within (k + n d + 2) 2^-23 sum |v g w| (tests/_pairs_grad_ref.py)."""
    extra, k = ACTIVATIONS[activation]
    cc = model("fp32", extra, b_dec=False)
    x, g = model_x("fp32"), model_x("fp32", seed=8)
    vals, idx = cc.encode_pairs(x, k)
    in_G = (torch.arange(MODEL_H, device="cuda") % 3 == 0)[idx.clamp(min=0).long()] & (idx >= 0)
    assert in_G.any(1).sum() > MODEL_ROWS // 2
    r1 = cc.decode_pairs(vals, idx)
    r0 = cc.decode_pairs(vals.masked_fill(in_G, 0), idx)
    left = (g.cpu().double() * (r1.cpu().double() - r0.cpu().double())).sum((1, 2))
    att = cc.pairs_attribution(vals, idx, g)
    right = torch.where(in_G.cpu().unsqueeze(-1), att.cpu().double(), torch.zeros((), dtype=torch.float64)).sum((1, 2))
    W, b = arena_operands(cc)
    assert (b == 0).all()
    dp = W.shape[1] // 2
    _, T = ref.values_f64(idx.cpu(), W, pad_flat(g, dp), 2, dp, MODEL_H, val=vals.cpu())
    tol = ref.identity_tol(k, 2, dp, T.sum((1, 2)))
    err = (left - right).abs()
    print("identity: max |left - right| / bound:", float((err / tol).max()), " max |left|:", float(left.abs().max()))
    assert (err <= tol).all() and float(left.abs().max()) > 0
