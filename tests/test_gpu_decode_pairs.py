"""The sparse decode on the GPU: cc_decode_pairs against its CPU restatements (tests/_decode_pairs_ref.py), what it leaves
untouched, and CrossCoder.encode_pairs / decode_pairs / pairs_sq_err and LatentAblation through the model.

bf16: the reconstruction equals the fp32 slot-order loop bit for bit (a product of two bf16 values is exact in fp32).
fp32: |recon - fp64| <= (k + 1) 2^-23 S elementwise, S = |b| + sum |v w| (a k-step fma chain; an indexing error shows
at order 1).  sq_err: (d + 4) 2^-23 relative, against fp64 sums over the kernel's own rounded reconstruction.  Both
bounds are derived in tests/_decode_pairs_ref.py.  No test feeds an index >= h: that side of the one unsigned compare
is covered on the CPU reference (tests/test_decode_pairs_host.py)."""
import functools

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops
from tests import _decode_pairs_ref as ref

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}

# (rows, n, d, h, k)
SHAPES = [(1, 1, 8, 8, 1),          # the minimum
          (3, 2, 40, 200, 5),       # K = 80: a model boundary inside a wave
          (257, 4, 64, 256, 32),    # an odd row count, 8 lanes per model
          (5, 3, 696, 64, 9),       # K = 2088: one 2048-column chunk plus a ragged 40, a non-power-of-two model stride
          (64, 2, 2304, 128, 33),   # config 2's row length (a model that continues over a chunk), k no multiple of 4
          (4, 2, 40, 16, 16),       # k = h
          (2051, 1, 8, 16, 2),      # rows past one grid pass (2048 workgroups), a model per lane
          (3, 2, 1032, 512, 300)]   # k beyond one staged tile of 256 slots, over two chunks
PITCH_SHAPES = [SHAPES[1], SHAPES[3]]


def sid(s):
    return "r%d_n%d_d%d_h%d_k%d" % s


@functools.lru_cache(maxsize=None)
def case(shape, dt):
    """The shared case of a shape: CPU operands and references (computed once, never written)."""
    rows, n, d, h, k = shape
    c = ref.make_case(rows, n, d, h, k, DT[dt])
    c["exact"], c["S"] = ref.decode_f64(c["val"], c["idx"], c["W"], c["b"], h)
    if dt == "bf16":
        c["bits"] = ref.decode_f32(c["val"], c["idx"], c["W"], c["b"], h)
    return c


def on_gpu(c, *names):
    return [c[name].cuda() for name in names]


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def check_recon(recon, c, shape, dt):
    rows, n, d, h, k = shape
    got = recon.cpu()
    if dt == "bf16":
        assert torch.equal(bits(got), bits(c["bits"]))
    else:
        err = (got.double() - c["exact"]).abs()
        tol = ref.chain_tol(k, c["S"])
        print("max |recon - fp64| / tol:", float((err / tol).max()))
        assert (err <= tol).all()
    empty = (c["idx"] < 0).all(1)
    assert rows < 2 or empty.any()
    assert torch.equal(bits(got[empty]), bits(c["b"].expand(int(empty.sum()), -1)))


def check_sq(sq, recon, c, shape):
    rows, n, d, h, k = shape
    want = ref.sq_err_f64(recon.cpu(), c["x"], n, d)
    err = (sq.cpu().double() - want).abs()
    tol = ref.sq_tol(d, want)
    print("max |sq_err - fp64| / tol:", float((err / tol.clamp(min=1e-300)).max()))
    assert sq.dtype == torch.float32 and tuple(sq.shape) == (rows, n)
    assert (err <= tol).all()


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_recon_against_cpu(shape, dt):
    rows, n, d, h, k = shape
    c = case(shape, dt)
    val, idx, W, b = on_gpu(c, "val", "idx", "W", "b")
    recon, none = ops.decode_pairs(val, idx, W, b, n, d)
    assert none is None and recon.dtype == DT[dt] and tuple(recon.shape) == (rows, n * d)
    check_recon(recon, c, shape, dt)
    # no valid slot in any row: b_dec's bits
    recon2, _ = ops.decode_pairs(val, torch.full_like(idx, -1), W, b, n, d)
    assert torch.equal(bits(recon2.cpu()), bits(c["b"].expand(rows, -1)))
    # a narrower h drops the latents beyond it (none of them is read)
    if h >= 2:
        keep = c["idx"].clone()
        keep[keep >= h // 2] = -1
        recon3, _ = ops.decode_pairs(val, idx, W, b, n, d, h=h // 2)
        recon4, _ = ops.decode_pairs(val, keep.cuda(), W, b, n, d)
        assert torch.equal(bits(recon3), bits(recon4))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_sq_err_is_reproducible_and_bounded(shape, dt):
    rows, n, d, h, k = shape
    c = case(shape, dt)
    val, idx, W, b, x = on_gpu(c, "val", "idx", "W", "b", "x")
    recon, _ = ops.decode_pairs(val, idx, W, b, n, d)
    none, sq1 = ops.decode_pairs(val, idx, W, b, n, d, x=x)
    assert none is None
    _, sq2 = ops.decode_pairs(val, idx, W, b, n, d, x=x)
    both = torch.empty_like(recon)
    r3, sq3 = ops.decode_pairs(val, idx, W, b, n, d, recon=both, x=x)
    assert r3 is both
    assert torch.equal(bits(sq1), bits(sq2))            # two calls
    assert torch.equal(bits(sq1), bits(sq3))            # with and without recon
    assert torch.equal(bits(both), bits(recon))
    check_sq(sq1, recon, c, shape)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", PITCH_SHAPES, ids=sid)
def test_pitches_and_what_stays_untouched(shape, dt):
    """W_dec, recon and x as column slices of wider tensors (their pitch is kept); canary columns and rows behind recon
    and canary rows behind sq_err keep their bits."""
    rows, n, d, h, k = shape
    K = n * d
    c = case(shape, dt)
    val, idx, W, b, x = on_gpu(c, "val", "idx", "W", "b", "x")
    want, _ = ops.decode_pairs(val, idx, W, b, n, d)
    _, want_sq = ops.decode_pairs(val, idx, W, b, n, d, x=x)
    CAN = 1234.0
    Ww = torch.full((h, K + 24), CAN, dtype=DT[dt], device="cuda")
    Ww[:, 8:8 + K] = W
    xw = torch.full((rows, K + 16), CAN, dtype=DT[dt], device="cuda")
    xw[:, 16:] = x
    rw = torch.full((rows + 2, K + 40), CAN, dtype=DT[dt], device="cuda")
    sq = torch.full((rows + 2, n), CAN, dtype=torch.float32, device="cuda")
    r, s = ops.decode_pairs(val, idx, Ww[:, 8:8 + K], b, n, d, recon=rw[:rows, 32:32 + K], x=xw[:, 16:], sq_err=sq[:rows])
    assert torch.equal(bits(r), bits(want)) and torch.equal(bits(s), bits(want_sq))
    assert (rw[:, :32] == CAN).all() and (rw[:, 32 + K:] == CAN).all() and (rw[rows:] == CAN).all()
    assert (sq[rows:] == CAN).all()
    assert (Ww[:, :8] == CAN).all() and (xw[:, :16] == CAN).all()
    # recon alone through the same pitches
    rw.fill_(CAN)
    ops.decode_pairs(val, idx, Ww[:, 8:8 + K], b, n, d, recon=rw[:rows, 32:32 + K])
    assert torch.equal(bits(rw[:rows, 32:32 + K]), bits(want))
    assert (rw[:, :32] == CAN).all() and (rw[:, 32 + K:] == CAN).all() and (rw[rows:] == CAN).all()


# ---------------------------------------------------------------- through the model
MODEL_ROWS, MODEL_D, MODEL_H = 96, 36, 200  # d_in 36: the kernels run on d = 40; 200 = kernel h
# activation -> (cfg keys, k of the pairs): k at least the largest row L0 of model_x (asserted below).  ReLU on the
# seeded init fires on 75..124 of the 200 latents per row, JumpReLU at threshold 0.05 on at most 86, the BatchTopK
# selection of rows * 12 pairs takes at most 25 of one row.
ACTIVATIONS = {"relu": ({}, 144),
               "topk": ({"activation": "topk", "k": 12}, 12),
               "batch_topk": ({"activation": "batch_topk", "k": 12}, 40),
               "jumprelu": ({"activation": "jumprelu", "l0_coeff": 1.0, "jump_threshold_init": 0.05}, 104)}


def model(dt, extra):
    cfg = {"seed": 49, "batch_size": MODEL_ROWS, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 640, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": MODEL_H, "seq_len": 1024, "enc_dtype": dt, "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": MODEL_D, "log_every": 100, "save_every": 30000}
    cc = ca.CrossCoder(dict(cfg, **extra))
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():  # (a non-zero b_dec: the init's is zero)
        cc.b_dec.copy_(torch.randn(2, MODEL_D, generator=g).to(DT[dt]))
    return cc


def model_x(dt, rows=MODEL_ROWS, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, 2, MODEL_D, generator=g).to(DT[dt]).cuda()


def arena_operands(cc):
    a = cc.arena()
    a.wait_pending()
    return a.W_dec_hk.cpu(), a.b_dec_flat.cpu()


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("activation", list(ACTIVATIONS))
def test_pairs_through_the_model(activation, dt):
    extra, k = ACTIVATIONS[activation]
    cc = model(dt, extra)
    x = model_x(dt)
    acts = cc.encode(x)
    l0 = (acts > 0).sum(1)
    print("row L0 min / max:", int(l0.min()), int(l0.max()), "k:", k)
    assert int(l0.max()) <= k, "the test's precondition: k covers every row"
    vals, idx = cc.encode_pairs(x, k)
    assert vals.dtype == DT[dt] and idx.dtype == torch.int32 and tuple(vals.shape) == tuple(idx.shape) == (MODEL_ROWS, k)
    # the pairs scattered into zeros are encode's activations, bit for bit
    valid = idx >= 0
    assert torch.equal(valid.sum(1), l0) and (idx < MODEL_H).all() and (vals[~valid] == 0).all()
    dense = torch.zeros_like(acts)
    r = torch.arange(MODEL_ROWS, device="cuda").unsqueeze(1).expand_as(idx)
    dense[r[valid], idx[valid].long()] = vals[valid]
    assert torch.equal(bits(dense), bits(acts))
    # decode_pairs: the CPU restatement on the arena's own weights (kernel dims: d = 40)
    W, b = arena_operands(cc)
    dp = W.shape[1] // 2
    got = cc.decode_pairs(vals, idx)
    assert tuple(got.shape) == (MODEL_ROWS, 2, MODEL_D) and got.dtype == DT[dt]
    v_cpu, i_cpu = vals.cpu(), idx.cpu()
    crop = lambda t: t.view(MODEL_ROWS, 2, dp)[:, :, :MODEL_D]  # noqa: E731
    if dt == "bf16":
        want = ref.decode_f32(v_cpu, i_cpu, W, b, MODEL_H)
        assert torch.equal(bits(got.cpu()), bits(crop(want)))
    else:
        exact, S = ref.decode_f64(v_cpu, i_cpu, W, b, MODEL_H)
        assert ((got.cpu().double() - crop(exact)).abs() <= crop(ref.chain_tol(k, S))).all()
    # int64 indices are converted
    assert torch.equal(bits(cc.decode_pairs(vals, idx.long())), bits(got))
    # pairs_sq_err against fp64 sums over the kernel's own reconstruction (the padding columns add (0 - 0)^2)
    sq = cc.pairs_sq_err(vals, idx, x)
    want = (got.cpu().double() - x.cpu().double()).pow(2).sum(-1)
    assert sq.dtype == torch.float32 and tuple(sq.shape) == (MODEL_ROWS, 2)
    assert ((sq.cpu().double() - want).abs() <= ref.sq_tol(dp, want)).all()
    assert torch.equal(bits(sq), bits(cc.pairs_sq_err(vals, idx, x)))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_latent_ablation(dt):
    """Two batches, two groups (one empty) on a ReLU crosscoder with k = 100 of 75..124 active latents per row: some
    rows use every slot.  Each entry against an fp64 restatement from the same pairs and masks."""
    k = 100
    cc = model(dt, {})
    even = torch.arange(MODEL_H) % 2 == 0
    ab = ca.LatentAblation(cc, {"even": even, "nothing": torch.zeros(0, dtype=torch.int64)}, k=k)
    batches = [model_x(dt, 96, seed=5), model_x(dt, 40, seed=6)]
    for x in batches:
        ab.update(x)
    res = ab.result()
    sq64 = {"baseline": 0, "even": 0}
    ev64 = {"baseline": 0, "even": 0}
    full = 0
    for x in batches:
        vals, idx = cc.encode_pairs(x, k)
        full += int((idx[:, -1] >= 0).sum())
        xd = x.cpu().double()
        tv = (xd - xd.mean(0)).pow(2).sum(-1)
        gone = even.cuda()[idx.clamp(min=0).long()]
        for name, v in (("baseline", vals), ("even", vals.masked_fill(gone, 0))):
            sq = (cc.decode_pairs(v, idx).cpu().double() - xd).pow(2).sum(-1)  # [rows, 2]
            sq64[name] = sq64[name] + sq.sum(0)
            ev64[name] = ev64[name] + (1 - sq / (tv + 1e-8)).sum(0)
    assert res["rows"] == 136 and res["full_rows"] == full
    assert 0 < full < 136, "the input should mix rows that use every slot with rows that do not"
    for name in ("baseline", "even"):
        mse, ev = sq64[name] / 136, ev64[name] / 136
        got = res[name]
        print(name, "mse", got["mse"].tolist(), "fp64", mse.tolist(), "ev", got["explained_variance"].tolist())
        assert ((got["mse"] - mse).abs() <= ref.sq_tol(40, mse)).all()
        assert ((got["explained_variance"] - ev).abs() <= 1e-5).all()
        assert torch.equal(got["delta_mse"], got["mse"] - res["baseline"]["mse"])
    # the empty group is the baseline, exactly
    for key in ("mse", "explained_variance"):
        assert torch.equal(res["nothing"][key], res["baseline"][key])
    assert (res["nothing"]["delta_mse"] == 0).all()
    assert (res["even"]["delta_mse"] != 0).all()
