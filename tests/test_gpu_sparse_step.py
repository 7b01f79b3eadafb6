"""The sparse TopK step on the GPU: cc_pairs_group, cc_decode_pairs_partial and cc_pairs_wgrad
against their CPU restatements (tests/_sparse_step_ref.py, where the bounds are derived) and against the parent's
cc_pairs_grad_decoder, then Trainer.step with cfg["sparse_step"] against the dense TopK step, fp64 and cc_adam_step.

The kernel cases are one step's backward operands (tests/_sparse_step_ref.make_case): the pairs are the reference top-k
of a real encode, so they carry the -1 padding of rows with fewer than k positive activations; the skewed case forces
one latent into every row (a list of 300: two full pieces of 128 and a rest), keeps 24 latents silent and starves some
rows, and asserts all three before use."""
import functools
import math

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops
from oracle import cpu_reference as O
from tests import _decode_pairs_ref as dref
from tests import _pairs_grad_ref as pref
from tests import _sparse_step_ref as ref
from tests._golden import load
from tests.test_gpu_parity import _Replay, envelope_ok, make_cc, rel
from tests.test_gpu_topk import masked_losses, small_cfg

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32, torch.int64: torch.int64}
# (B, n, d, h, k): base; nothing a tile multiple; n = 4; skewed
SHAPES = [(64, 2, 32, 256, 8), (96, 2, 40, 200, 5), (128, 4, 64, 256, 16), (300, 2, 32, 128, 8)]
SKEW = SHAPES[3]
# cc_pairs_wgrad only: 257 eight-column groups (a second, ragged pass of the lane loop) on SKEW's list of latent 3
WIDE_SKEW = (300, 1, 2056, 64, 8)
SKEWED = (SKEW, WIDE_SKEW)
# the decode only, cc_decode_pairs' cases (tests/_decode_pairs_ref.make_case): K = 2088, one chunk of 2048 columns and a
# ragged 40; k beyond one staged tile, staged again for each of two chunks; one small
DECODE_WIDE = [(5, 3, 696, 64, 9), (3, 2, 1032, 512, 300)]
DECODE_SMALL = (3, 2, 40, 200, 5)
CAN = 1234.0
ICAN = -77


def sid(s):
    return "B%d_n%d_d%d_h%d_k%d" % s


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


@functools.lru_cache(maxsize=None)
def case(shape, dt):
    """The shared case of a shape: CPU operands and references (computed once, never written)."""
    B, n, d, h, k = shape
    c = ref.make_case(B, n, d, h, k, DT[dt], skew=shape in SKEWED)
    if shape in SKEWED:
        ref.assert_skewed(c["idx"], h, k)
    c["perm"], c["seg"] = pref.by_latent_loop(c["idx"], h)
    c["len"] = torch.tensor(c["seg"][1:]) - torch.tensor(c["seg"][:-1])
    return c


@functools.lru_cache(maxsize=None)
def decode_case(shape, dt):
    """The shared decode-only case of a shape: cc_decode_pairs' operands under this file's names"""
    c = dref.make_case(*shape, DT[dt])
    return {"val": c["val"], "idx": c["idx"], "W_dec": c["W"]}


def on_gpu(c, *names):
    return [c[name].cuda() for name in names]


# ---------------------------------------------------------------- cc_pairs_group
HAND = torch.tensor([[5, -1, 5, 9], [200, 5, 0, 5], [-7, 9, 9, 9], [0, 63, 64, -2 ** 31], [5, 5, 5, 5]], dtype=torch.int32)


def group_inputs():
    g = torch.Generator().manual_seed(11)
    out = [("hand", HAND, 64), ("k1", torch.randint(-2, 12, (37, 1), generator=g, dtype=torch.int32), 10)]
    # three row blocks and two chunks of the scan (2056 x 3 cells); latent 2 in every row, twice in some
    wide = torch.randint(-1, 2056, (600, 4), generator=g, dtype=torch.int32)
    wide[:, 1] = 2
    wide[::7, 3] = 2
    out.append(("blocks", wide, 2056))
    for s in SHAPES:
        out.append((sid(s), case(s, "bf16")["idx"], s[3]))
    return out


@pytest.mark.parametrize("name,idx,h", group_inputs(), ids=[g[0] for g in group_inputs()])
def test_group_equals_pairs_by_latent(name, idx, h):
    Bk = idx.numel()
    dev = torch.device("cuda")
    idx_g = idx.cuda()
    want_perm, want_seg = ops.pairs_by_latent(idx_g, h)
    lp, ls = pref.by_latent_loop(idx, h)
    assert want_seg.cpu().tolist() == ls and want_perm[:ls[-1]].cpu().tolist() == lp
    need = ops.pairs_group_ws_bytes(idx.shape[0], idx.shape[1], h)
    runs = []
    for _ in range(2):
        perm = torch.full((Bk + 16,), ICAN, dtype=torch.int32, device=dev)
        seg = torch.full((h + 1 + 8,), ICAN, dtype=torch.int64, device=dev)
        ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=dev)
        ops.pairs_group(idx_g, h, perm=perm[:Bk], seg=seg[:h + 1], ws=ws)
        assert torch.equal(seg[:h + 1], want_seg), name
        assert torch.equal(perm[:ls[-1]], want_perm[:ls[-1]]), name
        rest = perm[ls[-1]:Bk]
        assert bool((rest >= 0).all()) and bool((rest < Bk).all())
        assert bool((perm[Bk:] == ICAN).all()) and bool((seg[h + 1:] == ICAN).all()) and bool((ws[need:] == 0x5A).all())
        runs.append((perm.clone(), seg.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])     # two calls: equal bits
    assert torch.equal(bits(idx_g.cpu()), bits(idx))
    alloc_perm, alloc_seg = ops.pairs_group(idx_g, h)                                      # the allocating form
    assert torch.equal(alloc_seg, want_seg) and torch.equal(alloc_perm[:ls[-1]], want_perm[:ls[-1]])


# ---------------------------------------------------------------- cc_decode_pairs_partial
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES + DECODE_WIDE, ids=sid)
def test_decode_partial_is_the_fma_chain(shape, dt):
    B, n, d, h, k = shape
    K = n * d
    c = decode_case(shape, dt) if shape in DECODE_WIDE else case(shape, dt)
    val, idx, W = on_gpu(c, "val", "idx", "W_dec")
    want = ref.decode_partial_f32(c["val"], c["idx"], c["W_dec"], h, K)
    got = ops.decode_pairs_partial(val, idx, W, K)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, K)
    assert torch.equal(bits(got.cpu()), bits(want))
    # invalid slots add nothing: -1 and >= h in the middle of rows, with values a kernel that read them would show
    bad = c["idx"].clone()
    bad[::3, k // 2] = -1
    bad[1::3, 0] = h + 5
    bad[2::3, k - 1] = -2 ** 31
    want_bad = ref.decode_partial_f32(c["val"], bad, c["W_dec"], h, K)
    assert not torch.equal(want_bad, want)
    assert torch.equal(bits(ops.decode_pairs_partial(val, bad.cuda(), W, K).cpu()), bits(want_bad))
    # a narrower h drops the latents beyond it
    half = ref.decode_partial_f32(c["val"], c["idx"], c["W_dec"], h // 2, K)
    assert torch.equal(bits(ops.decode_pairs_partial(val, idx, W, K, h=h // 2).cpu()), bits(half))
    # pitches: W_dec a column slice, recon a slice of a wider matrix
    Ww = torch.full((h, K + 24), CAN, dtype=DT[dt], device="cuda")
    Ww[:, 8:8 + K] = W
    rw = torch.full((B + 2, K + 12), CAN, dtype=torch.float32, device="cuda")
    out = ops.decode_pairs_partial(val, idx, Ww[:, 8:8 + K], K, recon=rw[:B, 4:4 + K])
    assert torch.equal(bits(out), bits(got))
    assert bool((rw[B:] == CAN).all()) and bool((rw[:, :4] == CAN).all()) and bool((rw[:, 4 + K:] == CAN).all())
    assert torch.equal(bits(ops.decode_pairs_partial(val, idx, W, K)), bits(got))           # two calls


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", DECODE_WIDE + [DECODE_SMALL], ids=sid)
def test_decode_pairs_is_the_rounded_partial(shape, dt):
    """cc_decode_pairs with a zero b_dec is cc_decode_pairs_partial rounded once: the same chain from +0"""
    B, n, d, h, k = shape
    K = n * d
    val, idx, W = on_gpu(decode_case(shape, dt), "val", "idx", "W_dec")
    recon, _ = ops.decode_pairs(val, idx, W, torch.zeros(K, dtype=DT[dt], device="cuda"), n, d)
    partial = ops.decode_pairs_partial(val, idx, W, K)
    assert float(partial.abs().sum()) > 0
    assert torch.equal(bits(recon), bits(partial.to(DT[dt])))


# ---------------------------------------------------------------- cc_pairs_wgrad
def run_wgrad(c, shape, dt, h_kernel=None, canaries=False):
    B, n, d, h, k = shape
    K = n * d
    hk = h if h_kernel is None else h_kernel
    dev = torch.device("cuda")
    val, gpre, gr, x = on_gpu(c, "val", "g_pre", "g_recon", "x")
    perm = torch.tensor(c["perm"] + [0] * (B * k - len(c["perm"])), dtype=torch.int32, device=dev)
    seg = torch.tensor(c["seg"] + [c["seg"][-1]] * (hk - h), dtype=torch.int64, device=dev)
    parts = ops.pairs_wgrad_parts(hk)
    pad = 8 if canaries else 0
    dWd = torch.full((hk + 2, K + 40), CAN, dtype=DT[dt], device=dev)
    dWe = torch.full((hk + 2, K + 40), CAN, dtype=DT[dt], device=dev)
    db = torch.full((hk + 8,), CAN, dtype=DT[dt], device=dev)
    sq = [torch.full((parts + pad,), CAN, dtype=torch.float32, device=dev) for _ in range(3)]
    ws = torch.full((ops.pairs_wgrad_ws_floats(B * k, K) + 64,), CAN, dtype=torch.float32, device=dev)
    ops.pairs_wgrad(perm, seg, val, gpre, gr, x, K, dWd[:hk, 32:32 + K], dWe[:hk, 32:32 + K], db[:hk], sq[0][:parts],
                    sq[1][:parts], sq[2][:parts], ws=ws)
    return {"perm": perm, "seg": seg, "dWd": dWd, "dWe": dWe, "db": db, "sq": sq, "ws": ws, "parts": parts}


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES + [WIDE_SKEW], ids=sid)
def test_wgrad_against_the_row_kernel_and_the_restatements(shape, dt):
    B, n, d, h, k = shape
    K = n * d
    c = case(shape, dt)
    r = run_wgrad(c, shape, dt, canaries=True)
    val, gpre, gr, x = on_gpu(c, "val", "g_pre", "g_recon", "x")
    parts = r["parts"]
    got_d, got_e, got_b = r["dWd"][:h, 32:32 + K], r["dWe"][:h, 32:32 + K], r["db"][:h]
    # both weight gradients: the parent's cc_pairs_grad_decoder on the same operands, bit for bit
    want_d = ops.pairs_grad_decoder(r["perm"], r["seg"], val, gr, K)
    want_e = ops.pairs_grad_decoder(r["perm"], r["seg"], gpre.to(DT[dt]), x, K)
    assert torch.equal(bits(got_d), bits(want_d)) and torch.equal(bits(got_e), bits(want_e))
    assert float(want_d.float().abs().sum()) > 0 and float(want_e.float().abs().sum()) > 0
    # db_enc in the documented order
    p = c["g_pre"].to(DT[dt])
    want_b = ref.lists_sum_f32(c["perm"], c["seg"], p)
    if dt == "bf16":
        assert torch.equal(bits(got_b.cpu()), bits(want_b.to(torch.bfloat16)))
    else:
        lat = torch.repeat_interleave(torch.arange(h), c["len"])
        slots = torch.tensor(c["perm"], dtype=torch.int64)
        flat = p.reshape(-1).double()[slots]
        exact = torch.zeros(h, dtype=torch.float64).index_add_(0, lat, flat)
        S = torch.zeros(h, dtype=torch.float64).index_add_(0, lat, flat.abs())
        err, tol = (got_b.cpu().double() - exact).abs(), (c["len"].double() + 1) * 2.0 ** -23 * S
        print("max |db_enc - fp64| / bound:", float((err / tol.clamp(min=1e-300)).max()))
        assert bool((err <= tol).all())
    # empty lists: rows of +0
    empty = c["len"] == 0
    assert shape not in SKEWED or int(empty.sum()) >= 24
    if empty.any():
        assert bool((bits(got_d.cpu())[empty] == 0).all()) and bool((bits(got_e.cpu())[empty] == 0).all())
        assert bool((bits(got_b.cpu())[empty] == 0).all())
    if shape in SKEWED:
        assert int(c["len"][3]) == B and B > 2 * ref.SPLIT and B % ref.SPLIT        # two full pieces and a rest
    # squared sums of the stored values.  D = 18: 8 additions for the one 8-column group a lane stores (K / 8 <= 256
    # groups, one row per workgroup), 6 for the butterfly, 4 for the waves (tests/_sparse_step_ref.py); WIDE_SKEW's lane
    # 0 stores a second group: 26
    D = ref.sq_chain_depth(h, K)
    assert D == (26 if shape == WIDE_SKEW else 18) and parts == h
    for name, part, stored in (("dW_dec", r["sq"][0], got_d), ("dW_enc", r["sq"][1], got_e), ("db_enc", r["sq"][2], got_b)):
        total = float(part[:parts].double().sum())
        exact = float(stored.double().pow(2).sum())
        print(name, "sq rel err / bound:", abs(total - exact) / max(exact, 1e-300) / ((D + 1) * 2.0 ** -24))
        assert exact > 0 and abs(total - exact) <= (D + 1) * 2.0 ** -24 * exact, name
        assert torch.equal(bits(part[:parts].cpu()), bits(ref.sq_partials(stored.cpu()))), name   # the documented order
        assert bool((part[parts:] == CAN).all()), name
    # what stays untouched
    for t in (r["dWd"], r["dWe"]):
        assert bool((t[h:] == CAN).all()) and bool((t[:, :32] == CAN).all()) and bool((t[:, 32 + K:] == CAN).all())
    assert bool((r["db"][h:] == CAN).all())
    need = ops.pairs_wgrad_ws_floats(B * k, K)
    assert bool((r["ws"][need:] == CAN).all())
    assert shape not in SKEWED or need == (B * k // ref.SPLIT) * (2 * K + 8)
    # two calls: equal bits
    r2 = run_wgrad(c, shape, dt, canaries=True)
    for key in ("dWd", "dWe", "db"):
        assert torch.equal(bits(r[key]), bits(r2[key])), key
    for a, b in zip(r["sq"], r2["sq"]):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_wgrad_padding_latents_get_rows_of_zero(dt):
    """The kernel h beyond the dictionary (padded_dims): latents without a list, rows of +0, the real rows unchanged"""
    shape = SHAPES[1]
    B, n, d, h, k = shape
    K = n * d
    c = case(shape, dt)
    r, rp = run_wgrad(c, shape, dt), run_wgrad(c, shape, dt, h_kernel=h + 8)
    for key in ("dWd", "dWe"):
        assert torch.equal(bits(r[key][:h]), bits(rp[key][:h])), key
        assert bool((bits(rp[key][h:h + 8, 32:32 + K]) == 0).all()), key
    assert torch.equal(bits(r["db"][:h]), bits(rp["db"][:h])) and bool((bits(rp["db"][h:h + 8]) == 0).all())


# ---------------------------------------------------------------- the step, through Trainer
def step_cfg(B, d, h, dtype, k, **kw):
    return small_cfg(B, d, h, dtype, "cuda:0", l1_coeff=0.0, activation="topk", k=k, **kw)


def trainer_of(cfg, n=2, rows=None, seed=3, b_enc=None):
    cc = ca.CrossCoder(cfg, n_models=n)
    if b_enc is not None:
        with torch.no_grad():
            cc.b_enc.copy_(b_enc.to(cc.b_enc.device))
    B = cfg["batch_size"]
    return ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=rows or 3 * B, n_models=n, seed=seed), crosscoder=cc)


def scattered_pairs(ws, h):
    """The sparse step's pairs scattered into zeros [B, h] (a padding slot lands in a column of its own)"""
    idx, val = ws.pair_idx.long(), ws.pair_val
    out = torch.zeros(idx.shape[0], ws.h + 1, dtype=val.dtype, device=val.device)
    out.scatter_(1, torch.where(idx >= 0, idx, torch.full_like(idx, ws.h)), val)
    return out[:, :h]


def skew_b_enc(h):
    b = torch.full((h,), -0.18)   # 1.6 standard deviations of a pre-activation at the initial weights
    b[3] = 5.0
    b[h - 24:] = -5.0
    return b


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,n,d,h,k", [(256, 2, 64, 512, 32), (96, 2, 40, 203, 5)], ids=["b256", "ragged-padded"])
def test_same_selection_as_the_dense_step(gpu, B, n, d, h, k, dtype):
    """One state, one batch: the pairs scattered into zeros are the dense step's masked activations, and the count
    and the raw fp32 l1 scalar have equal bits."""
    dense = trainer_of(step_cfg(B, d, h, dtype, k), n)
    sparse = trainer_of(step_cfg(B, d, h, dtype, k, sparse_step=True), n)
    assert sparse.sparse_step is True and dense.sparse_step is False
    dd, ds = dense.step(), sparse.step()
    l1 = [torch.tensor(float(t._mapped.f32[1])) for t in (dense, sparse)]
    dense.synchronize()
    sparse.synchronize()
    torch.cuda.synchronize()
    ws = sparse._last_ws
    assert ws.sparse and ws is sparse._sparse_ws and ws.g_pre is None and sparse.crosscoder._ws is None
    masked = dense.crosscoder._ws.acts[:, :h]
    assert torch.equal(bits(scattered_pairs(ws, h)), bits(masked))
    assert 0 < dd["l0_loss"] <= k and dd["l0_loss"] == ds["l0_loss"]
    assert torch.equal(bits(l1[0]), bits(l1[1])) and l1[0].item() > 0
    assert ds.keys() == dd.keys() and ds["l1_coeff"] == 0 and ds["loss"] == ds["l2_loss"]
    if sparse.crosscoder._hp > h:   # the padding latents' gradient rows are +0
        G = sparse.optimizer.grads
        assert bool((bits(G.W_enc_hk[h:]) == 0).all()) and bool((bits(G.W_dec_hk[h:]) == 0).all())
        assert bool((bits(G.b_enc[h:]) == 0).all())


def clip_reference(grads, dt):
    """(coefficient, total norm) of clip_grad_norm_(max_norm=1.0) on the stored gradients: torch's own arithmetic on
    the bf16 tensors, fp64 for fp32 ones"""
    if dt == torch.bfloat16:
        total = O.clip_grad_norm([g.detach().cpu().clone() for g in grads]).float().item()
    else:
        total = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
    return min(1.0, 1.0 / (total + 1e-6)), total


@pytest.mark.parametrize("name", ["step_b256_n2_d64_h512_bf16", "step_b96_n2_d40_h200_bf16",
                                  "step_b256_n2_d64_h512_fp32", "step_b96_n2_d40_h200_fp32"])
def test_losses_gradients_and_clip_with_the_gpu_mask(gpu, name):
    """test_gpu_topk.test_losses_and_gradients_with_the_gpu_mask's method and bounds on Trainer.step: with the step's own
    selection M imposed on the oracle, bf16 error against fp64 <= 2 x the CPU-bf16 error + 2e-3 (loss fields) / 5e-3
    (gradients), fp32 rel < 2e-5 -- for the sparse step and, in the same test, for the dense TopK step.  Then the clip:
    clip_out[0] against clip_grad_norm_'s arithmetic on the stored gradients, as cc_clip_finalize is checked
    (tests/test_gpu_step_ops.py): bf16 within one bf16 ulp (2^-7) of torch on the bf16 tensors; fp32 within 2^-19 of
    fp64 -- 2^-22 for the finaliser given the sums, plus half (the square root) of the sums' own (D + 1) 2^-24,
    D = 18."""
    r = load(name)
    cfg, P, x, n = r["cfg"], r["init"], r["x"][0], r["n_models"]
    dt = O.DTYPES[cfg["enc_dtype"]]
    k = 32
    base = dict(cfg, activation="topk", k=k, l1_coeff=0.0)
    out = {}
    for mode in ("sparse", "dense"):
        c = dict(base, sparse_step=True) if mode == "sparse" else base
        cc = make_cc(c, P, gpu, n)
        tr = ca.Trainer(dict(c, device=str(gpu)), buffer=_Replay([x], [torch.ones(n)], gpu), crosscoder=cc)
        assert tr.sparse_step == (mode == "sparse")
        dct = tr.step()
        tr.synchronize()
        torch.cuda.synchronize()
        ws = tr._last_ws
        h = cfg["dict_size"]
        M = ((scattered_pairs(ws, h) if mode == "sparse" else ws.acts[:, :h]) > 0).cpu()
        grads = {key: v.detach().clone() for key, v in tr.optimizer.grads.views().items()}
        out[mode] = (dct, M, grads, ws.clip_out[:2].cpu().clone())
    assert torch.equal(out["sparse"][1], out["dense"][1])
    M = out["sparse"][1]
    assert bool((M.sum(1) <= k).all()) and M.sum().item() > 0.9 * k * x.shape[0]

    def oracle(dtype):
        leaves = {key: v.detach().to(dtype).clone().requires_grad_(True) for key, v in P.items()}
        res = masked_losses(x.to(dt).to(dtype), leaves, dtype, M=M)
        res["l2_loss"].backward()
        return res, {key: leaves[key].grad for key in O.PARAM_ORDER}

    ref_, gref = oracle(dt)
    truth, gtruth = oracle(torch.float64)
    fields = ("l2_loss", "l1_loss", "explained_variance", "explained_variance_A", "explained_variance_B")
    for mode in ("sparse", "dense"):
        dct, _, grads, clip = out[mode]
        assert dct["l0_loss"] == M.sum(1).float().mean().item()
        for key in fields:
            ours = torch.tensor(dct[key], dtype=torch.float64)
            # (the step logs a vector's mean; the CPU reference forms it in its own dtype, as the reference trainer does)
            t, c_ = truth[key].detach().double().mean(), ref_[key].detach().mean().double()
            if dt == torch.float32:
                e = rel(ours, t)
                print(name, mode, key, "rel", e)
                assert e < 2e-5, (mode, key, e)
            else:
                ok, e = envelope_ok(ours, c_, t)
                print(name, mode, key, "(ours, cpu) vs fp64", e)
                assert ok, (mode, key, e)
        for key in O.PARAM_ORDER:
            g = grads[key]
            assert g.shape == gref[key].shape and g.dtype == gref[key].dtype, key
            if dt == torch.float32:
                e = rel(g, gtruth[key])
                print(name, mode, key, "grad rel", e)
                assert e < 2e-5, (mode, key, e)
            else:
                ok, e = envelope_ok(g, gref[key], gtruth[key], floor=5e-3)
                print(name, mode, key, "grad (ours, cpu) vs fp64", e)
                assert ok, (mode, key, e)
        coef, total = clip_reference([grads[key] for key in O.PARAM_ORDER], dt)
        tol = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -19
        print(name, mode, "clip", clip.tolist(), "reference", (coef, total))
        assert math.isclose(clip[1].item(), total, rel_tol=tol), (mode, clip[1].item(), total)
        assert math.isclose(clip[0].item(), coef, rel_tol=tol), (mode, clip[0].item(), coef)


@pytest.mark.parametrize("master", [False, True], ids=["bf16-state", "master-weights"])
def test_adam_consumed_these_gradients(gpu, master):
    """bf16.  After a step the parameters (master mode: the masters) and both moments are cc_adam_step of the previous
    state with the step's gradients and clip_out[0], bit for bit; with master weights the bf16 parameters are the
    rounded masters."""
    B, n, d, h, k = 256, 2, 64, 512, 32
    cfg = step_cfg(B, d, h, "bf16", k, sparse_step=True, lr=1e-2, master_weights=master)
    tr = trainer_of(cfg, n)
    o, a = tr.optimizer, tr.crosscoder.arena()
    assert o.master_mode == master
    for s in range(2):
        tr.synchronize()
        torch.cuda.synchronize()
        p0 = (o.master_for_update() if master else a).data.clone()
        m0, v0 = o.exp_avg.data.clone(), o.exp_avg_sq.data.clone()
        lr = o.param_groups[0]["lr"]
        tr.step()
        tr.synchronize()
        torch.cuda.synchronize()
        assert tr._last_ws.sparse
        g = o.grads.data
        b1, b2 = o.param_groups[0]["betas"]
        ops.adam_step(p0, g.float() if master else g, m0, v0, tr._last_ws.clip_out[0:1], lr, b1, b2,
                      o.param_groups[0]["eps"], o.t)
        torch.cuda.synchronize()
        now = (o.master if master else a).data
        assert torch.equal(bits(now), bits(p0)), (s, int((bits(now) != bits(p0)).sum()))
        assert torch.equal(bits(o.exp_avg.data), bits(m0)) and torch.equal(bits(o.exp_avg_sq.data), bits(v0)), s
        assert float(g.float().abs().sum()) > 0 and float(o.exp_avg.data.float().abs().sum()) > 0
        if master:
            assert torch.equal(bits(a.data), bits(o.master.data.to(torch.bfloat16))), s


@pytest.mark.parametrize("skew", [False, True], ids=["plain", "skewed"])
def test_sparse_steps_are_reproducible(gpu, skew):
    """Two sparse trainers from one cfg and buffer seed, 3 steps each, bf16: equal loss dicts and equal bits of all four
    parameters after every step.  skewed: SKEW's shape with one latent forced into every row through its b_enc, 24
    latents silenced and the rest pushed down until some rows hold fewer than k positive activations (asserted on the
    first step's pairs)."""
    B, n, d, h, k = SKEW if skew else (256, 2, 64, 512, 32)
    cfg = step_cfg(B, d, h, "bf16", k, sparse_step=True, lr=1e-2)

    def run():
        tr = trainer_of(cfg, n, rows=3 * B, b_enc=skew_b_enc(h) if skew else None)
        out = []
        for s in range(3):
            dct = tr.step()
            tr.synchronize()
            torch.cuda.synchronize()
            if skew and s == 0:
                ref.assert_skewed(tr._last_ws.pair_idx.cpu(), h, k)
            out.append((dct, [getattr(tr.crosscoder, p).detach().clone() for p in O.PARAM_ORDER]))
        return out

    a, b = run(), run()
    for s, ((d0, p0), (d1, p1)) in enumerate(zip(a, b)):
        assert d0 == d1, (s, d0, d1)
        for name, x, y in zip(O.PARAM_ORDER, p0, p1):
            assert torch.equal(bits(x), bits(y)), (s, name, int((bits(x) != bits(y)).sum()))
    assert not torch.equal(a[0][1][0], a[2][1][0])   # the steps did move W_enc


def test_checkpoint_round_trips_the_key(gpu, tmp_path, monkeypatch):
    B, n, d, h, k = 96, 2, 40, 203, 5
    cfg = step_cfg(B, d, h, "bf16", k, sparse_step=True)
    tr = trainer_of(cfg, n)
    tr.step()
    monkeypatch.chdir(tmp_path)
    tr.save()
    loaded = ca.CrossCoder.load("version_0", 0)
    assert loaded.cfg["sparse_step"] is True and loaded.activation == "topk" and loaded.k == k
    x = torch.randn(B, n, d, generator=torch.Generator(device=gpu).manual_seed(8), device=gpu)
    with torch.no_grad():
        e0, e1 = tr.crosscoder.encode(x), loaded.encode(x)
    assert torch.equal(bits(e0), bits(e1)) and int((e0 > 0).sum(1).max()) <= k
    assert ca.Trainer(loaded.cfg, buffer=tr.buffer, crosscoder=loaded).sparse_step is True
