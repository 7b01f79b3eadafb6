"""Latent scaling on the GPU: the fused GEMM (cc_latent_scaling) against fp64 sums of its own operands, what it
leaves untouched, and LatentScaling through the model against fp64 sums of the GPU's own activations and
reconstructions.

The bounds are derived, not measured (tests/_latent_scaling_ref.py): a launch over B rows and width d sums at most
d + B fp32 terms per latent, so |S - S64| <= (d + B + 8) 2^-23 A with A the sum of the terms' magnitudes; an
indexing error is of order A."""
import ctypes

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops
from tests import _latent_scaling_ref as ref
from tests._golden import load

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
CANARY = -12345.5


def zero_cols(h):
    return [1, h - 2]


# (B, d, h, n, m, acts pitch beyond h)
SHAPES = [(96, 40, 200, 2, 1, 0),    # one ragged tile, a K tail
          (300, 72, 520, 2, 0, 8),   # 2 x 3 tiles with ragged last row and column tiles, a K tail; lda = h + 8
          (256, 64, 512, 3, 2, 0),   # whole tiles, a non-power-of-two model stride
          (8, 8, 4, 1, 0, 0)]        # the minimum shape


def operands(B, d, h, n, pad, dtype, dev, seed=0):
    """Signed Y [B, n d], W [h, n d]; acts [B, lda] >= 0, about 10 % non-zero with magnitudes over 2^-6 .. 2^4 (a
    mask in place of the multiply would show), two all-zero columns, every other column with at least one
    non-zero, junk in the pitch columns past h."""
    g = torch.Generator().manual_seed(seed)
    Y = torch.randn(B, n * d, generator=g).to(dtype)
    W = torch.randn(h, n * d, generator=g).to(dtype)
    es = 2 if dtype == torch.bfloat16 else 4
    lda = h + pad
    lda += -lda % (16 // es)  # (the row pitch is 16-byte aligned: h = 4 in bf16 runs on lda = 8)
    mag = torch.exp2(torch.rand(B, lda, generator=g) * 10 - 6)
    acts = torch.where(torch.rand(B, lda, generator=g) < 0.1, mag, torch.zeros(()))
    cols = torch.arange(h)
    acts[cols % B, cols] = mag[cols % B, cols]
    acts[:, zero_cols(h)] = 0.0
    acts[:, h:] = 7.0
    return Y.to(dev), W.to(dev), acts.to(dtype).to(dev)


def run_kernel(Y, W, acts, B, d, h, m, want_sq=True):
    """One launch on model m's slices + the two reductions -> (S [h], Q [h] or None, the slabs)."""
    R = ops.col_part_rows(B)
    dot_part = torch.full((R + 2, h), CANARY, dtype=torch.float32, device=Y.device)
    sq_part = torch.full((R + 2, h), CANARY, dtype=torch.float32, device=Y.device) if want_sq else None
    ops.latent_scaling(Y[:, m * d:(m + 1) * d], W[:, m * d:(m + 1) * d], acts, dot_part[:R],
                       None if sq_part is None else sq_part[:R])
    S = torch.empty(h, dtype=torch.float32, device=Y.device)
    ops.reduce_rows(dot_part[:R], R, h, out_f32=S)
    Q = None
    if want_sq:
        Q = torch.empty(h, dtype=torch.float32, device=Y.device)
        ops.reduce_rows(sq_part[:R], R, h, out_f32=Q)
    return S, Q, dot_part, sq_part


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_d%d_h%d_n%d_m%d_pad%d" % s)
def test_kernel_against_fp64(gpu, shape, dtype):
    B, d, h, n, m, pad = shape
    Y, W, acts = operands(B, d, h, n, pad, DT[dtype], gpu)
    before = [t.clone() for t in (Y, W, acts)]
    S, Q, dot_part, sq_part = run_kernel(Y, W, acts, B, d, h, m)
    S2, Q2, _, _ = run_kernel(Y, W, acts, B, d, h, m)
    S3, _, _, _ = run_kernel(Y, W, acts, B, d, h, m, want_sq=False)
    torch.cuda.synchronize()
    S64, A, Q64 = ref.accumulators(acts[:, :h], Y[:, m * d:(m + 1) * d], W[:, m * d:(m + 1) * d])
    errS, errQ = (S.double() - S64).abs(), (Q.double() - Q64).abs()
    print(f"max |S - S64| / A = {(errS / A.clamp(min=1e-300)).max().item():.3e} (bound "
          f"{(d + B + 8) * 2.0 ** -23:.3e}), max |Q - Q64| / Q64 = "
          f"{(errQ / Q64.clamp(min=1e-300)).max().item():.3e} (bound {(B + 2) * 2.0 ** -23:.3e})")
    assert bool((A > 0).sum() == h - 2) and bool((S64.abs() > 0.01 * A).sum() > 0)
    assert bool((errS <= ref.s_bound(B, d, A)).all())
    assert bool((errQ <= ref.q_bound(B, Q64)).all())
    zc = zero_cols(h)
    assert torch.equal(S[zc], torch.zeros(2, device=gpu)) and torch.equal(Q[zc], torch.zeros(2, device=gpu))
    # the same inputs give the same bits, with or without the acts^2 sums
    assert torch.equal(S, S2) and torch.equal(Q, Q2) and torch.equal(S, S3)
    # nothing else is written: the inputs, and the slab rows past cc_col_part_rows(B)
    for t, b in zip((Y, W, acts), before):
        assert torch.equal(t, b)
    R = ops.col_part_rows(B)
    for slab in (dot_part, sq_part):
        assert bool((slab[R:] == CANARY).all()) and not bool((slab[:R] == CANARY).any())


def test_dense_slab_in_a_padded_allocation(gpu):
    """The slabs are dense [cc_col_part_rows(B)][h]: in an allocation sized for a pitch of h + 8, exactly the first
    R h floats are written, and they hold what the [R, h] slab of another launch holds."""
    B, d, h, n, m, pad = SHAPES[1]
    Y, W, acts = operands(B, d, h, n, pad, torch.bfloat16, gpu)
    R = ops.col_part_rows(B)
    flat = [torch.full((R * (h + 8),), CANARY, dtype=torch.float32, device=gpu) for _ in range(2)]
    Ym, Wm = Y[:, m * d:(m + 1) * d], W[:, m * d:(m + 1) * d]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = ops.lib().cc_latent_scaling(ptr(Ym), Y.stride(0), ptr(Wm), W.stride(0), ptr(acts), acts.stride(0),
                                     ptr(flat[0]), ptr(flat[1]), B, d, h, ops.dtype_code(Y.dtype),
                                     ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == 0
    _, _, dot_part, sq_part = run_kernel(Y, W, acts, B, d, h, m)
    torch.cuda.synchronize()
    for f, slab in zip(flat, (dot_part, sq_part)):
        assert torch.equal(f[:R * h].view(R, h), slab[:R])
        assert bool((f[R * h:] == CANARY).all())


# ----------------------------------------------------------------------------- the class
def make_cc(cfg, P, device, n_models, dead=()):
    cc = ca.CrossCoder(dict(cfg, device=str(device)), n_models=n_models)
    cc.load_state_dict({k: v for k, v in P.items()})
    if dead:
        with torch.no_grad():
            cc.b_enc[list(dead)] = -100.0
    return cc


def class_reference(cc, x, chunks, r):
    """fp64 sums over the GPU's own bits: f = cc.encode(x), R = cc.decode(f), E = T(float(x) - float(R)) -> S_err,
    S_rec [n, h], Q [h], their bounds summed over the chunks, G."""
    n, d, h = cc.n_models, cc.cfg["d_in"], cc.d_hidden
    W = cc.W_dec.detach()
    S = torch.zeros(2, n, h, dtype=torch.float64, device=x.device)
    bS, Q, bQ = torch.zeros_like(S), torch.zeros_like(S[0, 0]), torch.zeros_like(S[0, 0])
    for r0, r1 in chunks:
        xc = x[r0:r1]
        f = cc.encode(xc)
        R = cc.decode(f)
        E = (xc.float() - R.float()).to(cc.dtype)
        for t, Y in enumerate((E, R)):
            for m in range(n):
                s, A, q = ref.accumulators(f, Y[:, m], W[:, r])
                S[t, m] += s
                bS[t, m] += ref.s_bound(r1 - r0, d, A)
        Q += q
        bQ += ref.q_bound(r1 - r0, q)
    G = torch.einsum("hd,hmd->mh", W[:, r].double(), W.double())
    return S, bS, Q, bQ, G


DEAD = (3, 64, 117)


@pytest.mark.parametrize("name", ["step_b96_n2_d40_h200_bf16", "step_b96_n2_d40_h200_fp32",
                                  "step_b64_n4_d32_h128_bf16"])
def test_class_against_fp64(gpu, name):
    r = load(name)
    cfg, n = r["cfg"], r["n_models"]
    cc = make_cc(cfg, r["init"], gpu, n, dead=DEAD)
    x = r["x"][0].to(gpu).to(cc.dtype)
    rows, h, dm = x.shape[0], cc.d_hidden, n - 1
    runs = []
    with torch.no_grad():
        one = ca.LatentScaling(cc)
        one.update(x)
        runs.append((one.result(), [(0, rows)]))
        two = ca.LatentScaling(cc, chunk_rows=32)
        two.update(x[:64])
        two.update(x[64:])
        cuts = list(range(0, 64, 32)) + list(range(64, rows, 32)) + [rows]
        runs.append((two.result(), [(a, b) for a, b in zip(cuts, cuts[1:]) if b > a]))
        for res, chunks in runs:
            S, bS, Q, bQ, G = class_reference(cc, x, chunks, dm)
            fired = Q > 0
            assert int(fired.sum()) >= h // 4  # (the reference side: the test cannot pass vacuously)
            assert res["rows_seen"] == rows and torch.equal(res["fired"], fired)
            assert not bool(fired[list(DEAD)].any())
            for key, t in (("S_err", 0), ("S_rec", 1)):
                err = (res[key] - S[t]).abs()
                print(f"{name} {key}: max err / bound = {(err / bS[t].clamp(min=1e-300)).max().item():.3f}")
                assert res[key].dtype == torch.float64 and bool((err <= bS[t]).all()), key
            assert bool(((res["Q"] - Q).abs() <= bQ).all())
            torch.testing.assert_close(res["G"], G, rtol=1e-12, atol=1e-14)
            den = (Q * G[dm]).abs()
            want = {"beta_err": (S[0] + Q * G) / (Q * G[dm]), "beta_rec": (S[1] - Q * G) / (Q * G[dm])}
            for t, key in enumerate(("beta_err", "beta_rec")):
                got = res[key]
                assert got.shape == (n, h) and got.dtype == torch.float64
                assert bool(got[:, list(DEAD)].isnan().all()) and bool(res["nu" + key[4:]][:, list(DEAD)].isnan().all())
                tol = bS[t] / den  # S's bound over the denominator
                ratio = ((got - want[key]).abs() / tol)[:, fired].max().item()
                print(f"{name} {key}: max err / bound = {ratio:.3f}")
                assert bool(((got - want[key]).abs()[:, fired] <= tol[:, fired]).all()), key
                assert not bool(got[:, fired].isnan().any())
            torch.testing.assert_close(res["nu_err"][:, fired], (res["beta_err"] / res["beta_err"][dm])[:, fired],
                                       rtol=0, atol=0)


def test_padded_kernel_dims(gpu):
    """dict_size 203 and d_in 36 run on kernel dims 208 and 40 (zero padding latents and columns): the results
    cover the 203 latents and meet the same bounds against the reference-shaped tensors."""
    B, n, d, h = 80, 2, 36, 203
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": B * 100, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(gpu),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    cc = ca.CrossCoder(cfg, n_models=n)
    assert (cc._hp, cc._dp) == (208, 40)
    x = torch.randn(B, n, d, generator=torch.Generator().manual_seed(3)).to(gpu).to(cc.dtype)
    with torch.no_grad():
        ls = ca.LatentScaling(cc, decoder_model=0)
        ls.update(x)
        res = ls.result()
        S, bS, Q, bQ, G = class_reference(cc, x, [(0, B)], 0)
    assert int((Q > 0).sum()) >= h // 4 and res["Q"].shape == (h,) and res["beta_err"].shape == (n, h)
    for key, t in (("S_err", 0), ("S_rec", 1)):
        assert bool(((res[key] - S[t]).abs() <= bS[t]).all()), key
    assert bool(((res["Q"] - Q).abs() <= bQ).all())
    torch.testing.assert_close(res["G"], G, rtol=1e-12, atol=1e-14)


def test_topk_activations_enter(gpu):
    """A TopK crosscoder: the accumulators use its own activations -- Q is the column sums of squares of cc.encode(x)
    and at most k non-zeros per row entered."""
    r = load("step_b64_n2_d32_h256_bf16")
    k = 8
    cc = make_cc(dict(r["cfg"], activation="topk", k=k), r["init"], gpu, r["n_models"])
    x = r["x"][0].to(gpu).to(cc.dtype)
    with torch.no_grad():
        f = cc.encode(x)
        ls = ca.LatentScaling(cc)
        ls.update(x)
        res = ls.result()
    nz = (f > 0).sum(1)
    assert int(nz.max()) <= k and int(nz.sum()) > 0
    Q64 = (f.double() ** 2).sum(0)
    assert bool(((res["Q"] - Q64).abs() <= ref.q_bound(x.shape[0], Q64)).all())
    assert torch.equal(res["fired"], (f > 0).any(0))
    assert int(res["fired"].sum()) <= k * x.shape[0]
    relu = make_cc(r["cfg"], r["init"], gpu, r["n_models"])
    with torch.no_grad():
        assert int((relu.encode(x) > 0).any(0).sum()) > int(res["fired"].sum())  # (ReLU activations would show)


def test_parts_equal_the_whole(gpu):
    r = load("step_b96_n2_d40_h200_bf16")
    cc = make_cc(r["cfg"], r["init"], gpu, r["n_models"], dead=DEAD)
    x = r["x"][0].to(gpu).to(cc.dtype)
    with torch.no_grad():
        whole = ca.LatentScaling(cc)
        whole.update(x)
        f = cc.encode(x)
        R = cc.decode(f)
        E = (x.float() - R.float()).to(cc.dtype)
        parts = ca.LatentScaling(cc)
        parts.update_from_parts(f, E.flatten(1), R.flatten(1))
    a, b = whole.result(), parts.result()
    assert a["rows_seen"] == b["rows_seen"] == x.shape[0]
    for key in ("S_err", "S_rec", "Q", "G", "fired"):
        assert torch.equal(a[key], b[key]), key
    for key in ("beta_err", "beta_rec", "nu_err", "nu_rec"):
        assert torch.equal(a[key].isnan(), b[key].isnan()) and torch.equal(a[key].nan_to_num(), b[key].nan_to_num())
    parts.reset()
    assert parts.rows_seen == 0 and not bool(parts.result()["fired"].any())
