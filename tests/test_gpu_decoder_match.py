"""Decoder matching on the GPU: the fused GEMM (cc_decoder_match) and the key merge (cc_match_reduce) against the fp64
cosine matrix of their own operands, the key order, what they leave untouched, and match_decoders through the model.

The tolerance is derived, not measured (tests/_decoder_match_ref.py): tol = (2K + 16) 2^-23 per score with K the
contraction length; an indexing error shows as a difference of order 0.1 to 1."""
import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import decoder_match, ops
from tests import _decoder_match_ref as ref

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
CANARY = -2  # 0xff..fe: a high word of all ones is the image of a NaN score, which no finite input gives

# (candidates M, queries N, n, d, model)
SHAPES = [(200, 96, 2, 40, 1),    # one ragged tile, a K tail
          (520, 776, 2, 40, 0),   # 3 x 4 tiles with ragged last tiles
          (512, 256, 3, 64, 2),   # whole tiles, a non-power-of-two model stride
          (8, 8, 1, 8, 0)]        # the minimum
# (shape, model or None = joint, chunk_rows)
CASES = [(s, s[4], 4096) for s in SHAPES] + [(SHAPES[1], None, 4096), (SHAPES[1], 0, 256)]


def case_id(c):
    (M, N, n, d, _), model, chunk = c
    return "M%d_N%d_n%d_d%d_%s_chunk%d" % (M, N, n, d, "joint" if model is None else "m%d" % model, chunk)


def planted(M, N, n, d, dtype, seed=0, noise=0.05):
    """Random signed queries Wq [N, n d] and candidates Wc [M, n d], with noisy copies of a known permutation of half
    the queries (at most M / 2) planted among the candidates -> (Wc, Wq, query ids, their candidate rows), on the
    CPU in dtype."""
    g = torch.Generator().manual_seed(seed)
    Wq = torch.randn(N, n * d, generator=g)
    Wc = torch.randn(M, n * d, generator=g)
    P = min(M, N) // 2
    qid = torch.randperm(N, generator=g)[:P]
    row = torch.randperm(M, generator=g)[:P]
    Wc[row] = Wq[qid] + noise * torch.randn(P, n * d, generator=g)
    return Wc.to(dtype), Wq.to(dtype), qid, row


def slices(Wc, Wq, d, model):
    if model is None:
        return Wc, Wq
    return Wc[:, model * d:(model + 1) * d], Wq[:, model * d:(model + 1) * d]


def run(Wc, Wq, n, d, model, chunk_rows=4096, exclude_diag=False):
    """The launch sequence on device operands [., n d] through the ops wrappers, with canary rows behind the slab ->
    (best keys [N], index, cosine, the slab with its canary rows, the slab rows of a full chunk)."""
    cs, qs = (decoder_match.inverse_norms(W, n, d, model) for W in (Wc, Wq))
    A, B = slices(Wc, Wq, d, model)
    M, N = A.shape[0], B.shape[0]
    best = torch.zeros(N, dtype=torch.int64, device=Wq.device)
    rows = min(chunk_rows, M)
    slab = torch.full((ops.col_part_rows(rows) + 2, N), CANARY, dtype=torch.int64, device=Wq.device)
    for r0 in range(0, M, rows):
        r1 = min(M, r0 + rows)
        R = ops.col_part_rows(r1 - r0)
        ops.decoder_match(A[r0:r1], B, cs, qs, slab[:R], row0=r0, exclude_diag=exclude_diag)
        ops.match_reduce(slab[:R], best)
    index, cosine = decoder_match.decode_keys(best, qs)
    return best, index, cosine, slab, ops.col_part_rows(rows)


def check_against_fp64(index, cosine, Wc, Wq, K, exclude_diag=False, label=""):
    """Every query with a non-zero vector and at least one valid candidate: |cosine - cos64[index]| <= tol and
    cos64[index] >= max cos64 - 2 tol.  -> (cos64 masked, fp64 argmax)."""
    cos, ok_c, ok_q = ref.cosines(Wc, Wq)
    m = ref.masked(cos, ok_c, exclude_diag)
    index, cosine = index.cpu(), cosine.cpu().double()
    want = ok_q & bool(ok_c.any())
    assert torch.equal(index >= 0, want) and torch.equal(cosine.isnan(), ~want)
    j = torch.nonzero(want).flatten()
    got = m[index[j], j]
    t = ref.tol(K)
    err, short = (cosine[j] - got).abs().max().item(), (m[:, j].max(0).values - got).max().item()
    print(f"{label} max |cosine - cos64[index]| = {err:.3e}, max (max cos64 - cos64[index]) = {short:.3e}, tol {t:.3e}")
    assert bool(((cosine[j] - got).abs() <= t).all())
    assert bool((got >= m[:, j].max(0).values - 2 * t).all())
    return m, m.argmax(0)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_against_fp64(gpu, case, dtype):
    (M, N, n, d, _), model, chunk = case
    K = n * d if model is None else d
    Wc, Wq, qid, row = planted(M, N, n, d, DT[dtype])
    A64, B64 = slices(Wc, Wq, d, model)
    cos, ok_c, _ = ref.cosines(A64, B64)
    top2 = cos[:, qid].topk(2, dim=0).values  # of the fp64 reference alone: the planted matches are unambiguous
    assert bool((top2[0] - top2[1] > 4 * ref.tol(K)).all()) and torch.equal(cos[:, qid].argmax(0), row)
    dWc, dWq = Wc.to(gpu), Wq.to(gpu)
    before = [dWc.clone(), dWq.clone()]
    best, index, cosine, slab, R = run(dWc, dWq, n, d, model, chunk)
    best2 = run(dWc, dWq, n, d, model, chunk)[0]
    torch.cuda.synchronize()
    _, arg64 = check_against_fp64(index, cosine, A64, B64, K, label=case_id(case) + " " + dtype)
    assert torch.equal(index.cpu()[qid], row) and torch.equal(arg64[qid], row)
    assert torch.equal(best, best2)  # the same inputs give the same key bits
    # nothing else is written: the operands, and the slab rows past cc_col_part_rows
    assert torch.equal(dWc, before[0]) and torch.equal(dWq, before[1])
    assert bool((slab[R:] == CANARY).all()) and not bool((slab[:R] == CANARY).any())
    # the module's own launch loop gives the same keys
    cs, qs = (decoder_match.inverse_norms(W, n, d, model) for W in (dWc, dWq))
    A, B = slices(dWc, dWq, d, model)
    assert torch.equal(decoder_match.match_keys(A, cs, B, qs, chunk), best)


def negative_problem(M, N, n, d, dtype, zero_rows=()):
    """Queries near one direction u, candidates near -u: every true cosine is < 0.  zero_rows: all-zero candidates,
    whose score 0 would beat them all."""
    g = torch.Generator().manual_seed(11)
    u = torch.randn(n * d, generator=g)
    Wq = u + 0.3 * torch.randn(N, n * d, generator=g)
    Wc = -(u + 0.3 * torch.randn(M, n * d, generator=g))
    Wc[list(zero_rows)] = 0.0
    return Wc.to(dtype), Wq.to(dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("M,chunk", [(200, 4096), (520, 256)], ids=["M200", "M520_chunk256"])
def test_all_negative_queries_with_a_ragged_candidate_tail(gpu, M, chunk, dtype):
    """The zero-filled operand rows past M (56 of the only tile; 248 of the last chunk's tile) score 0 and must not
    win against negative cosines; nor may a zero candidate row."""
    N, n, d, model = 96, 2, 40, 1
    zero_rows = (3, M - 1)
    Wc, Wq = negative_problem(M, N, n, d, DT[dtype], zero_rows)
    A64, B64 = slices(Wc, Wq, d, model)
    cos, ok_c, _ = ref.cosines(A64, B64)
    assert bool((cos[ok_c] < -0.2).all()) and int((~ok_c).sum()) == 2
    _, index, cosine, _, _ = run(Wc.to(gpu), Wq.to(gpu), n, d, model, chunk)
    torch.cuda.synchronize()
    check_against_fp64(index, cosine, A64, B64, d, label=f"negative M{M} {dtype}")
    index, cosine = index.cpu(), cosine.cpu()
    assert bool(((index >= 0) & (index < M)).all()) and bool((cosine < 0).all())
    assert not bool(torch.isin(index, torch.tensor(zero_rows)).any())


# exact duplicates of query k at the two candidate rows: (in different wave row blocks of one tile), (different
# tiles), (different tiles, the ragged last one), (one lane's consecutive row groups), (neighbouring lanes),
# (last tile and first)
DUPLICATES = [(133, 7), (300, 131), (515, 260), (39, 23), (41, 40), (517, 2)]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_ties_go_to_the_smaller_index_whatever_the_chunking(gpu, dtype):
    M, N, n, d, model = 520, 96, 2, 40, 0
    Wc, Wq, _, _ = planted(M, N, n, d, DT[dtype], seed=2)
    for k, rows in enumerate(DUPLICATES):
        Wc[list(rows)] = Wq[k]
    dWc, dWq = Wc.to(gpu), Wq.to(gpu)
    keys = {chunk: run(dWc, dWq, n, d, model, chunk)[0] for chunk in (4096, 256, 136)}
    again = run(dWc, dWq, n, d, model, 4096)[0]
    index, cosine = decoder_match.decode_keys(keys[4096])
    torch.cuda.synchronize()
    # rows 7 / 133 ... hold the same bits: the same score, and the smaller index wins in the lane's walk, the
    # 16-lane max, the slab rows' merge and the chunks' merge
    assert index.cpu()[:len(DUPLICATES)].tolist() == [min(r) for r in DUPLICATES]
    assert bool(((cosine.cpu()[:len(DUPLICATES)] - 1).abs() <= ref.tol(d)).all())
    assert torch.equal(keys[4096], again)
    assert torch.equal(keys[4096], keys[256]) and torch.equal(keys[4096], keys[136])
    A64, B64 = slices(Wc, Wq, d, model)
    check_against_fp64(index, cosine, A64, B64, d, label=f"ties {dtype}")
    # the keys are the reference's keys of the decoded pairs
    got = ref.as_unsigned(keys[4096])
    assert got == [ref.key(c, i) for c, i in zip(cosine.cpu().tolist(), index.cpu().tolist())]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_zero_norms(gpu, dtype):
    M, N, n, d, model = 200, 96, 2, 40, 1
    Wc, Wq, qid, row = planted(M, N, n, d, DT[dtype], seed=3)
    Wc[row[:4]] = 0.0  # the planted best candidates of four queries vanish
    Wq[[5, 90]] = 0.0
    best, index, cosine, _, _ = run(Wc.to(gpu), Wq.to(gpu), n, d, model)
    torch.cuda.synchronize()
    A64, B64 = slices(Wc, Wq, d, model)
    m, _ = check_against_fp64(index, cosine, A64, B64, d, label=f"zero norms {dtype}")
    index, cosine = index.cpu(), cosine.cpu()
    assert not bool(torch.isin(index, row[:4]).any())  # a zero candidate is never chosen
    assert index[[5, 90]].tolist() == [-1, -1] and bool(cosine[[5, 90]].isnan().all())
    assert int((index >= 0).sum()) == N - 2
    # an all-zero candidate set (in the matched model's slice; the other model's stays): no key at all
    Wc2 = Wc.clone()
    Wc2[:, d:] = 0.0
    best, index, cosine, _, _ = run(Wc2.to(gpu), Wq.to(gpu), n, d, model)
    torch.cuda.synchronize()
    assert bool((best == 0).all()) and bool((index == -1).all()) and bool(cosine.isnan().all())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("chunk", [4096, 256])
def test_exclude_diag(gpu, chunk, dtype):
    """One dictionary against itself: no latent matches itself, although its own cosine 1 is the largest."""
    M, n, d, model = 520, 2, 40, 0
    W = torch.randn(M, n * d, generator=torch.Generator().manual_seed(4)).to(DT[dtype])
    W[400] = W[17]  # a duplicated latent: each is the other's best
    dW = W.to(gpu)
    _, index, cosine, _, _ = run(dW, dW, n, d, model, chunk, exclude_diag=True)
    _, with_diag, cos_diag, _, _ = run(dW, dW, n, d, model, chunk)
    torch.cuda.synchronize()
    A64, _ = slices(W, W, d, model)
    check_against_fp64(index, cosine, A64, A64, d, exclude_diag=True, label=f"self {dtype}")
    index, with_diag = index.cpu(), with_diag.cpu()
    assert not bool((index == torch.arange(M)).any())
    assert index[17] == 400 and index[400] == 17
    # without the flag every latent but the duplicate's second copy finds itself (400 ties with 17: the smaller)
    want = torch.arange(M)
    want[400] = 17
    assert torch.equal(with_diag, want) and bool(((cos_diag.cpu() - 1).abs() <= ref.tol(d)).all())


# ----------------------------------------------------------------------------- through the model
def make_cfg(h, d, dtype, dev):
    return {"seed": 49, "batch_size": 64, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 6400, "l1_coeff": 2,
            "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": dtype, "device": str(dev),
            "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_model_permutation(gpu, dtype):
    h, d, n = 204, 36, 2
    cc_a = ca.CrossCoder(make_cfg(h, d, dtype, gpu), n_models=n)
    assert (cc_a._hp, cc_a._dp) == (208, 40)
    perm = torch.randperm(h, generator=torch.Generator().manual_seed(6)).to(gpu)
    cc_b = ca.CrossCoder(make_cfg(h, d, dtype, gpu), n_models=n, init_W_dec=cc_a.W_dec.detach()[perm].clone())
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(h, device=gpu)
    for model, K in ((None, n * d), (1, d)):
        r = ca.match_decoders(cc_a, cc_b, model=model, chunk_rows=128)
        torch.cuda.synchronize()
        assert torch.equal(r["index"], inv) and torch.equal(r["index_rev"], perm)  # B[i] = A[perm[i]]
        for key in ("cosine", "cosine_rev"):
            assert r[key].dtype == torch.float32 and bool(((r[key] - 1).abs() <= ref.tol(K)).all())
        assert r["mutual"].dtype == torch.bool and bool(r["mutual"].all())
        assert all(r[key].shape == (h,) for key in ("index", "cosine", "index_rev", "cosine_rev", "mutual"))
        assert abs(r["mmcs"] - 1) <= ref.tol(K) and abs(r["mmcs_rev"] - 1) <= ref.tol(K)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_model_different_sizes(gpu, dtype):
    h_a, h_b, d, n = 204, 264, 36, 2
    cc_a = ca.CrossCoder(make_cfg(h_a, d, dtype, gpu), n_models=n)
    cc_b = ca.CrossCoder(dict(make_cfg(h_b, d, dtype, gpu), seed=50), n_models=n)
    Wa, Wb = (cc.reference_state_dict()["W_dec"].detach() for cc in (cc_a, cc_b))
    assert Wa.shape == (h_a, n, d) and Wb.shape == (h_b, n, d)
    for model in (None, 0, 1):
        K = n * d if model is None else d
        A64, B64 = (W.flatten(1) if model is None else W[:, model] for W in (Wa, Wb))
        r = ca.match_decoders(cc_a, cc_b, model=model)
        small = ca.match_decoders(cc_a, cc_b, model=model, chunk_rows=72)
        torch.cuda.synchronize()
        assert r["index"].shape == r["cosine"].shape == r["mutual"].shape == (h_a,)
        assert r["index_rev"].shape == r["cosine_rev"].shape == (h_b,)
        check_against_fp64(r["index"], r["cosine"], B64, A64, K, label=f"model {model} {dtype} forward")
        check_against_fp64(r["index_rev"], r["cosine_rev"], A64, B64, K, label=f"model {model} {dtype} reverse")
        assert bool((r["index"] < h_b).all()) and bool((r["index_rev"] < h_a).all())
        j = torch.arange(h_a, device=gpu)
        assert torch.equal(r["mutual"], r["index_rev"][r["index"]] == j)
        assert abs(r["mmcs"] - r["cosine"].double().mean().item()) < 1e-12
        assert abs(r["mmcs_rev"] - r["cosine_rev"].double().mean().item()) < 1e-12
        for key in ("index", "cosine", "index_rev", "cosine_rev", "mutual"):
            assert torch.equal(r[key], small[key]), key


def test_model_self_mode(gpu):
    """cc_b=None: the diagonal is excluded, a duplicated latent pair is mutual, the reverse tensors are the forward
    ones; a zero latent decodes to (-1, NaN) and is no one's match."""
    h, d, n = 204, 36, 2
    W = ca.CrossCoder(make_cfg(h, d, "bf16", gpu), n_models=n).W_dec.detach().clone()
    W[150] = W[9]
    W[77] = 0.0
    cc = ca.CrossCoder(make_cfg(h, d, "bf16", gpu), n_models=n, init_W_dec=W)
    r = ca.match_decoders(cc)
    torch.cuda.synchronize()
    assert r["index_rev"] is r["index"] and r["cosine_rev"] is r["cosine"] and r["index"].shape == (h,)
    assert not bool((r["index"] == torch.arange(h, device=gpu)).any())
    assert r["index"][9] == 150 and r["index"][150] == 9 and bool(r["mutual"][9]) and bool(r["mutual"][150])
    assert r["index"][77] == -1 and bool(r["cosine"][77].isnan()) and not bool(r["mutual"][77])
    assert not bool((r["index"] == 77).any()) and bool((r["index"] < h).all())
    flat = W.flatten(1)
    check_against_fp64(r["index"], r["cosine"], flat, flat, n * d, exclude_diag=True, label="self mode")
    ok = ~r["cosine"].isnan()
    assert int(ok.sum()) == h - 1 and abs(r["mmcs"] - r["cosine"][ok].double().mean().item()) < 1e-12
