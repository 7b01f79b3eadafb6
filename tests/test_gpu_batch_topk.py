"""BatchTopK crosscoders on the GPU: the batch selection kernels (cc_batch_topk, cc_threshold_mask) against the
pure-torch reference of tests/_batch_topk_ref.py, then the model, the losses and gradients, the Trainer and the
refusal built on them."""
import os

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops
from oracle import cpu_reference as O
from tests._batch_topk_ref import batch_topk_order, batch_topk_ref, threshold_ref
from tests._golden import load
from tests.test_gpu_parity import envelope_ok, make_cc, rel
from tests.test_gpu_topk import make_input, small_cfg

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
# the issue's shapes, then one on each side of the kernel's own boundaries: h = 8192 (below: whole rows per
# 1024-lane segment; from there: 8192-column segments of one row; 16392: a last segment of 8 columns) and 256
# segments (beyond: several segments per workgroup -- 260 rows of one segment each)
SHAPES = [(1, 8, 8), (3, 8, 16), (3, 200, 200), (700, 512, 520), (300, 2056, 2056), (64, 16384, 16384),
          (33, 24576, 24576), (5, 8184, 8184), (5, 8192, 8200), (3, 16392, 16400), (260, 4104, 4104)]
PAD = 7.0  # what the columns at or beyond h hold: positive, so a kernel that looked at them would select them


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def make_weight(wkind, h, seed):
    """None; random in [0.5, 2); or powers of two (cross-value ties: 2 * 1 == 1 * 2) with a few zeros, one negative
    and one NaN.  Column h // 2 (where make_case plants a tie) keeps a positive finite weight."""
    g = torch.Generator().manual_seed(seed)
    if wkind == "none":
        return None
    if wkind == "rand":
        return torch.rand(h, generator=g) * 1.5 + 0.5
    w = 2.0 ** torch.randint(-2, 3, (h,), generator=g).float()
    for i, bad in ((0, 0.0), (5, -1.0), (6, float("nan")), (h - 1, 0.0)):
        if i != h // 2:
            w[i] = bad
    return w


def make_case(kind, B, h, dtype, wkind, seed):
    """(v [B, h], weight or None): make_input's kinds, a tie planted across rows (B >= 3: rows 1 and B - 1 of column
    h // 2; "equal" is all ties as it is), and -- weighted -- no finite non-zero product subnormal, so that a
    flush-to-zero difference between host and device stays out of the comparison."""
    v = make_input(kind, B, h, dtype, seed)
    w = make_weight(wkind, h, seed + 1)
    if w is not None:
        x = v.float()
        v[(x.abs() < 1e-30) & (x != 0)] = 0.75
    if B >= 3 and kind != "equal":  # ("equal": every element ties already)
        v[1, h // 2] = 2.0
        v[B - 1, h // 2] = 2.0
    if w is not None:
        p = v.float() * w[None, :]
        fin = torch.isfinite(p) & (p != 0)
        assert bool((p[fin].abs() >= 2.0 ** -126).all())
    return v, w


def run_kernel(v, w, ld, n_keep, inplace=False, theta=None):
    """v [B, h] in a [B, ld] buffer whose other columns hold PAD -> every output of cc_batch_topk (theta given:
    of cc_threshold_mask)."""
    B, h = v.shape
    dev = torch.device("cuda:0")
    buf = torch.full((B, ld), PAD, dtype=v.dtype, device=dev)
    buf[:, :h] = v.to(dev)
    wd = None if w is None else w.to(dev)
    out = buf if inplace else torch.full((B, ld), PAD, dtype=v.dtype, device=dev)
    part = torch.full((ops.batch_topk_part_rows(B, h), h), float("nan"), device=dev)
    l0 = torch.full((ops.batch_topk_l0_parts(B, h),), float("nan"), device=dev)
    rc = torch.full((B,), -3, dtype=torch.int32, device=dev)
    info = torch.full((4,), -5, dtype=torch.int32, device=dev)
    if theta is None:
        # (a workspace full of ones: the call zeroes what it needs)
        ws = torch.full((ops.batch_topk_ws_bytes(B, h, v.dtype, w is not None),), 255, dtype=torch.uint8, device=dev)
        ops.batch_topk(buf, h, n_keep, weight=wd, out=out, colsum_part=part, l0_part=l0, row_count=rc, info=info,
                       ws=ws)
    else:
        ops.threshold_mask(buf, h, theta.to(dev).reshape(1), weight=wd, out=out, colsum_part=part, l0_part=l0,
                           row_count=rc)
    colsum = torch.empty(h, device=dev)
    ops.reduce_rows(part, part.shape[0], h, out_f32=colsum)
    return {"out": out, "part": part, "l0": l0, "rc": rc, "info": info, "colsum": colsum,
            "src": None if inplace else buf}


def check_masked(got, v, ld, ref, what):
    """The dense output, the counts, the column sums and the untouched columns against a reference selection."""
    B, h = v.shape
    out = got["out"].cpu()
    assert torch.equal(bits(out[:, :h]), bits(ref["dense"])), (what, "dense")
    assert torch.equal(got["rc"].cpu().long(), ref["row_count"]), (what, "row_count")
    assert got["l0"].sum().item() == ref["row_count"].sum().item(), (what, "l0")
    # any fixed-order fp32 sum of B terms: |err| <= B 2^-24 sum_b |a| (columns that hold +inf sum to +inf, and one
    # whose sum overflows fp32 is left alone)
    dense64, colsum = ref["dense"].double(), got["colsum"].double().cpu()
    total = dense64.sum(0)
    fin = total < 3.0e38
    err = (colsum - total).abs()[fin]
    assert bool((err <= B * 2.0 ** -24 * dense64.abs().sum(0)[fin]).all()), (what, "colsum", err.max().item())
    assert torch.equal(colsum[torch.isinf(total)], total[torch.isinf(total)]), (what, "colsum of +inf")
    if ld > h:
        assert bool((out[:, h:] == PAD).all()), (what, "padding columns written")
    if got["src"] is not None:
        assert torch.equal(bits(got["src"].cpu()[:, :h]), bits(v)), (what, "input changed")
        assert bool((got["src"][:, h:] == PAD).all().item())


def same_bits(a, b, keys, what):
    for key in keys:
        x, y = a[key], b[key]
        assert torch.equal(bits(x) if x.dtype in BITS else x, bits(y) if y.dtype in BITS else y), (what, key)


def check_against_ref(v, w, ld, n_keep, order, what):
    ref = batch_topk_ref(v, n_keep, w, order)
    got = run_kernel(v, w, ld, n_keep)
    what = (what, n_keep)
    check_masked(got, v, ld, ref, what)
    info = got["info"].cpu()
    assert info[0].item() == ref["T"].view(torch.int32).item(), (what, "T", info.tolist(), ref["T"].item())
    assert info[1:].tolist() == [ref["selected"], ref["ties"], ref["eligible"]], (what, info.tolist())
    inp = run_kernel(v, w, ld, n_keep, inplace=True)
    same_bits(inp, got, ("out", "part", "l0", "rc", "info"), (what, "in place"))
    return ref


def n_keeps(B, h, order):
    """1, B, 32 B, a value strictly inside a run of equal scores (None when the input has no such run), #eligible,
    #eligible + 1 and B h."""
    keys = order[0]
    eligible = int((keys > 0).sum())
    run = ((keys[1:] == keys[:-1]) & (keys[1:] > 0)).nonzero().flatten()
    inside = int(run[len(run) // 2]) + 1 if len(run) else None  # keeps keys[inside - 1], leaves its equal keys[inside]
    ks = {1, B, B * h, max(1, eligible), eligible + 1}
    if 32 * B <= B * h:
        ks.add(32 * B)
    return sorted(ks), inside


# ----------------------------------------------------------------------------- 1. the kernel against the reference
@pytest.mark.parametrize("wkind", ["none", "rand", "pow2"])
@pytest.mark.parametrize("kind", ["equal", "sparse", "bits", "special"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", SHAPES)
def test_kernel_matches_reference(gpu, B, h, ld, dtype, kind, wkind):
    v, w = make_case(kind, B, h, DT[dtype], wkind, seed=B + h)
    order = batch_topk_order(v, w)
    ks, inside = n_keeps(B, h, order)
    assert inside is not None or B < 3, "a tie is planted whenever B >= 3"
    for n_keep in ks:
        ref = check_against_ref(v, w, ld, n_keep, order, (kind, wkind))
        if kind == "sparse":
            assert ref["row_count"][0].item() == 0
            assert n_keep < B * h or ref["selected"] < n_keep  # fewer eligible than n_keep
        if kind == "special":
            assert not bool(ref["mask"][~(v > 0)].any())  # NaN, -0.0 and negatives are never selected
        if w is not None:
            assert not bool(ref["mask"][:, ~(w > 0)].any())  # nor anything under a zero, negative or NaN weight
    if inside is not None:
        ref = check_against_ref(v, w, ld, inside, order, (kind, wkind, "inside a tie run"))
        assert 0 < ref["ties"] < ref["ties_total"]  # the cut falls strictly inside the run: the flat order decides
    if kind == "equal" and wkind == "none" and B * h > 8:
        ref = batch_topk_ref(v, B * h // 2 + 3, w, order)  # every element ties: exactly the first n_keep flat indices
        assert torch.equal(ref["mask"].flatten().nonzero().flatten(), torch.arange(B * h // 2 + 3))
        check_against_ref(v, w, ld, B * h // 2 + 3, order, "equal, the cut inside a row")


# ----------------------------------------------------------------------------- 2. the threshold mask
@pytest.mark.parametrize("wkind", ["none", "rand", "pow2"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", [(3, 200, 200), (700, 512, 520), (64, 16384, 16384), (5, 8184, 8184)])
def test_threshold_mask(gpu, B, h, ld, dtype, wkind):
    v, w = make_case("special" if B < 64 else "bits", B, h, DT[dtype], wkind, seed=B + h + 2)
    order = batch_topk_order(v, w)
    eligible = int((order[0] > 0).sum())
    for n_keep in (B, 8 * B, eligible):
        sel = batch_topk_ref(v, n_keep, w, order)
        ref = threshold_ref(v, sel["T"], w)
        got = run_kernel(v, w, ld, 0, theta=sel["T"])
        check_masked(got, v, ld, ref, ("theta", wkind, n_keep))
        inp = run_kernel(v, w, ld, 0, inplace=True, theta=sel["T"])
        same_bits(inp, got, ("out", "part", "l0", "rc"), ("theta in place", n_keep))
        if sel["ties"] == sel["ties_total"]:  # every tie at T admitted: the threshold form is the batch selection
            assert torch.equal(ref["mask"], sel["mask"])
            same_bits(run_kernel(v, w, ld, n_keep), got, ("out", "rc", "l0", "colsum"), ("theta == batch", n_keep))
    assert sel["ties"] == sel["ties_total"]  # (n_keep = #eligible admits everything at the smallest score)
    for theta in (float("nan"), 0.0, -1.0, float("inf")):
        t = torch.tensor(theta)
        check_masked(run_kernel(v, w, ld, 0, theta=t), v, ld, threshold_ref(v, t, w), ("theta", theta))


# ----------------------------------------------------------------------------- 3. bit-reproducible
@pytest.mark.parametrize("wkind", ["none", "rand"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", [(700, 512, 520), (300, 2056, 2056), (64, 16384, 16384)])
def test_kernel_bit_reproducible(gpu, B, h, ld, dtype, wkind):
    v, w = make_case("bits", B, h, DT[dtype], wkind, seed=5)
    v[:, ::3] = -v[:, ::3]
    for n_keep in (33 * B, B * h):
        a, b = run_kernel(v, w, ld, n_keep), run_kernel(v, w, ld, n_keep)
        same_bits(a, b, ("out", "rc", "info"), n_keep)
        for key in ("part", "l0", "colsum"):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (n_keep, key)
    theta = batch_topk_ref(v, 33 * B, w)["T"]
    a, b = run_kernel(v, w, ld, 0, theta=theta), run_kernel(v, w, ld, 0, theta=theta)
    same_bits(a, b, ("out", "rc"), "theta")
    for key in ("part", "l0", "colsum"):
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), ("theta", key)


# ----------------------------------------------------------------------------- the model
def masked_losses(x, P, dtype, M=None, acts=None):
    """oracle.get_losses (crosscoder.py:96-130) restated with the activations relu(pre) * M (M: a 0/1 mask), or
    with `acts` given."""
    x = x.to(dtype)
    if acts is None:
        acts = O.encode(x, P) * M.to(dtype)
    recon = O.decode(acts, P)
    diff = recon.float() - x.float()
    l2_per_batch = diff.pow(2).sum(dim=(1, 2))
    total_variance = (x - x.mean(0)).pow(2).sum(dim=(1, 2))
    ev = 1 - l2_per_batch / (total_variance + 1e-8)
    ev_m = []
    for m in (0, 1):
        per_tok = (recon[:, m, :] - x[:, m, :]).pow(2).sum(dim=-1).squeeze()
        tv = (x[:, m, :] - x[:, m, :].mean(0)).pow(2).sum(-1).squeeze()
        ev_m.append(1 - per_tok / (tv + 1e-8))
    total_decoder_norm = P["W_dec"].norm(dim=-1).sum(dim=1)
    return {"l2_loss": l2_per_batch.mean(), "l1_loss": (acts * total_decoder_norm[None, :]).sum(-1).mean(0),
            "l0_loss": (acts > 0).float().sum(-1).mean(), "explained_variance": ev,
            "explained_variance_A": ev_m[0], "explained_variance_B": ev_m[1], "recon": recon}


# ----------------------------------------------------------------------------- 4. the model's selection
@pytest.mark.parametrize("weight", ["decoder_norm", "none"])
@pytest.mark.parametrize("k", [1, 8, 32])
def test_dyadic_known_answer(gpu, k, weight):
    """Dyadic data (every fp32 sum exact, full of ties): encode is the reference selection of the stored
    pre-activations under cc.selection_weights(), bit for bit, and decode / losses follow from it."""
    r = load("dyadic_b64_n2_d32_h128_fp32")
    P, x, fw = r["init"], r["x"][0], r["fwd"]
    cc = make_cc(dict(r["cfg"], activation="batch_topk", k=k, topk_weight=weight), P, gpu, 2)
    assert cc.activation == "batch_topk" and cc.k == k and cc.threshold.item() == -1.0
    xg = x.to(gpu)
    B = x.shape[0]
    w = cc.selection_weights()
    assert w.dtype == torch.float32 and w.shape == (128,)
    if weight == "none":
        assert bool((w == 1).all())
    else:
        assert rel(w, P["W_dec"].norm(dim=-1).sum(dim=1)) < 1e-6
    ref = batch_topk_ref(torch.relu(fw["pre"]), B * k, w.cpu())
    assert ref["eligible"] >= B * k and ref["selected"] == B * k
    with torch.no_grad():
        acts = cc.encode(xg, use_threshold=False).cpu()
        same = cc.encode(xg).cpu()  # (the threshold is unset: the batch selection)
        pre = cc.encode(xg, apply_relu=False).cpu()
        recon = cc.decode(acts.to(gpu)).cpu()
        with pytest.raises(ValueError):
            cc.encode(xg, use_threshold=True)
        lo = cc.get_losses(xg)
    assert torch.equal(pre, fw["pre"])  # apply_relu=False: the plain pre-activations
    assert torch.equal(bits(acts), bits(ref["dense"])) and torch.equal(bits(same), bits(acts))
    info = cc.batch_topk_info()  # get_losses selects with the same weights here (W_dec was never stepped)
    assert info["selected"] == B * k and info["eligible"] == ref["eligible"] and info["ties"] == ref["ties"]
    assert info["threshold"] == ref["T"].item()
    assert torch.equal(info["row_count"].cpu().long(), ref["row_count"])
    want = masked_losses(x, P, torch.float32, acts=ref["dense"])
    assert torch.equal(recon, O.decode(ref["dense"], P))
    assert rel(lo.l2_loss, want["l2_loss"]) < 2e-5
    assert rel(lo.l1_loss, want["l1_loss"]) < 2e-5
    for key in ("explained_variance", "explained_variance_A", "explained_variance_B"):
        assert rel(getattr(lo, key), want[key]) < 2e-5, key
    assert lo.l0_loss.item() == k


@pytest.mark.parametrize("weight", ["decoder_norm", "none"])
@pytest.mark.parametrize("B,n,d,h", [(256, 2, 64, 512), (96, 2, 40, 200), (64, 2, 32, 203)])
def test_encode_is_the_selection_of_the_relu_encode(gpu, B, n, d, h, weight):
    """G1 is bit-reproducible, so BatchTopK encode(x) is exactly the reference selection of the same crosscoder's
    ReLU-mode encode(x).  (203 latents run on 208 kernel latents.)"""
    k = 32
    relu_cc = ca.CrossCoder(small_cfg(B, d, h, "bf16", gpu), n_models=n)
    cc = ca.CrossCoder(small_cfg(B, d, h, "bf16", gpu, activation="batch_topk", k=k, topk_weight=weight), n_models=n)
    for c in (relu_cc, cc):
        with torch.no_grad():
            c.b_enc.copy_(torch.linspace(-0.05, 0.05, h, device=gpu))
    x = torch.randn(B, n, d, generator=torch.Generator(device=gpu).manual_seed(B + h), device=gpu)
    with torch.no_grad():
        dense = relu_cc.encode(x)
        got = cc.encode(x)
    ref = batch_topk_ref(dense.cpu(), B * k, cc.selection_weights().cpu())
    assert ref["eligible"] >= B * k  # about half of the latents are positive at the seed-49 init
    assert got.shape == (B, h) and torch.equal(bits(got.cpu()), bits(ref["dense"]))
    assert int((got > 0).sum()) == B * k


# ----------------------------------------------------------------------------- 5. losses and gradients, the GPU's mask
@pytest.mark.parametrize("name", ["step_b256_n2_d64_h512_bf16", "step_b96_n2_d40_h200_bf16",
                                  "step_b256_n2_d64_h512_fp32", "step_b96_n2_d40_h200_fp32"])
def test_losses_and_gradients_with_the_gpu_mask(gpu, name):
    """With the selection M of the GPU's own forward imposed on the oracle (acts = relu(pre) * M), only arithmetic
    differs, so the project's bounds carry over: bf16 error against fp64 <= 2 x the CPU-bf16 error + 2e-3 (forward) /
    5e-3 (gradients), fp32 rel < 2e-5.  The selection is a constant of the gradient (straight-through).  l1's
    weight 2.0: the masked column sums reach the L1 loss and dW_dec."""
    r = load(name)
    cfg, P, x, n = r["cfg"], r["init"], r["x"][0], r["n_models"]
    dt = O.DTYPES[cfg["enc_dtype"]]
    k = 32
    B = x.shape[0]
    cc = make_cc(dict(cfg, activation="batch_topk", k=k), P, gpu, n)
    xg = x.to(gpu)
    lo = cc.get_losses(xg)
    ws = cc._ws
    assert ws.batch_topk == k and ws.bt_weighted and ws.topk is None and not ws.tr
    M = (ws.acts[:, :cfg["dict_size"]] > 0).cpu()  # the step's own mask
    info = cc.batch_topk_info()
    assert M.sum().item() == info["selected"] == B * k and info["eligible"] >= B * k
    assert torch.equal(M.sum(1), info["row_count"].cpu().long())
    (lo.l2_loss + 2.0 * lo.l1_loss).backward()
    torch.cuda.synchronize()

    def oracle(dtype):
        leaves = {key: v.detach().to(dtype).clone().requires_grad_(True) for key, v in P.items()}
        out = masked_losses(x.to(dt).to(dtype), leaves, dtype, M=M)
        (out["l2_loss"] + 2.0 * out["l1_loss"]).backward()
        return out, {key: leaves[key].grad for key in O.PARAM_ORDER}

    ref, gref = oracle(dt)
    truth, gtruth = oracle(torch.float64)
    assert lo.l0_loss.item() == k
    fields = ("l2_loss", "l1_loss", "explained_variance", "explained_variance_A", "explained_variance_B")
    for key in fields:
        ours = getattr(lo, key).detach().float()
        if dt == torch.float32:
            e = rel(ours, truth[key].detach())
            print(name, key, "rel", e)
            assert e < 2e-5, (key, e)
        else:
            ok, e = envelope_ok(ours, ref[key].detach().float(), truth[key].detach())
            print(name, key, "(ours, cpu) vs fp64", e)
            assert ok, (key, e)
    for key in O.PARAM_ORDER:
        g = getattr(cc, key).grad
        assert g.shape == gref[key].shape and g.dtype == gref[key].dtype, key
        if dt == torch.float32:
            e = rel(g, gtruth[key])
            print(name, key, "grad rel", e)
            assert e < 2e-5, (key, e)
        else:
            ok, e = envelope_ok(g, gref[key], gtruth[key], floor=5e-3)
            print(name, key, "grad (ours, cpu) vs fp64", e)
            assert ok, (key, e)


# ----------------------------------------------------------------------------- 6. identity: k = dict_size
@pytest.mark.parametrize("weight", ["decoder_norm", "none"])
def test_k_equal_dict_size_is_the_relu_step(gpu, monkeypatch, weight):
    """k = dict_size selects every positive activation, so with l1_coeff = 0 a BatchTopK trainer and a ReLU trainer
    in the same (batch-major) step form walk the same parameters bit for bit (bf16: see the TopK test of the same
    name)."""
    from crosscoder_amd import engine
    B, n, d, h, steps = 256, 2, 64, 512, 3

    def run(**kw):
        cfg = small_cfg(B, d, h, "bf16", gpu, l1_coeff=0.0, **kw)
        cc = ca.CrossCoder(cfg, n_models=n)
        tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * steps, n_models=n, seed=3), crosscoder=cc)
        out = []
        for _ in range(steps):
            dct = tr.step()
            raw_l1 = float(tr._mapped.f32[1])
            tr.synchronize()
            # the snapshot is taken after a device synchronise: what is compared is the parameters the steps walk, not
            # how a reader on torch's stream is ordered after the side-stream Adam
            torch.cuda.synchronize()
            assert not cc._ws.tr
            out.append((dct, raw_l1, [getattr(cc, p).detach().clone() for p in O.PARAM_ORDER]))
        return out

    batch = run(activation="batch_topk", k=h, topk_weight=weight)
    monkeypatch.setattr(engine, "transposed_wgrad", lambda *a: False)  # the ReLU step in its batch-major form
    relu = run()
    for step, ((d0, l0, p0), (d1, l1, p1)) in enumerate(zip(relu, batch)):
        for name, a, b in zip(O.PARAM_ORDER, p0, p1):
            assert torch.equal(a, b), (step, name, int((a != b).sum()), (a.float() - b.float()).abs().max().item())
        assert d0["l2_loss"] == d1["l2_loss"] and d0["l0_loss"] == d1["l0_loss"]
        assert 0 < d0["l0_loss"] < h
        assert abs(l0 - l1) <= 1e-6 * abs(l0), (l0, l1)
        assert abs(d0["l1_loss"] - d1["l1_loss"]) <= 1e-6 * abs(d0["l1_loss"]), (d0["l1_loss"], d1["l1_loss"])


# ----------------------------------------------------------------------------- 7. the Trainer
def test_trainer_batch_topk(gpu, tmp_path, monkeypatch):
    B, n, d, h, k, steps, beta = 256, 2, 64, 512, 32, 5, 0.9
    cfg = small_cfg(B, d, h, "bf16", gpu, l1_coeff=0.0, activation="batch_topk", k=k, threshold_beta=beta)
    cc = ca.CrossCoder(cfg, n_models=n)
    st = ca.LatentStats(cc, k=4)
    tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * steps, n_models=n, seed=3), crosscoder=cc,
                    latent_stats=st)
    before = cc.W_enc.detach().clone()
    assert cc.threshold.item() == -1.0
    want = None
    for step in range(steps):
        dct = tr.step()
        assert len(dct) == 9 and dct["l0_loss"] == k, dct  # exactly B k pairs: the mean selected count is k
        assert dct["l2_loss"] > 0 and dct["loss"] == dct["l2_loss"]
        info = cc.batch_topk_info()
        assert info["eligible"] >= B * k and info["selected"] == B * k
        rc = info["row_count"]
        assert int(rc.sum()) == B * k and int(rc.min()) < k < int(rc.max())  # the counts vary across rows
        T = info["threshold"]
        assert T > 0
        want = T if want is None else beta * want + (1 - beta) * T  # the recurrence, on the host
        got = cc.threshold.item()
        assert abs(got - want) <= 1e-6 * want, (step, got, want)
        if step == 0:
            assert got == T
        want = got
    tr.synchronize()
    assert not torch.equal(before, cc.W_enc.detach())
    assert st.rows_seen == B * steps and int(st.result()["count"].sum()) == k * st.rows_seen  # the masked activations
    monkeypatch.chdir(tmp_path)
    tr.save()
    loaded = ca.CrossCoder.load("version_0", 0)
    assert loaded.activation == "batch_topk" and loaded.k == k and loaded.cfg["k"] == k
    assert loaded.topk_weight == "decoder_norm" and loaded.threshold_beta == beta
    assert loaded.threshold.item() == cc.threshold.item() > 0
    x = torch.randn(B, n, d, generator=torch.Generator(device=gpu).manual_seed(8), device=gpu)
    with torch.no_grad():
        a, b = cc.encode(x), loaded.encode(x)
        thr = loaded.encode(x, use_threshold=True)
        sel = loaded.encode(x, use_threshold=False)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(thr), bits(b))
    w = loaded.selection_weights()
    score = torch.where(a > 0, a.float() * w[None, :], torch.zeros((), device=gpu))
    assert bool((score[a > 0] >= loaded.threshold).all())  # encode(x) used the threshold
    dense = torch.relu(loaded.encode(x, apply_relu=False))
    assert torch.equal(a > 0, (dense > 0) & (dense.float() * w[None, :] >= loaded.threshold))
    assert int((sel > 0).sum()) == B * k  # the batch selection keeps exactly rows * k
    st2 = ca.LatentStats(loaded, k=4)  # LatentStats.update masks as encode does
    st2.update(x)
    assert torch.equal(st2.result()["count"], (a > 0).sum(0))
    # a checkpoint without the keys (the reference's) loads as ReLU, without the buffer
    ckpt = os.path.join(os.path.dirname(__file__), "golden", "ckpt", "version_0")
    plain = ca.CrossCoder.load_from_path(os.path.join(ckpt, "0_cfg.json"), os.path.join(ckpt, "0.pt"), device=gpu)
    assert plain.activation == "relu" and plain.k is None and not hasattr(plain, "threshold")
    assert list(plain.state_dict().keys()) == ["W_enc", "W_dec", "b_enc", "b_dec"]


# ----------------------------------------------------------------------------- 8. the sharded trainer refuses
def test_sharded_trainer_refuses_batch_topk(gpu):
    from crosscoder_amd import sharded
    cfg = small_cfg(64, 32, 256, "bf16", gpu, activation="batch_topk", k=8)
    with pytest.raises(ValueError, match="batch_topk"):
        sharded.ShardedTrainer(cfg, buffer=None)
    plain = {key: v for key, v in cfg.items() if key not in ("activation", "k")}
    with pytest.raises(ValueError, match="batch_topk"):  # (a BatchTopK crosscoder handed in)
        sharded.ShardedTrainer(plain, buffer=None, crosscoder=ca.CrossCoder(cfg))
