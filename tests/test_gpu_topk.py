"""TopK crosscoders on the GPU: the per-row top-k kernel (cc_topk_rows) against the pure-torch reference of
tests/_topk_ref.py, then the model, the losses and gradients, the Trainer and the refusals built on it."""
import os

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops
from oracle import cpu_reference as O
from tests._golden import load
from tests._topk_ref import tie_straddles, topk_order, topk_ref
from tests.test_gpu_parity import envelope_ok, make_cc, rel

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
SHAPES = [(1, 8, 8), (3, 200, 200), (130, 512, 520), (4, 16384, 16384), (2, 131072, 131072)]
PAD = 7.0  # what the columns at or beyond h hold: positive, so a kernel that looked at them would select them


def ks_for(h):
    return sorted({k for k in (1, 2, 31, 32, 33, 64, h - 1, h) if 1 <= k <= h})


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def run_kernel(v, ld, k, inplace=False):
    """v [B, h] (CPU or GPU) in a [B, ld] buffer whose other columns hold PAD -> every output of cc_topk_rows."""
    B, h = v.shape
    dev = torch.device("cuda:0")
    buf = torch.full((B, ld), PAD, dtype=v.dtype, device=dev)
    buf[:, :h] = v.to(dev)
    out = buf if inplace else torch.full((B, ld), PAD, dtype=v.dtype, device=dev)
    idx = torch.full((B, k), -7, dtype=torch.int32, device=dev)
    val = torch.full((B, k), 3.0, dtype=v.dtype, device=dev)
    part = torch.full((ops.topk_part_rows(B, h), h), float("nan"), device=dev)
    l0 = torch.full((ops.topk_l0_parts(B, h),), float("nan"), device=dev)
    ops.topk_rows(buf, h, k, out=out, idx_out=idx, val_out=val, colsum_part=part, l0_part=l0)
    colsum = torch.empty(h, device=dev)
    ops.reduce_rows(part, part.shape[0], h, out_f32=colsum)
    return {"out": out, "idx": idx, "val": val, "part": part, "l0": l0, "colsum": colsum,
            "src": None if inplace else buf}


def check_against_ref(v, ld, k, order, what):
    """Everything the kernel writes for (v, k), out of place and in place, against the reference."""
    B, h = v.shape
    ref = topk_ref(v, k, order)
    got = run_kernel(v, ld, k)
    out = got["out"].cpu()
    assert torch.equal(bits(out[:, :h]), bits(ref["dense"])), (what, k, "dense")
    assert torch.equal(got["idx"].cpu(), ref["idx"]), (what, k, "idx")
    assert torch.equal(bits(got["val"].cpu()), bits(ref["val"])), (what, k, "val")
    assert got["l0"].sum().item() == ref["count"].sum().item(), (what, k, "count")
    assert torch.equal((got["idx"] >= 0).sum(1).cpu(), ref["count"]), (what, k, "row counts")
    # any fixed-order fp32 sum of B terms: |err| <= B 2^-24 sum_b |a|
    # (the bound speaks of sums fp32 can hold: the terms are >= 0, so no partial sum exceeds the column's; a column
    # that holds +inf sums to +inf, and one whose sum overflows fp32 is left alone)
    dense64, colsum = ref["dense"].double(), got["colsum"].double().cpu()
    total = dense64.sum(0)
    fin = total < 3.0e38
    err = (colsum - total).abs()[fin]
    assert bool((err <= B * 2.0 ** -24 * dense64.abs().sum(0)[fin]).all()), (what, k, "colsum", err.max().item())
    assert torch.equal(colsum[torch.isinf(total)], total[torch.isinf(total)]), (what, k, "colsum of +inf")
    if ld > h:
        assert bool((out[:, h:] == PAD).all()), (what, k, "padding columns written")
        assert bool((got["src"][:, h:] == PAD).all().item())
    assert torch.equal(bits(got["src"][:, :h].cpu()), bits(v)), (what, k, "input changed")
    inp = run_kernel(v, ld, k, inplace=True)
    for key in ("out", "idx", "val", "part", "l0"):
        assert torch.equal(bits(inp[key]) if inp[key].dtype in BITS else inp[key],
                           bits(got[key]) if got[key].dtype in BITS else got[key]), (what, k, "in place", key)
    return ref


def oracle_acts():
    """Input (a): the oracle's encode of seeded randn at 2 x 64 -> 512 in bf16 (rounded activations tie)."""
    cfg = {"seed": 49, "dict_size": 512, "d_in": 64, "enc_dtype": "bf16", "dec_init_norm": 0.08}
    P = O.init_params(cfg)
    x = torch.randn(256, 2, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    return O.encode(x, P)


def make_input(kind, B, h, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "equal":  # (b) selects indices 0 .. k-1
        return torch.full((B, h), 1.5, dtype=dtype)
    if kind == "sparse":  # (c) rows with fewer than k eligible values, row 0 all zero
        v = -torch.rand(B, h, generator=g)
        dens = [0.0, 1.0 / h, 0.01, 0.1, 0.5]
        for b in range(B):
            on = torch.rand(h, generator=g) < dens[b % len(dens)]
            v[b] = torch.where(on, torch.rand(h, generator=g) + 0.01, v[b])
        v[0] = 0.0
        if B > 1:
            v[1, h // 2] = 2.0
        return v.to(dtype)
    if kind == "bits":  # (d) uniformly random finite positive bit patterns: every digit, subnormals
        hi = 0x7F80 if dtype == torch.bfloat16 else 0x7F800000
        return torch.randint(1, hi, (B, h), generator=g, dtype=torch.int64).to(BITS[dtype]).view(dtype)
    if kind == "special":  # (e) +inf, NaN, -0.0, negatives, subnormals among ordinary values
        v = torch.randn(B, h, generator=g).to(dtype)
        tiny = torch.tensor([1], dtype=BITS[dtype]).view(dtype)  # the smallest subnormal
        col = torch.arange(h)
        for b in range(B):
            c = (col + b) % 8
            v[b, c == 0] = float("inf")
            v[b, c == 1] = float("nan")
            v[b, c == 2] = -0.0
            v[b, c == 3] = -1.0
            v[b, c == 4] = tiny
            v[b, c == 5] = tiny * 3
        return v
    raise ValueError(kind)


# ----------------------------------------------------------------------------- 1. the kernel against the reference
@pytest.mark.parametrize("kind", ["equal", "sparse", "bits", "special"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", SHAPES)
def test_kernel_matches_reference(gpu, B, h, ld, dtype, kind):
    v = make_input(kind, B, h, DT[dtype], seed=B + h)
    order = topk_order(v)
    for k in ks_for(h):
        ref = check_against_ref(v, ld, k, order, kind)
        if kind == "equal":
            assert torch.equal(ref["idx"], torch.arange(k, dtype=torch.int32).expand(B, k))
        if kind == "sparse":
            assert ref["count"][0].item() == 0 and bool((ref["idx"][0] == -1).all())
            assert k < h or bool((ref["count"] < k).any())
        if kind == "special":
            assert not bool(ref["mask"][~(v > 0)].any())  # NaN, -0.0 and negatives are never selected
            if k == 1:
                assert bool(torch.isinf(ref["val"][:, 0].float()).all())  # +inf first, the smallest index of them


def test_kernel_on_oracle_activations(gpu):
    """(a) rounded bf16 activations: ties that straddle position k are the common case."""
    v = oracle_acts()
    assert v.dtype == torch.bfloat16 and v.shape == (256, 512)
    straddle = tie_straddles(v, 32).float().mean().item()
    assert straddle >= 0.10, straddle  # the test keeps its tie coverage
    order = topk_order(v)
    for k in ks_for(512):
        check_against_ref(v, 512, k, order, "oracle")
    pre = O.encode(torch.randn(256, 2, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16),
                   O.init_params({"seed": 49, "dict_size": 512, "d_in": 64, "enc_dtype": "bf16",
                                  "dec_init_norm": 0.08}), apply_relu=False)
    got = run_kernel(pre, 512, 32)  # apply_relu=False output is legal input: the same selection
    assert torch.equal(bits(got["out"].cpu()), bits(topk_ref(v, 32, order)["dense"]))


# ----------------------------------------------------------------------------- 2. bit-reproducible
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", [(700, 512, 520), (600, 2056, 2056), (300, 16384, 16384), (260, 24576, 24576)])
def test_kernel_bit_reproducible(gpu, B, h, ld, dtype):
    """More rows than workgroups in each of the kernel's four forms: several rows per workgroup."""
    v = make_input("bits", B, h, DT[dtype], seed=5)
    v[:, ::3] = -v[:, ::3]
    check_against_ref(v, ld, 33, topk_order(v), "rows in turn")
    a, b = run_kernel(v, ld, 33), run_kernel(v, ld, 33)
    for key in ("out", "idx", "val"):
        assert torch.equal(bits(a[key]) if a[key].dtype in BITS else a[key],
                           bits(b[key]) if b[key].dtype in BITS else b[key]), key
    for key in ("part", "l0", "colsum"):
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key


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


# ----------------------------------------------------------------------------- 3. dyadic known answer (fp32)
@pytest.mark.parametrize("k", [1, 8, 32, 128])
def test_dyadic_known_answer(gpu, k):
    """Dyadic data (every fp32 sum exact, full of ties): the TopK crosscoder's activations are the reference
    selection of the stored pre-activations, bit for bit, and decode / losses follow from them."""
    r = load("dyadic_b64_n2_d32_h128_fp32")
    P, x, fw = r["init"], r["x"][0], r["fwd"]
    cc = make_cc(dict(r["cfg"], activation="topk", k=k), P, gpu, 2)
    assert cc.activation == "topk" and cc.k == k
    xg = x.to(gpu)
    ref = topk_ref(torch.relu(fw["pre"]), k)
    with torch.no_grad():
        acts = cc.encode(xg).cpu()
        pre = cc.encode(xg, apply_relu=False).cpu()
        recon = cc.decode(acts.to(gpu)).cpu()
        fwd = cc.forward(xg).cpu()
        lo = cc.get_losses(xg)
    assert torch.equal(pre, fw["pre"])  # apply_relu=False: the plain pre-activations
    assert torch.equal(bits(acts), bits(ref["dense"]))
    if k < 128:
        assert bool(tie_straddles(torch.relu(fw["pre"]), k).any())  # the tie rule decides rows here
    want = masked_losses(x, P, torch.float32, acts=ref["dense"])
    assert torch.equal(recon, O.decode(ref["dense"], P)) and torch.equal(fwd, recon)
    assert rel(lo.l2_loss, want["l2_loss"]) < 2e-5
    for key in ("explained_variance", "explained_variance_A", "explained_variance_B"):
        assert rel(getattr(lo, key), want[key]) < 2e-5, key
    assert lo.l0_loss.item() == ref["count"].float().mean().item()
    assert torch.equal(lo.l0_loss.cpu(), want["l0_loss"])


# ----------------------------------------------------------------------------- 4. self-consistency in bf16
def small_cfg(B, d, h, dtype, dev, **kw):
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": B * 100, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": dtype, "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("B,n,d,h", [(256, 2, 64, 512), (96, 2, 40, 200), (64, 2, 32, 203)])
def test_encode_is_the_selection_of_the_relu_encode(gpu, B, n, d, h):
    """G1 is bit-reproducible, so TopK encode(x) is exactly the reference selection of the same crosscoder's
    ReLU-mode encode(x); encode_topk is its compact form.  (203 latents run on 208 kernel latents.)"""
    k = 32
    relu_cc = ca.CrossCoder(small_cfg(B, d, h, "bf16", gpu), n_models=n)
    topk_cc = ca.CrossCoder(small_cfg(B, d, h, "bf16", gpu, activation="topk", k=k), n_models=n)
    for cc in (relu_cc, topk_cc):
        with torch.no_grad():
            cc.b_enc.copy_(torch.linspace(-0.05, 0.05, h, device=gpu))
    x = torch.randn(B, n, d, generator=torch.Generator(device=gpu).manual_seed(B + h), device=gpu)
    with torch.no_grad():
        dense = relu_cc.encode(x)
        got = topk_cc.encode(x)
        vals, idx = topk_cc.encode_topk(x)
        vals_r, idx_r = relu_cc.encode_topk(x, k=k)  # any crosscoder serves it
        relu_cc.ENCODE_ROWS = 40  # (several chunks through the one buffer)
        vals_c, idx_c = relu_cc.encode_topk(x, k=k)
        vals_5, idx_5 = relu_cc.encode_topk(x, k=5)
    assert got.shape == (B, h) and vals.shape == (B, k) and idx.shape == (B, k) and idx.dtype == torch.int32
    ref = topk_ref(dense.cpu(), k)
    assert bool((ref["count"] == k).all())  # about half of the latents are positive
    assert torch.equal(bits(got.cpu()), bits(ref["dense"]))
    for v, i in ((vals, idx), (vals_r, idx_r), (vals_c, idx_c)):
        assert torch.equal(i.cpu(), ref["idx"]) and torch.equal(bits(v.cpu()), bits(ref["val"]))
        assert int(i.max()) < h
    ref5 = topk_ref(dense.cpu(), 5)
    assert torch.equal(idx_5.cpu(), ref5["idx"]) and torch.equal(bits(vals_5.cpu()), bits(ref5["val"]))
    with pytest.raises(ValueError):
        relu_cc.encode_topk(x)  # no cfg["k"] to default to
    with pytest.raises(ValueError):
        relu_cc.encode_topk(x, k=h + 1)


# ----------------------------------------------------------------------------- 5. losses and gradients, the GPU's mask
@pytest.mark.parametrize("name", ["step_b256_n2_d64_h512_bf16", "step_b96_n2_d40_h200_bf16",
                                  "step_b256_n2_d64_h512_fp32", "step_b96_n2_d40_h200_fp32"])
def test_losses_and_gradients_with_the_gpu_mask(gpu, name):
    """With M = encode(x) > 0 imposed on the oracle (acts = relu(pre) * M), only arithmetic differs, so the
    project's bounds carry over: bf16 error against fp64 <= 2 x the CPU-bf16 error + 2e-3 (forward) / 5e-3
    (gradients), fp32 rel < 2e-5.  l1's weight 2.0: the masked column sums reach the L1 loss and dW_dec."""
    r = load(name)
    cfg, P, x, n = r["cfg"], r["init"], r["x"][0], r["n_models"]
    dt = O.DTYPES[cfg["enc_dtype"]]
    k = 32
    cc = make_cc(dict(cfg, activation="topk", k=k), P, gpu, n)
    xg = x.to(gpu)
    with torch.no_grad():
        M = (cc.encode(xg.to(dt)) > 0).cpu()
    assert bool((M.sum(1) <= k).all()) and M.sum().item() > 0.9 * k * x.shape[0]
    lo = cc.get_losses(xg)
    assert cc._ws.topk == k and not cc._ws.tr
    (lo.l2_loss + 2.0 * lo.l1_loss).backward()
    torch.cuda.synchronize()

    def oracle(dtype):
        leaves = {key: v.detach().to(dtype).clone().requires_grad_(True) for key, v in P.items()}
        out = masked_losses(x.to(dt).to(dtype), leaves, dtype, M=M)
        (out["l2_loss"] + 2.0 * out["l1_loss"]).backward()
        return out, {key: leaves[key].grad for key in O.PARAM_ORDER}

    ref, gref = oracle(dt)
    truth, gtruth = oracle(torch.float64)
    assert lo.l0_loss.item() == M.sum(1).float().mean().item()
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
def test_k_equal_dict_size_is_the_relu_step(gpu, monkeypatch):
    """k = dict_size selects every positive activation, so with l1_coeff = 0 a TopK trainer and a ReLU trainer in
    the same (batch-major) step form walk the same parameters bit for bit.  l1_loss is compared as the fp32 scalar
    the step writes (its column sums are formed in another order: 1e-6 relative) and as the logged value, which is
    that scalar rounded to the parameter dtype.  bf16: a snapshot of W_dec taken right after an fp32 step is not
    reliably ordered after its side-stream Adam, with or without TopK (seen here as a
    whole stale W_dec after step 0), so parameters of fp32 trainers cannot be compared step by step."""
    from crosscoder_amd import engine
    dtype = "bf16"
    B, n, d, h, steps = 256, 2, 64, 512, 3

    def run(**kw):
        cfg = small_cfg(B, d, h, dtype, gpu, l1_coeff=0.0, **kw)
        cc = ca.CrossCoder(cfg, n_models=n)
        tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * steps, n_models=n, seed=3), crosscoder=cc)
        out = []
        for _ in range(steps):
            dct = tr.step()
            raw_l1 = float(tr._mapped.f32[1])
            tr.synchronize()
            assert not cc._ws.tr
            out.append((dct, raw_l1, [getattr(cc, p).detach().clone() for p in O.PARAM_ORDER]))
        return out

    topk = run(activation="topk", k=h)
    monkeypatch.setattr(engine, "transposed_wgrad", lambda *a: False)  # the ReLU step in its batch-major form
    relu = run()
    for step, ((d0, l0, p0), (d1, l1, p1)) in enumerate(zip(relu, topk)):
        for name, a, b in zip(O.PARAM_ORDER, p0, p1):
            assert torch.equal(a, b), (step, name, int((a != b).sum()), (a.float() - b.float()).abs().max().item())
        assert d0["l2_loss"] == d1["l2_loss"] and d0["l0_loss"] == d1["l0_loss"]
        assert 0 < d0["l0_loss"] < h
        assert abs(l0 - l1) <= 1e-6 * abs(l0), (l0, l1)
        assert abs(d0["l1_loss"] - d1["l1_loss"]) <= 1e-6 * abs(d0["l1_loss"]), (d0["l1_loss"], d1["l1_loss"])


# ----------------------------------------------------------------------------- 7. the Trainer
def test_trainer_topk(gpu, tmp_path, monkeypatch):
    B, n, d, h, k, steps = 256, 2, 64, 512, 32, 5
    cfg = small_cfg(B, d, h, "bf16", gpu, l1_coeff=0.0, activation="topk", k=k)
    cc = ca.CrossCoder(cfg, n_models=n)
    st = ca.LatentStats(cc, k=4)
    tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * steps, n_models=n, seed=3), crosscoder=cc,
                    latent_stats=st)
    before = cc.W_enc.detach().clone()
    for _ in range(steps):
        dct = tr.step()
        assert 0 < dct["l0_loss"] <= k, dct
        assert dct["l2_loss"] > 0 and dct["loss"] == dct["l2_loss"]
    tr.synchronize()
    assert not torch.equal(before, cc.W_enc.detach())
    assert st.rows_seen == B * steps
    fired = int(st.result()["count"].sum())
    assert 0 < fired <= k * st.rows_seen  # the hook saw the masked activations
    monkeypatch.chdir(tmp_path)
    tr.save()
    loaded = ca.CrossCoder.load("version_0", 0)
    assert loaded.activation == "topk" and loaded.k == k and loaded.cfg["k"] == k
    x = torch.randn(B, n, d, generator=torch.Generator(device=gpu).manual_seed(8), device=gpu)
    with torch.no_grad():
        a, b = cc.encode(x), loaded.encode(x)
    assert torch.equal(bits(a), bits(b)) and int((a > 0).sum(1).max()) <= k
    st2 = ca.LatentStats(loaded, k=4)  # LatentStats.update encodes as the crosscoder does
    st2.update(x)
    assert torch.equal(st2.result()["count"], (a > 0).sum(0))
    # a checkpoint without the keys (the reference's) loads as ReLU
    plain = ca.CrossCoder.load_from_path(os.path.join(os.path.dirname(__file__), "golden", "ckpt", "version_0",
                                                      "0_cfg.json"),
                                         os.path.join(os.path.dirname(__file__), "golden", "ckpt", "version_0", "0.pt"),
                                         device=gpu)
    assert plain.activation == "relu" and plain.k is None


# ----------------------------------------------------------------------------- 8. the sharded trainer refuses
def test_sharded_trainer_refuses_topk(gpu):
    from crosscoder_amd import sharded
    cfg = small_cfg(64, 32, 256, "bf16", gpu, activation="topk", k=8)
    with pytest.raises(ValueError, match="topk"):
        sharded.ShardedTrainer(cfg, buffer=None)
    plain = {key: v for key, v in cfg.items() if key not in ("activation", "k")}
    with pytest.raises(ValueError, match="topk"):  # (a TopK crosscoder handed in)
        sharded.ShardedTrainer(plain, buffer=None, crosscoder=ca.CrossCoder(cfg))
