"""LatentStats on the GPU: the update kernel (cc_latent_stats_update) against a plain torch reference on the
concatenated activations, through the model (LatentStats.update), at config 2's full size, and as the
Trainer's opt-in hook."""
import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def reference(acts, ids, k):
    """acts [N, h] (every batch concatenated), ids [N] -> count, fp64 sum, hist, topk values / rows."""
    a = acts.float()
    a = torch.where(a > 0, a, torch.zeros_like(a))  # (NaN > 0 is false)
    pos = a > 0
    N, h = a.shape
    count = pos.sum(0)
    s = a.double().sum(0)
    _, e = torch.frexp(a)  # a = m * 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    bins = (e.long() - 1 + 16).clamp(0, 31)
    hist = torch.zeros(h, 32, dtype=torch.int64, device=a.device)
    hist.scatter_add_(1, bins.t().contiguous(), pos.t().long().contiguous())
    order = torch.argsort(ids, stable=True)  # rows in ascending id order, then a stable descending sort
    a2, ids2 = a[order], ids[order]
    vals, idx = torch.sort(a2, dim=0, descending=True, stable=True)
    vals, rows = vals[:k], ids2[idx[:k]]
    if N < k:
        vals = torch.cat([vals, torch.zeros(k - N, h, device=a.device)])
        rows = torch.cat([rows, torch.full((k - N, h), -1, dtype=torch.int64, device=a.device)])
    rows = torch.where(vals > 0, rows, torch.full_like(rows, -1))
    return {"count": count, "sum": s, "hist": hist, "topk_val": vals.t().contiguous(),
            "topk_row": rows.t().contiguous()}


def fresh_state(h, k, dev, hist=True):
    return {"count": torch.zeros(h, dtype=torch.int64, device=dev),
            "sum": torch.zeros(h, dtype=torch.float32, device=dev),
            "hist": torch.zeros(h, 32, dtype=torch.int64, device=dev) if hist else None,
            "topk_val": torch.zeros(h, k, dtype=torch.float32, device=dev),
            "topk_row": torch.full((h, k), -1, dtype=torch.int64, device=dev)}


def run_kernel(batches, h, k, dev, ids=None, hist=True):
    """batches: [B, ld] tensors fed in order; ids: per-batch int64 id tensors, or None (rows numbered on)."""
    st = fresh_state(h, k, dev, hist)
    row0 = 0
    for i, a in enumerate(batches):
        ops.latent_stats_update(a, h, k, st["count"], st["sum"], st["hist"], st["topk_val"], st["topk_row"],
                                row_ids=None if ids is None else ids[i], row0=row0)
        row0 += a.shape[0]
    return st


def make_batches(B, h, ld, dtype, k, dev, seed, relu=True):
    """Three batches of seeded normals rounded to multiples of 1/8 (ties are common), with the built-in cases:
    column 0 all zero, column 1 fewer than k positives, column 2's largest values in the first batch, column 3's
    in the last.  The padding columns h..ld-1 hold large values the kernel must not look at."""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for i in range(3):
        a = torch.round(torch.randn(B, ld, generator=g, device=dev) * 8) / 8
        if relu:
            a = a.relu()
        a[:, 0] = 0 if relu else -a[:, 0].abs()
        a[:, 1] = 0 if relu else -1.0
        if i < min(k - 1, 3):
            a[(7 * i) % B, 1] = 0.5 + i  # k - 1 positives at the most
        if i == 0:
            a[:, 2] += 100 * (a[:, 2] > 0)
        if i == 2:
            a[:, 3] += 100 * (a[:, 3] > 0)
        a[:, h:] = 999.0
        out.append(a.to(dtype))
    return out


def check(st, ref, rows_total, hist=True):
    assert torch.equal(st["count"], ref["count"])
    if hist:
        assert torch.equal(st["hist"], ref["hist"])
        assert torch.equal(st["hist"].sum(1), st["count"])
    assert torch.equal(st["topk_val"], ref["topk_val"])
    assert torch.equal(st["topk_row"], ref["topk_row"])
    # the worst case of any fp32 summation order of rows_total non-negative terms
    err = (st["sum"].double() - ref["sum"]).abs()
    assert bool((err <= rows_total * 2.0 ** -24 * ref["sum"]).all()), err.max().item()


SHAPES = [(1, 8, 8), (64, 256, 256), (96, 200, 208), (300, 264, 264)]


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", SHAPES)
def test_kernel_small_shapes(gpu, B, h, ld, dtype, k):
    batches = make_batches(B, h, ld, DT[dtype], k, gpu, seed=B + h + k)
    st = run_kernel(batches, h, k, gpu)
    ref = reference(torch.cat(batches)[:, :h], torch.arange(3 * B, device=gpu), k)
    check(st, ref, 3 * B)
    assert st["count"][0].item() == 0 and st["topk_row"][0, 0].item() == -1  # the all-zero column
    assert st["topk_row"][1, k - 1].item() == -1 and st["topk_val"][1, k - 1].item() == 0.0  # (0, -1) slots
    if B > 1:
        assert int(st["topk_row"][2, 0]) < B and int(st["topk_row"][3, 0]) >= 2 * B


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", SHAPES)
def test_kernel_row_ids_out_of_order(gpu, B, h, ld, dtype):
    """Explicit ids, shuffled within a batch, batch 2's below batch 1's: exact, tie order included."""
    k = 16
    batches = make_batches(B, h, ld, DT[dtype], k, gpu, seed=17 + B)
    g = torch.Generator(device=gpu).manual_seed(5)
    base = [1000, 0, 5000]
    ids = [base[i] + torch.randperm(B, generator=g, device=gpu) for i in range(3)]
    st = run_kernel(batches, h, k, gpu, ids=ids)
    check(st, reference(torch.cat(batches)[:, :h], torch.cat(ids), k), 3 * B)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_kernel_ignores_negatives_and_nan(gpu, dtype):
    """apply_relu=False style input: the result is that of the ReLU'd, NaN -> 0 input."""
    B, h, ld, k = 96, 200, 208, 5
    raw = make_batches(B, h, ld, DT[dtype], k, gpu, seed=3, relu=False)
    raw[1][5, 7] = float("nan")
    assert bool((torch.cat(raw)[:, :h] < 0).any())
    clean = [torch.nan_to_num(a, nan=0.0).relu() for a in raw]
    st = run_kernel(raw, h, k, gpu)
    check(st, reference(torch.cat(clean)[:, :h], torch.arange(3 * B, device=gpu), k), 3 * B)
    st2 = run_kernel(clean, h, k, gpu)
    for key in st:
        assert torch.equal(st[key], st2[key]), key


def test_kernel_bit_reproducible(gpu):
    B, h, ld, k = 300, 264, 264, 16
    batches = make_batches(B, h, ld, torch.bfloat16, k, gpu, seed=11)
    a, b = run_kernel(batches, h, k, gpu), run_kernel(batches, h, k, gpu)
    assert torch.equal(a["sum"].view(torch.int32), b["sum"].view(torch.int32))
    for key in a:
        assert torch.equal(a[key], b[key]), key
    c = run_kernel(batches, h, k, gpu, hist=False)  # without the histogram: the rest unchanged
    for key in ("count", "sum", "topk_val", "topk_row"):
        assert torch.equal(a[key], c[key]), key


def small_cfg(B, d, h, dtype, dev, **kw):
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": B * 100, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": dtype, "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,n,d,h", [(96, 2, 40, 200), (64, 4, 32, 256), (64, 2, 32, 203)])
def test_through_the_model(gpu, B, n, d, h, dtype):
    """LatentStats.update in two chunks against the reference on cc.encode(x); dict_size 203 runs on 208 kernel
    latents whose padding must not show."""
    cc = ca.CrossCoder(small_cfg(B, d, h, dtype, gpu), n_models=n)
    with torch.no_grad():
        cc.b_enc.copy_(torch.linspace(-0.5, 0.5, h, device=gpu))  # from rarely to mostly active
    x = torch.randn(B, n, d, generator=torch.Generator(device=gpu).manual_seed(B + h), device=gpu)
    k = 8
    st = ca.LatentStats(cc, k=k)
    st.update(x[:40])
    st.update(x[40:])
    assert st.rows_seen == B
    r = st.result()
    acts = cc.encode(x)
    assert acts.shape == (B, h)
    ref = reference(acts, torch.arange(B, device=gpu), k)
    got = {"count": r["count"], "sum": r["sum"], "hist": r["hist"], "topk_val": r["topk_values"],
           "topk_row": r["topk_rows"]}
    for key, t in got.items():
        assert t.shape[0] == h, key  # no padding latents
    check(got, ref, B)
    assert torch.equal(r["dead"], ref["count"] == 0)
    assert torch.equal(r["max"], ref["topk_val"][:, 0])
    assert torch.allclose(r["frequency"].double(), ref["count"].double() / B, rtol=1e-6, atol=0)
    mean = torch.where(r["count"] > 0, r["sum"] / r["count"].clamp(min=1).float(), torch.zeros_like(r["sum"]))
    assert torch.equal(r["mean_active"], mean)
    assert r["hist_edges"].shape == (33,) and int(r["log10_frequency_hist"].sum()) == int((ref["count"] > 0).sum())
    st.reset()
    assert st.rows_seen == 0 and int(st.result()["count"].sum()) == 0
    # explicit ids on one chunk, and the argument checks
    st.update(x, row_ids=torch.arange(B - 1, -1, -1))
    assert torch.equal(st.result()["topk_rows"], reference(acts, torch.arange(B - 1, -1, -1, device=gpu), k)["topk_row"])
    with pytest.raises(ValueError):
        st.update(x[:, :1])
    with pytest.raises(ValueError):
        st.update(x, row_ids=torch.arange(B - 1))
    with pytest.raises(ValueError):
        st.update_from_acts(acts[:, :h - 8])
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError):
            ca.LatentStats(cc, k=bad)


def test_full_size_config2(gpu):
    """Config 2's activations (4096 x 16384 bf16), one batch, k = 16."""
    B, h, k = 4096, 16384, 16
    g = torch.Generator(device=gpu).manual_seed(2)
    acts = torch.randn(B, h, generator=g, device=gpu).relu().to(torch.bfloat16)
    st = run_kernel([acts], h, k, gpu)
    assert torch.equal(st["count"], (acts > 0).sum(0))
    assert torch.equal(st["hist"].sum(1), st["count"])
    top = torch.topk(acts.t().float(), k).values
    assert torch.equal(st["topk_val"], torch.where(top > 0, top, torch.zeros_like(top)))
    rows = st["topk_row"]
    assert bool(((rows >= 0) & (rows < B)).all())  # (every latent has more than k positives here)
    latent = torch.arange(h, device=gpu)[:, None].expand(h, k)
    assert torch.equal(acts[rows, latent].float(), st["topk_val"])
    assert bool((rows.sort(1).values.diff(dim=1) > 0).all())  # distinct rows per latent
    s = torch.where(acts > 0, acts, torch.zeros_like(acts)).double().sum(0)
    assert bool(((st["sum"].double() - s).abs() <= B * 2.0 ** -24 * s).all())


def test_trainer_hook(gpu):
    """bf16: the hook is refused for fp32 crosscoders (test_trainer_hook_refuses_fp32).  No device drain between
    the steps, as train() runs them."""
    dtype = "bf16"
    B, n, d, h, steps = 64, 2, 32, 256, 3

    def run(cfg, hook):
        cc = ca.CrossCoder(cfg, n_models=n)
        st = ca.LatentStats(cc, k=4) if hook else None
        tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * steps, n_models=n, seed=3), crosscoder=cc,
                        latent_stats=st)
        out = []
        for _ in range(steps):
            dct = tr.step()
            tr.synchronize()
            out.append((dct, [getattr(cc, p).detach().clone() for p in ("W_enc", "W_dec", "b_enc", "b_dec")]))
        return cc, st, out

    cfg = small_cfg(B, d, h, dtype, gpu)
    _, _, off = run(cfg, False)
    _, st, on = run(cfg, True)
    assert st.rows_seen == B * steps
    for (d0, p0), (d1, p1) in zip(off, on):
        assert list(d0) == list(d1) and len(d1) == 9
        assert all(d0[key] == d1[key] for key in d0), (d0, d1)
        for a, b in zip(p0, p1):
            assert torch.equal(a, b)
    # lr = 0: the parameters stay fixed, so the hook saw cc.encode of the same three normalised batches
    cfg0 = small_cfg(B, d, h, dtype, gpu, lr=0.0)
    cc, st, _ = run(cfg0, True)
    buf = ca.SyntheticBuffer(cfg0, rows=B * steps, n_models=n, seed=3)
    st2 = ca.LatentStats(cc, k=4)
    for _ in range(steps):
        st2.update(buf.next())
    r, r2 = st.result(), st2.result()
    assert int(r["count"].sum()) > 0
    for key in r:
        assert torch.equal(r[key], r2[key]), key


def test_trainer_hook_refuses_fp32(gpu):
    cfg = small_cfg(64, 32, 256, "fp32", gpu)
    cc = ca.CrossCoder(cfg)
    buf = ca.SyntheticBuffer(cfg, rows=64, seed=3)
    with pytest.raises(ValueError, match="bf16"):
        ca.Trainer(cfg, buffer=buf, crosscoder=cc, latent_stats=ca.LatentStats(cc, k=4))
    st = ca.LatentStats(cc, k=4)  # (the statistics themselves serve fp32)
    st.update(buf.next())
    assert st.rows_seen == 64 and int(st.result()["count"].sum()) > 0
    with pytest.raises(ValueError):
        ca.Trainer(cfg, buffer=buf, crosscoder=ca.CrossCoder(cfg), latent_stats=st)  # another crosscoder's


def test_errors_make_no_launch(gpu):
    B, h = 8, 16
    acts = torch.zeros(B, h, device=gpu)
    for k, hh in ((0, h), (17, h), (4, h + 8)):  # k out of range; ld < h
        st = fresh_state(hh, k, gpu)
        with pytest.raises(RuntimeError, match="crosscoder_hip error 3"):
            ops.latent_stats_update(acts, hh, k, st["count"], st["sum"], st["hist"], st["topk_val"], st["topk_row"])
    with pytest.raises(TypeError):
        st = fresh_state(h, 4, gpu)
        ops.latent_stats_update(acts.half(), h, 4, st["count"], st["sum"], st["hist"], st["topk_val"], st["topk_row"])
    assert ops.latent_stats_max_k() == 16
    torch.cuda.synchronize()
