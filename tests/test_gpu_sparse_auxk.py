"""AuxK under the sparse TopK step on the GPU: cc_dead_compact against torch.nonzero,
cc_compact_gather against torch indexing, cc_pairs_wgrad_add against cc_pairs_wgrad and the lane-order restatements of
tests/_sparse_step_ref.py, then Trainer.step with cfg["auxk_compact"] against the dense TopK + AuxK trainer (selection,
loss), the fp64 objective with the GPU's two masks imposed (gradients; tests/test_gpu_auxk.py's bounds), cc_adam_step, and
over steps: nothing dead, reproducibility with a skewed selection, capacity growth, revival.

The twin.  The dense TopK + AuxK step and the sparse step round their gradients in different orders, so two trainers
drift apart by rounding after one update.  Where a test compares selections over several steps, the twin takes the sparse
trainer's parameters before every step (CrossCoder.load_state_dict): each step then starts from one state on both
sides, and tokens_since_fired -- set once, through the setter -- evolves on each side by its own dead update."""
import ctypes
import functools
import math

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, engine, ops
from oracle import cpu_reference as O
from tests import _sparse_step_ref as ref
from tests._auxk_ref import auxk_loss_ref, step_loss_ref
from tests.test_gpu_auxk import FixedBatches
from tests.test_gpu_sparse_step import SKEW, bits, case, clip_reference, on_gpu, scattered_pairs, skew_b_enc
from tests.test_gpu_topk import small_cfg

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
DEAD_AFTER = 1000
CAN = 1234.0
ICAN = -77
N, D_IN, K_MAIN = 2, 32, 4          # K = 64


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


def dead_set(kind, h_real):
    """bool [h_real]: the issue's dead sets -- empty; one latent; five scattered, latent 0 and the last one among them;
    a count that is no multiple of the granule; every latent"""
    dead = torch.zeros(h_real, dtype=torch.bool)
    if kind == "one":
        dead[h_real // 3] = True
    elif kind == "five":
        dead[[0, 17, h_real // 2, h_real - 9, h_real - 1]] = True
    elif kind == "odd":
        dead[torch.arange(2, h_real, 7)[:engine.AUX_GRANULE + 3]] = True
    elif kind == "all":
        dead[:] = True
    elif kind == "20th":
        dead[::20] = True
    else:
        assert kind == "empty"
    return dead


def tsf_of(dead):
    """tokens_since_fired on both sides of the threshold, the threshold itself included"""
    i = torch.arange(dead.numel())
    return torch.where(dead, DEAD_AFTER + (i % 3) * 1000, (i * 7) % DEAD_AFTER).to(torch.int64)


# ---------------------------------------------------------------- cc_dead_compact
@pytest.mark.parametrize("kind", ["empty", "one", "five", "odd", "all", "20th"])
@pytest.mark.parametrize("h,h_real", [(256, 256), (208, 200), (1 << 17, (1 << 17) - 3)], ids=["h256", "h200", "h2^17"])
def test_dead_compact_is_nonzero_of_the_rule(gpu, h, h_real, kind):
    dead = dead_set(kind, h_real)
    tsf = torch.full((h,), 10 * DEAD_AFTER, dtype=torch.int64)      # padding latents: over the threshold, never dead
    tsf[:h_real] = tsf_of(dead)
    want = torch.nonzero(tsf[:h_real] >= DEAD_AFTER).flatten().to(torch.int32)
    D = want.numel()
    assert D == int(dead.sum())
    Dp = engine.aux_pad(D)
    assert kind != "odd" or D % engine.AUX_GRANULE
    want_slot = torch.full((h,), -1, dtype=torch.int32)
    want_slot[want.long()] = torch.arange(D, dtype=torch.int32)
    d_tsf = tsf.to(gpu)
    runs = []
    for _ in range(2):
        ids = torch.full((Dp + 16,), ICAN, dtype=torch.int32, device=gpu)
        slot = torch.full((h + 8,), ICAN, dtype=torch.int32, device=gpu)
        count = torch.full((3,), ICAN, dtype=torch.int32, device=gpu)
        ops.dead_compact(d_tsf, h_real, DEAD_AFTER, ids[:Dp], slot[:h], count[1:2])
        assert torch.equal(ids[:D].cpu(), want) and bool((ids[D:Dp] == -1).all())
        assert torch.equal(slot[:h].cpu(), want_slot)
        assert count.cpu().tolist() == [ICAN, D, ICAN]
        assert bool((ids[Dp:] == ICAN).all()) and bool((slot[h:] == ICAN).all())        # canaries
        runs.append((ids, slot))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(d_tsf.cpu(), tsf)
    if D > 8:   # a capacity below the count: the first d_pad dead latents, the rest dropped, the count says so
        ids = torch.full((8 + 16,), ICAN, dtype=torch.int32, device=gpu)
        slot = torch.full((h,), ICAN, dtype=torch.int32, device=gpu)
        count = torch.zeros(1, dtype=torch.int32, device=gpu)
        ops.dead_compact(d_tsf, h_real, DEAD_AFTER, ids[:8], slot, count)
        assert torch.equal(ids[:8].cpu(), want[:8]) and bool((ids[8:] == ICAN).all()) and int(count) == D
        assert torch.equal(slot.cpu(), torch.where(want_slot < 8, want_slot, torch.full_like(want_slot, -1)))


# ---------------------------------------------------------------- cc_compact_gather
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,h_real,kind", [(96, 256, 256, "five"), (288, 208, 200, "odd"), (96, 208, 200, "all"),
                                             (40, 4104, 4100, "all")],
                         ids=["B96-h256-five", "B288-h200-odd", "B96-h200-all", "two-column-chunks"])
def test_compact_gather_is_torch_indexing(gpu, B, h, h_real, kind, dt):
    K = N * D_IN
    g = torch.Generator().manual_seed(B + h)
    acts = torch.randn(B, h, generator=g).to(DT[dt])
    acts[::5, ::3] = -0.0
    W = torch.randn(h, K + 8, generator=g).to(DT[dt])
    dead = dead_set(kind, h_real)
    live = torch.nonzero(dead).flatten()
    D = live.numel()
    Dp = min(engine.aux_pad(D), h)
    ids = torch.full((Dp,), -1, dtype=torch.int32)
    ids[:D] = live.to(torch.int32)
    assert kind != "five" or (D == 5 and Dp == 8 and ids[0] == 0 and ids[4] == h_real - 1)
    assert kind != "two-column-chunks" or Dp > 2048
    zero = torch.zeros((), dtype=DT[dt])
    want_cols = torch.where(ids[None, :] >= 0, acts[:, ids.clamp(min=0).long()], zero)
    want_rows = torch.where(ids[:, None] >= 0, W[ids.clamp(min=0).long(), :K], zero)
    d_ids, d_acts, d_W = ids.to(gpu), acts.to(gpu), W.to(gpu)
    flat = torch.full((B * Dp + 64,), CAN, dtype=DT[dt], device=gpu)
    Wc = torch.full((Dp + 2, K + 16), CAN, dtype=DT[dt], device=gpu)
    ops.compact_gather(d_ids, h, acts=d_acts, acts_c=flat[:B * Dp].view(B, Dp))
    ops.compact_gather(d_ids, h, W=d_W[:, :K], Wc=Wc[:Dp, 8:8 + K])
    got_cols, got_rows = flat[:B * Dp].view(B, Dp).cpu(), Wc[:Dp, 8:8 + K].cpu()
    assert torch.equal(bits(got_cols), bits(want_cols)) and torch.equal(bits(got_rows), bits(want_rows))
    if Dp > D:   # +0 at the padding slots
        assert not bool(bits(got_cols)[:, D:].any()) and not bool(bits(got_rows)[D:].any())
    assert bool((flat[B * Dp:] == CAN).all())
    assert bool((Wc[Dp:] == CAN).all()) and bool((Wc[:, :8] == CAN).all()) and bool((Wc[:, 8 + K:] == CAN).all())
    assert torch.equal(bits(d_acts.cpu()), bits(acts)) and torch.equal(bits(d_W.cpu()), bits(W))
    # both groups in one call, and an index beyond h: +0
    both_c = torch.full((B, Dp), CAN, dtype=DT[dt], device=gpu)
    both_r = torch.full((Dp, K), CAN, dtype=DT[dt], device=gpu)
    ops.compact_gather(d_ids, h, W=d_W[:, :K], Wc=both_r, acts=d_acts, acts_c=both_c)
    assert torch.equal(bits(both_c.cpu()), bits(want_cols)) and torch.equal(bits(both_r.cpu()), bits(want_rows))
    narrow = int(ids[D - 1])    # h = the last dead latent: it is out of range now
    ops.compact_gather(d_ids, narrow, W=d_W[:, :K], Wc=both_r, acts=d_acts, acts_c=both_c)
    assert not bool(bits(both_c.cpu())[:, D - 1].any()) and not bool(bits(both_r.cpu())[D - 1].any())
    assert torch.equal(bits(both_c.cpu())[:, :D - 1], bits(want_cols)[:, :D - 1])


# ---------------------------------------------------------------- cc_pairs_wgrad_add
WG_SHAPES = [(96, N, D_IN, 256, K_MAIN), (288, N, D_IN, 200, K_MAIN), SKEW]


@functools.lru_cache(maxsize=None)
def wg_case(shape, dt):
    """test_gpu_sparse_step.case plus the latents that get a slot -- every fifth latent, the hot latent 3 (a list of
    two full pieces and a rest in the skewed case) and three latents with an empty list, if there are any -- and their
    addend rows (computed once, never written)"""
    c = dict(case(shape, dt))
    B, n, d, h, k = shape
    K = n * d
    g = torch.Generator().manual_seed(h + B)
    chosen = set(range(0, h, 5)) | {3, h - 1} | set(torch.nonzero(c["len"] == 0).flatten().tolist()[:3])
    lat = torch.tensor(sorted(chosen))
    D = lat.numel()
    Dp = engine.aux_pad(D)
    slot = torch.full((h,), -1, dtype=torch.int32)
    slot[lat] = torch.arange(D, dtype=torch.int32)
    c.update(slot=slot, lat=lat, Dp=Dp,
             aWd=(torch.randn(Dp, K, generator=g) / B).to(DT[dt]), aWe=(torch.randn(Dp, K, generator=g) / B).to(DT[dt]),
             ab=(torch.randn(Dp, generator=g) / B).to(DT[dt]))
    return c


def run_wgrad_add(c, shape, dt, slot=None, add=True):
    B, n, d, h, k = shape
    K = n * d
    dev = torch.device("cuda")
    val, gpre, gr, x = on_gpu(c, "val", "g_pre", "g_recon", "x")
    perm = torch.tensor(c["perm"] + [0] * (B * k - len(c["perm"])), dtype=torch.int32, device=dev)
    seg = torch.tensor(c["seg"], dtype=torch.int64, device=dev)
    parts = ops.pairs_wgrad_parts(h)
    dWd = torch.full((h + 2, K + 40), CAN, dtype=DT[dt], device=dev)
    dWe = torch.full((h + 2, K + 40), CAN, dtype=DT[dt], device=dev)
    db = torch.full((h + 8,), CAN, dtype=DT[dt], device=dev)
    sq = [torch.full((parts + 8,), CAN, dtype=torch.float32, device=dev) for _ in range(3)]
    ws = torch.full((ops.pairs_wgrad_ws_floats(B * k, K) + 64,), CAN, dtype=torch.float32, device=dev)
    args = (perm, seg, val, gpre, gr, x, K, dWd[:h, 32:32 + K], dWe[:h, 32:32 + K], db[:h], sq[0][:parts], sq[1][:parts],
            sq[2][:parts])
    if add:
        # (the addends as column slices of wider matrices: their pitches are kept)
        Dp = c["Dp"]
        wide = [torch.full((Dp, K + 24), CAN, dtype=DT[dt], device=dev) for _ in range(2)]
        wide[0][:, 8:8 + K], wide[1][:, 8:8 + K] = c["aWd"].to(dev), c["aWe"].to(dev)
        ops.pairs_wgrad_add(*args, (c["slot"] if slot is None else slot).to(dev), wide[0][:, 8:8 + K], wide[1][:, 8:8 + K],
                            c["ab"].to(dev), ws=ws)
    else:
        ops.pairs_wgrad(*args, ws=ws)
    torch.cuda.synchronize()
    return {"dWd": dWd, "dWe": dWe, "db": db, "sq": sq, "parts": parts}


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", WG_SHAPES, ids=lambda s: "B%d_h%d_k%d" % (s[0], s[3], s[4]))
def test_wgrad_add_against_wgrad_and_the_restatement(gpu, shape, dt):
    B, n, d, h, k = shape
    K = n * d
    c = wg_case(shape, dt)
    plain = run_wgrad_add(c, shape, dt, add=False)
    # slot all -1: cc_pairs_wgrad's bits in all six outputs (canaries included)
    off = run_wgrad_add(c, shape, dt, slot=torch.full((h,), -1, dtype=torch.int32))
    for key in ("dWd", "dWe", "db"):
        assert torch.equal(bits(off[key]), bits(plain[key])), key
    for a, b in zip(off["sq"], plain["sq"]):
        assert torch.equal(bits(a), bits(b))
    r = run_wgrad_add(c, shape, dt)
    lat, slot = c["lat"], c["slot"]
    view = lambda t: t[:h, 32:32 + K].cpu()  # noqa: E731
    got = {"dWd": view(r["dWd"]), "dWe": view(r["dWe"]), "db": r["db"][:h].cpu()}
    base = {"dWd": view(plain["dWd"]), "dWe": view(plain["dWe"]), "db": plain["db"][:h].cpu()}
    addend = {"dWd": torch.zeros(h, K), "dWe": torch.zeros(h, K), "db": torch.zeros(h)}
    addend["dWd"][lat], addend["dWe"][lat], addend["db"][lat] = (c[key][:lat.numel()].float() for key in ("aWd", "aWe", "ab"))
    has = slot >= 0
    empty = c["len"] == 0
    assert int((has & ~empty).sum()) > 0 and int((~has & ~empty).sum()) > 0
    assert shape != SKEW or (int((has & empty).sum()) >= 3 and int(c["len"][3]) == B and bool(has[3]))
    # the fp32 sums before the one rounding, in the documented lane order
    p = c["g_pre"].to(DT[dt])
    sums = {"dWd": ref.lists_f32(c["perm"], c["seg"], c["val"], c["g_recon"], K),
            "dWe": ref.lists_f32(c["perm"], c["seg"], p, c["x"], K), "db": ref.lists_sum_f32(c["perm"], c["seg"], p)}
    for key in ("dWd", "dWe", "db"):
        # a latent without a slot: cc_pairs_wgrad's bits
        assert torch.equal(bits(got[key])[~has], bits(base[key])[~has]), key
        # an empty list and a slot: the addend, bit for bit
        if (has & empty).any():
            assert torch.equal(bits(got[key])[has & empty], bits(addend[key].to(DT[dt]))[has & empty]), key
        if dt == "fp32":
            # the stored value is fp32(cc_pairs_wgrad's value + addend)
            assert torch.equal(bits(got[key]), bits(base[key] + addend[key])), key
        else:
            # the addend is added before the one rounding
            assert torch.equal(bits(got[key]), bits((sums[key] + addend[key]).to(torch.bfloat16))), key
            twice = (base[key].float() + addend[key]).to(torch.bfloat16)
            assert key == "db" or not torch.equal(bits(got[key]), bits(twice)), (key, "rounded twice would pass too")
    # the squared sums: of the stored values, in the lane's store order; within (D + 1) 2^-24 of fp64
    Dchain = ref.sq_chain_depth(h, K)
    for name, part, stored in (("dW_dec", r["sq"][0], got["dWd"]), ("dW_enc", r["sq"][1], got["dWe"]),
                               ("db_enc", r["sq"][2], got["db"])):
        parts = r["parts"]
        assert torch.equal(bits(part[:parts].cpu()), bits(ref.sq_partials(stored))), name
        total, exact = float(part[:parts].double().sum()), float(stored.double().pow(2).sum())
        print(name, "sq rel err / bound:", abs(total - exact) / max(exact, 1e-300) / ((Dchain + 1) * 2.0 ** -24))
        assert exact > 0 and abs(total - exact) <= (Dchain + 1) * 2.0 ** -24 * exact, name
        assert bool((part[parts:] == CAN).all()), name
    for t in (r["dWd"], r["dWe"]):
        assert bool((t[h:] == CAN).all()) and bool((t[:, :32] == CAN).all()) and bool((t[:, 32 + K:] == CAN).all())
    assert bool((r["db"][h:] == CAN).all())
    r2 = run_wgrad_add(c, shape, dt)    # two calls: equal bits
    for key in ("dWd", "dWe", "db"):
        assert torch.equal(bits(r[key]), bits(r2[key])), key
    for a, b in zip(r["sq"], r2["sq"]):
        assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------- the step, through Trainer
def aux_cfg(B, h, dtype, k_aux, sparse=True, aux=True, **kw):
    cfg = small_cfg(B, D_IN, h, dtype, "cuda:0", l1_coeff=0.0, activation="topk", k=K_MAIN)
    if aux:
        cfg.update(auxk_coeff=1.0 / 32, k_aux=k_aux, dead_tokens=DEAD_AFTER)
    if sparse:
        cfg.update(sparse_step=True)
        if aux:
            cfg.update(auxk_compact=True)
    cfg.update(kw)
    return cfg


def batches_of(B, dtype, steps, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N, D_IN, generator=g).to(DT[dtype]) for _ in range(steps)]


def trainer_of(cfg, batches, tsf=None, b_enc=None):
    cc = ca.CrossCoder(cfg, n_models=N)
    if b_enc is not None:
        with torch.no_grad():
            cc.b_enc.copy_(b_enc.to(cc.b_enc.device))
    tr = ca.Trainer(cfg, buffer=FixedBatches(batches, "cuda:0"), crosscoder=cc)
    if tsf is not None:
        tr.tokens_since_fired = tsf
    return tr


def settle(tr):
    tr.synchronize()
    torch.cuda.synchronize()


def params_of(tr):
    return {key: getattr(tr.crosscoder, key).detach().cpu().clone() for key in O.PARAM_ORDER}


def aux_scalars_ref(x, P, M, A, dtype):
    """(auxk_loss, den) of tests/_auxk_ref.py's objective with the masks imposed, in `dtype`"""
    x = x.to(dtype)
    P = {key: v.to(dtype) for key, v in P.items()}
    relu = torch.relu(torch.einsum("bnd,ndh->bh", x, P["W_enc"]) + P["b_enc"])
    recon = torch.einsum("bh,hnd->bnd", relu * M.to(dtype), P["W_dec"]) + P["b_dec"]
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    e = (x.to(wide) - recon.to(wide)).reshape(x.shape[0], -1)
    ehat = torch.einsum("bh,hnd->bnd", relu * A.to(dtype), P["W_dec"]).to(wide).reshape(x.shape[0], -1)
    loss, den, valid = auxk_loss_ref(e, ehat)
    assert valid
    return loss, den


SELECT = [(96, 256, "one", 1), (96, 256, "five", 8), (288, 200, "odd", 8), (288, 200, "all", 200), (96, 200, "five", 64)]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,kind,k_aux", SELECT, ids=["%s-B%d-h%d-kaux%d" % (s[2], s[0], s[1], s[3]) for s in SELECT])
def test_selection_and_loss_against_the_dense_twin(gpu, B, h, kind, k_aux, dtype):
    """Three steps.  Bit for bit the twin's: the main selection, the aux selection, the dead set, dead_latents and
    tokens_since_fired.  auxk_loss and den against fp64 in tests/test_gpu_auxk.py's bounds: fp32 rel < 2e-5, bf16 error
    <= 2 x the CPU-bf16 error + 2e-3.  The host's dead count is the device's."""
    steps = 3
    dt = DT[dtype]
    batches = batches_of(B, dtype, steps)
    tsf = tsf_of(dead_set(kind, h))
    sp = trainer_of(aux_cfg(B, h, dtype, k_aux), batches, tsf)
    tw = trainer_of(aux_cfg(B, h, dtype, k_aux, sparse=False), batches, tsf)
    assert sp.sparse_step and sp.auxk_compact and not tw.sparse_step
    active = 0
    for s in range(steps):
        settle(sp)
        P = params_of(sp)
        tw.crosscoder.load_state_dict(P)
        host_count = sp._dead_count
        assert host_count == tw._dead_count == int((sp.tokens_since_fired >= DEAD_AFTER).sum())
        ds, dw = sp.step(), tw.step()
        settle(sp)
        settle(tw)
        ws, st, sw = sp._last_ws, sp.auxk_state(), tw.auxk_state()
        assert len(ds) == 11 and ds.keys() == dw.keys()
        main = scattered_pairs(ws, h)
        assert torch.equal(bits(main), bits(tw._last_ws.acts[:, :h])), s
        assert torch.equal(bits(st["aux_acts"]), bits(sw["aux_acts"])), s
        assert torch.equal(st["dead"], sw["dead"]) and ds["dead_latents"] == dw["dead_latents"] == st["dead_latents"]
        assert torch.equal(sp.tokens_since_fired, tw.tokens_since_fired), s
        assert ws.aux_active == (host_count > 0) == tw._last_ws.aux_active
        if not ws.aux_active:
            assert ds["auxk_loss"] == 0.0 and st["dead_ids"].numel() == 0
            continue
        active += 1
        assert st["compact_count"] == host_count == int(st["dead"].sum())
        assert torch.equal(st["dead_ids"].cpu(), torch.nonzero(st["dead"].cpu()).flatten())
        assert ws.aux_Dp == engine.aux_pad(host_count) and ws.aux_Dp <= ws.aux_cap
        A, M = (st["aux_acts"] > 0).cpu(), (main > 0).cpu()
        assert bool((A.sum(1) <= min(k_aux, host_count)).all()) and not bool(A[:, ~st["dead"].cpu()].any())
        assert torch.equal(st["row_count"].cpu().long(), A.sum(1))
        if not A.any():     # (nothing eligible among the dead: e^ = 0, the loss is the ratio of e's moments)
            continue
        x = batches[s]
        t_loss, t_den = aux_scalars_ref(x, P, M, A, torch.float64)
        for name, ours, truth in (("auxk_loss", ds["auxk_loss"], t_loss), ("den", st["den"], t_den)):
            e = abs(ours - truth.item()) / truth.item()
            if dt == torch.float32:
                print(dtype, kind, s, name, "rel", e)
                assert e < 2e-5, (name, e)
            else:
                c_loss, c_den = aux_scalars_ref(x, P, M, A, dt)
                cpu = (c_loss if name == "auxk_loss" else c_den).item()
                e_ref = abs(cpu - truth.item()) / truth.item()
                print(dtype, kind, s, name, "(ours, cpu) vs fp64", e, e_ref)
                assert e <= 2 * e_ref + 2e-3, (name, e, e_ref)
        assert ds["auxk_loss"] == st["auxk_loss"] and ds["auxk_loss"] > 0
        assert abs(ds["loss"] - (ds["l2_loss"] + ds["auxk_loss"] / 32)) <= 1e-6 * abs(ds["loss"])
    assert active >= 1


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h", [(96, 256), (288, 200)])
def test_gradients_with_the_gpu_masks(gpu, B, h, dtype):
    """One step; every third latent dead, so that dead latents fire in the batch (both supports: the gradients add) and
    others do not.  All four gradients against the fp64 objective with the GPU's masks imposed, in
    tests/test_gpu_auxk.py's bounds (bf16 error <= 2 x the CPU-bf16 error + 5e-3, fp32 rel < 2e-5); b_dec's gradient is
    the aux-less sparse step's, bit for bit; clip_out against clip_grad_norm_'s arithmetic on the stored gradients
    (tests/test_gpu_sparse_step.py's tolerances)."""
    dt = DT[dtype]
    coeff = 1.0 / 32
    batches = batches_of(B, dtype, 1)
    dead = torch.zeros(h, dtype=torch.bool)
    dead[::3] = True
    tr0 = trainer_of(aux_cfg(B, h, dtype, 8, aux=False), batches)
    P = params_of(tr0)
    tr0.step()
    settle(tr0)
    g0 = {key: v.detach().cpu().clone() for key, v in tr0.optimizer.grads.views().items()}
    tr = trainer_of(aux_cfg(B, h, dtype, 8), batches, tsf_of(dead))
    dct = tr.step()
    settle(tr)
    ws, st = tr._last_ws, tr.auxk_state()
    g = {key: v.detach().cpu().clone() for key, v in tr.optimizer.grads.views().items()}
    M, A = (scattered_pairs(ws, h) > 0).cpu(), (st["aux_acts"] > 0).cpu()
    assert ws.aux_active and torch.equal(M, (scattered_pairs(tr0._last_ws, h) > 0).cpu())
    assert int((A & M).sum()) > 0 and int((A & ~M).sum()) > 0 and not bool(A[:, ~dead].any())
    assert torch.equal(bits(g["b_dec"]), bits(g0["b_dec"]))
    for key in ("W_enc", "b_enc", "W_dec"):
        assert not torch.equal(g[key], g0[key]), key
    x = batches[0]

    def oracle(dtype_):
        leaves = {key: v.detach().to(dtype_).clone().requires_grad_(True) for key, v in P.items()}
        total, parts = step_loss_ref(x.to(dtype_), leaves, M, A, 0.0, coeff)
        total.backward()
        return parts, {key: leaves[key].grad for key in O.PARAM_ORDER}

    _, gref = oracle(dt)
    _, gtruth = oracle(torch.float64)
    for key in O.PARAM_ORDER:
        assert g[key].shape == gref[key].shape and g[key].dtype == gref[key].dtype, key
        if dt == torch.float32:
            e = rel(g[key], gtruth[key])
            print(dtype, B, h, key, "grad rel", e)
            assert e < 2e-5, (key, e)
        else:
            e_ours, e_ref = rel(g[key], gtruth[key]), rel(gref[key], gtruth[key])
            print(dtype, B, h, key, "grad (ours, cpu) vs fp64", e_ours, e_ref)
            assert e_ours <= 2 * e_ref + 5e-3, (key, e_ours, e_ref)
    if tr.crosscoder._hp > h:   # the padding latents' gradient rows stay +0
        G = tr.optimizer.grads
        assert not bool(bits(G.W_enc_hk[h:]).any()) and not bool(bits(G.W_dec_hk[h:]).any()) and not bool(bits(G.b_enc[h:]).any())
    clip = ws.clip_out[:2].cpu()
    coef, total = clip_reference([g[key] for key in O.PARAM_ORDER], dt)
    tol = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -19
    print(dtype, B, h, "clip", clip.tolist(), "reference", (coef, total))
    assert math.isclose(clip[1].item(), total, rel_tol=tol) and math.isclose(clip[0].item(), coef, rel_tol=tol)
    assert len(dct) == 11 and dct["auxk_loss"] > 0


@pytest.mark.parametrize("master", [False, True], ids=["bf16-state", "master-weights"])
def test_adam_consumed_these_gradients(gpu, master):
    """bf16, active aux steps: parameters (master mode: the masters) and both moments are cc_adam_step of the previous
    state with the stored gradients and clip_out[0], bit for bit."""
    B, h = 96, 256
    dead = torch.zeros(h, dtype=torch.bool)
    dead[::3] = True
    tr = trainer_of(aux_cfg(B, h, "bf16", 8, lr=1e-2, master_weights=master), batches_of(B, "bf16", 2), tsf_of(dead))
    o, a = tr.optimizer, tr.crosscoder.arena()
    assert o.master_mode == master
    for s in range(2):
        settle(tr)
        p0 = (o.master_for_update() if master else a).data.clone()
        m0, v0 = o.exp_avg.data.clone(), o.exp_avg_sq.data.clone()
        lr = o.param_groups[0]["lr"]
        tr.step()
        settle(tr)
        assert tr._last_ws.sparse and tr._last_ws.aux_active
        g = o.grads.data
        b1, b2 = o.param_groups[0]["betas"]
        ops.adam_step(p0, g.float() if master else g, m0, v0, tr._last_ws.clip_out[0:1], lr, b1, b2,
                      o.param_groups[0]["eps"], o.t)
        torch.cuda.synchronize()
        now = (o.master if master else a).data
        assert torch.equal(bits(now), bits(p0)), (s, int((bits(now) != bits(p0)).sum()))
        assert torch.equal(bits(o.exp_avg.data), bits(m0)) and torch.equal(bits(o.exp_avg_sq.data), bits(v0)), s
        if master:
            assert torch.equal(bits(a.data), bits(o.master.data.to(torch.bfloat16))), s


class _CountingLib:
    """The loaded library with every call of an entry point that returns a status (the launching ones) logged"""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int and name != "cc_version":
            def wrapper(*a, _fn=fn, _name=name):
                self._log.append(_name)
                return _fn(*a)
            return wrapper
        return fn


def test_nothing_dead_is_the_plain_sparse_step_plus_the_dead_update(gpu, monkeypatch):
    """Three steps with nothing dead: the parameters and the loss dict's shared keys are the aux-less sparse trainer's bit
    for bit, auxk_loss is 0.0 and dead_latents 0; the third step calls the entry points of that trainer's third step plus
    cc_dead_update, and allocates what it allocates."""
    B, h, steps = 96, 256, 3
    batches = batches_of(B, "bf16", steps)

    def run(aux):
        tr = trainer_of(aux_cfg(B, h, "bf16", 8, aux=aux, dead_tokens=10 ** 12) if aux else
                        aux_cfg(B, h, "bf16", 8, aux=False), batches)
        out, log, allocs = [], [], 0
        for s in range(steps):
            if s == steps - 1:
                settle(tr)
                monkeypatch.setattr(_lib, "_lib", _CountingLib(_lib.load(), log))
                allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
            dct = tr.step()
            if s == steps - 1:
                allocs = torch.cuda.memory_stats()["allocation.all.allocated"] - allocs
                monkeypatch.undo()
            settle(tr)
            out.append((dct, [getattr(tr.crosscoder, p).detach().clone() for p in O.PARAM_ORDER]))
        return out, log, allocs

    (plain, log0, al0), (aux, log1, al1) = run(False), run(True)
    for s, ((d0, p0), (d1, p1)) in enumerate(zip(plain, aux)):
        assert len(d0) == 9 and len(d1) == 11 and d1["auxk_loss"] == 0.0 and d1["dead_latents"] == 0
        for key in d0:
            assert d0[key] == d1[key], (s, key)
        for name, a, b in zip(O.PARAM_ORDER, p0, p1):
            assert torch.equal(bits(a), bits(b)), (s, name)
    assert len(log0) > 5 and "cc_pairs_wgrad" in log0 and "cc_dead_update" not in log0
    rest = list(log1)
    rest.remove("cc_dead_update")
    assert rest == log0, (log0, log1)
    assert al1 == al0, (al0, al1)


@pytest.mark.parametrize("skew", [False, True], ids=["plain", "skewed"])
def test_steps_with_dead_latents_are_reproducible(gpu, skew):
    """Two trainers, 3 steps, bf16, dead latents present in every step: equal loss dicts and equal bits of all four
    parameters.  skewed: the sparse step's skewed case -- latent 3 in every row (a list of two full pieces and a rest),
    24 silent latents, starved rows -- with latent 3 and the silent latents dead at the start: latent 3 sits in both
    supports in step 0 and is revived by it; the silent ones stay dead."""
    B, n, d, h, k = SKEW if skew else (288, N, D_IN, 200, K_MAIN)
    cfg = small_cfg(B, d, h, "bf16", "cuda:0", l1_coeff=0.0, activation="topk", k=k, sparse_step=True, auxk_compact=True,
                    auxk_coeff=1.0 / 32, k_aux=8, dead_tokens=DEAD_AFTER, lr=1e-2)
    dead = torch.zeros(h, dtype=torch.bool)
    dead[h - 24:] = True
    dead[3] = True
    dead[10::9] = True
    g = torch.Generator().manual_seed(9)
    batches = [torch.randn(B, n, d, generator=g).to(torch.bfloat16) for _ in range(3)]

    def run():
        tr = trainer_of(cfg, batches, tsf_of(dead), b_enc=skew_b_enc(h) if skew else None)
        out = []
        for s in range(3):
            dct = tr.step()
            settle(tr)
            ws, st = tr._last_ws, tr.auxk_state()
            assert not (skew or s == 0) or (ws.aux_active and dct["auxk_loss"] > 0), s
            if skew and s == 0:
                ref.assert_skewed(ws.pair_idx.cpu(), h, k)
                M, A = scattered_pairs(ws, h) > 0, st["aux_acts"] > 0
                assert bool(M[:, 3].all()) and bool(A[:, 3].any()) and bool(st["dead"][3])     # both supports
                assert int(tr.tokens_since_fired[3]) == 0 and bool((tr.tokens_since_fired[h - 24:] >= DEAD_AFTER).all())
            if skew and s == 1:
                assert not bool(st["dead"][3]) and bool(st["dead"][h - 24:].all())               # revived; still dead
            out.append((dct, [getattr(tr.crosscoder, p).detach().clone() for p in O.PARAM_ORDER],
                        tr.tokens_since_fired.clone()))
        return out

    a, b = run(), run()
    for s, ((d0, p0, t0), (d1, p1, t1)) in enumerate(zip(a, b)):
        assert d0 == d1, (s, d0, d1)
        assert torch.equal(t0, t1)
        for name, x, y in zip(O.PARAM_ORDER, p0, p1):
            assert torch.equal(bits(x), bits(y)), (s, name, int((bits(x) != bits(y)).sum()))
    assert not torch.equal(a[0][1][0], a[2][1][0])


def test_capacity_growth_gives_the_bits_of_a_large_start(gpu):
    """h = 256 starts with room for 8 dead latents.  Five are dead in step 0; before step 1 the dead set grows to 30
    through the setter and the capacity to 32; a trainer that started with room for every latent walks the same bits."""
    B, h, steps = 96, 256, 3
    batches = batches_of(B, "bf16", steps)
    first, second = dead_set("five", h), torch.zeros(h, dtype=torch.bool)
    second[torch.arange(1, h, 8)[:30]] = True
    cfg = aux_cfg(B, h, "bf16", 8, lr=1e-2)

    def run(large):
        tr = trainer_of(cfg, batches, tsf_of(first))
        ws = tr._sparse_workspace(B, tr.crosscoder.arena())
        assert ws.aux_cap == h // engine.AUX_CAP_FRACTION == 8
        if large:
            assert ws.aux_reserve(h) and ws.aux_cap == h
        out, caps = [], []
        for s in range(steps):
            if s == 1:
                settle(tr)
                tr.tokens_since_fired = tsf_of(second)
            dct = tr.step()
            settle(tr)
            assert tr._last_ws is ws and (ws.aux_active or s == 2)
            if ws.aux_active:   # the device's count is the host's, which sized the step
                assert tr.auxk_state()["compact_count"] == ws.aux_D == (5, 30, ws.aux_D)[s]
            caps.append(ws.aux_cap)
            out.append((dct, [getattr(tr.crosscoder, p).detach().clone() for p in O.PARAM_ORDER]))
        return out, caps

    (small, caps_s), (big, caps_b) = run(False), run(True)
    assert caps_s[0] == 8 and caps_s[1] == 32 and caps_s[2] >= 32 and caps_b == [h] * steps     # grew, never shrank
    for s, ((d0, p0), (d1, p1)) in enumerate(zip(small, big)):
        assert d0 == d1, (s, d0, d1)
        for name, x, y in zip(O.PARAM_ORDER, p0, p1):
            assert torch.equal(bits(x), bits(y)), (s, name)


def test_revives_dead_latents(gpu):
    """tests/test_gpu_auxk.py::test_revives_dead_latents on the sparse step: 16 latents whose encoder rows are scaled by
    1/64 never reach a row's top 32.  The control, the sparse step without AuxK, gives their encoder rows a gradient of
    exactly zero in every step: they stay dead.  With the aux loss (dead_tokens = B) step 0 sees nothing dead; its dead
    update marks them, and from step 1 on the aux loss is positive and every one of the 16 rows has a gradient."""
    B, n, d, h, k, steps = 256, 2, 64, 512, 32, 4
    chosen = torch.arange(5, 5 + 16 * 31, 31)
    g = torch.Generator().manual_seed(11)
    batches = [torch.randn(B, n, d, generator=g).to(torch.bfloat16) for _ in range(steps)]

    def run(**kw):
        cfg = small_cfg(B, d, h, "bf16", "cuda:0", l1_coeff=0.0, activation="topk", k=k, sparse_step=True, **kw)
        cc = ca.CrossCoder(cfg, n_models=n)
        with torch.no_grad():
            cc.W_enc[:, :, chosen.to("cuda:0")] *= 1.0 / 64
        tr = ca.Trainer(cfg, buffer=FixedBatches(batches, "cuda:0"), crosscoder=cc)
        out = []
        for _ in range(steps):
            dct = tr.step()
            settle(tr)
            gr = tr.optimizer.grads.views()
            sel = scattered_pairs(tr._last_ws, h) > 0
            out.append({"dict": dct, "selected": bool(sel[:, chosen.to("cuda:0")].any()),
                        "W_enc": gr["W_enc"][:, :, chosen.to("cuda:0")].cpu().clone(),
                        "b_enc": gr["b_enc"][chosen.to("cuda:0")].cpu().clone()})
        return out

    for s, rec in enumerate(run()):
        assert not rec["selected"] and len(rec["dict"]) == 9, s
        assert not bool(bits(rec["W_enc"]).any()) and not bool(bits(rec["b_enc"]).any()), s
    a = run(auxk_coeff=1.0 / 32, auxk_compact=True, dead_tokens=B)
    assert a[0]["dict"]["auxk_loss"] == 0.0 and not bool(bits(a[0]["W_enc"]).any())
    assert a[0]["dict"]["dead_latents"] >= 16
    for s in range(1, steps):
        assert not a[s]["selected"], s
        assert a[s]["dict"]["auxk_loss"] > 0.0 and a[s]["dict"]["dead_latents"] >= 16, s
        assert bool((a[s]["W_enc"].float().abs().sum((0, 1)) > 0).all()), s
        assert bool((a[s]["b_enc"].float().abs() > 0).all()), s
