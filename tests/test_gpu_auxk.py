"""The AuxK dead-latent loss on the GPU: cc_auxk_rows, cc_dead_update, cc_auxk_loss and cc_add_rows against the
pure-torch reference of tests/_auxk_ref.py, then the step's gradients with the GPU's masks imposed, and the Trainer:
off means off, and it revives latents the plain TopK step leaves without gradient for good."""
import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _hip, ops
from oracle import cpu_reference as O
from tests._auxk_ref import aux_select, auxk_loss_ref, dead_update_ref, g_aux_ref, step_loss_ref
from tests._golden import load
from tests._topk_ref import topk_order, topk_ref

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
PAD = 7.0  # what the columns at or beyond h hold
SHAPES = [(70, 512, 520), (40, 2056, 2056), (24, 16384, 16384), (12, 24576, 24576)]  # one per instantiation
DEAD_AFTER = 1000


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


def make_input(kind, B, h, dtype, seed):
    """The four kinds of input of the top-k kernel's own test (restated)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "equal":
        return torch.full((B, h), 1.5, dtype=dtype)
    if kind == "sparse":  # rows with few eligible values, row 0 all zero
        v = -torch.rand(B, h, generator=g)
        dens = [0.0, 1.0 / h, 0.01, 0.1, 0.5]
        for b in range(B):
            on = torch.rand(h, generator=g) < dens[b % len(dens)]
            v[b] = torch.where(on, torch.rand(h, generator=g) + 0.01, v[b])
        v[0] = 0.0
        if B > 1:
            v[1, h // 2] = 2.0
        return v.to(dtype)
    if kind == "bits":  # uniformly random finite positive bit patterns: every digit, subnormals
        hi = 0x7F80 if dtype == torch.bfloat16 else 0x7F800000
        return torch.randint(1, hi, (B, h), generator=g, dtype=torch.int64).to(BITS[dtype]).view(dtype)
    if kind == "special":  # +inf, NaN, -0.0, negatives, subnormals among ordinary values
        v = torch.randn(B, h, generator=g).to(dtype)
        tiny = torch.tensor([1], dtype=BITS[dtype]).view(dtype)
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


def dead_sets(h):
    """name -> bool [h]: none, all, every third, fewer than k_aux = 33, exactly the columns one lane owns (lane 37 of
    a workgroup of 256 threads for h <= 2048, else of 1024: 8 consecutive columns in every chunk of 8 x threads)."""
    col = torch.arange(h)
    few = torch.zeros(h, dtype=torch.bool)
    few[torch.randperm(h, generator=torch.Generator().manual_seed(h))[:20]] = True
    chunk = 8 * (256 if h <= 2048 else 1024)
    return {"none": torch.zeros(h, dtype=torch.bool), "all": torch.ones(h, dtype=torch.bool), "third": col % 3 == 0,
            "few": few, "lane": (col % chunk) // 8 == 37}


def run_auxk_rows(buf, h, k_aux, tsf):
    B, ld = buf.shape
    out = torch.full((B, ld), PAD, dtype=buf.dtype, device=buf.device)
    rc = torch.full((B,), -7, dtype=torch.int32, device=buf.device)
    ops.auxk_rows(buf, h, k_aux, tsf, DEAD_AFTER, out=out, row_count=rc)
    return out, rc


# ----------------------------------------------------------------------------- 1. cc_auxk_rows, bit for bit
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", SHAPES)
def test_auxk_rows_matches_reference(gpu, B, h, ld, dtype):
    dt = DT[dtype]
    sets = dead_sets(h)
    for kind in ("equal", "sparse", "bits", "special"):
        v = make_input(kind, B, h, dt, seed=B + h)
        buf = torch.full((B, ld), PAD, dtype=dt, device=gpu)
        buf[:, :h] = v.to(gpu)
        for name, dead in sets.items():
            # counts on both sides of the threshold, the threshold itself included
            tsf = torch.where(dead, torch.tensor(DEAD_AFTER) + (torch.arange(h) % 3) * 1000,
                              (torch.arange(h) * 7) % DEAD_AFTER).to(torch.int64).to(gpu)
            order = topk_order(torch.where(dead[None, :], v, torch.zeros((), dtype=dt)))
            for k_aux in (1, 33, h):
                what = (kind, name, k_aux)
                ref = topk_ref(torch.where(dead[None, :], v, torch.zeros((), dtype=dt)), k_aux, order)
                out, rc = run_auxk_rows(buf, h, k_aux, tsf)
                assert torch.equal(bits(out[:, :h].cpu()), bits(ref["dense"])), what
                assert torch.equal(rc.cpu().long(), ref["count"]), what
                assert not bool(ref["mask"][:, ~dead].any()) and bool((ref["count"] <= k_aux).all())
                if ld > h:
                    assert bool((out[:, h:] == PAD).all()), (what, "padding columns written")
                    assert bool((buf[:, h:] == PAD).all())
                assert torch.equal(bits(buf[:, :h].cpu()), bits(v)), (what, "input changed")
                if name == "all":  # the bits of cc_topk_rows for k = k_aux
                    plain = torch.full((B, ld), PAD, dtype=dt, device=gpu)
                    ops.topk_rows(buf, h, k_aux, out=plain)
                    assert torch.equal(bits(out), bits(plain)), what
                if name == "none":
                    assert int(rc.abs().sum()) == 0
                if k_aux == 33:
                    out2, rc2 = run_auxk_rows(buf, h, k_aux, tsf)
                    assert torch.equal(bits(out), bits(out2)) and torch.equal(rc, rc2), (what, "two calls")
    assert aux_select(v, sets["third"], 33)["count"].sum().item() > 0  # (the shared reference selects something)


# ----------------------------------------------------------------------------- 2. cc_dead_update, exactly
@pytest.mark.parametrize("h,h_real", [(200, 197), (16384, 16384)])
def test_dead_update_matches_reference(gpu, h, h_real):
    g = torch.Generator().manual_seed(h)
    B, dead_after = 96, 1000
    colsum = torch.rand(h, generator=g)
    pick = torch.randint(0, 4, (h,), generator=g)
    colsum[pick == 0] = 0.0
    colsum[pick == 1] = torch.tensor([1], dtype=torch.int32).view(torch.float32)  # the smallest subnormal
    colsum[pick == 2] = float("inf")
    colsum[h_real:] = 0.0  # padding latents never fire
    # old counts around dead_after - B (the update crosses the threshold or not) and around dead_after itself
    tsf = torch.stack([torch.randint(dead_after - B - 2, dead_after - B + 3, (h,), generator=g),
                       torch.randint(dead_after - 2, dead_after + 3, (h,), generator=g),
                       torch.randint(0, 3, (h,), generator=g)])[torch.randint(0, 3, (h,), generator=g), torch.arange(h)]
    tsf[h_real:] = 10 * dead_after  # dead, and not to be counted
    new, count, was = dead_update_ref(colsum, tsf, B, dead_after, h_real)
    assert 0 < count < h_real and 0 < int(was.sum()) < h
    host = _hip.MappedHostBuffer(16)
    d_tsf, d_count = tsf.to(gpu), torch.full((1,), -1, dtype=torch.int32, device=gpu)
    d_was = torch.full((h,), 9, dtype=torch.uint8, device=gpu)
    ops.dead_update(colsum.to(gpu), d_tsf, h_real, B, dead_after, d_count, was_dead=d_was,
                    host_ptr=host.device_ptr.value + 4 * 10)
    torch.cuda.synchronize()
    assert torch.equal(d_tsf.cpu(), new)
    assert int(d_count) == count and int(host.u32[10]) == count
    assert torch.equal(d_was.cpu().bool(), was)
    assert not bool(host.u32[:10].any()) and not bool(host.u32[11:].any())  # one word


# ----------------------------------------------------------------------------- 3. cc_auxk_loss against fp64
def loss_inputs(B, n, d, dtype, seed):
    """A residual whose column means are about its standard deviation (the centred denominator matters)."""
    g = torch.Generator().manual_seed(seed)
    K = n * d
    x = (torch.randn(B, K, generator=g) + 1.0).to(dtype)
    recon = 0.3 * torch.randn(B, K, generator=g)
    b_dec = (0.1 * torch.randn(K, generator=g)).to(dtype)
    ehat = 0.5 * torch.randn(B, K, generator=g)
    return recon, b_dec, x, ehat


def run_auxk_loss(recon, b_dec, x, ehat, coeff, gpu):
    B, K = x.shape
    host = _hip.MappedHostBuffer(16)
    part = torch.full((ops.auxk_part_floats(B, K),), float("nan"), device=gpu)
    sc = torch.full((4,), float("nan"), device=gpu)
    g_aux = torch.full((B, K), 3.0, dtype=x.dtype, device=gpu)
    ops.auxk_loss(recon.to(gpu), b_dec.to(gpu), x.to(gpu), ehat.to(gpu), g_aux, part, sc, coeff,
                  host_ptr=host.device_ptr.value + 4 * 9)
    torch.cuda.synchronize()
    return sc.cpu(), g_aux.cpu(), float(host.f32[9])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B,n,d", [(96, 2, 40), (256, 2, 64)])
def test_auxk_loss_matches_fp64(gpu, B, n, d, dtype):
    dt, coeff = DT[dtype], 1.0 / 32
    recon, b_dec, x, ehat = loss_inputs(B, n, d, dt, seed=B + d)
    e64 = x.double() - (recon.double() + b_dec.double())
    assert 0.5 < (e64.mean(0).abs().mean() / e64.std(0).mean()).item() < 2.0
    loss, den, valid = auxk_loss_ref(e64, ehat.double())
    g64 = g_aux_ref(e64, ehat.double(), coeff, torch.float64)
    sc, g_aux, host_loss = run_auxk_loss(recon, b_dec, x, ehat, coeff, gpu)
    e_loss, e_den = abs(sc[0].item() - loss.item()) / loss.item(), abs(sc[1].item() - den.item()) / den.item()
    print(dtype, B, "auxk_loss rel", e_loss, "den rel", e_den, "g_aux rel", rel(g_aux, g64))
    # the scalars are fp32 sums of the same dtype-rounded inputs in either dtype: the fp32 bound
    assert valid and e_loss < 2e-5 and e_den < 2e-5
    assert sc[3].item() == 1.0 and host_loss == sc[0].item()
    assert abs(sc[2].item() - 2 * coeff / (B * den.item())) < 2e-5 * sc[2].item()
    if dt == torch.float32:
        assert rel(g_aux, g64) < 2e-5
    else:  # the same arithmetic on the CPU, in fp32 from the bf16 inputs, rounded to bf16
        e32 = x.float() - (recon + b_dec.float())
        cpu = g_aux_ref(e32, ehat, coeff, torch.bfloat16)
        e_ours, e_cpu = rel(g_aux, g64), rel(cpu, g64)
        print("bf16 g_aux (ours, cpu) vs fp64", e_ours, e_cpu)
        assert e_ours <= 2 * e_cpu + 5e-3


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["den0", "nan", "zero"])
def test_auxk_loss_forced_to_zero(gpu, dtype, case):
    dt = DT[dtype]
    recon, b_dec, x, ehat = loss_inputs(96, 2, 40, dt, seed=7)
    if case == "den0":  # a dyadic constant residual per column: every sum is exact, den is exactly 0, num is not
        x = torch.full_like(x, 0.5) * (1 + torch.arange(80) % 4).to(dt)
        recon, b_dec = torch.zeros_like(recon), torch.zeros_like(b_dec)
        x, recon = x[:64].contiguous(), recon[:64].contiguous()
        ehat = ehat[:64].contiguous()
    elif case == "nan":
        ehat[17, 33] = float("nan")
    else:
        x, recon, b_dec, ehat = torch.zeros_like(x), torch.zeros_like(recon), torch.zeros_like(b_dec), ehat * 0
    sc, g_aux, host_loss = run_auxk_loss(recon, b_dec, x, ehat, 1.0 / 32, gpu)
    assert sc[0].item() == 0.0 and host_loss == 0.0 and sc[2].item() == 0.0 and sc[3].item() == 0.0
    assert not bool(bits(g_aux).any())  # all +0
    if case == "den0":
        assert sc[1].item() == 0.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_add_rows(gpu, dtype):
    dt = DT[dtype]
    g = torch.Generator().manual_seed(3)
    full = torch.randn(2 * 70, 520, generator=g).to(dt).to(gpu)
    want = (full[:70, :512].float() + full[70:, :512].float()).to(dt)
    before = full.clone()
    ops.add_rows(full[:70, :512], full[70:, :512])
    assert torch.equal(bits(full[:70, :512]), bits(want))
    assert torch.equal(bits(full[70:]), bits(before[70:])) and torch.equal(bits(full[:70, 512:]), bits(before[:70, 512:]))


# ----------------------------------------------------------------------------- the step
class FixedBatches:
    """Buffer protocol over given batches (already in the parameter dtype, no normalisation)."""
    normalize = False

    def __init__(self, batches, device):
        self.batches = [b.to(device) for b in batches]
        self.i = 0

    def next_raw(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        return b, None


def make_cc(cfg, P, device, n_models):
    cc = ca.CrossCoder(dict(cfg, device=str(device)), n_models=n_models)
    cc.load_state_dict({k: v for k, v in P.items()})
    return cc


def one_step(r, gpu, activation, auxk_coeff, tsf=None):
    """One Trainer.step on the fixture's first batch, past the L1 warm-up -> (trainer, loss dict, grads on the CPU)."""
    cfg, P, n = r["cfg"], r["init"], r["n_models"]
    dt = O.DTYPES[cfg["enc_dtype"]]
    cfg = dict(cfg, activation=activation, k=32, k_aux=64, dead_tokens=DEAD_AFTER, num_tokens=cfg["batch_size"] * 100)
    if auxk_coeff:
        cfg["auxk_coeff"] = auxk_coeff
    cc = make_cc(cfg, P, gpu, n)
    tr = ca.Trainer(dict(cfg, device=str(gpu)), buffer=FixedBatches([r["x"][0].to(dt)], gpu), crosscoder=cc)
    tr.step_counter = 50  # past the warm-up ramp: l1_coeff in full
    if tsf is not None:
        tr.tokens_since_fired = tsf
    dct = tr.step()
    tr.synchronize()
    torch.cuda.synchronize()
    return tr, dct, {k: v.detach().cpu().clone() for k, v in tr.optimizer.grads.views().items()}


# ----------------------------------------------------------------------------- 4. gradients, the GPU's masks imposed
@pytest.mark.parametrize("activation", ["topk", "batch_topk"])
@pytest.mark.parametrize("name", ["step_b256_n2_d64_h512_bf16", "step_b96_n2_d40_h200_bf16",
                                  "step_b256_n2_d64_h512_fp32", "step_b96_n2_d40_h200_fp32"])
def test_step_gradients_with_the_gpu_masks(gpu, name, activation):
    """With M = (the step's masked activations > 0) and A = (its aux activations > 0) imposed on the reference
    objective, only arithmetic differs, so the bounds of the TopK step's own gradient test carry over: bf16 error
    against fp64 <= 2 x the CPU-bf16 error + 5e-3 (2e-3 for the loss), fp32 rel < 2e-5."""
    r = load(name)
    cfg, P, x = r["cfg"], r["init"], r["x"][0]
    dt = O.DTYPES[cfg["enc_dtype"]]
    h, coeff, l1c = cfg["dict_size"], 1.0 / 32, float(cfg["l1_coeff"])
    # the main mask of this very step, from a run without the aux loss (the same launches up to the mask)
    tr0, d0, g0 = one_step(r, gpu, activation, 0)
    M0 = (tr0._last_ws.acts[:, :h] > 0).cpu()
    assert len(d0) == 9
    fired = M0.any(0)
    # dead: every latent the main mask selects in no row (at these shapes there may be none), plus every third latent,
    # which the main mask selects in some rows (the overlap, where the gradients add) and not in others
    tsf = torch.where(fired, torch.zeros(h, dtype=torch.int64), torch.full((h,), DEAD_AFTER, dtype=torch.int64))
    tsf[::3] = DEAD_AFTER + 5
    tsf[1::3][fired[1::3]] = DEAD_AFTER - 1  # (live, just below the threshold)
    tr, dct, g = one_step(r, gpu, activation, coeff, tsf=tsf)
    ws, st = tr._last_ws, tr.auxk_state()
    M, A = (ws.acts[:, :h] > 0).cpu(), (st["aux_acts"] > 0).cpu()
    dead = st["dead"].cpu()
    assert ws.aux_active and torch.equal(M, M0) and torch.equal(dead, tsf >= DEAD_AFTER)
    assert not bool(A[:, ~dead].any()) and int(A.sum()) > 0
    assert bool((A.sum(1) <= 64).all()) and torch.equal(st["row_count"].cpu().long(), A.sum(1))
    assert int((A & M).sum()) > 0  # elements in both supports: the gradients add
    assert int((A & ~M).sum()) > 0  # and elements only the aux loss reaches
    assert len(dct) == 11 and dct["dead_latents"] == st["dead_latents"] and dct["auxk_loss"] == st["auxk_loss"]
    # nothing flows into b_dec: the gradient of the same step without the aux loss, bit for bit
    assert torch.equal(bits(g["b_dec"]), bits(g0["b_dec"]))
    for key in ("W_enc", "b_enc", "W_dec"):
        assert not torch.equal(g[key], g0[key]), key

    def oracle(dtype):
        leaves = {key: v.detach().to(dtype).clone().requires_grad_(True) for key, v in P.items()}
        total, parts = step_loss_ref(x.to(dt).to(dtype), leaves, M, A, l1c, coeff)
        total.backward()
        return parts, {key: leaves[key].grad for key in O.PARAM_ORDER}

    ref, gref = oracle(dt)
    truth, gtruth = oracle(torch.float64)
    ours = torch.tensor(dct["auxk_loss"])
    if dt == torch.float32:
        e = rel(ours, truth["auxk_loss"].detach())
        print(name, activation, "auxk_loss rel", e)
        assert e < 2e-5, e
        assert abs(dct["loss"] - (dct["l2_loss"] + l1c * dct["l1_loss"] + coeff * dct["auxk_loss"])) <= 1e-6 * dct["loss"]
    else:
        e_ours, e_ref = rel(ours, truth["auxk_loss"].detach()), rel(ref["auxk_loss"].detach().float(),
                                                                    truth["auxk_loss"].detach())
        print(name, activation, "auxk_loss (ours, cpu) vs fp64", e_ours, e_ref)
        assert e_ours <= 2 * e_ref + 2e-3, (e_ours, e_ref)
    for key in O.PARAM_ORDER:
        assert g[key].shape == gref[key].shape and g[key].dtype == gref[key].dtype, key
        if dt == torch.float32:
            e = rel(g[key], gtruth[key])
            print(name, activation, key, "grad rel", e)
            assert e < 2e-5, (key, e)
        else:
            e_ours, e_ref = rel(g[key], gtruth[key]), rel(gref[key], gtruth[key])
            print(name, activation, key, "grad (ours, cpu) vs fp64", e_ours, e_ref)
            assert e_ours <= 2 * e_ref + 5e-3, (key, e_ours, e_ref)


# ----------------------------------------------------------------------------- 5. off means off
def small_cfg(B, d, h, dev, **kw):
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": B * 100, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000, "activation": "topk", "k": 32}
    cfg.update(kw)
    return cfg


def test_off_means_off(gpu):
    """With nothing dead the aux trainer issues the plain step's launches plus the dead update: the same parameters
    and loss values as a trainer without the keys, bit for bit."""
    B, n, d, h, steps = 256, 2, 64, 512, 3

    def run(**kw):
        cfg = small_cfg(B, d, h, gpu, **kw)
        cc = ca.CrossCoder(cfg, n_models=n)
        tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * steps, n_models=n, seed=3), crosscoder=cc)
        out = []
        for _ in range(steps):
            dct = tr.step()
            tr.synchronize()
            # snapshot after a device synchronise, as the identity tests do: what is compared is the parameters the
            # steps walk, not how a reader on torch's stream is ordered after the side-stream Adam
            torch.cuda.synchronize()
            out.append((dct, [getattr(cc, p).detach().clone() for p in O.PARAM_ORDER]))
        return out

    plain = run()
    aux = run(auxk_coeff=1.0 / 32, dead_tokens=10 ** 12)
    for step, ((d0, p0), (d1, p1)) in enumerate(zip(plain, aux)):
        assert len(d0) == 9 and len(d1) == 11
        assert d1["auxk_loss"] == 0.0 and d1["dead_latents"] == 0
        for key in d0:
            assert d0[key] == d1[key], (step, key, d0[key], d1[key])
        for name, a, b in zip(O.PARAM_ORDER, p0, p1):
            assert torch.equal(bits(a), bits(b)), (step, name)


# ----------------------------------------------------------------------------- 6. it revives what the plain step cannot
def test_revives_dead_latents(gpu):
    """16 latents whose encoder rows are scaled by 1/64 are positive on some rows yet never in a row's top 32: with
    l1_coeff = 0 the plain TopK step gives their encoder rows a gradient of exactly zero, for good.  With the aux
    loss (dead_tokens = B) step 0 sees nothing dead and reports 0.0; its dead update marks the 16 dead, so from step 1
    on -- the first step whose dead set, the state step 0 left, holds them -- the aux loss is positive and their
    gradient rows are not zero."""
    B, n, d, h, k, steps = 256, 2, 64, 512, 32, 4
    chosen = torch.arange(5, 5 + 16 * 31, 31)
    g = torch.Generator().manual_seed(11)
    batches = [torch.randn(B, n, d, generator=g).to(torch.bfloat16) for _ in range(steps)]

    def run(**kw):
        cfg = small_cfg(B, d, h, gpu, l1_coeff=0.0, **kw)
        cc = ca.CrossCoder(cfg, n_models=n)
        with torch.no_grad():
            cc.W_enc[:, :, chosen.to(gpu)] *= 1.0 / 64
        tr = ca.Trainer(cfg, buffer=FixedBatches(batches, gpu), crosscoder=cc)
        out = []
        for _ in range(steps):
            before = {key: getattr(cc, key).detach().cpu().clone() for key in O.PARAM_ORDER}
            dct = tr.step()
            tr.synchronize()
            torch.cuda.synchronize()
            gr = tr.optimizer.grads.views()
            out.append({"dict": dct, "params": before, "W_enc": gr["W_enc"][:, :, chosen.to(gpu)].cpu().clone(),
                        "b_enc": gr["b_enc"][chosen.to(gpu)].cpu().clone(),
                        "tsf": tr.tokens_since_fired.cpu().clone() if kw else None})
        return out

    plain = run()
    for step, rec in enumerate(plain):
        # the reference, on the CPU, from the parameters the step started from: positive on some rows, in no top 32
        acts = O.encode(batches[step], rec["params"])
        sel = topk_ref(acts, k)
        assert bool((acts[:, chosen] > 0).any(0).all()), step
        assert not bool(sel["mask"][:, chosen].any()), step
        assert bool((sel["count"] == k).all())
        kth = torch.where(sel["mask"], acts.float(), torch.full((), float("inf"))).min(1).values
        assert bool((acts[:, chosen].float().max(1).values < 0.25 * kth).all()), step  # (far from the boundary)
        # the control: exactly zero, every step
        assert not bool(rec["W_enc"].view(torch.int16).any()) and not bool(rec["b_enc"].view(torch.int16).any()), step
        assert len(rec["dict"]) == 9
    a, b = run(auxk_coeff=1.0 / 32, dead_tokens=B), run(auxk_coeff=1.0 / 32, dead_tokens=B)
    for step, rec in enumerate(a):  # (the aux run's own parameters: still in no row's top 32)
        assert not bool(topk_ref(O.encode(batches[step], rec["params"]), k)["mask"][:, chosen].any()), step
    assert a[0]["dict"]["auxk_loss"] == 0.0
    assert not bool(a[0]["W_enc"].view(torch.int16).any())
    assert bool((a[0]["tsf"][chosen] >= B).all()) and a[0]["dict"]["dead_latents"] >= 16
    for step in range(1, steps):
        assert a[step]["dict"]["auxk_loss"] > 0.0, step
        assert a[step]["dict"]["dead_latents"] >= 16
        assert bool((a[step]["W_enc"].float().abs().sum((0, 1)) > 0).all()), step  # every one of the 16 rows
        assert bool((a[step]["b_enc"].float().abs() > 0).all()), step
    for ra, rb in zip(a, b):  # two identical runs, identical bits
        assert ra["dict"] == rb["dict"]
        assert torch.equal(bits(ra["W_enc"]), bits(rb["W_enc"])) and torch.equal(bits(ra["b_enc"]), bits(rb["b_enc"]))
        assert torch.equal(ra["tsf"], rb["tsf"])
        for key in O.PARAM_ORDER:
            assert torch.equal(bits(ra["params"][key]), bits(rb["params"][key])), key
