"""JumpReLU crosscoders on the GPU: the two streaming kernels (cc_jumprelu_mask, cc_jumprelu_bwd) against the
pure-torch reference of tests/_jumprelu_ref.py, then the model, the losses and the five gradients, the Trainer and
the refusals built on them."""
import math

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import engine, ops
from oracle import cpu_reference as O
from tests import _jumprelu_ref as R
from tests._golden import load
from tests.test_gpu_parity import _Replay, _bf16_ulp, envelope_ok, make_cc, rel
from tests.test_gpu_topk import DT, PAD, bits, make_input, small_cfg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (3, 200, 200), (130, 512, 520), (4, 16384, 16384), (600, 2056, 2056)]
# per-latent thresholds, cycled over the latents: <= 0 (plain ReLU), a subnormal, ordinary ones, far above everything
THETAS = [-1.0, 0.0, 1e-40, 1e-3, 0.5, 1.0, 7.5, 1e20, 0.0625]


def thetas_for(h, shift=0):
    t = torch.tensor(THETAS, dtype=torch.float32)
    return t[(torch.arange(h) + shift) % len(THETAS)].contiguous()


def run_mask(v, ld, theta, eps, inplace=False, gate=True):
    """v [B, h] in a [B, ld] buffer whose other columns hold PAD -> every output of cc_jumprelu_mask."""
    B, h = v.shape
    dev = torch.device("cuda:0")
    buf = torch.full((B, ld), PAD, dtype=v.dtype, device=dev)
    buf[:, :h] = v.to(dev)
    out = buf if inplace else torch.full((B, ld), PAD, dtype=v.dtype, device=dev)
    gt = torch.full((B, ld), PAD, dtype=v.dtype, device=dev) if gate else None
    part = torch.full((ops.jumprelu_part_rows(B, h), h), float("nan"), device=dev)
    l0 = torch.full((ops.jumprelu_l0_parts(B, h),), float("nan"), device=dev)
    ops.jumprelu_mask(buf, h, theta.to(dev), eps, out=out, gate=gt, colsum_part=part, l0_part=l0)
    colsum = torch.empty(h, device=dev)
    ops.reduce_rows(part, part.shape[0], h, out_f32=colsum)
    return {"out": out, "gate": gt, "part": part, "l0": l0, "colsum": colsum, "src": None if inplace else buf}


def run_bwd(g_in, gate_buf, ld, theta, eps, l0_scale):
    """g_in [B, h] in a [B, ld] buffer (PAD beyond h) and the mask kernel's gate buffer -> cc_jumprelu_bwd's outputs
    and theta.grad with its squared-sum partials from cc_reduce_rows."""
    B, h = g_in.shape
    dev = gate_buf.device
    g = torch.full((B, ld), PAD, dtype=g_in.dtype, device=dev)
    g[:, :h] = g_in.to(dev)
    rows = ops.jumprelu_part_rows(B, h)
    thr = torch.full((rows, h), float("nan"), device=dev)
    col = torch.full((rows, h), float("nan"), device=dev)
    ops.jumprelu_bwd(g, gate_buf, h, theta.to(dev), eps, l0_scale, gpre_colsum_part=col, thr_part=thr)
    grad = torch.empty(h, device=dev)
    sq = torch.empty(ops.reduce_parts(h), device=dev)
    ops.reduce_rows(thr, rows, h, out_t=grad, sq_part=sq)
    colsum = torch.empty(h, device=dev)
    ops.reduce_rows(col, rows, h, out_f32=colsum)
    return {"g": g, "thr": thr, "col": col, "grad": grad, "sq": sq, "colsum": colsum}


def sums_within_bound(got, terms64, B, what):
    """any fixed-order fp32 sum of B terms: |err| <= B 2^-24 sum_b |term| (columns whose sum fp32 cannot hold are
    left alone, a column that holds +inf sums to +inf)."""
    total = terms64.sum(0)
    got = got.double().cpu()
    fin = total.abs() < 3.0e38
    err = (got - total).abs()[fin]
    bound = B * 2.0 ** -24 * terms64.abs().sum(0)[fin]
    assert bool((err <= bound).all()), (what, (err - bound).max().item())
    inf = torch.isinf(total)
    assert torch.equal(got[inf], total[inf]), (what, "inf")


def check_kernels(v, ld, theta, eps, l0_scale, what, seed=0):
    """Everything both kernels write for (v, theta, eps), out of place and in place, against the reference; every
    output of a second launch has the same bits."""
    B, h = v.shape
    ref = R.jumprelu_ref(v, theta, eps)
    got = run_mask(v, ld, theta, eps)
    out, gate = got["out"].cpu(), got["gate"].cpu()
    assert torch.equal(bits(out[:, :h]), bits(ref["dense"])), (what, "kept rows")
    assert torch.equal(bits(gate[:, :h]), bits(ref["gate"])), (what, "gate")
    assert got["l0"].sum().item() == ref["count"].sum().item(), (what, "count")
    sums_within_bound(got["colsum"], ref["dense"].double(), B, (what, "colsum"))
    if ld > h:
        for key in ("out", "gate", "src"):
            assert bool((got[key][:, h:] == PAD).all().item()), (what, key, "padding columns written")
    assert torch.equal(bits(got["src"][:, :h].cpu()), bits(v)), (what, "input changed")
    inp = run_mask(v, ld, theta, eps, inplace=True)
    again = run_mask(v, ld, theta, eps)
    for other, name in ((inp, "in place"), (again, "second launch")):
        for key in ("out", "gate"):
            assert torch.equal(bits(other[key]), bits(got[key])), (what, name, key)
        for key in ("part", "l0", "colsum"):
            assert torch.equal(other[key].view(torch.int32), got[key].view(torch.int32)), (what, name, key)
    nogate = run_mask(v, ld, theta, eps, gate=False)  # inference: no gate
    assert torch.equal(bits(nogate["out"]), bits(got["out"])), (what, "no gate")
    # the backward pass: G3 leaves G (dtype-rounded) at the gated elements and 0 elsewhere
    G = torch.randn(B, h, generator=torch.Generator().manual_seed(seed + 17)).to(v.dtype)
    g_in = torch.where(ref["gated"], G, torch.zeros_like(G))
    b = run_bwd(g_in, got["gate"], ld, theta, eps, l0_scale)
    want_g = R.bwd_ref(g_in, ref)
    assert torch.equal(bits(b["g"][:, :h].cpu()), bits(want_g)), (what, "g_pre")
    if ld > h:
        assert bool((b["g"][:, h:] == PAD).all().item()), (what, "g_pre padding columns written")
    terms = R.theta_grad_terms(g_in, ref["window"], theta, eps, l0_scale)
    sums_within_bound(b["grad"], terms, B, (what, "theta.grad"))
    sums_within_bound(b["colsum"], want_g.double(), B, (what, "g_pre colsum"))
    if math.isfinite(b["sq"].sum().item()):  # segment 4 of the step's squared-sum slab
        assert math.isclose(b["sq"].sum().item(), b["grad"].double().pow(2).sum().item(), rel_tol=1e-5), what
    b2 = run_bwd(g_in, got["gate"], ld, theta, eps, l0_scale)
    assert torch.equal(bits(b2["g"]), bits(b["g"])), (what, "second launch", "g_pre")
    for key in ("thr", "col", "grad", "sq", "colsum"):
        assert torch.equal(b2[key].view(torch.int32), b[key].view(torch.int32)), (what, "second launch", key)
    return ref


# ----------------------------------------------------------------------------- 1. the kernels against the reference
@pytest.mark.parametrize("kind", ["bits", "special", "ordinary"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,h,ld", SHAPES)
def test_kernels_match_reference(gpu, B, h, ld, dtype, kind):
    """(3, 200, 200): a ragged h; (130, 512, 520): padding columns, which hold a positive sentinel; (4, 16384, 16384):
    the wide form (8 column blocks); (600, 2056, 2056): more rows than row groups, and a last column block of one
    lane.  Per-latent thresholds including <= 0; a bandwidth below and one above most of them."""
    if kind == "ordinary":  # activations as G1 leaves them, around the ordinary thresholds: full windows
        v = torch.relu(torch.randn(B, h, generator=torch.Generator().manual_seed(B + h)) * 0.6 + 0.3).to(DT[dtype])
    else:
        v = make_input(kind, B, h, DT[dtype], seed=B + h)
    for eps, shift in ((1e-3, 0), (4.0, 3), (0.125, 5)):
        theta = thetas_for(h, shift)
        ref = check_kernels(v, ld, theta, eps, 0.5 / B, (kind, eps), seed=B)
        assert not bool(ref["kept"][~(v > 0)].any())  # NaN, -0.0, zeros and negatives are never kept
        relu_cols = theta <= 0
        assert torch.equal(ref["kept"][:, relu_cols], (v > 0)[:, relu_cols])  # theta <= 0 is plain ReLU
        if kind == "ordinary" and B * h >= 600 and eps >= 0.125:
            assert ref["window"].any() and (ref["gated"] & ~ref["kept"]).any() and ref["kept"].any()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_boundaries_are_strict(gpu, dtype):
    """a == theta exactly is dropped but gated and in the window; d == -half is not gated; d == +half is kept and
    outside the window.  theta = 0.5, eps = 0.125: 0.4375, 0.5 and 0.5625 are exact in both dtypes."""
    B, h = 5, 64
    vals = torch.tensor([0.5, 0.4375, 0.5625, 0.46875, 0.53125, 0.0, 0.25, 2.0])
    v = vals[(torch.arange(h)[None, :] + torch.arange(B)[:, None]) % len(vals)].to(DT[dtype])
    theta = torch.full((h,), 0.5)
    ref = check_kernels(v, h, theta, 0.125, 0.25, "boundaries")
    f = v.float()
    assert not bool(ref["kept"][f == 0.5].any()) and bool(ref["gated"][f == 0.5].all()) and bool(ref["window"][f == 0.5].all())
    assert not bool(ref["gated"][f == 0.4375].any())
    assert bool(ref["kept"][f == 0.5625].all()) and not bool(ref["window"][f == 0.5625].any())
    assert bool(ref["window"][f == 0.46875].all()) and not bool(ref["kept"][f == 0.46875].any())
    assert bool((ref["window"] & ref["kept"])[f == 0.53125].all())


def test_mixed_clip_finaliser_matches_the_pinned_arithmetic(gpu):
    """cc_clip_finalize with emulate_bf16 = 2 over five parameters against tests/_jumprelu_ref.py's restatement, which
    tests/test_jumprelu_host.py pins against torch.nn.utils.clip_grad_norm_ on the CPU.  One exact squared sum per
    parameter, so nothing but the finaliser's own arithmetic is compared."""
    for scale in (1e-3, 30.0):
        sums = [v * scale for v in (3.7, 11.2, 0.013, 0.4, 0.9)]
        sq = torch.tensor(sums, dtype=torch.float32, device=gpu)
        exact = [float(v) for v in sq.cpu().double()]
        outs = {}
        for mode in (0, 1, 2):
            out = torch.zeros(8, device=gpu)
            ops.clip_finalize(sq, [0, 1, 2, 3, 4, 5], 1.0, mode, out)
            outs[mode] = out.cpu()
        coef, total, norms = R.clip_finaliser(exact, 1.0, emulate=2)
        got = outs[2]
        assert torch.equal(got[2:6], norms[:4]), (got, norms)  # the four bf16 norms
        assert math.isclose(got[6].item(), norms[4].item(), rel_tol=1e-6)
        assert math.isclose(got[1].item(), total.item(), rel_tol=1e-6) and math.isclose(got[0].item(), coef.item(), rel_tol=1e-6)
        assert (got[0].item() < 1.0) == (scale == 30.0)
        assert R.bf16r(got[1:2]).item() != got[1].item()  # an fp32 total ...
        assert R.bf16r(outs[1][1:2]).item() == outs[1][1].item()  # ... where the all-bf16 emulation rounds it
        assert not math.isclose(outs[0][1].item(), got[1].item(), rel_tol=1e-6)  # (and fp32 norms differ)


# ----------------------------------------------------------------------------- 2. dyadic known answer (fp32)
def jr_cfg(cfg, theta=0.125, eps=0.125, l0_coeff=0.5, **kw):
    return dict(cfg, activation="jumprelu", l0_coeff=l0_coeff, jump_bandwidth=eps, jump_threshold_init=theta, **kw)


def test_dyadic_known_answer(gpu):
    """Dyadic data (every fp32 sum exact): encode, decode, forward and get_losses are the reference mask of the stored
    pre-activations, bit for bit.  theta = eps = 0.125: about 8 % of all elements on each side of theta inside the
    window, and elements with a == theta exactly."""
    r = load("dyadic_b64_n2_d32_h128_fp32")
    P, x, fw = r["init"], r["x"][0], r["fwd"]
    cc = make_cc(jr_cfg(r["cfg"]), P, gpu, 2)
    assert cc.activation == "jumprelu" and cc.k is None
    a = torch.relu(fw["pre"])
    theta = torch.full((128,), 0.125)
    ref = R.jumprelu_ref(a, theta, 0.125)
    below = (ref["window"] & ~ref["kept"]).float().mean().item()
    above = (ref["window"] & ref["kept"]).float().mean().item()
    assert below >= 0.02 and above >= 0.02, (below, above)
    assert int((a == 0.125).sum()) > 0
    xg = x.to(gpu)
    with torch.no_grad():
        acts = cc.encode(xg).cpu()
        pre = cc.encode(xg, apply_relu=False).cpu()
        recon = cc.decode(acts.to(gpu)).cpu()
        fwd = cc.forward(xg).cpu()
        lo = cc.get_losses(xg)
    assert torch.equal(pre, fw["pre"])
    assert torch.equal(bits(acts), bits(ref["dense"]))
    want = R.jr_losses(x, P, theta, 0.125, torch.float32, masks=ref)
    assert torch.equal(recon, O.decode(ref["dense"], P)) and torch.equal(fwd, recon)
    assert torch.equal(bits(cc._ws.gate.cpu()), bits(ref["gate"]))
    assert rel(lo.l2_loss, want["l2_loss"]) < 2e-5
    for key in ("explained_variance", "explained_variance_A", "explained_variance_B"):
        assert rel(getattr(lo, key), want[key].detach()) < 2e-5, key
    assert lo.l0_loss.item() == ref["count"].float().mean().item()
    assert torch.equal(lo.l0_loss.cpu(), want["l0_loss"].detach())


# ----------------------------------------------------------------------------- 3. losses and the five gradients
def relu_acts(cfg, P, x, gpu, n, dt):
    """A: the ReLU-mode crosscoder's encode with the same weights (G1 is bit-reproducible)."""
    plain = {k: v for k, v in cfg.items() if k not in ("activation", "l0_coeff", "jump_bandwidth", "jump_threshold_init")}
    rc = make_cc(plain, P, gpu, n)
    with torch.no_grad():
        return rc.encode(x.to(gpu).to(dt)).cpu()


@pytest.mark.parametrize("name", ["step_b256_n2_d64_h512_bf16", "step_b96_n2_d40_h200_fp32"])
def test_losses_and_gradients_with_the_gpu_activations(gpu, name):
    """With the GPU's A = relu(pre) imposed on the reference (its values, the CPU graph's gradient), only arithmetic
    differs, so the project's bounds carry over to the losses and to all five gradients: bf16 error against fp64 <=
    2 x the CPU-bf16 error + 2e-3 (forward) / 5e-3 (gradients), fp32 rel < 2e-5.  theta = eps = 0.125,
    l0_coeff = 0.5, l1's weight 2.0."""
    r = load(name)
    cfg, P, x, n = r["cfg"], r["init"], r["x"][0], r["n_models"]
    dt = O.DTYPES[cfg["enc_dtype"]]
    h, B = cfg["dict_size"], x.shape[0]
    eps, l1w, l0c = 0.125, 2.0, 0.5
    cc = make_cc(jr_cfg(cfg, eps=eps, l0_coeff=l0c), P, gpu, n)
    A = relu_acts(cfg, P, x, gpu, n, dt)
    theta = torch.full((h,), 0.125)
    masks = R.jumprelu_ref(A, theta, eps)
    below = (masks["window"] & ~masks["kept"]).float().mean().item()
    above = (masks["window"] & masks["kept"]).float().mean().item()
    print(name, "window below / above theta", below, above, "a == theta", int((A.float() == 0.125).sum()))
    assert below >= 0.02 and above >= 0.02, (below, above)
    xg = x.to(gpu)
    with torch.no_grad():
        assert torch.equal(bits(cc.encode(xg.to(dt)).cpu()), bits(masks["dense"]))
        lo = cc.get_losses(xg)
    ws, arena = cc._ws, cc.arena()
    assert ws.jumprelu == eps and not ws.tr and len(ws.sq_off) == 6
    G = arena.like()
    tg = torch.full((cc._hp,), float("nan"), device=gpu)
    engine.backward(ws, arena, G, l1w, l0_coeff=l0c, theta_grad=tg)
    torch.cuda.synchronize()
    ours = dict(G.views(), jump_threshold=tg[:h])

    def oracle(dtype):
        return R.jr_loss_and_grads(x.to(dt), P, theta, eps, dtype, l1w, l0c, A=A)

    ref, _, gref = oracle(dt)
    truth, _, gtruth = oracle(torch.float64)
    assert lo.l0_loss.item() == masks["count"].float().mean().item()
    for key in ("l2_loss", "l1_loss", "explained_variance", "explained_variance_A", "explained_variance_B"):
        mine = getattr(lo, key).detach().float()
        if dt == torch.float32:
            e = rel(mine, truth[key].detach())
            print(name, key, "rel", e)
            assert e < 2e-5, (key, e)
        else:
            ok, e = envelope_ok(mine, ref[key].detach().float(), truth[key].detach())
            print(name, key, "(ours, cpu) vs fp64", e)
            assert ok, (key, e)
    for key in R.PARAMS5:
        g = ours[key]
        assert g.shape == gref[key].shape, key
        if dt == torch.float32:
            e = rel(g, gtruth[key])
            print(name, key, "grad rel", e)
            assert e < 2e-5, (key, e)
        else:
            ok, e = envelope_ok(g, gref[key], gtruth[key], floor=5e-3)
            print(name, key, "grad (ours, cpu) vs fp64", e)
            assert ok, (key, e)
    assert float(gtruth["jump_threshold"].abs().max()) > 0


# ----------------------------------------------------------------------------- 4. the Trainer
def test_trainer_steps_match_the_reference_step(gpu):
    """Three Trainer.step calls on step_b256_n2_d64_h512_bf16 against the reference step (autograd with the two
    straight-through estimators, torch's clip_grad_norm_ over five parameters, torch's Adam), which is handed the
    GPU's A = relu(pre) of each step's batch.  Bounds: test_gpu_parity.test_trainer_steps' for the loss dict and the
    four reference parameters in bf16; the thresholds, an fp32 parameter, to the fp32 bound on parameters (0.01 lr)
    and -- their gradient being formed from bf16 quantities -- the bf16 bound on moments (rel 0.05)."""
    r = load("step_b256_n2_d64_h512_bf16")
    n, steps = r["n_models"], 3
    cfg = jr_cfg(dict(r["cfg"], device=str(gpu)))
    dt = O.DTYPES[cfg["enc_dtype"]]
    cc = make_cc(cfg, r["init"], gpu, n)
    tr = ca.Trainer(cfg, buffer=_Replay(r["buf"], r["factor"], gpu), crosscoder=cc)
    theta0 = torch.full((cfg["dict_size"],), 0.125)
    ref = R.JumpReLUOracleTrainer(dict(cfg, device="cpu"), r["init"], theta0)
    lr, B, h = cfg["lr"], cfg["batch_size"], cfg["dict_size"]
    assert len(r["buf"]) >= steps
    for s in range(steps):
        # the step's own x and A: the prep kernel and G1 on the step's inputs and the parameters before the step
        arena = cc.arena()
        arena.wait_pending()
        xg = ops.prep_input(r["buf"][s].to(gpu), r["factor"][s].to(gpu), dt)
        A = ops.encode_fwd(xg, arena.W_enc_hk, arena.b_enc, torch.empty(B, h, dtype=dt, device=gpu), True).cpu()
        x = xg.cpu().view(B, n, -1)
        before = R.jumprelu_ref(A, cc.jump_threshold.detach().cpu().clone(), cfg["jump_bandwidth"])
        d = tr.step()
        assert torch.equal(bits(cc._ws.acts.cpu()), bits(before["dense"])), s  # A is what the step masked
        want = ref.step(x, A=A)
        assert list(d) == list(want)
        assert d["l1_coeff"] == want["l1_coeff"] and d["lr"] == want["lr"] and d["l0_coeff"] == want["l0_coeff"]
        l1_tol = 2 ** -7 * abs(want["l1_loss"])
        l0_tol = 1e-3 * h + 1.0 / B
        checks = {"l2_loss": 1e-4 * abs(want["l2_loss"]), "l1_loss": l1_tol, "l0_loss": l0_tol,
                  "explained_variance": 2e-3, "explained_variance_A": 4e-3, "explained_variance_B": 4e-3}
        checks["loss"] = (checks["l2_loss"] + d["l1_coeff"] * l1_tol * 2 + d["l0_coeff"] * l0_tol
                          + 1e-6 * abs(want["loss"]))
        for k, tol in checks.items():
            assert abs(d[k] - want[k]) <= tol, (s, k, d[k], want[k], tol)
        st = tr.optimizer.state  # (waits for the side-stream decoder half)
        torch.cuda.synchronize()
        for k in O.PARAM_ORDER:
            p, pr = getattr(cc, k).detach().cpu(), ref.P[k].detach()
            diff = (p.float() - pr.float()).abs()
            exact = (diff == 0).float().mean().item()
            print(f"step {s} {k}: bit-identical {exact:.4f}, max diff / lr {diff.max().item() / lr:.3f}")
            assert exact >= (0.94 if k.startswith("W") else 0.30), (s, k, exact)
            if k.startswith("W"):
                assert (diff <= 2 * _bf16_ulp(pr) + 3 * lr).all(), (s, k, (diff / lr).max().item())
            else:
                assert diff.max().item() <= 0.25 * lr, (s, k, diff.max().item() / lr)
            for i, mom in enumerate(("exp_avg", "exp_avg_sq")):
                e = rel(st[getattr(cc, k)][mom].cpu(), ref.moments(k)[i])
                assert e <= 0.05, (s, k, mom, e)
        th, thr = cc.jump_threshold.detach().cpu(), ref.P["jump_threshold"].detach()
        assert th.dtype == torch.float32
        diff = (th - thr).abs().max().item()
        print(f"step {s} jump_threshold: max diff / lr {diff / lr:.4f}, moved {float((th - theta0).abs().max()) / lr:.3f} lr")
        assert diff <= 0.01 * lr, (s, diff / lr)
        for i, mom in enumerate(("exp_avg", "exp_avg_sq")):
            m = st[cc.jump_threshold][mom]
            assert m.dtype == torch.float32 and m.shape == (h,)
            e = rel(m.cpu(), ref.moments("jump_threshold")[i])
            print(f"step {s} jump_threshold {mom} rel {e:.3e}")
            assert e <= 0.05, (s, mom, e)
    # the thresholds were trained: they stand ten times the parity bound or more away from where they started
    assert float((cc.jump_threshold.detach().cpu() - theta0).abs().max()) > 10 * 0.01 * lr


def test_zero_threshold_is_the_relu_step(gpu, monkeypatch):
    """jump_threshold_init = 0 and l0_coeff = 0: every positive activation is kept, every window term is
    -(0 / eps) G - 0 = 0, so the thresholds' gradient, their share of the clip norm and their update are exactly zero
    and the trainer walks the batch-major ReLU trainer's parameters bit for bit.  l1_coeff = 0 (the masked column
    sums are formed in another order), and inputs small enough that the clip is inactive in both trainers -- an active
    clip's coefficient is fp32 over the mixed five-parameter list and bf16 over the ReLU trainer's four, as torch has
    them.  Snapshots after a device synchronise."""
    B, n, d, h, steps = 256, 2, 64, 512, 3
    g = torch.Generator().manual_seed(11)
    bufs = [torch.randn(B, n, d, generator=g).to(torch.bfloat16) for _ in range(steps)]
    factors = [torch.full((n,), 0.05) for _ in range(steps)]

    def run(**kw):
        cfg = small_cfg(B, d, h, "bf16", gpu, l1_coeff=0.0, **kw)
        cc = ca.CrossCoder(cfg, n_models=n)
        tr = ca.Trainer(cfg, buffer=_Replay(bufs, factors, gpu), crosscoder=cc)
        out = []
        for _ in range(steps):
            dct = tr.step()
            tr.synchronize()
            torch.cuda.synchronize()
            assert not cc._ws.tr
            out.append((dct, cc._ws.clip_out.cpu().clone(), [getattr(cc, p).detach().clone() for p in O.PARAM_ORDER]))
        return out, cc, tr

    jr, cc, tr = run(activation="jumprelu", l0_coeff=0.0, jump_threshold_init=0.0, jump_bandwidth=0.125)
    monkeypatch.setattr(engine, "transposed_wgrad", lambda *a: False)  # the ReLU step in its batch-major form
    relu, _, _ = run()
    assert bool((cc.jump_threshold.detach() == 0).all()) and bool((tr.optimizer.theta_grad == 0).all())
    for step, ((d0, c0, p0), (d1, c1, p1)) in enumerate(zip(relu, jr)):
        assert c0[0].item() == 1.0 and c1[0].item() == 1.0, (step, c0, c1)  # the clip is inactive
        assert c1[6].item() == 0.0  # the thresholds' gradient norm
        for name, a, b in zip(O.PARAM_ORDER, p0, p1):
            assert torch.equal(a, b), (step, name, int((a != b).sum()), (a.float() - b.float()).abs().max().item())
        assert d0["l2_loss"] == d1["l2_loss"] and d0["l0_loss"] == d1["l0_loss"] and 0 < d0["l0_loss"] < h
        assert d1["loss"] == d0["loss"] and d1["l0_coeff"] == 0.0
    ws = cc._ws
    assert bool(((ws.gate > 0) & (ws.gate.float() < 0.0625)).any())  # the window was not empty: its terms were zero


def test_trainer_checkpoint_and_latent_stats(gpu, tmp_path, monkeypatch):
    B, n, d, h, steps = 256, 2, 64, 512, 3
    cfg = small_cfg(B, d, h, "bf16", gpu, activation="jumprelu", l0_coeff=0.02, jump_bandwidth=0.05,
                    jump_threshold_init=0.05)
    cc = ca.CrossCoder(cfg, n_models=n)
    st = ca.LatentStats(cc, k=4)
    tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * steps, n_models=n, seed=3), crosscoder=cc,
                    latent_stats=st)
    theta0 = cc.jump_threshold.detach().clone()
    for s in range(steps):
        dct = tr.step()
        assert list(dct)[-1] == "l0_coeff" and math.isclose(dct["l0_coeff"], 0.02 * min(1.0, s / 5.0), rel_tol=1e-12)
        assert 0 < dct["l0_loss"] < h and dct["l2_loss"] > 0
        # (the reference's logged loss: fp32 l2 + l1_coeff * the bf16 l1 tensor, a bf16 product; + l0_coeff * fp32 l0)
        want = (torch.tensor(dct["l2_loss"]) + dct["l1_coeff"] * torch.tensor(dct["l1_loss"], dtype=torch.bfloat16)
                + dct["l0_coeff"] * torch.tensor(dct["l0_loss"])).item()
        assert math.isclose(dct["loss"], want, rel_tol=1e-6), (dct, want)
    tr.synchronize()
    torch.cuda.synchronize()
    assert not torch.equal(theta0, cc.jump_threshold.detach())
    assert st.rows_seen == B * steps and int(st.result()["count"].sum()) > 0
    mom = tr.optimizer.state[cc.jump_threshold]
    assert mom["exp_avg"].dtype == torch.float32 and float(mom["exp_avg"].abs().max()) > 0
    monkeypatch.chdir(tmp_path)
    tr.save()
    loaded = ca.CrossCoder.load("version_0", 0)
    assert loaded.activation == "jumprelu" and loaded.cfg["l0_coeff"] == 0.02 and loaded.jump_bandwidth == 0.05
    assert torch.equal(loaded.jump_threshold.detach(), cc.jump_threshold.detach())
    x = torch.randn(B, n, d, generator=torch.Generator(device=gpu).manual_seed(8), device=gpu)
    with torch.no_grad():
        a, b = cc.encode(x), loaded.encode(x)
        dense = ops.encode_fwd(cc._flat_x(x), cc.arena().W_enc_hk, cc.arena().b_enc,
                               torch.empty(B, h, dtype=torch.bfloat16, device=gpu), True)
    assert torch.equal(bits(a), bits(b))
    ref = R.jumprelu_ref(dense.cpu(), cc.jump_threshold.detach().cpu(), 0.05)
    assert torch.equal(bits(a.cpu()), bits(ref["dense"])) and 0 < int(ref["kept"].sum()) < int((dense > 0).sum())
    st2 = ca.LatentStats(loaded, k=4)  # LatentStats.update encodes as the crosscoder does
    st2.update(x)
    assert torch.equal(st2.result()["count"], (a > 0).sum(0))


def test_refusals(gpu):
    from crosscoder_amd import sharded
    cfg = small_cfg(64, 32, 256, "bf16", gpu, activation="jumprelu", l0_coeff=0.5)
    with pytest.raises(ValueError, match="jumprelu"):
        sharded.ShardedTrainer(cfg, buffer=None)
    with pytest.raises(ValueError, match="jumprelu"):
        sharded.ShardedTrainer({k: v for k, v in cfg.items() if k not in ("activation", "l0_coeff")}, buffer=None,
                               crosscoder=ca.CrossCoder(cfg))
    with pytest.raises(ValueError, match="jumprelu"):
        ca.CrossCoder(dict(cfg, auxk_coeff=0.03))
    with pytest.raises(ValueError, match="theta"):  # the engine's forward needs the thresholds
        cc = ca.CrossCoder(cfg)
        engine.forward(cc._workspace(64), cc.arena(), torch.zeros(64, 2, 32, device=gpu))
