"""JumpReLU crosscoders, the parts that need no GPU: the cfg keys and refusals, the state-dict keys per activation, the
C ABI's declarations and argument checks, the mixed-dtype clip pinned against torch, and the reference's own
straight-through gradients against a hand-computed case."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, sharded
from crosscoder_amd.crosscoder import activation_of, auxk_options, jumprelu_options
from tests import _jumprelu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cc_jumprelu_mask", "cc_jumprelu_bwd", "cc_jumprelu_part_rows", "cc_jumprelu_l0_parts")


def cfg_of(**kw):
    cfg = {"seed": 49, "batch_size": 64, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 6400, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": 128, "seq_len": 1024, "enc_dtype": "fp32", "device": "cpu",
           "dec_init_norm": 0.08, "d_in": 32, "log_every": 100, "save_every": 30000}
    cfg.update(kw)
    return cfg


# ----------------------------------------------------------------------------- cfg
def test_cfg_keys_and_defaults():
    cfg = cfg_of(activation="jumprelu", l0_coeff=0.5)
    assert activation_of(cfg) == ("jumprelu", None)
    assert jumprelu_options(cfg) == (0.5, 1e-3, 1e-3)
    assert jumprelu_options(dict(cfg, l0_coeff=0, jump_bandwidth=0.125, jump_threshold_init=-1)) == (0.0, 0.125, -1.0)
    assert activation_of(cfg_of()) == ("relu", None)  # the default is unchanged


@pytest.mark.parametrize("bad", [{}, {"l0_coeff": -0.1}, {"l0_coeff": "1"}, {"l0_coeff": True},
                                 {"l0_coeff": float("nan")}, {"l0_coeff": float("inf")},
                                 {"l0_coeff": 1.0, "jump_bandwidth": 0}, {"l0_coeff": 1.0, "jump_bandwidth": -1e-3},
                                 {"l0_coeff": 1.0, "jump_bandwidth": 1e-60}, {"l0_coeff": 1.0, "jump_bandwidth": None},
                                 {"l0_coeff": 1.0, "jump_bandwidth": float("inf")},
                                 {"l0_coeff": 1.0, "jump_threshold_init": float("nan")},
                                 {"l0_coeff": 1.0, "jump_threshold_init": "0"}])
def test_cfg_validation(bad):
    with pytest.raises(ValueError, match="l0_coeff|jump_bandwidth|jump_threshold_init"):
        activation_of(cfg_of(activation="jumprelu", **bad))
    with pytest.raises(ValueError):
        ca.CrossCoder(cfg_of(activation="jumprelu", **bad))


def test_refusals():
    cfg = cfg_of(activation="jumprelu", l0_coeff=0.5)
    with pytest.raises(ValueError, match="jumprelu"):  # AuxK's aux rows have no threshold gradient
        auxk_options(dict(cfg, auxk_coeff=0.03))
    with pytest.raises(ValueError, match="jumprelu"):
        ca.CrossCoder(dict(cfg, auxk_coeff=0.03))
    assert auxk_options(dict(cfg, auxk_coeff=0)) is None
    with pytest.raises(ValueError, match="jumprelu"):
        sharded.ShardedTrainer(cfg, buffer=None)
    plain = {k: v for k, v in cfg.items() if k not in ("activation", "l0_coeff")}
    with pytest.raises(ValueError, match="jumprelu"):  # (a JumpReLU crosscoder handed in)
        sharded.ShardedTrainer(plain, buffer=None, crosscoder=ca.CrossCoder(cfg))


# ----------------------------------------------------------------------------- the fifth parameter
def test_state_dict_keys_per_activation():
    four = ["W_enc", "W_dec", "b_enc", "b_dec"]
    assert list(ca.CrossCoder(cfg_of()).state_dict()) == four
    assert list(ca.CrossCoder(cfg_of(activation="topk", k=8)).state_dict()) == four
    assert list(ca.CrossCoder(cfg_of(activation="batch_topk", k=8)).state_dict()) == four + ["threshold"]
    cc = ca.CrossCoder(cfg_of(activation="jumprelu", l0_coeff=0.5, jump_threshold_init=0.25, dict_size=203))
    assert list(cc.state_dict()) == four + ["jump_threshold"]
    assert list(cc.reference_state_dict()) == four
    th = cc.jump_threshold
    assert th.dtype == torch.float32 and th.shape == (203,) and bool((th == 0.25).all()) and th.requires_grad
    assert [n for n, _ in cc.named_parameters()] == four + ["jump_threshold"]
    # the kernels' buffer: the kernel h (208), zero thresholds for the padding latents, the parameter its head
    buf = cc.theta()
    assert buf.shape == (208,) and buf.data_ptr() == th.data_ptr() and bool((buf[203:] == 0).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_threshold_round_trips(dtype, tmp_path, monkeypatch):
    cfg = cfg_of(activation="jumprelu", l0_coeff=0.5, jump_bandwidth=0.125, enc_dtype=dtype, dict_size=203)
    cc = ca.CrossCoder(cfg)
    new = torch.linspace(-0.5, 2.0, 203)
    with torch.no_grad():
        cc.jump_threshold.copy_(new)
    assert torch.equal(cc.theta()[:203], new)  # written through the parameter, read by the kernels' buffer
    monkeypatch.chdir(tmp_path)
    cc.save()
    saved = torch.load(tmp_path / "checkpoints" / "version_0" / "0.pt", weights_only=True)
    assert set(saved) == {"W_enc", "W_dec", "b_enc", "b_dec", "jump_threshold"}
    loaded = ca.CrossCoder.load("version_0", 0)
    assert loaded.activation == "jumprelu" and loaded.jump_bandwidth == 0.125 and loaded.l0_coeff == 0.5
    assert torch.equal(loaded.jump_threshold.detach(), new) and loaded.jump_threshold.dtype == torch.float32
    for k in ("W_enc", "W_dec", "b_enc", "b_dec"):
        assert torch.equal(getattr(loaded, k).detach(), getattr(cc, k).detach())
    other = ca.CrossCoder(cfg)
    other.load_state_dict(cc.state_dict())
    assert torch.equal(other.theta()[:203], new)
    # the reference's four tensors load as they are: the thresholds then stay what they are
    other.load_state_dict(ca.CrossCoder(cfg_of(enc_dtype=dtype, dict_size=203)).state_dict())
    assert torch.equal(other.jump_threshold.detach(), new)
    # a replaced parameter (.to(), .double() ...) is packed again
    other.jump_threshold = torch.nn.Parameter(new.clone() + 1)
    assert torch.equal(other.theta()[:203], new + 1) and other.theta().data_ptr() == other.jump_threshold.data_ptr()


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    lib = _lib.load()
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    exported = {path: {ln.split()[-1] for ln in subprocess.run([nm, "-D", "--defined-only", path], check=True,
                                                                capture_output=True, text=True).stdout.splitlines()
                       if ln.strip()} for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH)}
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name
        for path, syms in exported.items():
            assert name in syms, (name, path)
        assert name in _lib.SIGNATURES
        getattr(lib, name)
    assert len(_lib.SIGNATURES["cc_jumprelu_mask"][1]) == 12 and len(_lib.SIGNATURES["cc_jumprelu_bwd"][1]) == 12
    for B, h in ((1, 8), (3, 200), (130, 512), (4, 16384), (600, 2056), (4096, 16384), (2, 131072)):
        rows, parts = lib.cc_jumprelu_part_rows(B, h), lib.cc_jumprelu_l0_parts(B, h)
        assert 1 <= rows <= min(B, 256) and rows <= parts and parts % rows == 0, (B, h, rows, parts)
    assert lib.cc_jumprelu_part_rows(600, 2056) == 256  # more rows than row groups
    assert lib.cc_jumprelu_part_rows(0, 8) == 0 and lib.cc_jumprelu_l0_parts(4, 12) == 0


def test_argument_validation_needs_no_gpu():
    """Errors are returned before any launch, in cc_topk_rows' order (host pointers are never touched)."""
    lib = _lib.load()
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    assert p % 16 == 0
    q = p + 1024
    shape, null, dtype, large, align = 3, 1, 2, 5, 4

    def mask(acts=p, ld=16, B=4, h=16, dt=_lib.CC_F32, theta=p, eps=0.125, out=p, gate=q, colsum=None, l0=None):
        return lib.cc_jumprelu_mask(acts, ld, B, h, dt, theta, eps, out, gate, colsum, l0, None)

    def bwd(g=p, gate=q, ld=16, B=4, h=16, dt=_lib.CC_F32, theta=p, eps=0.125, l0s=0.1, colsum=None, thr=None):
        return lib.cc_jumprelu_bwd(g, gate, ld, B, h, dt, theta, eps, l0s, colsum, thr, None)

    for f in (mask, bwd):
        assert f(ld=17) == shape and f(ld=20) == shape and f(ld=8) == shape
        assert f(h=12) == shape and f(B=0) == shape and f(h=0) == shape
        assert f(eps=0.0) == shape and f(eps=-1.0) == shape and f(eps=float("nan")) == shape
        assert f(eps=float("inf")) == shape
        assert f(theta=None) == null
        assert f(dt=7) == dtype
        assert f(h=1 << 18, ld=1 << 18) == large and f(B=1 << 20, h=1 << 12, ld=1 << 12) == large
        assert f(theta=p + 4) == align
        assert f(B=0, theta=None, dt=7) == shape and f(theta=None, dt=7) == null  # the order
        assert f(dt=7, h=1 << 18, ld=1 << 18) == dtype
    assert mask(acts=None) == null and mask(out=None) == null
    assert mask(acts=p + 2) == align and mask(out=p + 8) == align and mask(gate=p + 8) == align
    assert mask(colsum=p + 4) == align and mask(l0=p + 2) == align
    assert bwd(g=None) == null and bwd(gate=None) == null and bwd(gate=p) == null  # g_pre == gate
    assert bwd(g=p + 8) == align and bwd(thr=p + 4) == align and bwd(colsum=p + 8) == align


# ----------------------------------------------------------------------------- the mixed-dtype clip: torch is the spec
@pytest.mark.parametrize("scale", [3e-3, 0.3])  # clip inactive / active
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_mixed_clip_matches_torch(seed, scale):
    """clip_grad_norm_ over four bf16 gradients and one fp32 gradient, on the CPU: torch forms the four bf16 norms in
    bf16, stacks them with the fp32 fifth (fp32; the fifth FIRST: torch groups the list by dtype, and that is the order
    its grouping yields), keeps the total and the coefficient in fp32 and multiplies each
    gradient in its own dtype by that fp32 coefficient.  The finaliser's arithmetic (tests/_jumprelu_ref.py, emulate
    = 2: what grad_tail.h runs on the GPU) is pinned in two halves: from torch's own per-tensor norms it gives torch's
    total and torch's clipped gradients bit for bit; and its per-parameter norms from exact squared sums are torch's
    to the rounding of one norm (a bf16 norm: one bf16 ulp where the fp32 sums straddle a rounding boundary, else
    equal; the fp32 norm: 1e-6, the project's bound for an fp32 sum in another order).  The all-bf16 emulation (1)
    and the all-fp32 one (0) miss torch's total by far more than that."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(2, 20, 48), (48, 2, 20), (48,), (2, 20), (48,)]
    dts = [torch.bfloat16] * 4 + [torch.float32]
    grads = [(torch.randn(s, generator=g) * scale).to(dt) for s, dt in zip(shapes, dts)]
    params = [torch.nn.Parameter(torch.zeros(s, dtype=dt)) for s, dt in zip(shapes, dts)]
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
    assert total.dtype == torch.float32
    tnorms = [torch.linalg.vector_norm(gr, 2.0) for gr in grads]
    assert [t.dtype for t in tnorms] == dts
    # (1) stack, total, coefficient and the multiply, from torch's own norms: bit for bit
    coef, tot = R.clip_from_norms(tnorms, 1.0, emulate=2)
    assert tot.item() == total.item(), (tot.item(), total.item())
    assert (coef.item() < 1.0) == (scale == 0.3)
    for p, gr in zip(params, grads):
        assert torch.equal(p.grad, (gr.float() * coef).to(gr.dtype))  # cc_adam_step: g' = dtype(g * coef)
    # (2) the per-parameter norms from the squared sums
    sq = [gr.double().pow(2).sum().item() for gr in grads]
    norms = R.clip_param_norms(sq, emulate=2)
    for i, (mine, theirs) in enumerate(zip(norms, tnorms)):
        tol = 2.0 ** -8 if i < 4 else 1e-6
        assert abs(mine.item() - theirs.float().item()) <= tol * theirs.float().item(), (i, mine, theirs)
        if i < 4:
            assert R.bf16r(mine).item() == mine.item()  # a bf16 value
    assert sum(m.item() == t.float().item() for m, t in zip(norms[:4], tnorms[:4])) >= 3
    coef2, tot2, _ = R.clip_finaliser(sq, 1.0, emulate=2)
    assert abs(tot2.item() - total.item()) <= 2.0 ** -8 * total.item()
    # the other emulations are not this arithmetic
    _, tot1, _ = R.clip_finaliser(sq, 1.0, emulate=1)
    _, tot0, _ = R.clip_finaliser(sq, 1.0, emulate=0)
    assert R.bf16r(tot1).item() == tot1.item() and R.bf16r(total).item() != total.item()
    assert tot0.item() != tot2.item()
    # all five in fp32 (an fp32 crosscoder): the plain arithmetic, one more norm
    p32 = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for p, gr in zip(p32, grads):
        p.grad = gr.float().clone()
    t32 = torch.nn.utils.clip_grad_norm_(p32, max_norm=1.0)
    assert abs(tot0.item() - t32.item()) <= 1e-6 * t32.item()


# ----------------------------------------------------------------------------- the reference's own gradients
def test_reference_masks_on_the_boundaries():
    """a == theta is dropped and d == +-half is outside the window: all three comparisons are strict."""
    theta = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, -1.0, 0.0, 0.5])
    a = torch.tensor([[0.5, 0.4375, 0.5625, 0.46875, 0.53125, 0.25, 0.0, float("nan")],
                      [float("inf"), -0.0, -1.0, 0.4375 + 2 ** -9, 0.5625 - 2 ** -8, 0.0, 1e-40, 0.75]])
    for dt in (torch.float32, torch.bfloat16):
        r = R.jumprelu_ref(a.to(dt), theta, 0.125)
        assert r["kept"].tolist() == [[False, False, True, False, True, True, False, False],
                                      [True, False, False, False, True, False, True, True]]
        assert r["gated"].tolist() == [[True, False, True, True, True, True, False, False],
                                       [True, False, False, True, True, False, True, True]]
        assert r["window"].tolist() == [[True, False, False, True, True, False, False, False],
                                        [False, False, False, True, True, False, True, False]]
        assert not bool(torch.signbit(r["dense"][~r["kept"]]).any()) and bool((r["dense"][~r["kept"]] == 0).all())


def test_reference_ste_against_a_hand_computed_case():
    """2 x 3, one model... the objective l2 + l1c l1 + l0c l0 with W_dec rows of norm 1 per model: theta.grad by hand.
    Latent 0: both rows kept, row 1 in the window above theta; latent 1: row 0 in the window below theta (gated, not
    kept), row 1 zero (never in the window although theta < eps / 2 there); latent 2: kept far above, no window."""
    eps, l1c, l0c, B = 0.5, 0.25, 3.0, 2
    theta = torch.tensor([1.0, 0.125, 0.5], dtype=torch.float64)
    A = torch.tensor([[2.0, 0.0625, 4.0], [1.125, 0.0, 3.0]], dtype=torch.float64)
    # a decoder with orthonormal rows per model and x = 0, b_dec = 0: recon = acts @ W_dec, dL2/dacts = 2/B * n * acts
    n, d, h = 2, 3, 3
    W_dec = torch.eye(3, dtype=torch.float64)[:, None, :].repeat(1, n, 1)
    P = {"W_enc": torch.zeros(n, d, h, dtype=torch.float64), "W_dec": W_dec,
         "b_enc": torch.ones(h, dtype=torch.float64), "b_dec": torch.zeros(n, d, dtype=torch.float64)}
    x = torch.zeros(B, n, d, dtype=torch.float64)
    masks = R.jumprelu_ref(A.float(), theta.float(), eps)
    assert masks["kept"].tolist() == [[True, False, True], [True, False, True]]
    assert masks["window"].tolist() == [[False, True, False], [True, False, False]]
    lo, loss, grads = R.jr_loss_and_grads(x, P, theta, eps, torch.float64, l1c, l0c, A=A)
    kept = masks["kept"].double()
    acts = A * kept
    assert torch.equal(lo["acts"].detach(), acts) and lo["l0_loss"].item() == 2.0
    tn = torch.full((h,), float(n), dtype=torch.float64)  # sum over models of the unit norms
    G = 2.0 / B * n * acts + l1c / B * tn[None, :]  # dL/d acts: the reconstruction's and the L1 term's
    want = torch.stack([-(theta[0] / eps) * G[1, 0] - (l0c / B) / eps,
                        -(theta[1] / eps) * G[0, 1] - (l0c / B) / eps,
                        torch.tensor(0.0, dtype=torch.float64)])
    assert torch.allclose(grads["jump_threshold"], want, rtol=1e-12, atol=0), (grads["jump_threshold"], want)
    # the same from the kernel's formula
    terms = R.theta_grad_terms(G, masks["window"], theta.float(), eps, l0c / B)
    assert torch.allclose(terms.sum(0), want, rtol=1e-6, atol=0)
    # b_enc sees the straight-through g_pre: G at the kept elements only
    assert torch.allclose(grads["b_enc"], (G * kept).sum(0), rtol=1e-12, atol=0)
