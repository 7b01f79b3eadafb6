"""tests/_step_ops_ref.py on the CPU: the fp64 references, chained into one training step, agree with torch autograd
over oracle.cpu_reference.get_losses; and the comparator with its derived bounds rejects the errors a kernel makes
(a dropped k element, a dropped batch row, a shifted column, a missing L1 term, a wrong inverse norm, a wrong mask,
a few ulps) while it accepts the correctly rounded result."""
import pytest
import torch

from oracle import cpu_reference as O
from tests import _step_ops_ref as ref

F64 = torch.float64


def make_case(B, n, d, h, seed, edges):
    """fp64 parameters and a batch; edges: decoder row 3 all zero, latent 1 dead on every row, latent h - 2 on."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=F64) * sc  # noqa: E731
    P = {"W_enc": r(n, d, h, sc=0.2), "W_dec": r(h, n, d, sc=0.2), "b_enc": r(h, sc=0.1), "b_dec": r(n, d, sc=0.1)}
    x_in, factor = r(B, n, d), torch.rand(n, generator=g, dtype=F64) + 0.5
    if edges:
        P["W_dec"][3] = 0.0
        P["W_enc"][:, :, 1] = 0.0
        P["b_enc"][1] = -1.0
        P["W_enc"][:, :, h - 2] = 0.0
        P["b_enc"][h - 2] = 1.0
    return P, x_in, factor


@pytest.mark.parametrize("B,n,d,h,edges", [(24, 2, 8, 16, False), (33, 3, 16, 40, False), (24, 2, 8, 16, True),
                                           (33, 3, 16, 40, True)])
def test_chained_references_match_autograd(B, n, d, h, edges, monkeypatch):
    # get_losses casts recon and x with .float() (crosscoder.py:104, a no-op in the reference's fp32 mode), which would
    # cut the fp64 evaluation down to fp32 (as (acts > 0).float() does the l0 mean): for the length of this test
    # .float() gives fp64 on fp64 and bool tensors
    to_float = torch.Tensor.float
    monkeypatch.setattr(torch.Tensor, "float",
                        lambda t, *a, **k: t.double() if t.dtype in (F64, torch.bool) else to_float(t, *a, **k))
    l1c, K = 2.0, n * d
    P, x_in, factor = make_case(B, n, d, h, B + h, edges)
    # the reference chain
    x, xsum, _ = ref.prep(x_in, factor, F64)
    W_enc_hk = P["W_enc"].permute(2, 0, 1).reshape(h, K)
    W_dec_hk = P["W_dec"].reshape(h, K)
    pre, _ = ref.encode(x, W_enc_hk, P["b_enc"])
    acts = torch.relu(pre)
    recon, _ = ref.decode(acts, W_dec_hk)
    norms, tn, inv = ref.dec_norms(W_dec_hk, n, d)
    lo = ref.loss(recon, P["b_dec"].reshape(K), x, xsum / B, 2.0 / B, n, d, F64)
    sc = ref.loss_scalars(lo["l2"], lo["tv"], (acts * tn).sum(), (acts > 0).sum(), B)
    g_pre, _ = ref.dacts(lo["g"], W_dec_hk, acts, tn, l1c / B)
    gW_dec, _, l1_term = ref.wgrad_dec(acts, lo["g"], W_dec_hk, inv, acts.sum(0), l1c / B, n, d)
    gW_enc, _ = ref.wgrad_enc(g_pre, x)
    gb_enc, _ = ref.colsum(g_pre)
    # autograd over the oracle
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = O.get_losses(x.reshape(B, n, d), leaves, F64)
    (want["l2_loss"] + l1c * want["l1_loss"]).backward()
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-14)  # noqa: E731
    close(sc["l2"], want["l2_loss"].detach())
    close(torch.tensor(sc["l1"], dtype=F64), want["l1_loss"].detach())
    close(torch.tensor(sc["l0"], dtype=F64), want["l0_loss"].detach().double())
    close(sc["ev"], want["explained_variance"].detach())
    close(sc["ev_a"], want["explained_variance_A"].detach())  # (models 0 and 1, also where n = 3)
    close(sc["ev_b"], want["explained_variance_B"].detach())
    close(sc["mean_ev"], want["explained_variance"].detach().mean())
    close(gW_dec.reshape(h, n, d), leaves["W_dec"].grad)
    close(gW_enc, leaves["W_enc"].grad.permute(2, 0, 1).reshape(h, K))
    close(gb_enc, leaves["b_enc"].grad)
    close(lo["colsum"].reshape(n, d), leaves["b_dec"].grad)
    if edges:
        # the zero decoder row: the norm backward is 0 there, so the row is acts^T g_recon alone; the dead latent:
        # every gradient row of it is exactly 0
        assert bool((inv[3] == 0).all()) and bool((norms[3] == 0).all()) and bool((l1_term[3] == 0).all())
        assert bool((acts[:, 1] == 0).all()) and bool((acts[:, h - 2] > 0).all())
        for t in (gW_dec[1], gW_enc[1], g_pre[:, 1], leaves["W_dec"].grad[1].reshape(K), gb_enc[1:2]):
            assert bool((t == 0).all())
        assert bool((gW_dec[3] == acts[:, 3] @ lo["g"]).all())


def test_single_model_ev_b_is_zero():
    sc = ref.loss_scalars(torch.rand(5, 1, dtype=F64), torch.rand(5, 1, dtype=F64) + 1, 3.0, 7, 5)
    assert bool((sc["ev_b"] == 0).all()) and float(sc["mean_ev_b"]) == 0.0 and bool((sc["ev_a"] == sc["ev"]).all())


def test_prep_is_bit_exact_fp32_arithmetic():
    g = torch.Generator().manual_seed(1)
    x_in, factor = torch.randn(9, 2, 8, generator=g), torch.tensor([0.7, 1.3]).to(torch.bfloat16)
    for dt in (torch.float32, torch.bfloat16):
        x, s, A = ref.prep(x_in, factor, dt)
        assert x.dtype == dt and torch.equal(x, (x_in * factor.float()[None, :, None]).to(dt).reshape(9, 16))
        assert torch.equal(s, x.double().sum(0)) and torch.equal(A, x.double().abs().sum(0))
        assert torch.equal(ref.prep(x_in, None, dt)[0], x_in.to(dt).reshape(9, 16))


# ----------------------------------------------------------------------------- seeded errors
BF = torch.bfloat16
SB, SN, SD, SH = 96, 2, 40, 200
L1_SCALE = 0.05


@pytest.fixture(scope="module")
def seeded():
    """The GPU tests' inputs at (96, 2, 40, 200) in bf16, and the fp64 results the seeded errors start from."""
    B, n, d, h, K = SB, SN, SD, SH, SN * SD
    g = torch.Generator().manual_seed(7)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(BF)  # noqa: E731
    c = {"x": mk(B, K), "W_enc": mk(h, K, sc=0.05), "b_enc": mk(h, sc=0.1), "W_dec": mk(h, K, sc=0.05),
         "g_recon": mk(B, K, sc=1e-2), "tn": torch.rand(h, generator=g) + 0.5}
    c["W_dec"][3] = 0
    c["pre"], c["A_pre"] = ref.encode(c["x"], c["W_enc"], c["b_enc"])
    c["acts"] = ref.round_dt(torch.relu(c["pre"]), BF)
    c["g_pre"], c["A_gpre"] = ref.dacts(c["g_recon"], c["W_dec"], c["acts"], c["tn"], L1_SCALE)
    c["norms"], c["tot"], c["inv"] = ref.dec_norms(c["W_dec"], n, d)
    c["colsum_acts"] = c["acts"].float().sum(0)
    c["gW"], c["A_gW"], c["l1_term"] = ref.wgrad_dec(c["acts"], c["g_recon"], c["W_dec"], c["inv"].float(),
                                                     c["colsum_acts"], L1_SCALE, n, d)
    return c


def rejects(ours, v64, bound, name):
    with pytest.raises(AssertionError, match=name):
        ref.check(ours, v64, bound, name)


def test_correctly_rounded_results_pass(seeded):
    c, K = seeded, SN * SD
    for name, v, A, L in (("pre", c["pre"], c["A_pre"], K), ("g_pre", c["g_pre"], c["A_gpre"], K),
                          ("gW", c["gW"], c["A_gW"], SB)):
        r = ref.check(ref.round_dt(v, BF), v, ref.acc_bound(L, A) + ref.store_bound(v, BF), name)
        assert 0 < r <= 1.0
        assert ref.check(ref.round_dt(v, torch.float32), v, ref.acc_bound(L, A), name + "_f32") <= 1.0
    s, A = ref.colsum(c["acts"])
    assert ref.check(s.float(), s, ref.acc_bound(SB, A), "colsum") <= 1.0


def test_dropped_last_k_element_is_rejected(seeded):
    c, K = seeded, SN * SD
    short, _ = ref.encode(c["x"][:, :K - 1], c["W_enc"][:, :K - 1], c["b_enc"])
    rejects(ref.round_dt(short, BF), c["pre"], ref.acc_bound(K, c["A_pre"]) + ref.store_bound(c["pre"], BF), "pre")


def test_dropped_last_batch_row_of_a_column_sum_is_rejected(seeded):
    c = seeded
    s, A = ref.colsum(c["acts"])
    short, _ = ref.colsum(c["acts"][:-1])
    assert bool((c["acts"][-1] > 0).any())
    rejects(short.float(), s, ref.acc_bound(SB, A), "colsum")                        # the fp32 slab
    rejects(ref.round_dt(short, BF), s, ref.acc_bound(SB, A) + ref.store_bound(s, BF), "colsum")  # a bf16 bias grad


def test_shifted_output_column_is_rejected(seeded):
    c, K = seeded, SN * SD
    ours = ref.round_dt(c["pre"], BF)
    ours[:, 17] = ours[:, 18]
    rejects(ours, c["pre"], ref.acc_bound(K, c["A_pre"]) + ref.store_bound(c["pre"], BF), "pre")


def test_missing_l1_term_on_one_row_is_rejected(seeded):
    c = seeded
    bound = ref.acc_bound(SB, c["A_gW"]) + ref.store_bound(c["gW"], BF)
    # (the GPU tests assert the same: with l1_scale = 0.05 the L1 term exceeds its element's bound on every live row)
    live = c["colsum_acts"] > 0
    live[3] = False
    assert bool((c["l1_term"].abs()[live] > 2 * bound[live]).any(1).all())
    ours = c["gW"].clone()
    ours[9] -= c["l1_term"][9]
    rejects(ref.round_dt(ours, BF), c["gW"], bound, "gW")


def test_unit_inverse_norm_on_the_zero_row_is_rejected(seeded):
    c = seeded
    assert bool((c["inv"][3] == 0).all())
    rel = (SD / 2 + 8) * ref.EPS23
    assert ref.check(c["inv"].float(), c["inv"], rel * c["inv"], "inv_norms") <= 1.0
    ours = c["inv"].float()
    ours[3] = 1.0
    rejects(ours, c["inv"], rel * c["inv"], "inv_norms")
    # ... and a dW_dec formed with it on a row whose decoder is NOT zero (stale norms) carries a visible L1 term
    inv = c["inv"].float()
    inv[9] = 0.0
    gW, A, _ = ref.wgrad_dec(c["acts"], c["g_recon"], c["W_dec"], inv, c["colsum_acts"], L1_SCALE, SN, SD)
    rejects(ref.round_dt(c["gW"], BF), gW, ref.acc_bound(SB, A) + ref.store_bound(gW, BF), "gW")


def test_unmasked_element_is_rejected(seeded):
    c, K = seeded, SN * SD
    full, _ = ref.dacts(c["g_recon"], c["W_dec"], torch.ones_like(c["acts"]), c["tn"], L1_SCALE)
    masked = c["acts"] == 0
    i = int(torch.where(masked, full.abs(), torch.zeros_like(full)).argmax())
    ours = ref.round_dt(c["g_pre"], BF)
    assert ours.view(-1)[i] == 0
    ours.view(-1)[i] = ref.round_dt(full, BF).view(-1)[i]
    rejects(ours, c["g_pre"], ref.acc_bound(K, c["A_gpre"]) + ref.store_bound(c["g_pre"], BF), "g_pre")


def test_four_ulps_are_rejected(seeded):
    c, K = seeded, SN * SD
    bound = ref.acc_bound(K, c["A_pre"]) + ref.store_bound(c["pre"], BF)
    # (an element that is not a cancellation: 4 ulps of a value far below its own A are accumulation noise)
    i = int((c["pre"].abs() / c["A_pre"]).argmax())
    ours = ref.round_dt(c["pre"], BF)
    ours.view(torch.int16).view(-1)[i] += 4  # (4 ulps away from zero)
    rejects(ours, c["pre"], bound, "pre")
    ours.view(torch.int16).view(-1)[i] -= 8
    rejects(ours, c["pre"], bound, "pre")
