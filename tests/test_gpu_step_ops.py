"""The training-step kernels, each entry point alone, element-wise against fp64 references of the operands it was
handed (tests/_step_ops_ref.py): cc_prep_input, cc_encode_fwd(_t), cc_decode_fwd, cc_loss_fwd_bwd(_rows),
cc_loss_finalize, cc_dacts_bwd(_t), cc_wgrad_dec / _enc / _both, cc_dec_norms, cc_reduce_rows, cc_clip_finalize and
cc_gemm_f32out.

The bounds are derived, not measured: |ours - v64| <= (L + 16) 2^-23 A + (bf16: 2^-8 |v64|) with L the number of
fp32 terms summed and A the sum of their magnitudes; an indexing error, a dropped term or a wrong mask is of order A.
Every test prints its max(err / bound) ("STEPOPS ..." lines; DESIGN.md holds the table).

Shapes (B, n, d, h) are the smallest at which a tiling decision changes: tiles are 256 x 256, row groups 128, loss
blocks 32 rows x 512 columns, prep blocks 64 rows.  Every output is allocated with two extra rows (or a tail) of a
canary, which must survive, while none may remain inside the logical extent; the inputs must be unchanged.  Where
h >= 8, latent 1 is dead on every row, latent h - 2 is on on every row, decoder row 3 is all zero and b_dec is not
zero.  bf16 runs through both main loops (ping-pong and, in the debug build, two-stage)."""
import functools
import math
import types

import pytest
import torch

from crosscoder_amd import ops
from oracle import cpu_reference as O
from tests import _jumprelu_ref as JR
from tests import _step_ops_ref as ref

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = {"fp32": F32, "bf16": BF16}
CANARY = -12288.0  # (exact in bf16; no output of these inputs comes near it)
L1_SCALE = 0.05    # large enough that every L1 term exceeds its element's bound (asserted where it is used)

SHAPES = [(1, 1, 8, 8),         # the minimum the ABI admits
          (96, 2, 40, 200),     # one ragged tile, K = 80 tail
          (300, 3, 24, 520),    # 2 x 3 tiles with ragged last row and column tiles, K = 72
          (256, 2, 32, 256),    # whole tiles, K = 64: the whole-tile ReLU epilogue below the q4 loop's K >= 128
          (512, 2, 64, 512)]    # 2 x 2 whole tiles, K = 128: the product's default main loop for the step shape
WIDE = (33, 2, 520, 64)         # prep / loss / loss_finalize / dec_norms: two 512-column blocks per model, the second
                                # ragged, and one row past a 32-row block
sid = lambda s: "B%d_n%d_d%d_h%d" % s  # noqa: E731


@pytest.fixture
def dbg_lib():
    """ops.* routed through the test-only debug build (launch-form setters); product defaults afterwards."""
    from crosscoder_amd import _lib
    with _lib.debug_library() as lib:
        yield lib


@pytest.fixture
def pp_mask(dbg_lib):
    """Selects which layouts run the ping-pong main loop (debug build); restored afterwards."""
    yield dbg_lib.cc_debug_set_pp_mask


@pytest.fixture(params=["fp32", "bf16", "bf16_two_stage"])
def mode(request):
    """The storage dtype and, for bf16, the GEMM main loop: the product's, or the two-stage loop (pp_mask 0)."""
    if request.param == "bf16_two_stage":
        request.getfixturevalue("pp_mask")(0)
    return request.param


def dtype_of(mode):
    return DT[mode.split("_")[0]]


def report(entry, mode, shape, **ratios):
    print("STEPOPS %s %s %s %s" % (entry, mode, sid(shape) if isinstance(shape, tuple) else shape,
                                   " ".join(f"{k}={v:.3f}" for k, v in ratios.items())))


# ----------------------------------------------------------------------------- inputs and their fp64 references
@functools.lru_cache(maxsize=None)
def case(shape, dtname):
    """CPU inputs of every entry at one shape and dtype with their fp64 references, computed once and shared (the
    tests only read them)."""
    B, n, d, h = shape
    K, dt = n * d, DT[dtname]
    g = torch.Generator().manual_seed(B * 1000 + h * 7 + d)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dt)  # noqa: E731
    c = types.SimpleNamespace(B=B, n=n, d=d, h=h, K=K, dt=dt)
    c.x, c.W_enc, c.b_enc = mk(B, K), mk(h, K, sc=0.05), mk(h, sc=0.1)
    c.W_dec, c.b_dec, c.g_recon = mk(h, K, sc=0.05), mk(K, sc=0.1), mk(B, K, sc=1e-2)
    c.tn = torch.rand(h, generator=g) + 0.5
    c.recon = torch.randn(B, K, generator=g) * 0.3
    if h >= 8:
        c.W_enc[1], c.b_enc[1] = 0.0, -1.0       # dead: pre = -1 on every row
        c.W_enc[h - 2], c.b_enc[h - 2] = 0.0, 1.0  # always on
        c.W_dec[3] = 0.0
    assert bool((c.b_dec != 0).any())
    c.pre, c.A_pre = ref.encode(c.x, c.W_enc, c.b_enc)
    c.acts = ref.round_dt(torch.relu(c.pre), dt)
    c.x_mean = c.x.float().mean(0)
    c.loss = ref.loss(c.recon, c.b_dec, c.x, c.x_mean, 2.0 / B, n, d, dt)
    c.gpre, c.A_gpre = ref.dacts(c.g_recon, c.W_dec, c.acts, c.tn, L1_SCALE)
    c.g_pre = ref.round_dt(c.gpre, dt)
    c.norms, c.tot, c.inv = ref.dec_norms(c.W_dec, n, d)
    c.inv32 = c.inv.float()
    c.colsum_acts = c.acts.float().sum(0)
    c.gWd, c.A_gWd, c.l1_term = ref.wgrad_dec(c.acts, c.g_recon, c.W_dec, c.inv32, c.colsum_acts, L1_SCALE, n, d)
    c.gWe, c.A_gWe = ref.wgrad_enc(c.g_pre, c.x)
    return c


class Dev:
    """The named inputs of a case on the GPU; unchanged() compares them with the CPU originals afterwards."""

    def __init__(self, c, dev, *names):
        self._c, self._names = c, names
        for k in names:
            setattr(self, k, getattr(c, k).to(dev))

    def unchanged(self):
        for k in self._names:
            a, b = getattr(self, k).cpu(), getattr(self._c, k)
            assert torch.equal(a.view(torch.uint8), b.contiguous().view(torch.uint8)), f"input {k} was written"


def canaried(rows, cols, dtype, dev, extra_rows=2):
    return torch.full((rows + extra_rows, cols), CANARY, dtype=dtype, device=dev)


def canaried1(numel, dev, dtype=F32):
    return torch.full((numel + 8,), CANARY, dtype=dtype, device=dev)


def intact(full, extent, name):
    """The canary past the logical extent (rows of a 2-D output, elements of a 1-D one) survived and none is left
    inside."""
    assert bool((full[extent:] == CANARY).all()), f"{name}: written past its extent"
    assert not bool((full[:extent] == CANARY).any()), f"{name}: elements inside its extent were not written"


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def transposed_ok(B, K, h, dt):
    return bool(ops.lib().cc_transposed_ok(B, K, h, ops.dtype_code(dt)))


# ----------------------------------------------------------------------------- cc_prep_input
@pytest.mark.parametrize("shape", SHAPES + [WIDE], ids=sid)
def test_prep_input(gpu, shape):
    B, n, d, _ = shape
    K, R = n * d, ops.prep_part_rows(B)
    g = torch.Generator().manual_seed(B + d)
    raw, fac = torch.randn(B, n, d, generator=g) * 3, torch.tensor([0.7, 1.3, 0.9][:n])
    worst = 0.0
    for in_dt in (F32, BF16):
        for f_dt in (F32, BF16, None):
            for out_dt in (BF16, F32):
                name = f"prep {in_dt} * {f_dt} -> {out_dt}"
                x_in = raw.to(in_dt)
                factor = None if f_dt is None else fac.to(f_dt)
                want, s64, A = ref.prep(x_in, factor, out_dt)
                xg, fg = x_in.to(gpu), None if factor is None else factor.to(gpu)
                out, part, out2 = canaried(B, K, out_dt, gpu), canaried(R, K, F32, gpu), canaried(B, K, out_dt, gpu)
                ops.prep_input(xg, fg, out_dt, out=out, colsum_part=part)
                ops.prep_input(xg, fg, out_dt, out=out2)
                torch.cuda.synchronize()
                assert same_bits(out[:B].cpu(), want), name
                assert same_bits(out2, out), name
                intact(out, B, name)
                intact(part, R, name + " colsum_part")
                assert same_bits(xg.cpu(), x_in) and (fg is None or same_bits(fg.cpu(), factor))
                worst = max(worst, ref.check(part[:R].double().sum(0), s64, ref.acc_bound(B, A), name + " colsum"))
    report("prep_input", "all", shape, colsum=worst)


# ----------------------------------------------------------------------------- cc_encode_fwd
WAVE_TERMS = 128 * 64  # outputs of one wave's sub-tile: the fp32 terms of one l1 partial (8 per 256 x 256 tile)


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_encode_fwd(gpu, mode, shape):
    B, n, d, h = shape
    dt = dtype_of(mode)
    c = case(shape, mode.split("_")[0])
    K, R, nw = c.K, ops.col_part_rows(B), ops.wave_parts(B, h)
    D = Dev(c, gpu, "x", "W_enc", "b_enc", "tn")
    tn64 = ref.f64(c.tn)

    def run(relu, want):
        acts = canaried(B, h, dt, gpu)
        col = canaried(R, h, F32, gpu) if "col" in want else None
        l1 = canaried1(nw, gpu) if "l1" in want else None
        l0 = canaried1(nw, gpu) if "l0" in want else None
        ops.encode_fwd(D.x, D.W_enc, D.b_enc, acts, relu, tn=D.tn, colsum_part=col, l1_part=l1, l0_part=l0)
        return acts, col, l1, l0

    def check_sides(tag, acts, col, l1, l0):
        """The side outputs against fp64 sums of the launch's own stored activations."""
        stored, r = ref.f64(acts[:B]), {}
        intact(acts, B, tag + " acts")
        if col is not None:
            intact(col, R, tag + " colsum_part")
            r["colsum"] = ref.check(col[:R].double().sum(0), stored.sum(0), ref.acc_bound(B, stored.abs().sum(0)),
                                    tag + " colsum")
        if l1 is not None:
            intact(l1, nw, tag + " l1_part")
            r["l1"] = ref.check(l1[:nw].double().sum(), (stored * tn64).sum(),
                                ref.acc_bound(WAVE_TERMS, (stored.abs() * tn64).sum()), tag + " l1")
        if l0 is not None:
            intact(l0, nw, tag + " l0_part")
            assert l0[:nw].double().sum().item() == float((stored > 0).sum()), tag + " l0"
        return r

    for relu in (False, True):
        tag = f"encode relu={int(relu)}"
        runs = [run(relu, w) for w in (("col", "l1", "l0"), ("col",), ("l1",), ("l0",), ("col", "l0"), ())]
        torch.cuda.synchronize()
        acts = runs[0][0]
        v64 = torch.relu(c.pre) if relu else c.pre
        bound = ref.acc_bound(K, c.A_pre) + ref.store_bound(v64, dt)
        r = {"acts": ref.check(acts[:B], v64, bound, tag + " acts")}
        r.update(check_sides(tag, *runs[0]))
        for other in runs[1:]:  # the side outputs requested alone: the same acts bits, the same checks
            assert same_bits(other[0], acts), tag
            check_sides(tag + " alone", *other)
        if relu:
            stored = ref.f64(acts[:B])
            assert bool((stored >= 0).all())
            if h >= 8:
                assert bool((stored[:, 1] == 0).all()) and bool((stored[:, h - 2] > 0).all())
            # the active set is the reference's wherever |pre64| exceeds its bound; the band holds < 1 % of the elements
            clear = c.pre.abs() > ref.acc_bound(K, c.A_pre) + ref.store_bound(c.pre, dt)
            assert bool(((stored > 0) == (c.pre > 0))[clear].all()), tag + " active set"
            assert float((~clear).double().mean()) < 0.01
        report("encode_fwd", mode, shape, relu=float(relu), **r)
    # the transposed-output form the step runs (mask bits given): the same acts bits, acts_t their transpose
    if transposed_ok(B, K, h, dt):
        acts_r = runs[0][0]
        acts2, acts_t = canaried(B, h, dt, gpu), canaried(h, B, dt, gpu)
        col, l0 = canaried(R, h, F32, gpu), canaried1(nw, gpu)
        bits = torch.zeros(ops.mask_bits_words(B, h) + 8, dtype=torch.int32, device=gpu)
        ops.encode_fwd_t(D.x, D.W_enc, D.b_enc, acts2, acts_t, True, colsum_part=col, l0_part=l0, mask_bits=bits)
        torch.cuda.synchronize()
        assert same_bits(acts2, acts_r), "encode_fwd_t acts"
        assert same_bits(acts_t[:h], acts2[:B].t().contiguous()), "encode_fwd_t acts_t"
        intact(acts_t, h, "encode_fwd_t acts_t")
        assert not bool(bits[-8:].any())
        v64 = torch.relu(c.pre)
        r = {"acts": ref.check(acts2[:B], v64, ref.acc_bound(K, c.A_pre) + ref.store_bound(v64, dt), "encode_fwd_t")}
        r.update(check_sides("encode_fwd_t", acts2, col, None, l0))
        report("encode_fwd_t", mode, shape, **r)
    D.unchanged()


# ----------------------------------------------------------------------------- cc_decode_fwd
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_decode_fwd(gpu, mode, shape):
    B, n, d, h = shape
    dt = dtype_of(mode)
    c = case(shape, mode.split("_")[0])
    K = c.K
    D = Dev(c, gpu, "acts", "W_dec", "b_dec")
    r32, r32_nb, rt, r32_both, rt_both = (canaried(B, K, F32, gpu), canaried(B, K, F32, gpu), canaried(B, K, dt, gpu),
                                          canaried(B, K, F32, gpu), canaried(B, K, dt, gpu))
    ops.decode_fwd(D.acts, D.W_dec, D.b_dec, recon_f32=r32)
    ops.decode_fwd(D.acts, D.W_dec, None, recon_f32=r32_nb)
    ops.decode_fwd(D.acts, D.W_dec, D.b_dec, recon_t=rt)
    ops.decode_fwd(D.acts, D.W_dec, D.b_dec, recon_f32=r32_both, recon_t=rt_both)
    torch.cuda.synchronize()
    v, A = ref.decode(c.acts, c.W_dec, c.b_dec)
    v_nb, A_nb = ref.decode(c.acts, c.W_dec)
    # (the contraction is over h: h = 200 and 520 are the k tails of the MN-layout operand)
    r = {"recon_f32": ref.check(r32[:B], v, ref.acc_bound(h, A), "recon_f32"),
         "no_bias": ref.check(r32_nb[:B], v_nb, ref.acc_bound(h, A_nb), "recon_f32 without b_dec"),
         "recon_t": ref.check(rt[:B], v, ref.acc_bound(h, A) + ref.store_bound(v, dt), "recon_t")}
    assert same_bits(r32_both, r32) and same_bits(rt_both, rt)
    for t, nm in ((r32, "recon_f32"), (r32_nb, "recon_f32 without b_dec"), (rt, "recon_t")):
        intact(t, B, nm)
    # the bias reaches the output: on most columns b_dec is far beyond the column's largest bound
    assert float((ref.f64(c.b_dec).abs() > 4 * ref.acc_bound(h, A).max(0).values).double().mean()) > 0.5
    D.unchanged()
    report("decode_fwd", mode, shape, **r)


# ----------------------------------------------------------------------------- cc_loss_fwd_bwd(_rows)
def loss_launch(D, c, gpu, ranges=None, raw_entry=False):
    """cc_loss_fwd_bwd over the whole batch (raw_entry: the entry itself, else cc_loss_fwd_bwd_rows), or one
    cc_loss_fwd_bwd_rows call per (row0, rows) range -> the canaried g_recon, row_part (flat), col_part."""
    B, n, d, K = c.B, c.n, c.d, c.K
    ncb, R = ops.loss_col_blocks(d), ops.loss_part_rows(B)
    g = canaried(B, K, c.dt, gpu)
    rp, cp = canaried1(2 * n * ncb * B, gpu), canaried(R, K, F32, gpu)
    if raw_entry:
        p = lambda t: t.data_ptr()  # noqa: E731
        ops.check(ops.lib().cc_loss_fwd_bwd(p(D.recon), p(D.b_dec), p(D.x), p(D.x_mean), p(g), p(rp), p(cp), 2.0 / B,
                                            B, n, d, ops.dtype_code(c.dt), torch.cuda.current_stream(gpu).cuda_stream))
    else:
        for row0, rows in (ranges or [(0, B)]):
            ops.loss_fwd_bwd(D.recon, D.b_dec, D.x, D.x_mean, g, rp, cp, 2.0 / B, B, n, d, row0=row0, rows=rows)
    return g, rp, cp


def row_terms(rp, B, n, d):
    """row_part [2][n * ncb][B] -> (l2, tv) [B, n] in fp64: a model's column blocks summed."""
    ncb = ops.loss_col_blocks(d)
    t = rp[:2 * n * ncb * B].double().cpu().view(2, n, ncb, B).sum(2)
    return t[0].t(), t[1].t()


@pytest.mark.parametrize("dtname", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + [WIDE], ids=sid)
def test_loss_fwd_bwd(gpu, shape, dtname):
    B, n, d, _ = shape
    c = case(shape, dtname)
    K, dt = c.K, c.dt
    ncb, R = ops.loss_col_blocks(d), ops.loss_part_rows(B)
    D = Dev(c, gpu, "recon", "b_dec", "x", "x_mean")
    g, rp, cp = loss_launch(D, c, gpu)
    g_raw, rp_raw, cp_raw = loss_launch(D, c, gpu, raw_entry=True)
    split = loss_launch(D, c, gpu, ranges=[(32, B - 32), (0, 32)]) if B > 32 else None
    torch.cuda.synchronize()
    lo = c.loss
    r = {"g_recon": ref.check(g[:B], lo["g"], 8 * ref.EPS23 * lo["Ag"] + ref.store_bound(lo["g"], dt), "g_recon")}
    l2, tv = row_terms(rp, B, n, d)
    r["l2_rows"] = ref.check(l2, lo["l2"], ref.acc_bound(d, lo["A_l2"]), "row_part l2")
    r["tv_rows"] = ref.check(tv, lo["tv"], ref.acc_bound(d, lo["A_tv"]), "row_part tv")
    stored = ref.f64(g[:B])
    r["col_part"] = ref.check(cp[:R].double().sum(0), stored.sum(0), ref.acc_bound(B, stored.abs().sum(0)), "col_part")
    intact(g, B, "g_recon")
    intact(rp, 2 * n * ncb * B, "row_part")
    intact(cp, R, "col_part")
    assert same_bits(g_raw, g) and same_bits(rp_raw, rp) and same_bits(cp_raw, cp)
    if split is not None:  # the whole batch in one call and the ranges [0, 32), [32, B): the same bits
        for a, b, nm in zip(split, (g, rp, cp), ("g_recon", "row_part", "col_part")):
            assert same_bits(a, b), nm + " from two row ranges"
    D.unchanged()
    report("loss_fwd_bwd", dtname, shape, **r)


# ----------------------------------------------------------------------------- cc_loss_finalize
@pytest.mark.parametrize("dtname", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + [WIDE], ids=sid)
def test_loss_finalize(gpu, shape, dtname):
    """From the kernels' own row_part (cc_loss_fwd_bwd), l1_part and l0_part (cc_encode_fwd) against loss_scalars
    fed the same slabs in fp64.  ev_a / ev_b are models 0 and 1 for every n >= 2 (as get_losses indexes them; n = 3
    here too), and ev_b is exactly 0 for a single model."""
    B, n, d, h = shape
    c = case(shape, dtname)
    ncb, nw = ops.loss_col_blocks(d), ops.wave_parts(B, h)
    D = Dev(c, gpu, "recon", "b_dec", "x", "x_mean", "W_enc", "b_enc", "tn")
    _, rp, _ = loss_launch(D, c, gpu)
    acts, l1, l0 = torch.empty(B, h, dtype=c.dt, device=gpu), canaried1(nw, gpu), canaried1(nw, gpu)
    ops.encode_fwd(D.x, D.W_enc, D.b_enc, acts, True, tn=D.tn, l1_part=l1, l0_part=l0)
    rp_before, l1_before = rp.clone(), l1.clone()
    ev, ev_a, ev_b = canaried1(B, gpu), canaried1(B, gpu), canaried1(B, gpu)
    ns = ops.loss_scalars_len(B)
    scalars, l1l0 = canaried1(ns, gpu), canaried1(2, gpu)
    ops.loss_finalize(rp, l1, nw, l0, nw, ev, ev_a, ev_b, scalars, B, n, d, l1l0_out=l1l0)
    torch.cuda.synchronize()
    l2_rm, tv_rm = row_terms(rp, B, n, d)
    B_l1, active = l1[:nw].double().sum().item(), l0[:nw].double().sum().item()
    sc = ref.loss_scalars(l2_rm, tv_rm, B_l1, active, B)
    L = B + n * ncb
    eps = 1e-8
    A_ev = 1 + l2_rm.sum(1) / (tv_rm.sum(1) + eps)
    A_a = 1 + l2_rm[:, 0] / (tv_rm[:, 0] + eps)
    A_b = 1 + l2_rm[:, -1 if n == 1 else 1] / (tv_rm[:, -1 if n == 1 else 1] + eps)
    r = {"ev": ref.check(ev[:B], sc["ev"], ref.acc_bound(L, A_ev), "ev"),
         "ev_a": ref.check(ev_a[:B], sc["ev_a"], ref.acc_bound(L, A_a), "ev_a")}
    if n == 1:
        assert bool((ev_b[:B] == 0).all()) and scalars[5].item() == 0.0
    else:
        r["ev_b"] = ref.check(ev_b[:B], sc["ev_b"], ref.acc_bound(L, A_b), "ev_b")
    want = [sc["l2"], sc["l1"], sc["l0"], sc["mean_ev"], sc["mean_ev_a"], sc["mean_ev_b"]]
    mags = [sc["l2"], l1[:nw].double().abs().sum().item() / B, sc["l0"], A_ev.sum() / B, A_a.sum() / B, A_b.sum() / B]
    for i, nm in enumerate(("l2", "l1", "l0", "mean_ev", "mean_ev_a", "mean_ev_b")):
        if n == 1 and nm == "mean_ev_b":
            continue
        r[nm] = ref.check(scalars[i], want[i], ref.acc_bound(L, float(mags[i])), "scalars " + nm)
    assert scalars[6].item() == 0.0 and scalars[7].item() == 0.0
    assert same_bits(l1l0[:2], scalars[1:3])
    for t, ext, nm in ((ev, B, "ev"), (ev_a, B, "ev_a"), (ev_b, B, "ev_b"), (scalars, ns, "scalars"), (l1l0, 2, "l1l0")):
        intact(t, ext, nm)
    assert same_bits(rp, rp_before) and same_bits(l1, l1_before)
    D.unchanged()
    report("loss_finalize", dtname, shape, **r)


# ----------------------------------------------------------------------------- cc_dacts_bwd
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_dacts_bwd(gpu, mode, shape):
    B, n, d, h = shape
    dt = dtype_of(mode)
    c = case(shape, mode.split("_")[0])
    K, R = c.K, ops.col_part_rows(B)
    D = Dev(c, gpu, "g_recon", "W_dec", "acts", "tn", "x", "W_enc", "b_enc")
    g_pre, col, g_pre2 = canaried(B, h, dt, gpu), canaried(R, h, F32, gpu), canaried(B, h, dt, gpu)
    ops.dacts_bwd(D.g_recon, D.W_dec, D.acts, D.tn, L1_SCALE, g_pre, colsum_part=col)
    ops.dacts_bwd(D.g_recon, D.W_dec, D.acts, D.tn, L1_SCALE, g_pre2)
    torch.cuda.synchronize()
    bound = ref.acc_bound(K, c.A_gpre) + ref.store_bound(c.gpre, dt)
    on = ref.f64(c.acts) > 0
    # the L1 term is visible: on every unmasked element it exceeds the element's bound
    assert bool((L1_SCALE * ref.f64(c.tn)[None, :].expand_as(bound)[on] > 2 * bound[on]).all())
    r = {"g_pre": ref.check(g_pre[:B], c.gpre, bound, "g_pre")}
    stored = ref.f64(g_pre[:B])
    assert bool((stored[~on] == 0).all()), "masked elements of g_pre"  # (the mask comes from the given acts: exact)
    if h >= 8:
        assert bool((stored[:, 1] == 0).all()) and bool(on[:, h - 2].all())
    r["colsum"] = ref.check(col[:R].double().sum(0), stored.sum(0), ref.acc_bound(B, stored.abs().sum(0)), "colsum_part")
    intact(g_pre, B, "g_pre")
    intact(col, R, "colsum_part")
    assert same_bits(g_pre2, g_pre)
    report("dacts_bwd", mode, shape, **r)
    if transposed_ok(B, K, h, dt):
        # the step's form: acts and their mask bits from cc_encode_fwd_t, g_pre stored transposed only
        acts = torch.empty(B, h, dtype=dt, device=gpu)
        acts_t = torch.empty(h, B, dtype=dt, device=gpu)
        bits = torch.zeros(ops.mask_bits_words(B, h), dtype=torch.int32, device=gpu)
        ops.encode_fwd_t(D.x, D.W_enc, D.b_enc, acts, acts_t, True, mask_bits=bits)
        outs = []
        for mb in (bits, None):
            gt, colt = canaried(h, B + 8, dt, gpu), canaried(R, h, F32, gpu)
            ops.dacts_bwd_t(D.g_recon, D.W_dec, acts, D.tn, L1_SCALE, gt[:h, :B], colsum_part=colt, mask_bits=mb)
            outs.append((gt, colt))
        torch.cuda.synchronize()
        v, A = ref.dacts(c.g_recon, c.W_dec, acts, c.tn, L1_SCALE)
        gt, colt = outs[0]
        rt = {"g_pre_t": ref.check(gt[:h, :B].t(), v, ref.acc_bound(K, A) + ref.store_bound(v, dt), "g_pre_t")}
        st = ref.f64(gt[:h, :B]).t()
        assert bool((st[ref.f64(acts) <= 0] == 0).all())
        rt["colsum"] = ref.check(colt[:R].double().sum(0), st.sum(0), ref.acc_bound(B, st.abs().sum(0)), "colsum_part (t)")
        assert bool((gt[h:] == CANARY).all()) and bool((gt[:h, B:] == CANARY).all())
        assert not bool((gt[:h, :B] == CANARY).any())
        intact(colt, R, "colsum_part (t)")
        assert same_bits(outs[1][0], gt), "g_pre_t with and without mask bits"
        report("dacts_bwd_t", mode, shape, **rt)
    D.unchanged()


# ----------------------------------------------------------------------------- cc_wgrad_dec / _enc / _both
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_wgrad(gpu, mode, shape):
    B, n, d, h = shape
    dt = dtype_of(mode)
    c = case(shape, mode.split("_")[0])
    K, P = c.K, ops.wgrad_parts(h, c.K, dt)
    D = Dev(c, gpu, "acts", "g_recon", "W_dec", "inv32", "colsum_acts", "g_pre", "x")
    gd, ge, gd2, ge2 = (canaried(h, K, dt, gpu) for _ in range(4))
    sd, se, sd2, se2 = (canaried1(P, gpu) for _ in range(4))
    ops.wgrad_dec(D.acts, D.g_recon, D.W_dec, D.inv32, D.colsum_acts, L1_SCALE, gd, sd, n, d)
    ops.wgrad_enc(D.g_pre, D.x, ge, se)
    ops.wgrad_both(D.acts, D.g_recon, D.W_dec, D.inv32, D.colsum_acts, L1_SCALE, gd2, sd2, D.g_pre, D.x, ge2, se2, n, d)
    torch.cuda.synchronize()
    # (the contraction is over B: B = 1, 96 and 300 are the k tails)
    bound_d = ref.acc_bound(B, c.A_gWd) + ref.store_bound(c.gWd, dt)
    r = {"dW_dec": ref.check(gd[:h], c.gWd, bound_d, "dW_dec"),
         "dW_enc": ref.check(ge[:h], c.gWe, ref.acc_bound(B, c.A_gWe) + ref.store_bound(c.gWe, dt), "dW_enc")}
    if h >= 8:
        live = ref.f64(c.colsum_acts) > 0
        live[3] = False
        # the L1 term is visible on every live row; the zero-norm row has none; the dead latent's row is exactly 0
        assert int(live.sum()) >= 1 and bool((c.l1_term.abs()[live] > 2 * bound_d[live]).any(1).all())
        assert bool((c.l1_term[3] == 0).all()) and bool((c.inv32[3] == 0).all())
        assert bool((gd[1] == 0).all()) and bool((ge[1] == 0).all())
    for grad, sq, nm in ((gd, sd, "dW_dec"), (ge, se, "dW_enc")):
        ss = ref.f64(grad[:h]).pow(2).sum()
        r["sq_" + nm] = ref.check(sq[:P].double().sum(), ss, ref.acc_bound(h * K / 64, ss), "sq_part " + nm)
        intact(grad, h, nm)
        intact(sq, P, "sq_part " + nm)
    assert same_bits(gd2, gd) and same_bits(ge2, ge) and same_bits(sd2, sd) and same_bits(se2, se), "cc_wgrad_both"
    D.unchanged()
    report("wgrad", mode, shape, **r)


# ----------------------------------------------------------------------------- cc_dec_norms
@pytest.mark.parametrize("dtname", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + [WIDE], ids=sid)
def test_dec_norms(gpu, shape, dtname):
    B, n, d, h = shape
    c = case(shape, dtname)
    D = Dev(c, gpu, "W_dec")
    norms, tot, inv = canaried(h, n, F32, gpu), canaried1(h, gpu), canaried(h, n, F32, gpu)
    tot2 = canaried1(h, gpu)
    ops.dec_norms(D.W_dec, h, n, d, norms=norms, total=tot, inv_norms=inv)
    ops.dec_norms(D.W_dec, h, n, d, total=tot2)
    torch.cuda.synchronize()
    rel = (d / 2 + 8) * ref.EPS23
    r = {"norms": ref.check(norms[:h], c.norms, rel * c.norms, "norms"),
         "total": ref.check(tot[:h], c.tot, rel * c.tot, "total"),
         "inv": ref.check(inv[:h], c.inv, rel * c.inv, "inv_norms")}
    if h >= 8:
        assert bool((c.norms[3] == 0).all())
        assert bool((norms[3] == 0).all()) and tot[3].item() == 0.0 and bool((inv[3] == 0).all())
    assert same_bits(tot2, tot)
    intact(norms, h, "norms")
    intact(tot, h, "total")
    intact(inv, h, "inv_norms")
    D.unchanged()
    report("dec_norms", dtname, shape, **r)


# ----------------------------------------------------------------------------- cc_reduce_rows
@pytest.mark.parametrize("R", [1, 2, 5])
@pytest.mark.parametrize("C", [8, 200, 520])
def test_reduce_rows(gpu, C, R):
    ld, scale, nb = C + 8, 0.37, ops.reduce_parts(C)
    g = torch.Generator().manual_seed(C + R)
    slab = torch.randn(R + 2, ld, generator=g)
    w = torch.rand(C, generator=g) + 0.5
    sg, wg = slab.to(gpu), w.to(gpu)
    s64, A = ref.colsum(slab[:R, :C])
    s64, A = s64 * float(torch.tensor(scale)), A * float(torch.tensor(scale))  # (the fp32 value of the scale)
    r = {}
    for dt in (F32, BF16):
        out32, out_t, sq, dot = canaried1(C, gpu), canaried1(C, gpu, dt), canaried1(nb, gpu), canaried1(nb, gpu)
        ops.reduce_rows(sg, R, C, scale=scale, out_f32=out32, out_t=out_t, sq_part=sq, ld=ld, dot_w=wg, dot_part=dot)
        only32 = canaried1(C, gpu)
        ops.reduce_rows(sg, R, C, scale=scale, out_f32=only32, ld=ld)
        torch.cuda.synchronize()
        nm = f"reduce_rows {dt}"
        r["out_f32"] = ref.check(out32[:C], s64, ref.acc_bound(R, A), nm + " out_f32")
        r[f"out_t_{dt}".replace("torch.", "")] = ref.check(out_t[:C], s64, ref.acc_bound(R, A) + ref.store_bound(s64, dt),
                                                           nm + " out_t")
        assert same_bits(out_t[:C], out32[:C].to(dt)) and same_bits(only32, out32)
        # per 64-column block: the squares of the stored out_t, and out_f32 . dot_w
        pad = lambda v: torch.cat([v, v.new_zeros(nb * 64 - C)]).view(nb, 64)  # noqa: E731
        q = pad(ref.f64(out_t[:C]).pow(2)).sum(1)
        r["sq_part"] = ref.check(sq[:nb], q, ref.acc_bound(64, q), nm + " sq_part")
        terms = ref.f64(out32[:C]) * ref.f64(w)
        r["dot_part"] = ref.check(dot[:nb], pad(terms).sum(1), ref.acc_bound(64, pad(terms.abs()).sum(1)), nm + " dot_part")
        for t, ext, tn_ in ((out32, C, "out_f32"), (out_t, C, "out_t"), (sq, nb, "sq_part"), (dot, nb, "dot_part")):
            intact(t, ext, nm + " " + tn_)
        assert same_bits(sg.cpu(), slab) and same_bits(wg.cpu(), w)
    report("reduce_rows", "both", f"C{C}_R{R}", **r)


# ----------------------------------------------------------------------------- cc_clip_finalize
def clip_run(gpu, sq, off, max_norm, emulate):
    out = canaried1(2 + len(off) - 1, gpu)
    ops.clip_finalize(sq, off, max_norm, emulate, out)
    torch.cuda.synchronize()
    intact(out, 2 + len(off) - 1, "clip out")
    return out.cpu()


def test_clip_finalize(gpu):
    sizes = (1000, 3000, 16, 40)
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    # an all-zero gradient list: coefficient exactly 1, norms exactly 0, in every mode
    for emulate in (0, 1, 2):
        out = clip_run(gpu, torch.zeros(off[-1], device=gpu), off, 1.0, emulate)
        assert out[0].item() == 1.0 and bool((out[1:6] == 0).all())
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(s, generator=g) for s in sizes]
    norm0 = math.sqrt(sum(float(t.double().pow(2).sum()) for t in base))
    worst = 0.0
    for target in (0.999, 1.001, 1e-3, 30.0):  # total norms just below and just above max_norm = 1, and far from it
        grads = [t * (target / norm0) for t in base]
        # fp32 mode: fp64 is the reference
        sq = torch.cat([t.pow(2) for t in grads]).to(gpu)
        out = clip_run(gpu, sq, off, 1.0, 0)
        sums = [float(sq[a:b].double().sum()) for a, b in zip(off, off[1:])]
        total, coef, norms = ref.clip(sums, 1.0)
        rel = 2.0 ** -22
        worst = max(worst, ref.check(out[1], total, rel * total, "clip total"), ref.check(out[0], coef, rel * coef, "clip coef"),
                    ref.check(out[2:6], norms, rel * norms, "clip norms"))
        assert (out[0].item() == 1.0) == (target < 1.0)
        # bf16 mode: torch's clip_grad_norm_ on bf16 tensors with these squared sums (the rounding is torch's: one bf16
        # ulp, 2^-7, between two roundings of nearly the same number)
        gb = [t.to(BF16) for t in grads]
        sqb = torch.cat([t.float().pow(2) for t in gb]).to(gpu)
        out = clip_run(gpu, sqb, off, 1.0, 1)
        tt = O.clip_grad_norm([t.clone() for t in gb]).float().item()
        assert math.isclose(out[1].item(), tt, rel_tol=2.0 ** -7)
        assert math.isclose(out[0].item(), min(1.0, 1.0 / (tt + 1e-6)), rel_tol=2.0 ** -7)
        # mode 2 (four bf16 gradients, then fp32 ones): the restatement tests/test_jumprelu_host.py pins against torch
        off5 = off + [off[-1] + 24]
        sq5 = torch.cat([sqb, torch.full((24,), (0.3 * target) ** 2 / 24, device=gpu)])
        out = clip_run(gpu, sq5, off5, 1.0, 2)
        sums5 = [float(sq5[a:b].double().sum()) for a, b in zip(off5, off5[1:])]
        coef2, total2, norms2 = JR.clip_finaliser(sums5, 1.0, emulate=2)
        assert torch.equal(out[2:6], norms2[:4].float())
        assert math.isclose(out[6].item(), norms2[4].item(), rel_tol=1e-6)
        assert math.isclose(out[1].item(), total2.item(), rel_tol=1e-6) and math.isclose(out[0].item(), coef2.item(), rel_tol=1e-6)
    report("clip_finalize", "fp32", "4_params", worst=worst)


# ----------------------------------------------------------------------------- cc_gemm_f32out
@pytest.mark.parametrize("M,N,K,dtname", [(1, 8, 8, "fp32"), (1, 8, 8, "bf16"), (8, 4, 8, "fp32"), (264, 260, 72, "fp32")])
def test_gemm_f32out(gpu, M, N, K, dtname):
    """The four operand layouts, ldc > N.  A layout whose contiguous dimension is not a whole number of 16-byte
    vectors (include/crosscoder_hip.h: M = 1 with an M-contiguous A) is refused with CC_ERR_SHAPE."""
    dt = DT[dtname]
    epc = 16 // torch.empty(0, dtype=dt).element_size()
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    A, Bm = torch.randn(M, K, generator=g).to(dt), torch.randn(K, N, generator=g).to(dt)
    v, mag = ref.f64(A) @ ref.f64(Bm), ref.f64(A).abs() @ ref.f64(Bm).abs()
    worst, ran = 0.0, 0
    for al in (0, 1):
        for bl in (0, 1):
            A_st = (A.contiguous() if al == 0 else A.t().contiguous()).to(gpu)
            B_st = (Bm.t().contiguous() if bl == 0 else Bm.contiguous()).to(gpu)
            C = canaried(M, N + 4, F32, gpu)
            admitted = (K if al == 0 else M) % epc == 0 and (K if bl == 0 else N) % epc == 0
            if not admitted:
                with pytest.raises(RuntimeError, match="crosscoder_hip error 3"):
                    ops.gemm_f32out(A_st, al, B_st, bl, M, N, K, out=C)
                continue
            ops.gemm_f32out(A_st, al, B_st, bl, M, N, K, out=C)
            torch.cuda.synchronize()
            worst = max(worst, ref.check(C[:M, :N], v, ref.acc_bound(K, mag), f"gemm layouts ({al}, {bl})"))
            assert bool((C[M:] == CANARY).all()) and bool((C[:M, N:] == CANARY).all())
            assert not bool((C[:M, :N] == CANARY).any())
            ran += 1
    assert ran >= 2
    report("gemm_f32out", dtname, f"M{M}_N{N}_K{K}", worst=worst, layouts=float(ran))
