"""Dead-latent resampling on the GPU: cc_row_norms, cc_resample_pick and cc_resample_write
against the fp64 restatements and derived bounds of tests/_resample_ref.py, LatentResampler through the model, and
the invalidation list (nothing derived from the parameters is stale after a resample) through Trainer."""
import math

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops
from tests import _resample_ref as ref

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------- cc_row_norms
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("rows,K,ld", [(1, 8, 8), (5, 80, 80), (3, 2088, 2088), (64, 4608, 4608), (2051, 8, 8),
                                       (7, 520, 1048)])
def test_row_norms(gpu, dtype, rows, K, ld):
    g = torch.Generator().manual_seed(rows * 131 + K)
    full = (torch.randn(rows, ld, generator=g) * torch.rand(rows, 1, generator=g) * 3).to(DT[dtype])
    if rows > 2:
        full[2] = 0  # a zero row: norm +0
    W = full.to(gpu)[:, :K]
    out = torch.full((rows + 8,), -7.0, dtype=torch.float32, device=gpu)
    got = ops.row_norms(W, out=out[:rows])
    want = ref.row_norms(full[:, :K])
    err = ((got.cpu().double() - want).abs() / want.clamp(min=1e-300)).max().item()
    print(f"row_norms {dtype} ({rows}, {K}, ld {ld}): max rel err {err:.3e}, bound {ref.row_norm_tol(K):.3e}")
    assert err <= ref.row_norm_tol(K)
    if rows > 2:
        assert got[2].item() == 0.0
    assert bool((out[rows:] == -7.0).all())          # nothing past the rows
    assert same_bits(ops.row_norms(W), got)          # a second run: the same bits


# ---------------------------------------------------------------- cc_resample_pick
def pick_losses(R, seed=0):
    """seeded positive losses with a few exact zeros, one NaN and one negative (where R has room for them)"""
    g = torch.Generator().manual_seed(1000 + R + seed)
    loss = torch.rand(R, generator=g) * 4 + 0.01
    if R >= 8:
        loss[torch.randperm(R, generator=g)[:max(3, R // 16)]] = 0.0
        loss[R // 3], loss[R - 2] = float("nan"), -2.5
        loss[R // 2] = 3.0  # (a row with weight whatever the draw)
    return loss


@pytest.mark.parametrize("J", [1, 300])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 1025, 70001])
def test_pick(gpu, R, J):
    loss = pick_losses(R)
    c = ref.cdf(loss)
    w = ref.weights(loss)
    total = float(c[-1])
    safe = ref.safe_rows(loss)
    assert safe.numel() > 0
    g = torch.Generator().manual_seed(R * 7 + J)
    chosen = safe[torch.randint(safe.numel(), (J,), generator=g)]
    u = ref.midpoints(c, chosen)
    # the margin, on the CPU reference: every target sits at least 5e-7 of the total inside its row's interval, and
    # neither prefix sum is off by more than (R + 300) 2^-53 of the total (tests/_resample_ref.py)
    t = u * total
    lo = torch.where(chosen > 0, c[(chosen - 1).clamp(min=0)], torch.zeros((), dtype=torch.float64))
    margin = torch.minimum(t - lo, c[chosen] - t).min().item() / total
    assert margin >= 4.9e-7 and (R + 300) * ref.U64 + ref.pick_scan_tol(R) < 1e-3 * margin
    assert ref.pick(c, u).tolist() == chosen.tolist()
    rows, cdf = ops.resample_pick(loss.to(gpu), u.to(gpu))
    assert rows.dtype == torch.int64 and rows.cpu().tolist() == chosen.tolist()
    err = ((cdf.cpu() - c).abs().max() / total).item()
    print(f"pick R {R} J {J}: cdf max err / total {err:.3e}, bound {ref.pick_scan_tol(R) + R * ref.U64:.3e}")
    assert err <= ref.pick_scan_tol(R) + R * ref.U64
    # the prefix sums never decrease, and a row of weight 0 repeats its predecessor's bits
    cd = cdf.cpu()
    assert bool((cd[1:] >= cd[:-1]).all())
    zero = torch.nonzero(w == 0).flatten()
    zero = zero[zero > 0]
    assert same_bits(cd[zero], cd[zero - 1])
    # two runs: identical bits
    rows2, cdf2 = ops.resample_pick(loss.to(gpu), u.to(gpu))
    assert same_bits(cdf2, cdf) and torch.equal(rows2, rows)
    if J == 300:
        # a second set of seeded uniforms (with both ends of [0, 1)): never a zero-, NaN- or negative-loss row
        u2 = torch.rand(300, dtype=torch.float64, generator=g)
        u2[0], u2[1] = 0.0, 1.0 - 2.0 ** -53
        r2 = ops.resample_pick(loss.to(gpu), u2.to(gpu))[0].cpu()
        assert bool(((r2 >= 0) & (r2 < R)).all()) and bool((w[r2] > 0).all())
        # ... and each is the reference's row or, within the scan's rounding of an interval's end, its neighbour
        want = ref.pick(c, u2)
        off = torch.nonzero(r2 != want).flatten()
        for j in off.tolist():
            tj = float(u2[j]) * total
            edge = min(abs(float(c[r]) - tj) for r in (int(r2[j]), int(want[j]), max(int(min(r2[j], want[j])) - 1, 0)))
            assert edge <= 2 * (ref.pick_scan_tol(R) + R * ref.U64) * total, (j, int(r2[j]), int(want[j]))


@pytest.mark.parametrize("R", [1, 65, 5000])
def test_pick_without_weight(gpu, R):
    loss = torch.zeros(R)
    if R > 2:
        loss[1], loss[R - 1] = float("inf"), -1.0
        loss[2] = float("nan")
    u = torch.rand(17, dtype=torch.float64, generator=torch.Generator().manual_seed(R))
    rows, cdf = ops.resample_pick(loss.to(gpu), u.to(gpu))
    assert rows.cpu().tolist() == [-1] * 17
    assert bool((bits(cdf) == 0).all())


# ---------------------------------------------------------------- cc_resample_write
def arena_numel(h, K):
    return 2 * h * K + h + K


def row_slices(h, K, l):
    """the element ranges of latent l in an arena: W_enc row, b_enc entry, W_dec row"""
    return (slice(l * K, (l + 1) * K), slice(h * K + l, h * K + l + 1),
            slice(h * K + h + l * K, h * K + h + (l + 1) * K))


WRITE_SHAPES = [(8, 1, 8, 4, 1), (200, 2, 40, 96, 5), (64, 3, 696, 33, 7), (128, 2, 2304, 64, 16), (16, 2, 40, 8, 15)]


@pytest.mark.parametrize("mode", ["params", "opt", "opt-f32state", "master"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("h,n,d,R,J", WRITE_SHAPES)
def test_write(gpu, h, n, d, R, J, dtype, mode):
    """mode: params -- no optimizer, no masters; opt -- moments of the parameter dtype; opt-f32state -- fp32 moments;
    master -- fp32 masters and fp32 moments."""
    dt = DT[dtype]
    K = n * d
    N = arena_numel(h, K)
    g = torch.Generator().manual_seed(h * 1009 + K + J)
    X = (torch.randn(R, K, generator=g) * 1.7).to(dt)
    # latents: distinct, 0 and h - 1 among them; rows: repeated where J allows, one zero source row
    lat = torch.randperm(h, generator=g)[:J]
    if J >= 2:
        lat = torch.cat([torch.tensor([0, h - 1]), lat[(lat != 0) & (lat != h - 1)]])[:J]
    rows = torch.randint(R, (J,), generator=g)
    if J >= 3:
        rows[2] = rows[1]
    zero_j = None
    if J >= 5:
        zero_j = 3
        zrow = int(rows[zero_j])
        X[zrow] = 0
        rows = torch.where(rows == zrow, torch.tensor((zrow + 1) % R), rows)
        rows[zero_j] = zrow
    sdt = dt if mode == "opt" else torch.float32
    P0 = ref.pattern(N, dt, 1)
    M0, V0 = (ref.pattern(N, sdt, s) for s in (2, 3)) if mode != "params" else (None, None)
    W0 = ref.pattern(N, torch.float32, 4) if mode == "master" else None
    dev = lambda t: None if t is None else t.to(gpu)  # noqa: E731
    P, M, V, Wm = dev(P0), dev(M0), dev(V0), dev(W0)
    enc_norm, dec_norm = 0.0371, 0.913
    done = ops.resample_write(X.to(gpu), rows.to(gpu), lat.to(gpu), h, enc_norm, dec_norm, P, master=Wm, exp_avg=M,
                              exp_avg_sq=V)
    want_done = [0 if j == zero_j else 1 for j in range(J)]
    assert done.cpu().tolist() == want_done
    Pc = P.cpu()
    touched = torch.zeros(N, dtype=torch.bool)
    tol32 = ref.write_tol(K)
    tol = tol32 if dt == torch.float32 else ref.write_tol_bf16(K)
    worst = 0.0
    for j in range(J):
        if j == zero_j:
            continue
        l = int(lat[j])
        s_enc, s_benc, s_dec = row_slices(h, K, l)
        for sl, norm in ((s_enc, enc_norm), (s_dec, dec_norm)):
            want = ref.reseed(X[int(rows[j])], norm)
            got = Pc[sl].double()
            e = ((got - want).abs() / want.abs().clamp(min=1e-300))[want != 0]
            worst = max(worst, e.max().item() if e.numel() else 0.0)
            assert bool((got[want == 0] == 0).all())
            if Wm is not None:
                mw = Wm.cpu()[sl]
                em = ((mw.double() - want).abs() / want.abs().clamp(min=1e-300))[want != 0]
                assert em.numel() == 0 or em.max().item() <= tol32, (j, em.max().item(), tol32)
                assert same_bits(Pc[sl], mw.to(dt))  # the parameter is the master rounded to nearest-even
            touched[sl] = True
        assert bits(Pc[s_benc]).item() == 0
        touched[s_benc] = True
        for A in (M, V, Wm):
            if A is not None:
                assert bits(A.cpu()[s_benc]).item() == 0
        for A in (M, V):
            if A is not None:
                assert bool((bits(A.cpu()[s_enc]) == 0).all()) and bool((bits(A.cpu()[s_dec]) == 0).all())
    print(f"write {dtype} {mode} {(h, n, d, R, J)}: max rel err {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol
    # every other element of every arena, b_dec included, is what it was
    for A, A0 in ((P, P0), (M, M0), (V, V0), (Wm, W0)):
        if A is not None:
            assert same_bits(A.cpu()[~touched], A0[~touched])
    assert not bool(touched[2 * h * K + h:].any())


def test_write_skips_out_of_range(gpu):
    """a row index outside [0, R) (the -1 of an empty pick) and a latent outside [0, h) write nothing"""
    h, K, R = 16, 16, 4
    P0 = ref.pattern(arena_numel(h, K), torch.float32, 9)
    P = P0.to(gpu)
    X = torch.ones(R, K, device=gpu)
    done = ops.resample_write(X, torch.tensor([-1, R, 1, 2], device=gpu), torch.tensor([3, 4, -1, h], device=gpu), h,
                              1.0, 1.0, P)
    assert done.cpu().tolist() == [0, 0, 0, 0] and same_bits(P.cpu(), P0)


# ---------------------------------------------------------------- through the model
def small_cfg(dtype="bf16", B=64, d=64, h=256, **kw):
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 1e-3, "num_tokens": B * 100, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": dtype, "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    cfg.update(kw)
    return cfg


def kill(cc, D):
    with torch.no_grad():
        cc.b_enc[D] = -1e3


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_through_the_model(gpu, dtype):
    """Kill D, fill from four batches, apply.  With u32 = 2^-24, v = 2^-8 and e = write_tol / write_tol_bf16 of the
    shape (the re-seeded elements' relative error):
      encode(x)[l] = sum_c x_c W_enc[l][c] + 0 is a sum of K positive terms x_c^2 es (1 + e_c): an fp32 accumulation in
      any order is within K u32 of its exact value, relatively, the elements within e, and a bf16 output rounds once
      more (v): |acts - enc_norm ||x||| <= (e + K u32 + [v] + 1e-6) enc_norm ||x||, the 1e-6 for second-order terms.
      the full-row decoder norm sqrt(sum_m norms[l, m]^2): the elements within e move the norm by at most e, each
      per-model norm is an fp32 sum of d squares and a root ((d + 8) / 2 + 2 roundings at most, as for cc_row_norms
      with one more butterfly level): bound e + (d / 2 + 6) u32 + 1e-6."""
    B, d, h, n = 64, 64, 256, 2
    K = n * d
    cfg = small_cfg(dtype)
    cc = ca.CrossCoder(cfg)
    buf = ca.SyntheticBuffer(cfg, rows=4 * B, seed=3)
    D = torch.tensor([0, 17, 100, 101, 255], device=gpu)
    kill(cc, D)
    before = {k: v.detach().clone() for k, v in cc.state_dict().items()}
    rs = ca.LatentResampler(cc, rows=4 * B, seed=5)
    for _ in range(4):
        rs.add(buf.next())
    assert rs.filled == 4 * B
    with pytest.raises(ValueError, match="do not fit"):
        rs.add(buf.next())
    dead = rs.dead()
    assert dead.dtype == torch.bool and bool(dead[D].all())
    # the pool's losses are get_losses' squared errors
    x0 = rs._x[:B].view(B, n, d)
    with torch.no_grad():
        lo = cc.get_losses(x0.float())
    assert math.isclose(rs._loss[:B].double().mean().item(), lo.l2_loss.item(), rel_tol=1e-5)
    out = rs.apply()
    J = int(dead.sum())
    assert out["resampled"] == J == out["latents"].numel() and bool(out["written"].all())
    assert torch.equal(out["latents"], torch.nonzero(dead).flatten())
    assert set(out) == {"latents", "rows", "written", "enc_norm", "dec_norm", "resampled"}
    rows, lat = out["rows"], out["latents"]
    assert bool(((rows >= 0) & (rows < 4 * B)).all())
    # the norms: scale x the alive latents' mean row norm, from the parameters before the write
    alive = ~dead.cpu()
    W_enc_rows = before["W_enc"].permute(2, 0, 1).reshape(h, K).double().cpu()
    W_dec_rows = before["W_dec"].reshape(h, K).double().cpu()
    want_enc = 0.2 * W_enc_rows.pow(2).sum(1).sqrt()[alive].mean().item()
    want_dec = 1.0 * W_dec_rows.pow(2).sum(1).sqrt()[alive].mean().item()
    assert math.isclose(out["enc_norm"], want_enc, rel_tol=2 * ref.row_norm_tol(K))
    assert math.isclose(out["dec_norm"], want_dec, rel_tol=2 * ref.row_norm_tol(K))
    e = ref.write_tol(K) if dtype == "fp32" else ref.write_tol_bf16(K)
    xs = rs._x[rows]                               # [J, K], the crosscoder's dtype
    acts = cc.encode(xs.view(J, n, d))
    got = acts[torch.arange(J, device=gpu), lat].double().cpu()
    enc32 = float(torch.tensor(out["enc_norm"], dtype=torch.float32))
    want = enc32 * xs.double().pow(2).sum(1).sqrt().cpu()
    tol = e + K * ref.U32 + (ref.UBF if dtype == "bf16" else 0.0) + 1e-6
    err = ((got - want).abs() / want).max().item()
    print(f"encode of the source rows {dtype}: max rel err {err:.3e}, bound {tol:.3e}")
    assert bool((got > 0).all()) and err <= tol
    norms = ca.decoder_stats(cc)["norms"][lat].double().cpu()
    full = norms.pow(2).sum(1).sqrt()
    dec32 = float(torch.tensor(out["dec_norm"], dtype=torch.float32))
    tol = e + (d / 2 + 6) * ref.U32 + 1e-6
    err = ((full - dec32).abs() / dec32).max().item()
    print(f"decoder norms of the re-seeded latents {dtype}: max rel err {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    # b_enc of the re-seeded latents is 0, b_dec and the alive latents are untouched
    after = cc.state_dict()
    assert bool((after["b_enc"][lat] == 0).all())
    assert same_bits(after["b_dec"], before["b_dec"])
    keep = torch.nonzero(~dead).flatten()
    for k in ("W_dec", "b_enc"):
        assert same_bits(after[k][keep], before[k][keep]), k
    assert same_bits(after["W_enc"][:, :, keep], before["W_enc"][:, :, keep])
    # nothing to do: says so and writes nothing
    rs.reset()
    assert rs.filled == 0 and rs.apply(dead=D)["resampled"] == 0            # an empty pool
    rs.add(buf.next())
    snap = cc.arena().data.clone()
    assert rs.apply(dead=torch.zeros(h, dtype=torch.bool))["resampled"] == 0   # none dead
    assert rs.apply(dead=torch.ones(h, dtype=torch.bool))["resampled"] == 0    # all dead: no alive norm to take
    rs._loss.zero_()
    out = rs.apply(dead=D)                                                      # no row has weight
    assert out["resampled"] == 0 and out["rows"].cpu().tolist() == [-1] * 5
    assert same_bits(cc.arena().data, snap)


# ---------------------------------------------------------------- nothing stale
PARAMS = ("W_enc", "W_dec", "b_enc", "b_dec")
STALE_CASES = {"relu": {}, "relu-master": {"master_weights": True},
               "topk-auxk": {"activation": "topk", "k": 8, "auxk_coeff": 0.03, "k_aux": 16, "dead_tokens": 64},
               "topk-auxk-master": {"activation": "topk", "k": 8, "auxk_coeff": 0.03, "k_aux": 16, "dead_tokens": 64,
                                    "master_weights": True}}


def trainer_of(cfg, rows, seed=0):
    return ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=rows, seed=seed), crosscoder=ca.CrossCoder(cfg))


@pytest.mark.parametrize("case", list(STALE_CASES))
def test_nothing_stale(gpu, case):
    """A: 3 steps, a few latents killed, a resample with fixed u through Trainer.resample_dead_latents, 2 more steps.
    B: built fresh from A's CrossCoder.state_dict() and Trainer.state_dict() taken right after the resample, its buffer
    at A's position, the same 2 steps.  B derives everything from the parameters and the saved state; A carries the
    step workspace's decoder norms (and partials pending their finaliser), the masters' token, the AuxK counters and
    Arena.updates across the write.  Loss dicts and the four parameters must be bit-equal.
    The pool is filled before the three steps, so that no forward stands between the third step's Adam -- which leaves
    the decoder norms' partials pending their finaliser -- and the write."""
    B, d, h = 256, 64, 512
    cfg = small_cfg("bf16", B=B, d=d, h=h, lr=1e-2, **STALE_CASES[case])
    A = trainer_of(cfg, rows=9 * B)
    rs = ca.LatentResampler(A.crosscoder, rows=4 * B)
    for _ in range(4):
        rs.add(A.buffer.next())
    A.buffer.buffer_pointer = 0  # (the pool's batches are not taken from A's training stream here)
    for _ in range(3):
        A.step()
    A.synchronize()
    D = torch.tensor([0, 5, 64, 300, 511], device=gpu)
    kill(A.crosscoder, D)
    upd = A.crosscoder.arena().updates
    u = torch.linspace(0.03, 0.97, 5, dtype=torch.float64)
    out = A.resample_dead_latents(rs, dead=D, u=u)
    assert out["resampled"] == 5 and torch.equal(out["latents"], D)
    assert A.crosscoder.arena().updates == upd + 1
    o = A.optimizer
    if o.master_mode:
        assert o._master_token == o._arena_token(A.crosscoder.arena())  # valid without a re-seed
        a = A.crosscoder.arena()
        assert same_bits(o.master.data.to(torch.bfloat16), a.data)
    if A.auxk is not None:
        assert bool((A.tokens_since_fired[out["latents"]] == 0).all())
        assert A._dead_count == int((A.tokens_since_fired >= A.auxk[2]).sum())
    saved_cc = {k: v.detach().clone() for k, v in A.crosscoder.state_dict().items()}
    saved_tr = A.state_dict()
    Bt = trainer_of(cfg, rows=9 * B)
    Bt.crosscoder.load_state_dict(saved_cc)
    Bt.load_state_dict(saved_tr)
    Bt.buffer.buffer_pointer = A.buffer.buffer_pointer
    la = [A.step() for _ in range(2)]
    lb = [Bt.step() for _ in range(2)]
    assert la == lb, (la, lb)
    for k in PARAMS:
        assert same_bits(getattr(A.crosscoder, k).detach(), getattr(Bt.crosscoder, k).detach()), k
    A.synchronize()
    Bt.synchronize()
    for x, y in ((A.optimizer.exp_avg, Bt.optimizer.exp_avg), (A.optimizer.exp_avg_sq, Bt.optimizer.exp_avg_sq)):
        assert same_bits(x.data, y.data)
    # the re-seeded latents fire again: their encoder rows point at inputs of this distribution
    assert all(math.isfinite(v) for dct in la for v in dct.values())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_resample_every(gpu, dtype):
    """cfg["resample_every"] = 2 on a 6-step run: "resampled" on the resample steps only, the pool's batches consumed
    from the buffer, and the run bit-identical when repeated; without the key the loss dicts carry no such entry."""
    B, d, h = 64, 64, 256
    cfg = small_cfg(dtype, B=B, d=d, h=h, lr=1e-2, num_tokens=10 * B, resample_every=2, resample_rows=2 * B)

    def run():
        tr = trainer_of(cfg, rows=16 * B)
        kill(tr.crosscoder, torch.tensor([1, 2, 3], device=gpu))
        losses, ptrs = [], []
        for _ in range(6):
            losses.append(tr.step())
            ptrs.append(tr.buffer.buffer_pointer)
        tr.synchronize()
        return losses, ptrs, tr.crosscoder.arena().data.clone()

    l1, p1, a1 = run()
    l2, p2, a2 = run()
    assert ["resampled" in x for x in l1] == [False, True, False, True, False, True]
    assert l1[1]["resampled"] >= 3 and all(isinstance(x["resampled"], int) for x in l1[1::2])
    assert p1 == [B, 4 * B, 5 * B, 8 * B, 9 * B, 12 * B] == p2   # two pool batches consumed per resample
    assert l1 == l2 and same_bits(a1, a2)
    plain = trainer_of({k: v for k, v in cfg.items() if not k.startswith("resample")}, rows=16 * B)
    assert all("resampled" not in plain.step() for _ in range(3)) and plain._resampler is None
