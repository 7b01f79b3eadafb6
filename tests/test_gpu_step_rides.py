"""Work of the step that rides in launches that exist anyway, against the launches of its own, bit for bit:
the next batch's prep in the encoder-half Adam launch (cc_adam_step_prep, engine.PREP_IN_ADAM) and b_dec's update in
the side-stream decoder-half Adam (cc_adam_dec_norms over the whole decoder half, engine.BDEC_IN_SIDE_ADAM)."""
import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import engine, ops
from tests._golden import load, step_fixtures

pytestmark = pytest.mark.gpu
STEP_FIXTURES = step_fixtures()

bf16 = torch.bfloat16
HP = (5e-5, 0.9, 0.999, 1e-8, 3)  # lr, beta1, beta2, eps, step


def _bits(t):
    return t.view(torch.int16) if t.dtype == bf16 else t


def _adam_operands(numel, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(numel, generator=g) * 0.1).to(bf16).to(gpu)
    gr = (torch.randn(numel, generator=g) * 1e-3).to(bf16).to(gpu)
    m = (torch.randn(numel, generator=g) * 1e-3).to(bf16).to(gpu)
    v = (torch.rand(numel, generator=g) * 1e-6).to(bf16).to(gpu)
    return p, gr, m, v


PREP_JOBS = [pytest.param(coef, B, d, pair[0], pair[1],
                          id=f"{coef}-{B}-{d}-in_dtype{k}-" + ("None" if pair[1] is None else f"factor_dtype{k}"))
             for k, pair in enumerate(((bf16, bf16), (torch.float32, torch.float32), (bf16, None)))
             for B, d in ((256, 64), (264, 64), (256, 128), (264, 128))
             for coef in (0.37, -1.0)]
# the other two (input, factor) dtype pairs, so that every pair runs with a factor that is read: one full 64-row
# block + 8 rows, K = 144 past one 128-column narrow block
PREP_JOBS += [pytest.param(0.37, 72, 72, torch.float32, bf16, id="0.37-72-72-fp32-bf16"),
              pytest.param(0.37, 72, 72, bf16, torch.float32, id="0.37-72-72-bf16-fp32")]


@pytest.mark.parametrize("coef,B,d,in_dtype,factor_dtype", PREP_JOBS)
def test_adam_with_prep_job_matches_the_two_launches(gpu, B, d, in_dtype, factor_dtype, coef):
    """cc_adam_step_prep against cc_adam_step then cc_prep_input_t: p, m, v, x, x^T and the column-sum partials.
    B 264: a last row block of 8 rows; h 520: a last Adam workgroup that is not full; coef -1 (CC_CLIP_ABORTED): no
    update, the prep still runs."""
    n, h = 2, 520
    K = n * d
    numel = h * K + h
    g = torch.Generator().manual_seed(B + d)
    x_in = (torch.randn(B, n, d, generator=g) * 3).to(in_dtype).to(gpu)
    factor = None if factor_dtype is None else torch.tensor([0.2759, 0.2442]).to(factor_dtype).to(gpu)
    c = torch.tensor([coef], device=gpu)
    rows = ops.prep_part_rows(B)
    outs = []
    for ride in (False, True):
        p, gr, m, v = _adam_operands(numel, gpu, 7)
        x = torch.full((B, K), 9.0, dtype=bf16, device=gpu)
        x_t = torch.full((K, B), 9.0, dtype=bf16, device=gpu)
        part = torch.full((rows, K), 9.0, device=gpu)
        if ride:
            assert ops.prep_job_ok(x_in, factor, bf16, x_t)
            ops.adam_step_prep(p, gr, m, v, c, *HP, ops.prep_job(x_in, factor, x, part, x_t))
        else:
            ops.adam_step(p, gr, m, v, c, *HP)
            ops.prep_input(x_in, factor, bf16, out=x, colsum_part=part, out_t=x_t)
        torch.cuda.synchronize()
        outs.append((p, m, v, x, x_t, part))
    for name, a, b in zip(("p", "m", "v", "x", "x_t", "colsum_part"), *outs):
        assert torch.equal(_bits(a), _bits(b)), name
    p0 = _adam_operands(numel, gpu, 7)[0]
    assert torch.equal(_bits(outs[1][0]), _bits(p0)) == (coef < 0)  # (updated, or the aborted step's untouched)
    assert torch.equal(outs[1][3].float(), (x_in.float() * (1 if factor is None else factor.float()[None, :, None]))
                       .to(bf16).float().view(B, K))


@pytest.mark.parametrize("h,d", [(520, 64), (64, 128)])
def test_adam_dec_norms_with_the_trailing_bias_matches_the_two_launches(gpu, h, d):
    """cc_adam_dec_norms over W_dec and b_dec in one capped launch against W_dec's launch followed by b_dec's own:
    p, m, v, the norm partials (none for b_dec) and the done counter."""
    n = 2
    K = n * d
    numel = h * K + K
    c = torch.tensor([0.61], device=gpu)
    outs = []
    for one in (False, True):
        p, gr, m, v = _adam_operands(numel, gpu, 11)
        part = torch.full((ops.dec_norms_part_floats(h, n, d),), 9.0, device=gpu)
        done = torch.zeros(8, dtype=torch.int32, device=gpu)
        if one:
            nb = ops.adam_dec_norms(p, gr, m, v, h, K, *HP, part, coef=c, max_blocks=4, done_ctr=done)
        else:
            nb = ops.adam_dec_norms(p[:h * K], gr[:h * K], m[:h * K], v[:h * K], h, K, *HP, part, coef=c,
                                    max_blocks=4, done_ctr=done)
            ops.adam_step(p[h * K:], gr[h * K:], m[h * K:], v[h * K:], c, *HP)
        torch.cuda.synchronize()
        assert int(done[0]) == nb
        outs.append((p, m, v, part))
    for name, a, b in zip(("p", "m", "v", "norm_part"), *outs):
        assert torch.equal(_bits(a), _bits(b)), name
    assert not torch.equal(_bits(outs[1][0][h * K:]), _bits(_adam_operands(numel, gpu, 11)[0][h * K:]))


def _cfg(gpu, B=512, d=128, h=1024):
    return dict(load(STEP_FIXTURES[0])["cfg"], d_in=d, dict_size=h, batch_size=B, enc_dtype="bf16",
                num_tokens=B * 20, device=str(gpu))


def _snapshot(cc, tr):
    st = tr.optimizer.state  # (orders after the side-stream Adam)
    m = torch.cat([st[p]["exp_avg"].detach().flatten().float() for p in cc.parameters()])
    v = torch.cat([st[p]["exp_avg_sq"].detach().flatten().float() for p in cc.parameters()])
    torch.cuda.synchronize()
    return cc.arena().data.clone(), m, v


@pytest.fixture(scope="module")
def plain_run(gpu):
    """3 steps with both rides forced off: loss dicts, params, both moments."""
    old = engine.PREP_IN_ADAM, engine.BDEC_IN_SIDE_ADAM
    engine.PREP_IN_ADAM = engine.BDEC_IN_SIDE_ADAM = False
    try:
        cfg = _cfg(gpu)
        cc = ca.CrossCoder(cfg)
        tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=cfg["batch_size"] * 3, seed=4), crosscoder=cc)
        dicts = [tr.step() for _ in range(3)]
        return dicts, _snapshot(cc, tr)
    finally:
        engine.PREP_IN_ADAM, engine.BDEC_IN_SIDE_ADAM = old


@pytest.mark.parametrize("prep,bias", [(True, True), (True, False), (False, True)])
def test_trainer_steps_are_bit_identical_with_the_rides(gpu, plain_run, monkeypatch, prep, bias):
    """3 Trainer steps (the buffer wraps around after the third batch's peek) with the prep and / or b_dec riding
    against both forced off: loss dicts, params and both moments; the prep launch really was skipped."""
    monkeypatch.setattr(engine, "PREP_IN_ADAM", prep)
    monkeypatch.setattr(engine, "BDEC_IN_SIDE_ADAM", bias)
    launches = []
    orig = ops.prep_input
    monkeypatch.setattr(ops, "prep_input", lambda *a, **k: (launches.append(1), orig(*a, **k))[1])
    cfg = _cfg(gpu)
    cc = ca.CrossCoder(cfg)
    tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=cfg["batch_size"] * 3, seed=4), crosscoder=cc)
    dicts = [tr.step() for _ in range(3)]
    assert len(launches) == (1 if prep else 3)  # (the first step has nothing to ride in)
    assert (cc._workspace(cfg["batch_size"], step=True).prep_token is not None) == prep
    snap = _snapshot(cc, tr)
    assert dicts == plain_run[0]
    for a, b in zip(snap, plain_run[1]):
        assert torch.equal(a, b)


def test_a_step_fed_another_batch_does_not_use_the_peeked_prep(gpu):
    """After a step whose Adam launch prepped the peeked batch, a step that is handed other rows (the buffer advanced
    in between; then rows rewritten in place; then a get_losses() on the shared workspace in between) runs its own
    prep: the same losses and params as a trainer with the ride off that sees the same batches."""
    cfg = _cfg(gpu)
    B = cfg["batch_size"]

    def run(ride):
        old = engine.PREP_IN_ADAM
        engine.PREP_IN_ADAM = ride
        try:
            cc = ca.CrossCoder(cfg)
            buf = ca.SyntheticBuffer(cfg, rows=B * 4, seed=5)
            tr = ca.Trainer(cfg, buffer=buf, crosscoder=cc)
            out = [tr.step()]
            buf.next_raw()  # (batch 1 goes elsewhere: the step gets batch 2, not the peeked batch 1)
            out.append(tr.step())
            # the peeked rows (batch 3) change in place before the step reads them
            buf.buffer[3 * B:4 * B] = buf.buffer[0:B] * 0.5
            out.append(tr.step())
            # another forward on the step's workspace between the peek (batch 0 again) and the step
            with torch.no_grad():
                cc.get_losses(buf.buffer[B:2 * B].float())
            out.append(tr.step())
            return out, _snapshot(cc, tr)
        finally:
            engine.PREP_IN_ADAM = old

    (d0, s0), (d1, s1) = run(False), run(True)
    assert d0 == d1
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)
