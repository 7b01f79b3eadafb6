"""Master weights on the GPU (cfg["master_weights"]): cc_adam_master_step bit for bit against
the fp32 cc_adam_step plus torch's rounding, and against torch.optim.Adam on the CPU; Trainer.step in master mode
checked per step (masters, moments, the rounded parameters, the next step's losses), across torch writes, against
the fp32 oracle beside the default mode, and across a save / resume; and the default mode unchanged."""
import math

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import ops
from oracle import cpu_reference as O
from tests._master_adam_ref import MasterAdamRef

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 5e-5, 0.9, 0.999, 1e-8
BULK_TAIL = 8 * 256 * 2 + 5
STRIDED = 8 * 256 * 3 * 4  # with max_blocks = 3: every workgroup runs 4 rounds


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def operands(numel, seed=0):
    """(p32, g16, m32, v32) on the CPU.  Element i is of kind i % 8:
      0  all zero;  1  g = v = 0, so den = eps (m and p random);
      2 / 3  g = m = 0, so p32 stays, and p32 is exactly halfway between two bf16 values whose lower neighbour has an
             even (2) / odd (3) last bit: ties to even;
      4 / 5  the same midpoints (parities alternating) one fp32 ulp above (4) / below (5);
      6, 7   random."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(numel, generator=gen) * 0.05
    g = (torch.randn(numel, generator=gen) * 1e-3).to(torch.bfloat16)
    m = torch.randn(numel, generator=gen) * 1e-4
    v = torch.rand(numel, generator=gen) * 1e-6
    kind = torch.arange(numel) % 8
    z = kind == 0
    p[z], m[z], v[z] = 0.0, 0.0, 0.0
    g[z | (kind == 1)] = 0.0
    v[kind == 1] = 0.0
    mid = (kind >= 2) & (kind <= 5)
    g[mid] = 0.0
    m[mid] = 0.0
    low = bits(p.to(torch.bfloat16)).to(torch.int64) & 0xFFFF  # a bf16 value's bits: the lower neighbour
    parity = torch.where(kind == 2, 0, torch.where(kind == 3, 1, (torch.arange(numel) // 8) % 2))
    low = (low & ~1) | parity
    word = (low << 16) | 0x8000  # exactly halfway to the next bf16 value (away from zero)
    word = word + (kind == 4).long() - (kind == 5).long()
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)
    p[mid] = word.view(torch.float32)[mid]
    return p, g, m, v


def run_master(dev, ops_cpu, coef, step, beta1, max_blocks):
    p, g, m, v = (t.to(dev) for t in ops_cpu)
    p16 = torch.full_like(g, 7.0)
    c = None if coef is None else torch.tensor([coef], dtype=torch.float32, device=dev)
    ops.adam_master_step(p, g, m, v, p16, c, LR, beta1, B2, EPS, step, max_blocks=max_blocks)
    return p, m, v, p16


@pytest.mark.parametrize("numel,max_blocks", [(7, 0), (BULK_TAIL, 0), (BULK_TAIL, 1), (STRIDED, 3)])
def test_kernel_bits_match_fp32_adam_step(gpu, numel, max_blocks):
    """p32 / m32 / v32 == the fp32 cc_adam_step on (p32, g16.float(), m32, v32), p16 == p32.to(bfloat16): no
    tolerance.  numel 7 is only the tail, BULK_TAIL one chunk per thread plus the tail (and, capped to one workgroup,
    the grid-stride loop plus the tail), STRIDED four rounds of three workgroups."""
    cpu = operands(numel)
    for coef in (1.0, 0.37):
        for step in (1, 2, 1000):
            for beta1 in (0.9, 0.4):  # (both lerp forms)
                p, m, v, p16 = run_master(gpu, cpu, coef, step, beta1, max_blocks)
                pr, g32, mr, vr = (cpu[0].to(gpu), cpu[1].to(gpu).float(), cpu[2].to(gpu), cpu[3].to(gpu))
                ops.adam_step(pr, g32, mr, vr, torch.tensor([coef], device=gpu), LR, beta1, B2, EPS, step,
                              max_blocks=max_blocks)
                case = (coef, step, beta1)
                assert same_bits(p, pr) and same_bits(m, mr) and same_bits(v, vr), case
                assert same_bits(p16, pr.to(torch.bfloat16)), case
    # the midpoints did what they are there for: ties went to the even neighbour, in both directions
    kind = torch.arange(numel) % 8
    p0, p16c = cpu[0], p16.cpu()
    for k in (2, 3):
        sel = kind == k
        if sel.any():
            assert same_bits(p.cpu()[sel], p0[sel])  # g = m = 0: the master stayed at the midpoint
            low = (bits(p0[sel]) >> 16) & 0xFFFF
            want = low + (low & 1)  # even: down to it; odd: up (away from zero) to the even one above
            assert torch.equal(bits(p16c[sel]).to(torch.int32) & 0xFFFF, want)
    for k, up in ((4, 1), (5, 0)):
        sel = kind == k
        if sel.any():
            low = ((bits(p0[sel]) - (1 if up else -1)) >> 16) & 0xFFFF
            assert torch.equal(bits(p16c[sel]).to(torch.int32) & 0xFFFF, low + up)


def test_kernel_coef_null_is_one(gpu):
    cpu = operands(BULK_TAIL, seed=2)
    a = run_master(gpu, cpu, None, 3, 0.9, 0)
    b = run_master(gpu, cpu, 1.0, 3, 0.9, 0)
    assert all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("numel,max_blocks", [(7, 0), (BULK_TAIL, 0), (STRIDED, 3)])
def test_kernel_aborted_step_touches_nothing(gpu, numel, max_blocks):
    """coef[0] < 0 (CC_CLIP_ABORTED): p16, p32, m32 and v32 keep their bits."""
    cpu = operands(numel, seed=1)
    p, m, v, p16 = run_master(gpu, cpu, -1.0, 5, 0.9, max_blocks)
    assert same_bits(p.cpu(), cpu[0]) and same_bits(m.cpu(), cpu[2]) and same_bits(v.cpu(), cpu[3])
    assert bool((p16 == 7.0).all())


def ordered(t):
    """fp32 bits as integers in the values' order (one step = one ulp)."""
    i = bits(t).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


_TORCH_CASE = {}


def adam_state(numel, seed):
    """(p32, g16, m32, v32) on the CPU as an optimizer can hold them: test_adam_matches_torch's distributions (p ~
    0.05 N, g ~ 1e-3 N, m ~ 1e-4 N, v ~ 1e-6 U, the same draw order), the gradient rounded to bf16.  Not
    operands()'s special elements: a state with m != 0 beside v = 0 (den = eps) is one Adam never reaches, and its
    update of 1e4 lr is as large as the parameter."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(numel, generator=gen) * 0.05
    g = (torch.randn(numel, generator=gen) * 1e-3).to(torch.bfloat16)
    m = torch.randn(numel, generator=gen) * 1e-4
    v = torch.rand(numel, generator=gen) * 1e-6
    return p, g, m, v


def torch_case(dev):
    """One step of the kernel and of torch.optim.Adam on the CPU from the same state (computed once)."""
    if not _TORCH_CASE:
        cpu = adam_state(BULK_TAIL, seed=3)
        ref = MasterAdamRef(cpu[0], lr=LR, betas=(B1, B2), eps=EPS, exp_avg=cpu[2], exp_avg_sq=cpu[3], step=6)
        ref_p16 = ref.step(cpu[1], 0.37)
        p, m, v, p16 = run_master(dev, cpu, 0.37, 7, B1, 0)
        _TORCH_CASE.update(p32=(p, ref.p32.detach()), m32=(m, ref.exp_avg), v32=(v, ref.exp_avg_sq),
                           p16=(p16, ref_p16))
    return _TORCH_CASE


@pytest.mark.parametrize("name", ["p32", "m32", "v32"])
def test_kernel_matches_torch_adam(gpu, name):
    """Against torch.optim.Adam(foreach=False) on the CPU (tests/_master_adam_ref.py), the Adam parity bar of
    DESIGN.md section 4 applied to the fp32 state: bit-identical on >= 99.9 % of the elements and within one ulp
    elsewhere.

    The state is one an optimizer can hold (adam_state: the existing parity test's distributions).  Measured on
    MI355X: p32 99.976 %, m32 100 %, v32 99.976 % bit-identical, all within one ulp.  The kernel and
    torch's CPU kernel are not the same arithmetic in the last operation: torch's CPU addcdiv_ computes
    p + (value * m) / den, cc_adam_step -- whose fp32 bits this kernel carries, and which follows torch's GPU kernel --
    p + value * (m / den).  The two differ by at most one ulp of the UPDATE, which is about lr, 1000 times smaller
    than a parameter of 0.05: it moves p's rounding on about 1e-4 of the elements, and exceeds one ulp of the result
    only where p and the update nearly cancel (|p + update| below about lr / 2; restating both forms in torch on the
    CPU at test_adam_matches_torch's 100 003 elements: 99.991 % bit-identical, one element 4 ulps apart).  An
    earlier version of this test fed operands()'s den = eps elements (m != 0 beside v = 0, an update of 1e4 lr):
    there p32 read 96.12 % and 64 ulps, which measured those unreachable states, not the kernel."""
    ours, want = torch_case(gpu)[name]
    d = (ordered(ours.cpu()) - ordered(want)).abs()
    exact = (d == 0).float().mean().item()
    print(f"{name}: bit-identical {exact:.5f}, max ulps {int(d.max())}, max |diff| / lr "
          f"{(ours.cpu() - want).abs().max().item() / LR:.3e}")
    assert exact >= 0.999 and int(d.max()) <= 1, (name, exact, int(d.max()))


def test_kernel_p16_is_its_own_master_rounded(gpu):
    """p16 equals the rounding of the kernel's own p32 everywhere (also in the comparison with torch above)."""
    case = torch_case(gpu)
    p16, ref_p16 = case["p16"]
    assert same_bits(p16, case["p32"][0].to(torch.bfloat16))
    print("p16 == torch's p16 on", (p16.cpu() == ref_p16).float().mean().item(), "of the elements")


# ----------------------------------------------------------------------------- Trainer
def cfg_of(B, d, h, **kw):
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": LR, "num_tokens": B * 100, "l1_coeff": 2,
           "beta1": B1, "beta2": B2, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    cfg.update(kw)
    return cfg


def trainer_of(cfg, rows, seed=0):
    cc = ca.CrossCoder(cfg)
    return ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=rows, seed=seed), crosscoder=cc)


def opt_state(tr):
    """(master or None, exp_avg, exp_avg_sq): clones of the flat arenas, after the step's launches."""
    tr.synchronize()
    o = tr.optimizer
    return (o.master.data.clone() if o.master is not None else None, o.exp_avg.data.clone(),
            o.exp_avg_sq.data.clone())


def fp32_update(tr, prev, lr, dev):
    """The fp32 cc_adam_step of the last step's gradient and clip coefficient on clones of `prev`."""
    o = tr.optimizer
    p, m, v = (t.clone() for t in prev)
    b1, b2 = o.param_groups[0]["betas"]
    ops.adam_step(p, o.grads.data.float(), m, v, tr._last_ws.clip_out[0:1], lr, b1, b2, o.param_groups[0]["eps"], o.t)
    return p, m, v


STEP_LOSS_KEYS = ("l2_loss", "l1_loss", "l0_loss", "explained_variance", "explained_variance_A",
                  "explained_variance_B")


def fresh_losses(tr, cfg, raw, factor):
    """get_losses of a fresh default-mode CrossCoder loaded from the trainer's crosscoder, on the batch (raw, factor)
    as the step normalises it."""
    plain = {k: v for k, v in cfg.items() if k != "master_weights"}
    cc = ca.CrossCoder(plain)
    cc.load_state_dict({k: v.detach().clone() for k, v in tr.crosscoder.state_dict().items()})
    with torch.no_grad():
        lo = cc.get_losses(raw.float() * factor.float()[None, :, None])
    # ("loss" as the reference's trainer forms it from these tensors: the caller's l1_coeff times the bf16 l1, + the
    # fp32 l2)
    return {"loss": lambda l1c: (lo.l2_loss + l1c * lo.l1_loss).item(),
            "l2_loss": lo.l2_loss.item(), "l1_loss": lo.l1_loss.item(), "l0_loss": lo.l0_loss.item(),
            "explained_variance": lo.explained_variance.mean().item(),
            "explained_variance_A": lo.explained_variance_A.mean().item(),
            "explained_variance_B": lo.explained_variance_B.mean().item()}


@pytest.mark.parametrize("B,d,h,extra", [(256, 64, 512, {}), (96, 40, 200, {}), (96, 36, 203, {}),
                                         (256, 64, 512, {"activation": "topk", "k": 8})],
                         ids=["relu", "relu-ragged", "relu-padded", "topk"])
def test_trainer_steps_in_master_mode(gpu, B, d, h, extra):
    """4 steps at lr 1e-2 (every step moves the parameters by many bf16 ulps, so derived state left a step behind
    would show).  After each: masters and both moments == the fp32 cc_adam_step of the previous state under the
    step's gradient and clip coefficient, bit for bit; the bf16 parameters == the masters rounded; the padding is 0.
    Each step's loss dict against get_losses of a fresh default-mode crosscoder holding the same parameters, within
    the bf16 bounds of test_trainer_steps: l2 rel 1e-4, l1 one bf16 ulp, l0 1e-3 h + 1 / B,
    EV 2e-3, EV_A / EV_B 4e-3, loss to the sum of those.  get_losses returns no "loss": it is formed here as the
    reference's trainer forms it, l2 + l1_coeff * l1 on get_losses' tensors with the step's own l1_coeff."""
    cfg = cfg_of(B, d, h, lr=1e-2, master_weights=True, **extra)
    tr = trainer_of(cfg, rows=4 * B)
    cc, o = tr.crosscoder, tr.optimizer
    assert o.master_mode and o.exp_avg.data.dtype == torch.float32
    a = cc.arena()
    for s in range(4):
        prev = opt_state(tr)
        lr = o.param_groups[0]["lr"]
        raw, factor = tr.buffer.peek_raw()
        want = fresh_losses(tr, cfg, raw, factor)
        got = tr.step()
        tol = {"l2_loss": 1e-4 * abs(want["l2_loss"]), "l1_loss": 2 ** -7 * abs(want["l1_loss"]),
               "l0_loss": 1e-3 * h + 1.0 / B, "explained_variance": 2e-3, "explained_variance_A": 4e-3,
               "explained_variance_B": 4e-3}
        want["loss"] = want["loss"](got["l1_coeff"])
        tol["loss"] = tol["l2_loss"] + got["l1_coeff"] * tol["l1_loss"] * 2 + 1e-6 * abs(want["loss"])
        for k in STEP_LOSS_KEYS + ("loss",):
            print(f"step {s} {k}: step {got[k]!r} fresh {want[k]!r}")
            assert abs(got[k] - want[k]) <= tol[k], (s, k, got[k], want[k], tol[k])
        now = opt_state(tr)
        exp = fp32_update(tr, prev, lr, gpu)
        for name, x, y in zip(("master", "exp_avg", "exp_avg_sq"), now, exp):
            assert same_bits(x, y), (s, name, int((bits(x) != bits(y)).sum()))
        assert not same_bits(now[0], prev[0])  # (an update did happen)
        assert same_bits(a.data, now[0].to(torch.bfloat16)), s
        m = o.master
        if a.padded:
            assert float(m.W_dec_hk[h:].abs().sum()) == 0 and float(m.W_enc_hk[h:].abs().sum()) == 0
            assert float(m.b_enc[h:].abs().sum()) == 0
            for t in (m.W_dec_hk, m.W_enc_hk):
                assert float(t.view(m.h, m.n, m.d)[:, :, d:].abs().sum()) == 0
            assert float(m.b_dec_flat.view(m.n, m.d)[:, d:].abs().sum()) == 0
        st = o.state[cc.W_dec]
        assert st["master"].dtype == torch.float32 and st["master"].shape == cc.W_dec.shape
        assert same_bits(st["master"].to(torch.bfloat16).contiguous(), cc.W_dec.detach().contiguous())


def test_torch_writes_between_steps(gpu):
    """W_dec rows and b_enc entries written through torch between two steps: the next update starts from the written
    values there, and everywhere else from the masters with their extra bits."""
    B, d, h = 256, 64, 512
    cfg = cfg_of(B, d, h, lr=1e-2, master_weights=True)
    tr = trainer_of(cfg, rows=2 * B)
    cc, o = tr.crosscoder, tr.optimizer
    tr.step()
    prev = opt_state(tr)
    assert bool((prev[0].to(torch.bfloat16).float() != prev[0]).float().mean() > 0.5)  # extra bits to lose
    with torch.no_grad():
        new_rows = (cc.W_dec[5:9] * -1.5).detach().clone()
        cc.W_dec[5:9] = new_rows
        cc.b_enc[10:20] = 0.5
    start = o.master.like()
    start.data.copy_(prev[0])
    start.W_dec()[5:9] = new_rows.float()
    start.b_enc_ref()[10:20] = 0.5
    lr = o.param_groups[0]["lr"]
    tr.step()
    now = opt_state(tr)
    exp = fp32_update(tr, (start.data, prev[1], prev[2]), lr, gpu)
    for name, x, y in zip(("master", "exp_avg", "exp_avg_sq"), now, exp):
        assert same_bits(x, y), (name, int((bits(x) != bits(y)).sum()))
    assert same_bits(cc.arena().data, now[0].to(torch.bfloat16))
    # (had the masters overwritten the writes, b_enc[10:20] would be near its old value, not near 0.5)
    assert bool(((cc.b_enc[10:20].detach().float() - 0.5).abs() <= 0.02).all())


ORACLE_TOL = {"l2_loss": 1e-2, "l1_loss": 1e-2, "loss": 1e-2}


def test_master_mode_is_closer_to_the_fp32_oracle(gpu):
    """The whole schedule (num_tokens = 10 batches, 10 steps: warm-up and lr decay) from the same bf16-valued init
    on the same bf16-valued batches: OracleTrainer in fp32, the Trainer in default and in master mode.  For each
    parameter the relative Frobenius error of master mode's masters against the oracle is below that of default
    mode's parameters; both modes' loss dicts stay within the bf16 bounds against the oracle (DESIGN.md section 4:
    l2 / l1 / loss rel 1e-2, EVs 1e-2, l0 2e-3 h)."""
    B, d, h, steps = 256, 64, 512, 10
    cfg = cfg_of(B, d, h, num_tokens=B * steps)
    trs = {"default": trainer_of(cfg, rows=steps * B), "master": trainer_of(dict(cfg, master_weights=True),
                                                                           rows=steps * B)}
    cc0 = trs["default"].crosscoder
    P = {k: getattr(cc0, k).detach().float().cpu() for k in O.PARAM_ORDER}
    orc = O.OracleTrainer(dict(cfg, enc_dtype="fp32", device="cpu"), P)
    buf = trs["default"].buffer
    for s in range(steps):
        raw = buf.buffer[s * B:(s + 1) * B].cpu()
        x32 = O.buffer_next(raw, buf.normalisation_factor.cpu()).to(torch.bfloat16).float()
        ref = orc.step(x32)
        for mode, tr in trs.items():
            got = tr.step()
            assert got["l1_coeff"] == ref["l1_coeff"] and got["lr"] == ref["lr"], (s, mode)
            for k, tol in ORACLE_TOL.items():
                assert math.isclose(got[k], ref[k], rel_tol=tol, abs_tol=1e-6), (s, mode, k, got[k], ref[k])
            for k in ("explained_variance", "explained_variance_A", "explained_variance_B"):
                assert abs(got[k] - ref[k]) <= 1e-2, (s, mode, k, got[k], ref[k])
            assert abs(got["l0_loss"] - ref["l0_loss"]) <= 2e-3 * h, (s, mode, got["l0_loss"], ref["l0_loss"])
    assert ref["lr"] < cfg["lr"] and ref["l1_coeff"] == cfg["l1_coeff"]
    st = trs["master"].optimizer.state
    errs = {}
    for k in O.PARAM_ORDER:
        want = orc.P[k].detach()
        e_def = ((getattr(trs["default"].crosscoder, k).detach().float().cpu() - want).norm() / want.norm()).item()
        e_mas = ((st[getattr(trs["master"].crosscoder, k)]["master"].cpu() - want).norm() / want.norm()).item()
        errs[k] = (e_mas, e_def)
        print(f"{k}: rel. Frobenius error against the fp32 oracle: master {e_mas:.3e}, default {e_def:.3e}")
    for k, (e_mas, e_def) in errs.items():
        assert e_mas < e_def, (k, e_mas, e_def)


@pytest.mark.parametrize("master", [False, True], ids=["default", "master"])
def test_resume_is_bit_identical(gpu, master):
    """6 steps uninterrupted == 3 steps, CrossCoder.state_dict() + Trainer.state_dict() into a fresh pair (the
    buffer at the same position), 3 more steps: loss dicts, parameters, masters and moments, bit for bit.  6 batches
    in all, so the resumed half runs through the lr decay."""
    B, d, h = 256, 64, 512
    cfg = cfg_of(B, d, h, num_tokens=6 * B, lr=1e-3, master_weights=master)
    ref = trainer_of(cfg, rows=6 * B)
    ref_losses = [ref.step() for _ in range(6)]
    first = trainer_of(cfg, rows=6 * B)
    losses = [first.step() for _ in range(3)]
    saved_cc = {k: v.detach().clone() for k, v in first.crosscoder.state_dict().items()}
    saved_tr = first.state_dict()
    assert saved_tr["optimizer"]["master_weights"] is master and ("master" in saved_tr["optimizer"]) == master
    second = trainer_of(cfg, rows=6 * B)
    second.crosscoder.load_state_dict(saved_cc)
    second.load_state_dict(saved_tr)
    second.buffer.buffer_pointer = first.buffer.buffer_pointer
    del first
    losses += [second.step() for _ in range(3)]
    assert losses == ref_losses
    assert losses[5]["lr"] < losses[3]["lr"] == cfg["lr"]
    for k in O.PARAM_ORDER:
        assert same_bits(getattr(second.crosscoder, k).detach().contiguous(),
                         getattr(ref.crosscoder, k).detach().contiguous()), k
    for x, y in zip(opt_state(second), opt_state(ref)):
        assert (x is None and y is None and not master) or same_bits(x, y)
    assert second.optimizer.t == ref.optimizer.t == 6 and second.step_counter == 6


def test_default_mode_is_unchanged(gpu):
    """cfg["master_weights"] = False is the run without the key: loss dicts, parameters and moments bit for bit,
    bf16 moments, no masters."""
    B, d, h = 256, 64, 512
    a = trainer_of(cfg_of(B, d, h), rows=3 * B)
    b = trainer_of(cfg_of(B, d, h, master_weights=False), rows=3 * B)
    assert [a.step() for _ in range(3)] == [b.step() for _ in range(3)]
    for tr in (a, b):
        assert tr.optimizer.master_mode is False and tr.optimizer.master is None
        assert tr.optimizer.exp_avg.data.dtype == torch.bfloat16
    assert same_bits(a.crosscoder.arena().data, b.crosscoder.arena().data)
    for x, y in zip(opt_state(a)[1:], opt_state(b)[1:]):
        assert same_bits(x, y)
