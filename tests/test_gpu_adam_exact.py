"""The bf16 Adam's fast arithmetic (csrc/adam.hip: adam_sqrt2, adam_udiv, adam_quot2, adam_pair) against the
reference arithmetic it replaced (adam_elem: IEEE divisions, correctly rounded sqrtf), bit for bit.  The test
library evaluates each primitive and its reference over a whole domain on the device (cc_debug_adam_prims) and can
run every Adam entry on the reference arithmetic (cc_debug_set_adam_ref).  Two NaNs count as equal; everything
else is compared as raw bits."""
import ctypes

import pytest
import torch

from crosscoder_amd import _lib, ops

pytestmark = pytest.mark.gpu

# bf16 patterns outside adam_sqrt2's domain (+0 or a positive normal): the sign bit set (32768), the
# positive non-finite (128) and the positive denormals (127)
GUARDED_16 = 32768 + 128 + 127
POS_NORMAL = 254 * 128
LR, BETA1, BETA2 = 5e-5, 0.9, 0.999


@pytest.fixture(scope="module")
def dbg(gpu):
    with _lib.debug_library() as lib:
        yield lib


def prims(dbg, kind, beta2=0.0, lo=0, hi=0):
    out = (ctypes.c_uint64 * 4)()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ops.check(dbg.cc_debug_adam_prims(kind, beta2, lo, hi, out, st))
    res = dict(mismatches=out[0], guarded=out[1], first=None if out[2] == 2**64 - 1 else hex(out[2]), aux=out[3])
    print(f"adam prims kind {kind} beta2 {beta2} steps {lo}..{hi}: {res}")
    return res


def test_sqrt_every_bf16_pattern(dbg):
    """bf16(v_sqrt_f32(vj)) == bf16(sqrtf(vj)) for all 2^16 patterns; the guard takes exactly the negative,
    non-finite and denormal ones."""
    r = prims(dbg, 0)
    assert r["mismatches"] == 0, r
    assert r["guarded"] == GUARDED_16, r


@pytest.mark.parametrize("beta2,steps", [(0.999, 20000), (0.99, 2000), (0.95, 2000)])
def test_uniform_divide_every_divisor(dbg, beta2, steps):
    """bf16(den / bc2s) through the reciprocal for all 2^16 den patterns x bc2s of steps 1..steps (after ~16k steps
    at 0.999 the fp32 divisor is 1: every divisor the benchmark's beta2 can produce).  The update forms den as
    bf16(sqrt(vj)) of a vj that passed the sqrt's guard, so it is +0 or in [2^-63, 2^64]; the check takes the
    primitive's whole domain, +0 and [2^-67, 2^64] (131 binades and 2^64 itself), and sends the other patterns
    -- which the update cannot produce; adam_udiv has no guard of its own for them: towards the top of the fp32
    range den * rb overflows (from 2^108 on for the largest rb, 2^20), below 2^-67 the residual is no longer
    exact -- to the reference."""
    r = prims(dbg, 1, beta2, 1, steps)
    assert r["mismatches"] == 0, r
    assert r["guarded"] == (65536 - (131 * 128 + 1 + 1)) * steps, r


def test_quotient_every_pair(dbg):
    """mj / den through the fp64 reciprocal, two exact-residual corrections and one rounding to fp32: the fp32
    quotient's bits for all 2^16 x 2^16 pairs (denormal and overflowing quotients included), and the guarded share =
    the pairs with a non-finite or denormal member or den <= 0, nothing more."""
    r = prims(dbg, 2)
    outside = 2**32 - POS_NORMAL * 2 * (POS_NORMAL + 1)
    print(f"quotient: guarded {r['guarded']} = {r['guarded'] / 2**32:.6f} of the pairs; with a non-finite / denormal "
          f"member or den <= 0: {outside} = {outside / 2**32:.6f}; guarded beyond those (range): {r['aux']}")
    assert r["mismatches"] == 0, r
    assert r["guarded"] == outside, r


# ---------------------------------------------------------------- the whole update
# The guard is per wave: one out-of-domain lane sends the 512 elements of its wave's chunks (64 lanes x 8, or 8 rows
# x 64 columns in the transposing form) to the reference arithmetic.  So the operands are laid out in bands of 2^16
# elements (64 rows of the K = 1024 matrix, whole waves in every launch form):
#   bands 0-10  in the fast arithmetic's domain for every parameter set: g, v, m sweep all in-domain bf16 patterns
#               (g: +-[2^-50, 2^55]; v: [2^-120, 2^120]; m: +-0 and +-[2^-100, 2^60]), paired differently in each
#               512-element run -- extreme but normal exponents, no special
#   band 11     v = 0 (den = the root of the gradient term alone), g as above
#   band 12     g = 0 and v = 0 (a latent that never fired: den = eps), m = 0 or normal: in the domain unless eps = 0
#   bands 13-14 g and v sweep ALL 2^16 patterns against each other, p and m with zeros, infinities, NaN, denormals
#   band 15     as bands 0-10, with exactly one out-of-domain lane in every fourth 512-element run (m = NaN, m = inf
#               or a negative v)
# A test runs the bands that are in the domain on their own and requires that no chunk was redone there (so the fast
# arithmetic produced the compared bits), and the whole array, where some but not all chunks must be redone.
BAND = 1 << 16
N = 16 * BAND
K = 1024
H = N // K


def bits_equal(a, b):
    if a.dtype == torch.bfloat16:
        same = a.view(torch.int16) == b.view(torch.int16)
    else:
        same = a.view(torch.int32) == b.view(torch.int32)
    return bool((same | (a.isnan() & b.isnan())).all())


def as_bf16(pattern):
    """int64 in [0, 2^16) -> the bf16 with those bits"""
    return torch.where(pattern >= 32768, pattern - 65536, pattern).to(torch.int16).view(torch.bfloat16)


def patterns(lo_exp, hi_exp, signs, zeros=False, device="cpu"):
    """the bf16 bit patterns of +-2^lo_exp .. 2^hi_exp (whole binades), optionally the zeros"""
    mag = torch.arange((lo_exp + 127) << 7, (hi_exp + 128) << 7, dtype=torch.int64, device=device)
    out = [mag] + ([mag | 0x8000] if signs else [])
    if zeros:
        out.append(torch.tensor([0, 0x8000] if signs else [0], dtype=torch.int64, device=device))
    return torch.cat(out)


def make_operands(device):
    e = torch.arange(N, device=device, dtype=torch.int64)
    run, band = e >> 9, e >> 16
    Gt = patterns(-50, 54, True, device=device)
    Vt = patterns(-120, 119, False, device=device)
    Mt = patterns(-100, 59, True, zeros=True, device=device)
    g = Gt[(e * 7919 + run * 131) % Gt.numel()]
    v = Vt[(e * 4099 + run * 4111) % Vt.numel()]
    m = Mt[(e * 6151 + run * 17) % Mt.numel()]
    gen = torch.Generator(device=device).manual_seed(5)
    p = (torch.randn(N, device=device, generator=gen) * 0.05).to(torch.bfloat16)
    p[::97] = 0.0
    v = torch.where(band == 11, torch.zeros_like(v), v)
    dead = band == 12
    g = torch.where(dead, torch.zeros_like(g), g)
    v = torch.where(dead, torch.zeros_like(v), v)
    m = torch.where(dead & (e % 3 != 0), torch.zeros_like(m), m)
    sweep = (band == 13) | (band == 14)
    g = torch.where(sweep, e & 0xFFFF, g)
    v = torch.where(sweep, ((e & 0xFFFF) * 4099 + band * 4111) & 0xFFFF, v)
    g, v, m = as_bf16(g), as_bf16(v), as_bf16(m)
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1e-39, -3e-40, 9.2e-41],
                           device=device).to(torch.bfloat16)
    where = 13 * BAND + torch.randint(0, 2 * BAND, (BAND // 8,), device=device, generator=gen)
    for t, salt in ((p, 1), (m, 2)):
        t[where] = special[(where + salt) % special.numel()]
    # band 15: one bad lane in every fourth run
    runs = torch.arange(15 * BAND // 512, 16 * BAND // 512, 4, device=device, dtype=torch.int64)
    pos = runs * 512 + (runs * 37) % 512
    kind = (runs // 4) % 3
    m[pos[kind == 0]] = float("nan")
    m[pos[kind == 1]] = float("inf")
    v[pos[kind == 2]] = -3e38
    return p, g, m, v


@pytest.fixture(scope="module")
def operands(gpu):
    return make_operands(gpu)


def run_form(form, operands, coef, beta1, step, eps):
    p, g, m, v = (t.clone() for t in operands)
    n = p.numel()
    h = n // K
    hp = (LR, beta1, BETA2, eps, step)
    extra = []
    if form == "one_pass":
        ops.adam_step(p, g, m, v, coef, *hp)
    elif form == "capped":
        ops.adam_step(p, g, m, v, coef, *hp, max_blocks=64)
    elif form == "capped_tail":  # (numel % 8 != 0: the general grid-stride kernel, whole chunks + a partial one)
        ops.adam_step(p[:n - 5], g[:n - 5], m[:n - 5], v[:n - 5], coef, *hp, max_blocks=64)
    elif form == "side":  # (the last 8 rows beyond the norm matrix, like b_dec)
        part = torch.zeros((h - 8) * (K // 64), device=p.device)
        ops.adam_dec_norms(p, g, m, v, h - 8, K, *hp, part, coef=coef, max_blocks=64)
        extra = [part]
    elif form == "transposed":
        wt = torch.zeros(K, h, device=p.device, dtype=torch.bfloat16)
        part = torch.zeros(h * (K // 64), device=p.device)
        ops.adam_dec_transposed(p.view(h, K), g.view(h, K), m.view(h, K), v.view(h, K), coef, *hp, wt, part)
        extra = [part, wt]
    return [p, m, v] + extra


FORMS = ("one_pass", "capped", "capped_tail", "side", "transposed")
GRID = [(c, 0.9, s, e) for c in (1.0, 0.37) for s in (1, 7, 5000) for e in (1e-8, 0.0)]
GRID.append((0.37, 0.4, 7, 1e-8))  # (lerp weight >= 0.5: the kernels' other lerp form)


@pytest.mark.parametrize("coef,beta1,step,eps", GRID)
def test_whole_update_fast_equals_reference(dbg, operands, coef, beta1, step, eps):
    """p, m, v and the norm partials (and W_dec^T) of every launch form: the fast arithmetic against the same
    launch on the reference arithmetic, and every form's p / m / v against the one-pass form's -- on the in-domain
    bands alone, where no chunk may be redone with the reference arithmetic, and on the whole array, where the
    chunks of the waves with an out-of-domain lane, and only those, are."""
    c = torch.tensor([coef], device=operands[0].device)
    clean = (13 if eps > 0 else 12) * BAND
    for n in (clean, N):
        ops_n = [t[:n] for t in operands]
        base = None
        for form in FORMS:
            dbg.cc_debug_set_adam_ref(1)
            try:
                ref = run_form(form, ops_n, c, beta1, step, eps)
            finally:
                dbg.cc_debug_set_adam_ref(0)
            assert dbg.cc_debug_adam_redone(1) >= 0
            fast = run_form(form, ops_n, c, beta1, step, eps)
            redone = dbg.cc_debug_adam_redone(1)
            print(f"{form} coef {coef} beta1 {beta1} step {step} eps {eps}: {redone} of {n // 8} chunks redone")
            if n == clean:
                assert redone == 0, (form, redone)
            else:
                # every wave of bands 13-14 (and of band 12 if eps = 0) and the 32 waves of band 15 with a bad lane
                # (in the transposing form a bad lane's wave is 8 rows x 64 columns: as many), 64 chunks each
                assert redone == ((3 if eps == 0 else 2) * 128 + 32) * 64, (form, redone)
            for name, a, b in zip(("p", "m", "v", "norm partials", "W_dec^T"), fast, ref):
                assert bits_equal(a, b), (form, name)
            if form == "one_pass":
                base = ref
            elif form != "capped_tail":
                for name, a, b in zip(("p", "m", "v"), fast, base):
                    assert bits_equal(a, b), (form, name, "against the one-pass form")


@pytest.mark.parametrize("h,K,max_blocks", [(1003, 320, 3), (1003, 64, 1)])
def test_norm_partial_indexing_carry(dbg, gpu, h, K, max_blocks):
    """cc_adam_dec_norms' (row, column) carried through the grid-stride loop: a stride (max_blocks x 2048 elements)
    that is no multiple of K, so the carry fires on some iterations only, and a launch that ends in the b_dec tail
    beyond norm_rows x K -- against the reference arithmetic and against the flat form (one chunk per thread)."""
    hp = -(-h // 8) * 8  # (the engine's row padding)
    numel = hp * K + K
    gen = torch.Generator(device=gpu).manual_seed(11)
    src = [(torch.randn(numel, device=gpu, generator=gen) * s).to(torch.bfloat16) for s in (0.05, 1e-3, 1e-3)]
    src.append((torch.rand(numel, device=gpu, generator=gen) * 1e-6).to(torch.bfloat16))
    coef = torch.ones(1, device=gpu)

    def run(blocks, ref):
        p, g, m, v = (t.clone() for t in src)
        part = torch.full((hp * (K // 64),), -1.0, device=gpu)
        dbg.cc_debug_set_adam_ref(int(ref))
        try:
            ops.adam_dec_norms(p, g, m, v, hp, K, LR, BETA1, BETA2, 1e-8, 3, part, coef=coef, max_blocks=blocks)
        finally:
            dbg.cc_debug_set_adam_ref(0)
        return p, m, v, part

    carried = run(max_blocks, False)
    assert (carried[3] >= 0).all()  # every (row, block) partial written
    for other in (run(max_blocks, True), run(0, False)):
        for name, a, b in zip(("p", "m", "v", "norm partials"), carried, other):
            assert bits_equal(a, b), name
