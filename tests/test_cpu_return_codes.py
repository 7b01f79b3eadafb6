"""CPU: the return codes of the step's host checks, one call per failure a check can report.  Every call passes fake
16-byte-aligned pointers with exactly one thing wrong, so each fails a check and none reaches a launch: the table pins
which code a caller gets for which mistake, for every entry point that validates prep, Adam, loss-row or clip
arguments."""
import ctypes

import pytest

from crosscoder_amd import _lib

NULL, DTYPE, SHAPE, ALIGN = 1, 2, 3, 4
BF16, F32, BAD_DT = 1, 2, 7
null, fake, odd = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)
_f, _d = ctypes.c_float, ctypes.c_double
OFF = (ctypes.c_int64 * 10)(*range(10))
ADAM_HP = (_d(1e-3), _d(0.9), _d(0.999), _d(1e-8))  # lr, beta1, beta2, eps


def prep_input(lib, x_in=fake, in_dtype=BF16, factor=fake, factor_dtype=F32, x_out=fake, B=72, n=2, d=72, dtype=BF16):
    return lib.cc_prep_input(x_in, in_dtype, factor, factor_dtype, x_out, fake, B, n, d, dtype, null)


def prep_input_t(lib, x_in=fake, in_dtype=BF16, factor=fake, factor_dtype=F32, x_out=fake, x_t=fake, B=72, n=2, d=72,
                 dtype=BF16):
    return lib.cc_prep_input_t(x_in, in_dtype, factor, factor_dtype, x_out, x_t, fake, B, n, d, dtype, null)


def adam_step(lib, p=fake, g=fake, m=fake, v=fake, numel=4096, step=1, max_blocks=0, dtype=BF16):
    return lib.cc_adam_step(p, g, m, v, numel, fake, *ADAM_HP, step, max_blocks, dtype, null)


def adam_step_clip(lib, p=fake, v=fake, numel=4096, sums=fake, nparams=4, step=1, max_blocks=0, dtype=BF16):
    return lib.cc_adam_step_clip(p, fake, fake, v, numel, sums, nparams, _f(1.0), 1, fake, *ADAM_HP, step, max_blocks,
                                 dtype, null)


def adam_step_prep(lib, p=fake, m=fake, numel=4096, step=1, dtype=BF16, x_in=fake, in_dtype=BF16, factor=fake,
                   factor_dtype=F32, x_out=fake, x_t=fake, B=72, n=2, d=72):
    job = _lib.PrepJob(x_in.value, in_dtype, factor.value, factor_dtype, x_out.value, x_t.value, fake.value, B, n, d)
    return lib.cc_adam_step_prep(p, fake, m, fake, numel, fake, *ADAM_HP, step, dtype, ctypes.byref(job), null)


def adam_master_step(lib, p32=fake, g16=fake, v32=fake, p16=fake, numel=4096, step=1, max_blocks=0):
    return lib.cc_adam_master_step(p32, g16, fake, v32, p16, numel, fake, *ADAM_HP, step, max_blocks, null)


def adam_dec_norms(lib, p=fake, g=fake, numel=64 * 128, coef=fake, sums=null, nparams=0, step=1, max_blocks=0,
                   norm_part=fake, h=64, K=128, dtype=BF16, done_ctr=null):
    return lib.cc_adam_dec_norms(p, g, fake, fake, numel, coef, sums, nparams, _f(1.0), 1, *ADAM_HP, step, max_blocks,
                                 norm_part, h, K, dtype, done_ctr, null)


def adam_dec_transposed(lib, p=fake, m=fake, h=64, K=128, step=1, W_dec_t=fake, part=fake, dtype=BF16):
    return lib.cc_adam_dec_transposed(p, fake, m, fake, h, K, fake, *ADAM_HP, step, 0, W_dec_t, part, dtype, null)


def loss_rows(lib, recon=fake, b_dec=fake, x=fake, x_mean=fake, g_recon=fake, row_part=fake, row0=0, rows=36, B=36,
              n=2, d=72, dtype=BF16):
    return lib.cc_loss_fwd_bwd_rows(recon, b_dec, x, x_mean, g_recon, row_part, fake, _f(0.01), row0, rows, B, n, d,
                                    dtype, null)


def loss_rows_t(lib, recon=fake, b_dec=fake, x=fake, x_mean=fake, g_recon=fake, g_recon_t=fake, row_part=fake, row0=0,
                rows=72, B=72, n=2, d=72, dtype=BF16):
    return lib.cc_loss_fwd_bwd_rows_t(recon, b_dec, x, x_mean, g_recon, g_recon_t, row_part, fake, _f(0.01), row0, rows,
                                      B, n, d, dtype, null)


def clip_finalize(lib, sq=fake, off=OFF, nparams=4, out=fake):
    return lib.cc_clip_finalize(sq, off, nparams, _f(1.0), 1, out, null)


def segment_sums(lib, sq=fake, off=OFF, nparams=4, out=fake):
    return lib.cc_segment_sums(sq, off, nparams, 0, out, null)


CASES = [
    # cc_prep_input
    (prep_input, dict(x_in=null), NULL),
    (prep_input, dict(x_out=null), NULL),
    (prep_input, dict(B=0), SHAPE),
    (prep_input, dict(d=76), SHAPE),                      # d % 8
    (prep_input, dict(B=1 << 31), SHAPE),                 # B, n * d are the kernel's ints
    (prep_input, dict(n=1 << 20, d=1 << 12), SHAPE),
    (prep_input, dict(x_in=odd), ALIGN),
    (prep_input, dict(x_out=odd), ALIGN),
    (prep_input, dict(factor_dtype=BAD_DT), DTYPE),
    (prep_input, dict(in_dtype=BAD_DT), DTYPE),
    (prep_input, dict(dtype=BAD_DT), DTYPE),
    # cc_prep_input_t (x_t given: bf16 out, B % 8 == 0)
    (prep_input_t, dict(x_in=null), NULL),
    (prep_input_t, dict(x_out=null), NULL),
    (prep_input_t, dict(n=0), SHAPE),
    (prep_input_t, dict(d=76), SHAPE),
    (prep_input_t, dict(B=76), SHAPE),                    # B % 8
    (prep_input_t, dict(B=1 << 31), SHAPE),
    (prep_input_t, dict(n=1 << 20, d=1 << 12), SHAPE),
    (prep_input_t, dict(dtype=F32), DTYPE),
    (prep_input_t, dict(factor_dtype=BAD_DT), DTYPE),
    (prep_input_t, dict(in_dtype=BAD_DT), DTYPE),
    (prep_input_t, dict(x_in=odd), ALIGN),
    (prep_input_t, dict(x_t=odd), ALIGN),
    # cc_adam_step (the dtype is checked where the launch form is chosen, in each form)
    (adam_step, dict(p=null), NULL),
    (adam_step, dict(v=null), NULL),
    (adam_step, dict(numel=0), SHAPE),
    (adam_step, dict(step=0), SHAPE),
    (adam_step, dict(g=odd), ALIGN),
    (adam_step, dict(dtype=BAD_DT), DTYPE),               # bulk
    (adam_step, dict(dtype=BAD_DT, numel=5), DTYPE),      # the < 8-element tail alone
    (adam_step, dict(dtype=BAD_DT, max_blocks=2), DTYPE),  # capped
    # cc_adam_step_clip
    (adam_step_clip, dict(p=null), NULL),
    (adam_step_clip, dict(sums=null), NULL),
    (adam_step_clip, dict(numel=0), SHAPE),
    (adam_step_clip, dict(step=0), SHAPE),
    (adam_step_clip, dict(nparams=0), SHAPE),
    (adam_step_clip, dict(nparams=7), SHAPE),             # at most 6 in-kernel
    (adam_step_clip, dict(v=odd), ALIGN),
    (adam_step_clip, dict(dtype=BAD_DT), DTYPE),
    (adam_step_clip, dict(dtype=BAD_DT, max_blocks=2), DTYPE),
    # cc_adam_step_prep (prep given)
    (adam_step_prep, dict(p=null), NULL),
    (adam_step_prep, dict(x_in=null), NULL),
    (adam_step_prep, dict(x_out=null), NULL),
    (adam_step_prep, dict(x_t=null), NULL),
    (adam_step_prep, dict(dtype=F32), DTYPE),
    (adam_step_prep, dict(factor_dtype=BAD_DT), DTYPE),
    (adam_step_prep, dict(in_dtype=BAD_DT), DTYPE),
    (adam_step_prep, dict(numel=0), SHAPE),
    (adam_step_prep, dict(numel=4100), SHAPE),            # numel % 8
    (adam_step_prep, dict(step=0), SHAPE),
    (adam_step_prep, dict(B=0), SHAPE),
    (adam_step_prep, dict(d=76), SHAPE),
    (adam_step_prep, dict(B=76), SHAPE),
    (adam_step_prep, dict(B=1 << 31), SHAPE),
    (adam_step_prep, dict(n=1 << 20, d=1 << 12), SHAPE),
    (adam_step_prep, dict(m=odd), ALIGN),
    (adam_step_prep, dict(x_in=odd), ALIGN),
    (adam_step_prep, dict(x_out=odd), ALIGN),
    (adam_step_prep, dict(x_t=odd), ALIGN),
    # cc_adam_master_step (no dtype: fp32 masters, bf16 gradient)
    (adam_master_step, dict(p32=null), NULL),
    (adam_master_step, dict(p16=null), NULL),
    (adam_master_step, dict(numel=0), SHAPE),
    (adam_master_step, dict(step=0), SHAPE),
    (adam_master_step, dict(numel=1 << 43), SHAPE),       # more than 2^31 - 1 workgroups, uncapped
    (adam_master_step, dict(numel=1 << 43, max_blocks=1 << 31), SHAPE),  # and capped
    (adam_master_step, dict(g16=odd), ALIGN),
    (adam_master_step, dict(p16=odd), ALIGN),
    # cc_adam_dec_norms
    (adam_dec_norms, dict(p=null), NULL),
    (adam_dec_norms, dict(norm_part=null), NULL),
    (adam_dec_norms, dict(coef=null), NULL),              # neither coef nor sums
    (adam_dec_norms, dict(done_ctr=fake), SHAPE),         # the signal needs a capped grid
    (adam_dec_norms, dict(h=0), SHAPE),
    (adam_dec_norms, dict(step=0), SHAPE),
    (adam_dec_norms, dict(K=96, numel=64 * 96), SHAPE),   # K % 64
    (adam_dec_norms, dict(numel=64 * 128 - 8), SHAPE),    # the norm matrix is past the arena
    (adam_dec_norms, dict(h=1 << 24, numel=1 << 31), SHAPE),  # h * K reaches 2^31
    (adam_dec_norms, dict(sums=fake, nparams=0), SHAPE),
    (adam_dec_norms, dict(sums=fake, nparams=7), SHAPE),
    (adam_dec_norms, dict(g=odd), ALIGN),
    (adam_dec_norms, dict(norm_part=odd), ALIGN),
    (adam_dec_norms, dict(dtype=BAD_DT), DTYPE),
    (adam_dec_norms, dict(dtype=BAD_DT, sums=fake, nparams=4, max_blocks=2), DTYPE),
    # cc_adam_dec_transposed
    (adam_dec_transposed, dict(p=null), NULL),
    (adam_dec_transposed, dict(W_dec_t=null), NULL),
    (adam_dec_transposed, dict(part=null), NULL),
    (adam_dec_transposed, dict(dtype=F32), DTYPE),
    (adam_dec_transposed, dict(h=60), SHAPE),             # h % 8
    (adam_dec_transposed, dict(K=96), SHAPE),             # K % 64
    (adam_dec_transposed, dict(step=0), SHAPE),
    (adam_dec_transposed, dict(h=(1 << 30) + 8), SHAPE),
    (adam_dec_transposed, dict(m=odd), ALIGN),
    (adam_dec_transposed, dict(W_dec_t=odd), ALIGN),
    # cc_loss_fwd_bwd_rows
    (loss_rows, dict(recon=null), NULL),
    (loss_rows, dict(x=null), NULL),
    (loss_rows, dict(g_recon=null), NULL),
    (loss_rows, dict(row_part=null), NULL),
    (loss_rows, dict(d=76), SHAPE),
    (loss_rows, dict(n=0), SHAPE),
    (loss_rows, dict(rows=0), SHAPE),
    (loss_rows, dict(row0=32, rows=8), SHAPE),            # past the batch
    (loss_rows, dict(row0=8, rows=8), SHAPE),             # row0 % 32
    (loss_rows, dict(recon=odd), ALIGN),
    (loss_rows, dict(b_dec=odd), ALIGN),
    (loss_rows, dict(x_mean=odd), ALIGN),
    (loss_rows, dict(dtype=BAD_DT), DTYPE),
    # cc_loss_fwd_bwd_rows_t (g_recon_t given: bf16, B % 8 == 0, rows % 8 == 0)
    (loss_rows_t, dict(recon=null), NULL),
    (loss_rows_t, dict(row_part=null), NULL),
    (loss_rows_t, dict(d=76), SHAPE),
    (loss_rows_t, dict(B=76, rows=72), SHAPE),            # B % 8
    (loss_rows_t, dict(rows=36), SHAPE),                  # rows % 8
    (loss_rows_t, dict(row0=64, rows=16), SHAPE),
    (loss_rows_t, dict(row0=8, rows=8), SHAPE),
    (loss_rows_t, dict(dtype=F32), DTYPE),
    (loss_rows_t, dict(x=odd), ALIGN),
    (loss_rows_t, dict(g_recon_t=odd), ALIGN),
    (loss_rows_t, dict(x_mean=odd), ALIGN),
    # cc_clip_finalize, cc_segment_sums
    (clip_finalize, dict(sq=null), NULL),
    (clip_finalize, dict(off=None), NULL),
    (clip_finalize, dict(out=null), NULL),
    (clip_finalize, dict(nparams=0), SHAPE),
    (clip_finalize, dict(nparams=9), SHAPE),
    (segment_sums, dict(sq=null), NULL),
    (segment_sums, dict(off=None), NULL),
    (segment_sums, dict(out=null), NULL),
    (segment_sums, dict(nparams=0), SHAPE),
    (segment_sums, dict(nparams=9), SHAPE),
]


def _show(v):
    return {null.value: "null", fake.value: "fake", odd.value: "odd"}.get(v.value) if isinstance(v, ctypes.c_void_p) else v


@pytest.mark.parametrize("call,wrong,code", CASES,
                         ids=[f"{c.__name__}-{'-'.join(f'{k}={_show(v)}' for k, v in w.items())}" for c, w, _ in CASES])
def test_one_wrong_argument_gives_its_code(call, wrong, code):
    assert call(_lib.load(), **wrong) == code
