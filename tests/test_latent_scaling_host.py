"""LatentScaling, the parts that need no GPU: the public name, the C ABI's declaration, the argument checks of
cc_latent_scaling, and the closed-form scales (latent_scaling.betas) against a brute-force least squares."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, latent_scaling, ops
from tests import _latent_scaling_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_name():
    assert ca.LatentScaling is latent_scaling.LatentScaling
    for method in ("update", "update_from_parts", "result", "reset"):
        assert callable(getattr(ca.LatentScaling, method))
    assert callable(latent_scaling.betas) and callable(ops.latent_scaling)


def test_entry_point_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    lib = _lib.load()
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    assert re.search(r"\bint\s+cc_latent_scaling\s*\(", header)
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):  # (exports.map's cc_* pattern lets it through)
        out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert "cc_latent_scaling" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    assert len(_lib.SIGNATURES["cc_latent_scaling"][1]) == 13
    getattr(lib, "cc_latent_scaling")


def test_argument_validation_needs_no_gpu():
    """Every check comes before any launch: the fake device pointers are never touched.  (A valid-looking call is
    not made: it would launch.)"""
    lib = _lib.load()
    p = 1 << 20

    def call(Y=p, ldy=16, W=p, ldw=16, acts=p, lda=24, dot=p, sq=None, B=4, d=16, h=8, dtype=_lib.CC_BF16):
        return lib.cc_latent_scaling(Y, ldy, W, ldw, acts, lda, dot, sq, B, d, h, dtype, None)

    NULL, DTYPE, SHAPE, ALIGN = 1, 2, 3, 4
    assert [call(Y=None), call(W=None), call(acts=None), call(dot=None)] == [NULL] * 4
    assert call(dtype=7) == DTYPE and call(dtype=0) == DTYPE
    assert [call(B=0), call(d=0, ldy=16), call(h=0), call(B=-1)] == [SHAPE] * 4
    assert call(d=12) == SHAPE and call(d=20, ldy=24, ldw=24) == SHAPE          # d % 8
    assert call(h=6) == SHAPE and call(h=10) == SHAPE                          # h % 4
    assert [call(ldy=8), call(ldw=8), call(lda=4)] == [SHAPE] * 3               # a pitch below the row
    assert [call(Y=p + 8), call(W=p + 4), call(acts=p + 2), call(dot=p + 8), call(sq=p + 4)] == [ALIGN] * 5
    assert [call(ldy=20), call(ldw=36), call(lda=12)] == [ALIGN] * 3           # bf16: 40 / 72 / 24-byte pitches
    assert call(lda=10, dtype=_lib.CC_F32) == ALIGN and call(ldy=18, dtype=_lib.CC_F32) == ALIGN
    assert b"alig" in lib.cc_strerror(ALIGN).lower()


def problem(rows, n, d, h, seed, dead):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    W_dec, b_dec, x = 0.3 * rnd(h, n, d), 0.1 * rnd(n, d), rnd(rows, n, d)
    f = torch.relu(rnd(rows, h) - 0.8)  # ReLU-sparse: about a fifth of the entries fire
    f[:, dead] = 0.0
    assert bool((f[:, [j for j in range(h) if j != dead]] > 0).any(0).all())
    R = torch.einsum("bh,hnd->bnd", f, W_dec) + b_dec
    return f, x - R, R, W_dec


@pytest.mark.parametrize("n,decoder_models", [(2, (0, 1)), (3, (0, 2, -1))])
def test_betas_against_brute_force_least_squares(n, decoder_models):
    rows, d, h, dead = 50, 8, 12, 5
    f, E, R, W_dec = problem(rows, n, d, h, seed=7 + n, dead=dead)
    alive = [j for j in range(h) if j != dead]
    for r in decoder_models:
        S_err = torch.stack([ref.accumulators(f, E[:, m], W_dec[:, r])[0] for m in range(n)])
        S_rec = torch.stack([ref.accumulators(f, R[:, m], W_dec[:, r])[0] for m in range(n)])
        Q = ref.accumulators(f, E[:, 0], W_dec[:, r])[2]
        G = torch.einsum("hd,hmd->mh", W_dec[:, r], W_dec)
        be, br, ne, nr = latent_scaling.betas(S_err, S_rec, Q, G, r)
        want_e, want_r = ref.brute_force_betas(f, E, R, W_dec, r)
        for got, want in ((be, want_e), (br, want_r)):
            assert got.dtype == torch.float64 and got.shape == (n, h)
            torch.testing.assert_close(got[:, alive], want[:, alive], rtol=1e-9, atol=0)
            assert bool(got[:, dead].isnan().all()) and bool(want[:, dead].isnan().all())
        rr = r % n
        torch.testing.assert_close(ne[:, alive], (want_e / want_e[rr])[:, alive], rtol=1e-9, atol=0)
        torch.testing.assert_close(nr[:, alive], (want_r / want_r[rr])[:, alive], rtol=1e-9, atol=0)
        assert bool(ne[:, dead].isnan().all()) and bool(nr[:, dead].isnan().all())
        assert torch.equal(ne[rr, alive], torch.ones(len(alive), dtype=torch.float64))


def test_betas_zero_decoder_direction_is_nan():
    """G[r][j] = 0 (the decoder model's vector is zero): no direction to scale, NaN for that latent only."""
    n, h = 2, 4
    S = torch.full((n, h), 3.0, dtype=torch.float64)  # (beta_rec = S - Q G = 2, not 0: its ratios are finite)
    Q = torch.ones(h, dtype=torch.float64)
    G = torch.ones(n, h, dtype=torch.float64)
    G[1, 2] = 0.0
    out = latent_scaling.betas(S, S, Q, G, 1)
    for t in out:
        assert bool(t[:, 2].isnan().all()) and not bool(t[:, [0, 1, 3]].isnan().any())
    with pytest.raises(ValueError):
        latent_scaling.betas(S, S, Q, G, 2)
