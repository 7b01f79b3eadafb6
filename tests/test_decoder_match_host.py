"""Decoder matching, the parts that need no GPU: the public name, the C ABI's declarations, the argument checks of
cc_decoder_match / cc_match_reduce, of the ops wrappers and of match_decoders, the key order, and the key decoding."""
import os
import random
import re
import shutil
import subprocess
import types

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, decoder_match, ops
from tests import _decoder_match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_name():
    assert ca.match_decoders is decoder_match.match_decoders
    assert callable(ops.decoder_match) and callable(ops.match_reduce)


def test_entry_points_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    lib = _lib.load()
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    for name, nargs in (("cc_decoder_match", 14), ("cc_match_reduce", 5)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):  # (exports.map's cc_* pattern lets them through)
            out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
            assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
        assert len(_lib.SIGNATURES[name][1]) == nargs
        getattr(lib, name)
    assert "finite" in header[header.index("Decoder matching"):header.index("int cc_decoder_match")]


def test_c_abi_validation_needs_no_gpu():
    """Every check comes before any launch: the fake device pointers are never touched.  (A valid-looking call is
    not made: it would launch.)"""
    lib = _lib.load()
    p = 1 << 20

    def call(Wc=p, ldc=16, Wq=p, ldq=16, cs=p, qs=p, keys=p, M=4, N=8, K=16, row0=0, diag=0, dtype=_lib.CC_BF16):
        return lib.cc_decoder_match(Wc, ldc, Wq, ldq, cs, qs, keys, M, N, K, row0, diag, dtype, None)

    NULL, DTYPE, SHAPE, ALIGN, TOO_LARGE = 1, 2, 3, 4, 5
    assert [call(Wc=None), call(Wq=None), call(cs=None), call(qs=None), call(keys=None)] == [NULL] * 5
    assert call(dtype=7) == DTYPE and call(dtype=0) == DTYPE
    assert [call(M=0), call(N=0), call(K=0), call(M=-1), call(row0=-1)] == [SHAPE] * 5
    assert call(K=12) == SHAPE and call(K=20, ldc=24, ldq=24) == SHAPE            # K % 8
    assert call(N=6) == SHAPE and call(N=10) == SHAPE                            # N % 4
    assert [call(ldc=8), call(ldq=8)] == [SHAPE] * 2                             # a pitch below the row
    assert [call(Wc=p + 8), call(Wq=p + 4), call(qs=p + 8), call(keys=p + 8), call(cs=p + 2)] == [ALIGN] * 5
    assert [call(ldc=20), call(ldq=36)] == [ALIGN] * 2                           # bf16: 40 / 72-byte pitches
    assert call(ldc=18, dtype=_lib.CC_F32) == ALIGN
    assert call(M=8, row0=(1 << 32) - 8) == TOO_LARGE                            # row0 + M must fit in 32 bits
    assert call(ldc=1 << 23, ldq=1 << 23) == TOO_LARGE                           # 256 rows of 16 MiB: past 2 GiB

    def red(part=p, R=4, N=8, best=p):
        return lib.cc_match_reduce(part, R, N, best, None)

    assert [red(part=None), red(best=None)] == [NULL] * 2
    assert [red(R=0), red(N=0), red(R=-1)] == [SHAPE] * 3
    assert [red(part=p + 4), red(best=p + 2)] == [ALIGN] * 2


def test_key_orders_score_descending_then_index_ascending():
    rnd = random.Random(5)
    scores = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1e-30, -1e-30, 1 - 2.0 ** -24, 1 + 2.0 ** -23, -3.5, 2.0 ** -149,
              -(2.0 ** -149)]
    scores = [struct_round(s) for s in scores + [rnd.uniform(-1, 1) for _ in range(40)]]
    idx = [0, 1, 2, 255, 256, 65535, 2 ** 17 - 1, 2 ** 31, 2 ** 32 - 1]
    pairs = [(s, i) for s in scores for i in idx]
    for s, i in pairs:
        k = ref.key(s, i)
        assert 0 < k < 2 ** 64
        got_s, got_i = ref.unkey(k)
        assert got_i == i and got_s == s and str(got_s) == str(s + 0.0)   # (-0 comes back as +0)
    by_key = sorted(pairs, key=lambda p: ref.key(*p), reverse=True)
    by_rule = sorted(pairs, key=lambda p: (-(p[0] + 0.0), p[1]))
    assert [(s + 0.0, i) for s, i in by_key] == [(s + 0.0, i) for s, i in by_rule]
    # -0 and +0 are one score: the index decides
    assert ref.key(-0.0, 3) == ref.key(0.0, 3) and ref.key(-0.0, 3) > ref.key(0.0, 4)
    # a negative score beats a more negative one and loses to any zero or positive one; everything beats "no candidate"
    assert ref.key(-0.25, 9) > ref.key(-0.5, 0) and ref.key(0.0, 2 ** 32 - 1) > ref.key(-1e-30, 0)
    assert ref.key(-3.0e38, 2 ** 32 - 1) > 0 and ref.unkey(0)[1] == -1


def struct_round(x):
    """x rounded to fp32 (the keys hold fp32 scores)."""
    return float(torch.tensor(x, dtype=torch.float32))


def test_decode_keys_inverts_the_key_map():
    pairs = [(0.75, 5), (-0.75, 0), (0.0, 7), (-0.0, 2 ** 17 - 1), (1.0, 2 ** 31 + 3), (-1e-20, 1)]
    ks = [ref.key(s, i) for s, i in pairs] + [0]
    best = torch.tensor([k - 2 ** 64 if k >= 2 ** 63 else k for k in ks], dtype=torch.int64)
    assert ref.as_unsigned(best) == ks
    index, cosine = decoder_match.decode_keys(best)
    assert index.dtype == torch.int64 and cosine.dtype == torch.float32
    assert index.tolist() == [i for _, i in pairs] + [-1]
    assert cosine[:-1].tolist() == [struct_round(s) + 0.0 for s, _ in pairs] and bool(cosine[-1].isnan())
    q_scale = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    index, cosine = decoder_match.decode_keys(best, q_scale)
    assert index.tolist()[:3] == [5, -1, 7] and cosine.isnan().tolist() == [False, True] + [False] * 4 + [True]


def fake_cc(n=2, d_in=16, dtype=torch.bfloat16, device="cuda:0"):
    arena = types.SimpleNamespace(data=types.SimpleNamespace(device=torch.device(device)))
    return types.SimpleNamespace(n_models=n, cfg={"d_in": d_in}, dtype=dtype, d_hidden=32, arena=lambda: arena)


def test_match_decoders_validates_before_any_launch():
    a = fake_cc()
    for bad in (2, -3, 1.0, True, "0"):
        with pytest.raises(ValueError, match="model"):
            ca.match_decoders(a, fake_cc(), model=bad)
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="chunk_rows"):
            ca.match_decoders(a, fake_cc(), chunk_rows=bad)
    for other in (fake_cc(n=3), fake_cc(d_in=24), fake_cc(dtype=torch.float32)):
        with pytest.raises(ValueError, match="differ"):
            ca.match_decoders(a, other)
    with pytest.raises(ValueError, match="devices"):
        ca.match_decoders(a, fake_cc(device="cuda:1"))


def test_ops_wrappers_check_shapes_and_dtypes():
    M, N, K = 12, 8, 16
    Wc, Wq = torch.zeros(M, K, dtype=torch.bfloat16), torch.zeros(N, K, dtype=torch.bfloat16)
    cs, qs = torch.zeros(M), torch.zeros(N)
    R = ops.col_part_rows(M)
    keys = torch.zeros(R, N, dtype=torch.int64)
    bad = [dict(Wq=torch.zeros(N, K + 8, dtype=torch.bfloat16)), dict(Wq=Wq.float()), dict(c_scale=cs[:M - 1]),
           dict(c_scale=cs.double()), dict(q_scale=torch.zeros(N + 4)), dict(q_scale=qs.to(torch.bfloat16)),
           dict(key_part=torch.zeros(R + 1, N, dtype=torch.int64)), dict(key_part=keys.to(torch.int32)),
           dict(key_part=torch.zeros(R, 2 * N, dtype=torch.int64)[:, :N]), dict(row0=-1), dict(row0=1),
           dict(Wc=torch.zeros(M, 2 * K, dtype=torch.bfloat16)[:, ::2])]
    for kw in bad:
        args = dict(Wc=Wc, Wq=Wq, c_scale=cs, q_scale=qs, key_part=keys, row0=0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.decoder_match(**args)
    with pytest.raises(RuntimeError, match="ROCm"):  # everything checked: only the device is missing
        ops.decoder_match(Wc, Wq, cs, qs, keys)
    best = torch.zeros(N, dtype=torch.int64)
    for k, b in ((keys.to(torch.int32), best), (keys, best[:N - 1]), (keys, best.to(torch.int32)), (keys[0], best),
                 (torch.zeros(R, 2 * N, dtype=torch.int64)[:, :N], best)):
        with pytest.raises(ValueError):
            ops.match_reduce(k, b)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.match_reduce(keys, best)
