"""CPU: the dead-latent resampling surface (cc_row_norms, cc_resample_pick, cc_resample_write, ops.*, LatentResampler,
Trainer.resample_dead_latents, cfg["resample_every"]) exists and validates its arguments before any launch, and the
CPU reference's picker (tests/_resample_ref.py) agrees with torch.searchsorted on an fp64 cumsum."""
import ctypes
import os
import re

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, ops, sharded
from crosscoder_amd.trainer import resample_options
from tests import _resample_ref as ref
from tests.test_cpu_host import _cfg, _dynamic_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DTYPE, SHAPE, ALIGN, TOO_LARGE = 0, 1, 2, 3, 4, 5
NAMES = {"cc_row_norms": 7, "cc_resample_pick": 7, "cc_resample_write": 18}


def test_public_names_exist():
    assert callable(ca.LatentResampler)
    assert callable(ca.Trainer.resample_dead_latents)
    for name in ("row_norms", "resample_pick", "resample_write"):
        assert callable(getattr(ops, name))


def test_entry_points_are_declared_exported_and_typed():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read(), flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt).group(1)
        assert len(decl.split(",")) == nargs, name
        assert name in _dynamic_exports(_lib.LIB_PATH), name
        assert name in _dynamic_exports(_lib.DEBUG_LIB_PATH), name


FAKE = 1 << 20  # a 16-byte aligned address that is never dereferenced: every call below fails a check first
p = lambda v: ctypes.c_void_p(v)  # noqa: E731


def norms(**kw):
    good = dict(W=FAKE, ld=80, rows=4, K=80, dtype=1, out=FAKE + 4096)
    a = dict(good, **kw)
    assert a != good, "a call with valid arguments would launch"
    return _lib.load().cc_row_norms(p(a["W"]), a["ld"], a["rows"], a["K"], a["dtype"], p(a["out"]), p(0))


def test_row_norms_checks():
    for bad in (dict(rows=0), dict(rows=-1), dict(K=0), dict(K=-8), dict(K=4), dict(K=84, ld=88), dict(ld=72)):
        assert norms(**bad) == SHAPE, bad
    assert norms(rows=0, W=0, dtype=7) == SHAPE
    assert norms(W=0) == NULL and norms(out=0) == NULL
    assert norms(W=0, dtype=7) == NULL
    assert norms(dtype=0) == DTYPE and norms(dtype=3) == DTYPE
    assert norms(rows=1 << 31) == TOO_LARGE
    assert norms(W=FAKE + 8) == ALIGN and norms(out=FAKE + 2) == ALIGN
    assert norms(ld=84) == ALIGN                 # bf16: 168 bytes
    assert norms(ld=82, dtype=2) == ALIGN        # fp32: 328 bytes


def pick(**kw):
    good = dict(loss=FAKE, R=64, u=FAKE + 4096, J=4, cdf=FAKE + 8192, rows_out=FAKE + 12288)
    a = dict(good, **kw)
    assert a != good, "a call with valid arguments would launch"
    return _lib.load().cc_resample_pick(p(a["loss"]), a["R"], p(a["u"]), a["J"], p(a["cdf"]), p(a["rows_out"]), p(0))


def test_resample_pick_checks():
    for bad in (dict(R=0), dict(R=-5), dict(J=0), dict(J=-1)):
        assert pick(**bad) == SHAPE, bad
    assert pick(R=0, loss=0) == SHAPE
    for name in ("loss", "u", "cdf", "rows_out"):
        assert pick(**{name: 0}) == NULL, name
    assert pick(R=1 << 31) == TOO_LARGE and pick(J=1 << 31) == TOO_LARGE
    assert pick(loss=FAKE + 2) == ALIGN
    for name in ("u", "cdf", "rows_out"):
        assert pick(**{name: FAKE + 4}) == ALIGN, name


def write(**kw):
    good = dict(X=FAKE, ldx=80, R=16, rows=FAKE + 4096, latents=FAKE + 8192, J=4, h=64, K=80, dtype=1, enc=0.1, dec=1.0,
                params=FAKE + 65536, master=FAKE + 2 * 65536, m=FAKE + 3 * 65536, v=FAKE + 4 * 65536, sdt=1,
                done=FAKE + 12288)
    a = dict(good, **kw)
    assert a != good, "a call with valid arguments would launch"
    return _lib.load().cc_resample_write(p(a["X"]), a["ldx"], a["R"], p(a["rows"]), p(a["latents"]), a["J"], a["h"],
                                         a["K"], a["dtype"], a["enc"], a["dec"], p(a["params"]), p(a["master"]),
                                         p(a["m"]), p(a["v"]), a["sdt"], p(a["done"]), p(0))


def test_resample_write_checks():
    for bad in (dict(R=0), dict(J=0), dict(J=-3), dict(h=0), dict(h=-8), dict(h=60), dict(K=0), dict(K=-8),
                dict(K=84, ldx=88), dict(ldx=72)):
        assert write(**bad) == SHAPE, bad
    assert write(J=0, X=0, dtype=9) == SHAPE
    for name in ("X", "rows", "latents", "params"):
        assert write(**{name: 0}) == NULL, name
    assert write(m=0) == NULL and write(v=0) == NULL     # the moments go together
    assert write(X=0, dtype=9) == NULL
    assert write(dtype=0) == DTYPE and write(dtype=3) == DTYPE
    assert write(sdt=0) == DTYPE and write(sdt=5) == DTYPE
    assert write(dtype=9, h=1 << 31) == DTYPE
    assert write(h=1 << 31) == TOO_LARGE and write(R=1 << 31) == TOO_LARGE
    for name in ("X", "params", "master", "m", "v"):
        assert write(**{name: FAKE + 8}) == ALIGN, name
    assert write(ldx=84) == ALIGN and write(ldx=82, dtype=2) == ALIGN
    assert write(rows=FAKE + 4100) == ALIGN and write(latents=FAKE + 8196) == ALIGN and write(done=FAKE + 12290) == ALIGN


def test_latent_resampler_argument_errors():
    cfg = _cfg("fp32")
    cc = ca.CrossCoder(cfg)
    with pytest.raises(ValueError, match="jumprelu"):
        ca.LatentResampler(ca.CrossCoder(dict(cfg, activation="jumprelu", l0_coeff=0.1)), rows=8)
    for bad in (0, -4, 2.5, True):
        with pytest.raises(ValueError, match="rows"):
            ca.LatentResampler(cc, rows=bad)
    for kw in (dict(enc_scale=0), dict(enc_scale=float("nan")), dict(dec_scale=-1.0), dict(dec_scale=float("inf"))):
        with pytest.raises(ValueError, match="scale"):
            ca.LatentResampler(cc, rows=8, **kw)
    rs = ca.LatentResampler(cc, rows=8)
    assert rs.filled == 0 and tuple(rs.dead().shape) == (cfg["dict_size"],)
    with pytest.raises(ValueError, match="do not fit"):   # pool overflow, before any launch
        rs.add(torch.zeros(9, 2, cfg["d_in"]))
    with pytest.raises(ValueError, match="expected x"):
        rs.add(torch.zeros(4, 3, cfg["d_in"]))
    with pytest.raises(ValueError, match="distinct"):     # a duplicated latent index
        rs.apply(dead=torch.tensor([3, 7, 3]))
    with pytest.raises(ValueError, match=r"\[0, 256\)"):
        rs.apply(dead=torch.tensor([3, 256]))
    with pytest.raises(ValueError, match="mask"):
        rs.apply(dead=torch.zeros(255, dtype=torch.bool))
    with pytest.raises(ValueError, match="dead must be"):
        rs.apply(dead=torch.tensor([0.5]))
    with pytest.raises(ValueError, match="one float per dead latent"):
        rs.apply(dead=torch.tensor([1, 2]), u=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="optimizer"):
        rs.apply(optimizer=ca.trainer.FusedAdam(ca.CrossCoder(cfg), 1e-4, (0.9, 0.999)), dead=torch.tensor([1]))
    # an empty pool resamples nothing and says so, without a launch (this machine has no device)
    out = rs.apply(dead=torch.tensor([5, 1]))
    assert out["resampled"] == 0 and out["latents"].tolist() == [1, 5] and out["rows"].tolist() == [-1, -1]
    assert out["enc_norm"] == 0.0 and out["dec_norm"] == 0.0 and not bool(out["written"].any())


def test_trainer_argument_errors():
    cfg = _cfg("fp32")
    assert resample_options(cfg) is None and resample_options(dict(cfg, resample_every=0)) is None
    assert resample_options(dict(cfg, resample_every=5, resample_rows=128)) == (5, 128, 0.2)
    assert resample_options(dict(cfg, resample_every=5))[1] == 819200
    for bad in (dict(resample_every=-1), dict(resample_every=2.0), dict(resample_every=True),
                dict(resample_every=2, resample_rows=63), dict(resample_every=2, resample_rows=1e5),
                dict(resample_every=2, resample_enc_scale=0), dict(resample_every=2, resample_enc_scale="a"),
                dict(resample_every=2, activation="jumprelu", l0_coeff=0.1)):
        with pytest.raises(ValueError, match="resample_every|resample_rows|resample_enc_scale"):
            resample_options(dict(cfg, **bad))
    with pytest.raises(ValueError, match="resample_every"):
        ca.Trainer(dict(cfg, resample_every=-2), buffer=object(), crosscoder=ca.CrossCoder(cfg))
    tr = ca.Trainer(cfg, buffer=object(), crosscoder=ca.CrossCoder(cfg))
    assert tr.resample is None and tr._resampler is None
    with pytest.raises(ValueError, match="this trainer's crosscoder"):
        tr.resample_dead_latents(ca.LatentResampler(ca.CrossCoder(cfg), rows=8))


def test_sharded_trainer_refuses_resample_every():
    cfg = _cfg("bf16")
    with pytest.raises(ValueError, match="resample_every"):
        sharded.ShardedTrainer(dict(cfg, resample_every=100), buffer=None)
    with pytest.raises(ValueError, match="resample_every"):
        sharded.ShardedTrainer(cfg, buffer=None, crosscoder=ca.CrossCoder(dict(cfg, resample_every=100)))


def _losses(R, seed):
    g = torch.Generator().manual_seed(seed)
    loss = torch.rand(R, generator=g) + 0.05
    if R >= 8:
        loss[torch.randperm(R, generator=g)[:R // 8]] = 0.0
        loss[1], loss[R - 2] = float("nan"), -3.0
    return loss


@pytest.mark.parametrize("R", [1, 2, 63, 1025])
def test_reference_picker_against_searchsorted(R):
    loss = _losses(R, R)
    c = ref.cdf(loss)
    assert torch.equal(c, torch.cumsum(torch.where(torch.isfinite(loss) & (loss >= 0), loss.double() ** 2,
                                                   torch.zeros(R, dtype=torch.float64)), 0))
    g = torch.Generator().manual_seed(R + 1)
    u = torch.cat([torch.rand(200, dtype=torch.float64, generator=g), torch.tensor([0.0, 1.0 - 2.0 ** -53])])
    want = torch.searchsorted(c, u * c[-1], right=True).clamp(max=R - 1)
    assert ref.pick(c, u).tolist() == want.tolist() == ref.pick_loop(c, u)
    w = ref.weights(loss)
    assert bool((w[want] > 0).all())  # never a zero-weight row
    # the midpoint of a row's interval picks that row
    rows = ref.safe_rows(loss)
    assert rows.numel() > 0
    assert ref.pick(c, ref.midpoints(c, rows)).tolist() == rows.tolist()
    zero = torch.zeros(R)
    assert ref.pick(ref.cdf(zero), u).tolist() == [-1] * u.shape[0] == ref.pick_loop(ref.cdf(zero), u)


def test_bounds_are_what_the_derivation_says():
    assert ref.row_norm_tol(8) == (14 / 2 + 2) * 2.0 ** -24
    assert ref.row_norm_tol(4608) == ((8 * 9 + 6) / 2 + 2) * 2.0 ** -24
    assert ref.write_tol(4608) == ((8 * 3 + 9) / 2 + 4) * 2.0 ** -24
    assert ref.write_tol_bf16(1 << 16) < 2.0 ** -8
    x = torch.tensor([3.0, 4.0])
    assert torch.equal(ref.reseed(x, 2.0), torch.tensor([1.2, 1.6], dtype=torch.float64))
    assert ref.row_norms(x[None]).tolist() == [5.0]
