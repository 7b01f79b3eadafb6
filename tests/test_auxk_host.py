"""The AuxK dead-latent loss, the parts that need no GPU: the reference itself, the cfg keys and their checkpoint
round trip, the C ABI's argument checks and the sharded trainer's refusal."""
import json

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, sharded
from crosscoder_amd.crosscoder import auxk_options, write_checkpoint
from tests._auxk_ref import aux_select, aux_select_brute, auxk_loss_ref, dead_update_ref, g_aux_ref

SHAPE, NULL, DTYPE, TOO_LARGE, ALIGN = 3, 1, 2, 5, 4  # CC_ERR_*


def cfg_for(**kw):
    cfg = {"seed": 49, "batch_size": 64, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 6400, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": 256, "seq_len": 1024, "enc_dtype": "bf16", "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": 32, "log_every": 100, "save_every": 30000, "activation": "topk", "k": 8}
    cfg.update(kw)
    return cfg


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_selection_matches_a_plain_loop(dtype):
    g = torch.Generator().manual_seed(0)
    v = (torch.randint(-3, 6, (6, 16), generator=g).float() / 2).to(dtype)  # few distinct values: ties
    v[1] = 0.0
    v[2, 3], v[2, 4], v[2, 5] = float("inf"), float("nan"), -0.0
    dead = torch.tensor([True, False, True, True, False, True, True, True,
                         False, False, True, True, True, False, True, True])
    for k_aux in (1, 2, 5, 16):
        ref = aux_select(v, dead, k_aux)
        want = aux_select_brute(v.float().tolist(), dead.tolist(), k_aux)
        for b in range(6):
            assert ref["mask"][b].nonzero().flatten().tolist() == want[b], (b, k_aux)
            assert ref["count"][b].item() == len(want[b])
        assert not bool(ref["mask"][:, ~dead].any())  # never a live latent
        dense = ref["dense"]
        assert torch.equal(dense[ref["mask"]].float(), v[ref["mask"]].float())
        assert bool((dense[~ref["mask"]].float() == 0).all()) and not bool(torch.signbit(dense[~ref["mask"]]).any())
    assert aux_select(v, torch.zeros(16, dtype=torch.bool), 4)["count"].sum().item() == 0


def test_reference_dead_update_and_loss_against_plain_loops():
    colsum = torch.tensor([0.0, 1e-42, float("inf"), 3.0, 0.0, 0.0])
    tsf = torch.tensor([0, 90, 95, 100, 100, 89], dtype=torch.int64)
    new, count, was = dead_update_ref(colsum, tsf, 10, 100, 5)
    assert new.tolist() == [10, 0, 0, 0, 110, 99] and count == 1 and was.tolist() == [False] * 3 + [True, True, False]
    assert dead_update_ref(colsum, tsf, 11, 100, 6)[1] == 2  # the last latent crosses, and is counted below h_real 6
    g = torch.Generator().manual_seed(1)
    e = torch.randn(6, 16, generator=g, dtype=torch.float64) + 1.0
    ehat = torch.randn(6, 16, generator=g, dtype=torch.float64)
    num = sum((ehat[b, k] - e[b, k]).item() ** 2 for b in range(6) for k in range(16)) / 6
    den = 0.0
    for k in range(16):
        mean = sum(e[b, k].item() for b in range(6)) / 6
        den += sum((e[b, k].item() - mean) ** 2 for b in range(6)) / 6
    loss, d, valid = auxk_loss_ref(e, ehat)
    assert valid and abs(loss.item() - num / den) < 1e-12 * num / den and abs(d.item() - den) < 1e-12 * den
    eh = ehat.clone().requires_grad_(True)
    (0.25 * auxk_loss_ref(e, eh)[0]).backward()
    assert torch.allclose(eh.grad, g_aux_ref(e, ehat, 0.25, torch.float64), rtol=1e-12, atol=0)
    # forced to 0: a constant residual per column (den = 0), a NaN, everything zero
    const = torch.full((6, 16), 0.5, dtype=torch.float64)
    for ee, hh in ((const, ehat), (e, torch.full_like(ehat, float("nan"))), (const * 0, ehat * 0)):
        loss, _, valid = auxk_loss_ref(ee, hh)
        assert not valid and loss.item() == 0.0
        assert not bool(g_aux_ref(ee, hh, 0.25, torch.float32).view(torch.int32).any())


# ----------------------------------------------------------------------------- cfg
def test_cfg_validation():
    assert auxk_options(cfg_for()) is None and auxk_options(cfg_for(auxk_coeff=0)) is None
    assert auxk_options(cfg_for(activation="relu", k_aux=-3)) is None  # off: the other keys are not looked at
    assert auxk_options(cfg_for(auxk_coeff=0.03125)) == (0.03125, 32, 10_000_000)  # k_aux: n_models * d_in // 2
    assert auxk_options(cfg_for(auxk_coeff=1, dict_size=16, k=4)) == (1.0, 16, 10_000_000)  # capped at dict_size
    assert auxk_options(cfg_for(auxk_coeff=0.5, k_aux=256, dead_tokens=1, activation="batch_topk")) == (0.5, 256, 1)
    assert auxk_options(cfg_for(auxk_coeff=0.5), n_models=4)[1] == 64
    for bad in (dict(auxk_coeff=-1.0), dict(auxk_coeff="1"), dict(auxk_coeff=True), dict(auxk_coeff=float("nan")),
                dict(auxk_coeff=float("inf")),
                dict(auxk_coeff=0.5, activation="relu"), dict(auxk_coeff=0.5, k_aux=0), dict(auxk_coeff=0.5, k_aux=257),
                dict(auxk_coeff=0.5, k_aux=4.0), dict(auxk_coeff=0.5, k_aux=True), dict(auxk_coeff=0.5, dead_tokens=0),
                dict(auxk_coeff=0.5, dead_tokens=1.5), dict(auxk_coeff=0.5, dead_tokens=False)):
        with pytest.raises(ValueError):
            auxk_options(cfg_for(**bad))
        with pytest.raises(ValueError):  # at construction, before anything touches the device
            ca.CrossCoder(cfg_for(**bad))
    cfg = cfg_for(auxk_coeff=0.5)
    del cfg["activation"]  # absent: the reference's ReLU
    with pytest.raises(ValueError, match="activation"):
        auxk_options(cfg)


def test_sharded_trainer_refuses_auxk():
    cfg = cfg_for(auxk_coeff=0.5)
    for key in ("activation", "k"):
        del cfg[key]
    with pytest.raises(ValueError, match="auxk"):
        sharded.ShardedTrainer(cfg, buffer=None)


def test_checkpoint_cfg_round_trip(tmp_path):
    cfg = cfg_for(auxk_coeff=0.03125, k_aux=48, dead_tokens=12345, device="cpu")
    write_checkpoint({}, cfg, tmp_path, 0)
    back = json.load(open(tmp_path / "0_cfg.json"))
    assert (back["auxk_coeff"], back["k_aux"], back["dead_tokens"]) == (0.03125, 48, 12345)
    assert auxk_options(back) == auxk_options(cfg) == (0.03125, 48, 12345)


# ----------------------------------------------------------------------------- the C ABI's argument checks
def test_signatures_typed():
    for name, nargs in (("cc_auxk_rows", 11), ("cc_dead_update", 10), ("cc_auxk_loss", 13), ("cc_add_rows", 7),
                        ("cc_auxk_part_floats", 2)):
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        getattr(_lib.load(), name)


def test_auxk_rows_argument_errors_in_topk_rows_order():
    """Shape / NULL / dtype / size / alignment errors are returned before any launch (host pointers are never
    touched), in cc_topk_rows' order."""
    lib = _lib.load()
    buf, other = torch.zeros(256), torch.zeros(256)
    p, q = buf.data_ptr(), other.data_ptr()
    tsf = torch.zeros(64, dtype=torch.int64).data_ptr()

    def call(acts=p, ld=16, B=4, h=16, dtype=_lib.CC_F32, k=4, since=tsf, out=q, rc=None):
        return lib.cc_auxk_rows(acts, ld, B, h, dtype, k, since, 5, out, rc, None)

    assert call(k=0) == SHAPE and call(k=17) == SHAPE
    assert call(ld=17) == SHAPE and call(ld=20) == SHAPE and call(ld=8) == SHAPE
    assert call(h=12, ld=16) == SHAPE and call(B=0) == SHAPE
    assert call(acts=None) == NULL and call(since=None) == NULL and call(out=None) == NULL
    assert call(out=p) == NULL  # aux_out must not be acts
    assert call(k=0, acts=None) == SHAPE and call(acts=None, dtype=7) == NULL  # the order
    assert call(dtype=7) == DTYPE
    assert call(dtype=7, h=1 << 18, ld=1 << 18) == DTYPE
    assert call(h=1 << 18, ld=1 << 18) == TOO_LARGE
    assert call(out=q + 4) == ALIGN and call(since=tsf + 4) == ALIGN and call(rc=q + 2) == ALIGN
    assert call(h=1 << 18, ld=1 << 18, out=q + 4) == TOO_LARGE


def test_small_kernels_argument_errors():
    lib = _lib.load()
    f = torch.zeros(256).data_ptr()
    i64 = torch.zeros(64, dtype=torch.int64).data_ptr()

    def dead(colsum=f, since=i64, h=16, h_real=16, B=4, count=f):
        return lib.cc_dead_update(colsum, since, h, h_real, B, 5, None, count, None, None)

    assert dead(h=0) == SHAPE and dead(h_real=17) == SHAPE and dead(h_real=-1) == SHAPE and dead(B=0) == SHAPE
    assert dead(colsum=None) == NULL and dead(since=None) == NULL and dead(count=None) == NULL
    assert dead(h=(1 << 17) + 8, h_real=0) == TOO_LARGE
    assert dead(since=i64 + 4) == ALIGN and dead(count=f + 2) == ALIGN

    def loss(recon=f, b=f, x=f, ehat=f, g=f, part=f, sc=f, B=4, K=16, dtype=_lib.CC_F32):
        return lib.cc_auxk_loss(recon, b, x, ehat, g, part, sc, None, 0.5, B, K, dtype, None)

    assert loss(B=0) == SHAPE and loss(K=12) == SHAPE and loss(K=0) == SHAPE
    for name in ("recon", "b", "x", "ehat", "g", "part", "sc"):
        assert loss(**{name: None}) == NULL, name
    assert loss(dtype=0) == DTYPE and loss(g=f + 8) == ALIGN
    # per 32-row block: K column sums + 2 squared sums per 2048 columns; then one fp64 per 64 columns
    assert lib.cc_auxk_part_floats(0, 16) == 0 and lib.cc_auxk_part_floats(96, 80) == 3 * (80 + 2) + 2 * 2
    assert lib.cc_auxk_part_floats(4096, 4608) == 128 * (4608 + 2 * 3) + 2 * 72

    def add(dst=f, src=f + 512, rows=4, cols=16, ld=16, dtype=_lib.CC_BF16):
        return lib.cc_add_rows(dst, src, rows, cols, ld, dtype, None)

    assert add(rows=0) == SHAPE and add(cols=12) == SHAPE and add(ld=8) == SHAPE and add(ld=20) == SHAPE
    assert add(dst=None) == NULL and add(src=None) == NULL and add(dtype=3) == DTYPE and add(src=f + 8) == ALIGN
