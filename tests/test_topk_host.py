"""TopK crosscoders, the parts that need no GPU: the selection reference itself, the C ABI's declarations and
argument checks, the cfg keys and the sharded trainer's refusal."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, sharded
from crosscoder_amd.crosscoder import activation_of
from tests._topk_ref import tie_straddles, topk_brute, topk_order, topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cc_topk_rows", "cc_topk_part_rows", "cc_topk_l0_parts")


def test_stable_descending_sort_orders_ties_by_index():
    v = torch.tensor([[1.0, 3, 3, 0, 3, 2, 0, 3]])
    assert topk_order(v)[1].tolist() == [[1, 2, 4, 7, 5, 0, 3, 6]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_matches_brute_force(dtype):
    g = torch.Generator().manual_seed(0)
    rows = [[1.0, 3, 3, 0, 3, 2, 0, 3], [0.0] * 8, [-1.0, -0.0, float("nan"), 2, 2, 2, float("inf"), -2],
            [0.5] * 8, [0.0, 0, 0, 0, 0, 0, 0, 7]]
    rows += (torch.randint(-2, 4, (40, 8), generator=g).float() / 2).tolist()  # few distinct values: ties
    v = torch.tensor(rows).to(dtype)
    for k in range(1, 9):
        ref = topk_ref(v, k)
        for b, row in enumerate(v.float().tolist()):
            want = topk_brute(row, k)
            assert ref["count"][b].item() == len(want)
            assert ref["idx"][b].tolist() == want + [-1] * (k - len(want)), (b, k)
            assert ref["mask"][b].nonzero().flatten().tolist() == want
            assert ref["val"][b].float().tolist()[:len(want)] == [row[i] for i in want]
            assert all(x == 0 for x in ref["val"][b].float().tolist()[len(want):])
        dense = ref["dense"].float()
        assert torch.equal(dense[ref["mask"]], v.float()[ref["mask"]]) and bool((dense[~ref["mask"]] == 0).all())
        assert not bool(torch.signbit(dense[~ref["mask"]]).any())  # the rest is +0
    assert tie_straddles(v, 2).tolist()[:4] == [True, False, True, True]


def test_entry_points_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    lib = _lib.load()
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    exported = {path: {ln.split()[-1] for ln in subprocess.run([nm, "-D", "--defined-only", path], check=True,
                                                                capture_output=True, text=True).stdout.splitlines()
                       if ln.strip()} for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH)}
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), name
        for path, syms in exported.items():
            assert name in syms, (name, path)
        assert name in _lib.SIGNATURES
        getattr(lib, name)
    assert len(_lib.SIGNATURES["cc_topk_rows"][1]) == 12
    for B, h in ((1, 8), (4096, 16384), (2, 131072), (700, 512)):
        rows, parts = lib.cc_topk_part_rows(B, h), lib.cc_topk_l0_parts(B, h)
        assert 1 <= rows <= B and 1 <= parts <= B


def test_argument_validation_needs_no_gpu():
    """Shape / NULL / dtype errors are returned before any launch (host pointers are never touched)."""
    lib = _lib.load()
    buf = torch.zeros(256)
    p = buf.data_ptr()

    def call(acts=p, ld=16, B=4, h=16, dtype=_lib.CC_F32, k=4, out=p, idx=None, val=None):
        return lib.cc_topk_rows(acts, ld, B, h, dtype, k, out, idx, val, None, None, None)

    shape, null, dtype = 3, 1, 2  # CC_ERR_SHAPE, CC_ERR_NULL, CC_ERR_DTYPE
    assert call(k=0) == shape and call(k=17) == shape
    assert call(ld=17) == shape  # odd ld
    assert call(ld=20) == shape  # not a multiple of 8
    assert call(ld=8) == shape  # ld < h
    assert call(h=12, ld=16) == shape and call(B=0) == shape
    assert call(acts=None) == null
    assert call(idx=p) == null  # the pairs' two outputs go together
    assert call(dtype=7) == dtype
    assert call(h=1 << 18, ld=1 << 18) == 5  # CC_ERR_TOO_LARGE: h beyond 2^17


def cfg_for(**kw):
    cfg = {"seed": 49, "batch_size": 64, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 6400, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": 256, "seq_len": 1024, "enc_dtype": "bf16", "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": 32, "log_every": 100, "save_every": 30000}
    cfg.update(kw)
    return cfg


def test_cfg_validation():
    assert activation_of(cfg_for()) == ("relu", None)  # the keys absent: the reference's ReLU
    assert activation_of(cfg_for(activation="relu", k=5)) == ("relu", None)
    assert activation_of(cfg_for(activation="topk", k=1)) == ("topk", 1)
    assert activation_of(cfg_for(activation="topk", k=256)) == ("topk", 256)
    for bad in (dict(activation="batchtopk", k=4), dict(activation="topk"), dict(activation="topk", k=0),
                dict(activation="topk", k=257), dict(activation="topk", k=4.0), dict(activation="topk", k=True)):
        with pytest.raises(ValueError):
            activation_of(cfg_for(**bad))
        with pytest.raises(ValueError):  # at construction, before anything touches the device
            ca.CrossCoder(cfg_for(**bad))


def test_sharded_trainer_refuses_topk():
    with pytest.raises(ValueError, match="topk"):
        sharded.ShardedTrainer(cfg_for(activation="topk", k=8), buffer=None)
