"""BatchTopK crosscoders, the parts that need no GPU: the selection reference itself, the C ABI's declarations and
argument checks, the cfg keys, the sharded trainer's refusal and the unchanged ReLU state dict."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, sharded
from crosscoder_amd.crosscoder import activation_of, batch_topk_options
from tests._batch_topk_ref import batch_topk_brute, batch_topk_key, batch_topk_order, batch_topk_ref, threshold_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cc_batch_topk", "cc_threshold_mask", "cc_batch_topk_part_rows", "cc_batch_topk_l0_parts",
                "cc_batch_topk_ws_bytes")

# ties across the row boundary (3.0: row 0 columns 1 and 7, row 1 columns 0 and 1); a = 2 under w = 1 against a = 1 under
# w = 2 (columns 2 and 3); 2^-100 under 2^-60, a product that underflows to 0 (column 4); ineligible values
ROWS = [[1.0, 3, 2, 1, 2.0 ** -100, 0, -1, 3],
        [3.0, 3, 2, 1, 0.5, float("nan"), -0.0, 0.25],
        [0.0] * 8,
        [0.5, 0.5, 1, 2, 2.0 ** -100, float("inf"), 0.5, 0.5]]
WEIGHT = [1.0, 1, 1, 2, 2.0 ** -60, 1, 1, 1]


def test_stable_descending_sort_orders_ties_by_flat_index():
    v = torch.tensor([[1.0, 3, 0, 3], [3.0, 2, 3, 0]])
    assert batch_topk_order(v)[1].tolist()[:6] == [1, 3, 4, 6, 5, 0]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_matches_brute_force(dtype, weighted):
    g = torch.Generator().manual_seed(0)
    rows = ROWS + (torch.randint(-2, 4, (12, 8), generator=g).float() / 2).tolist()  # few distinct values: ties
    v = torch.tensor(rows).to(dtype)
    w = torch.tensor(WEIGHT) if weighted else None
    B, h = v.shape
    key = batch_topk_key(v, w)
    if weighted:
        assert key[0, 2] == key[0, 3] == 2.0 and key[0, 4] == 0 and key[3, 4] == 0  # the cross-value tie, the underflow
    assert key[0, 7] == key[1, 0] == key[1, 1]  # the tie across the row boundary
    order = batch_topk_order(v, w)
    eligible = int((key > 0).sum())
    straddled = 0
    for n_keep in list(range(1, 40)) + [eligible, eligible + 1, B * h]:
        ref = batch_topk_ref(v, n_keep, w, order)
        want = batch_topk_brute(v.float().tolist(), n_keep, WEIGHT if weighted else None)
        assert ref["mask"].flatten().nonzero().flatten().tolist() == want, n_keep
        assert ref["selected"] == len(want) == min(n_keep, eligible) and ref["eligible"] == eligible
        assert ref["row_count"].tolist() == [sum(1 for i in want if i // h == b) for b in range(B)]
        scores = [key.flatten()[i].item() for i in want]
        assert ref["T"].item() == (min(scores) if want else 0.0)
        assert ref["ties"] == sum(1 for s in scores if s == ref["T"].item())
        assert ref["ties_total"] == int((key == ref["T"]).sum()) or not want
        straddled += ref["ties"] < ref["ties_total"]
        dense = ref["dense"].float()
        assert torch.equal(dense[ref["mask"]], v.float()[ref["mask"]]) and bool((dense[~ref["mask"]] == 0).all())
        assert not bool(torch.signbit(dense[~ref["mask"]]).any())  # the rest is +0
        assert ref["row_count"][2].item() == 0  # the all-zero row
        th = threshold_ref(v, ref["T"], w)
        if want and ref["ties"] == ref["ties_total"]:
            assert torch.equal(th["mask"], ref["mask"])  # every tie at T admitted: score >= T is the selection
    assert straddled > 5  # cuts inside tie runs were exercised
    # 3.0 sits at flat indices 1, 7, 8 and 9: the earlier row first, then the smaller latent
    if not weighted:
        inf_first = batch_topk_ref(v, 1, w, order)["mask"].flatten().nonzero().flatten().tolist()
        assert inf_first == [3 * 8 + 5]  # +inf is eligible and the largest
        assert batch_topk_ref(v, 3, w, order)["mask"].flatten().nonzero().flatten().tolist() == [1, 7, 3 * 8 + 5]
        assert batch_topk_ref(v, 4, w, order)["mask"].flatten().nonzero().flatten().tolist() == [1, 7, 8, 3 * 8 + 5]


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
    assert len(_lib.SIGNATURES["cc_topk_rows"][1]) == 12  # the per-row entry keeps its arguments
    for B, h in ((1, 8), (4096, 16384), (2, 131072), (700, 512), (16384, 131072)):
        rows, parts = lib.cc_batch_topk_part_rows(B, h), lib.cc_batch_topk_l0_parts(B, h)
        assert 1 <= rows <= min(B * h // 8, 1024) and 1 <= parts <= min(B * h // 8, 1024)
        for dtype in (_lib.CC_BF16, _lib.CC_F32):
            for weighted in (0, 1):
                assert 16 <= lib.cc_batch_topk_ws_bytes(B, h, dtype, weighted) <= 1 << 22
    assert lib.cc_batch_topk_ws_bytes(4, 12, _lib.CC_F32, 0) == 0 and lib.cc_batch_topk_ws_bytes(4, 16, 7, 0) == 0
    assert lib.cc_batch_topk_part_rows(0, 16) == 0 and lib.cc_batch_topk_l0_parts(16385, 131072) == 0


def test_argument_validation_needs_no_gpu():
    """Shape / NULL / dtype / size / alignment errors are returned before any launch (host pointers are never
    touched), in cc_topk_rows' order."""
    lib = _lib.load()
    buf = torch.zeros(256)
    p = buf.data_ptr()
    assert p % 16 == 0
    shape, null, dtype, align, large = 3, 1, 2, 4, 5  # CC_ERR_SHAPE, _NULL, _DTYPE, _ALIGN, _TOO_LARGE

    def call(acts=p, ld=16, B=4, h=16, dtype=_lib.CC_F32, weight=None, n_keep=4, out=p, part=None, rc=None,
             info=None, ws=p, ws_bytes=1 << 22, l0=None, ema=None, beta=0.5):
        return lib.cc_batch_topk(acts, ld, B, h, dtype, weight, n_keep, out, part, l0, rc, info, ema, beta, ws, ws_bytes,
                                 None)

    def mask(acts=p, ld=16, B=4, h=16, dtype=_lib.CC_F32, weight=None, theta=p, out=p, part=None, rc=None, l0=None):
        return lib.cc_threshold_mask(acts, ld, B, h, dtype, weight, theta, out, part, l0, rc, None)

    for f in (call, mask):
        assert f(ld=17) == shape and f(ld=20) == shape and f(ld=8) == shape  # odd, not a multiple of 8, ld < h
        assert f(h=12, ld=16) == shape and f(B=0) == shape and f(h=0, ld=0) == shape
        assert f(acts=None) == null and f(out=None) == null  # no output at all
        assert f(dtype=7) == dtype
        assert f(h=1 << 18, ld=1 << 18) == large  # h beyond 2^17
        assert f(B=(1 << 27) + 1, h=16) == large  # B h beyond 2^31
        assert f(acts=p + 4) == align and f(out=p + 8) == align and f(weight=p + 4) == align and f(part=p + 4) == align
        assert f(B=0, acts=None, dtype=7) == shape and f(acts=None, dtype=7) == null  # the order of the checks
        assert f(dtype=7, h=1 << 18, ld=1 << 18) == dtype and f(h=1 << 18, ld=1 << 18, acts=p + 4) == large
        assert f(l0=p + 2) == align and f(rc=p + 2) == align  # the 4-byte outputs
    assert call(n_keep=0) == shape and call(n_keep=-3) == shape
    assert call(ema=p, beta=1.0) == shape and call(ema=p, beta=-0.5) == shape and call(ema=p + 2) == align
    # the workspace / the threshold belong to the NULL stage: before dtype, size and alignment
    for f, kw in ((call, dict(ws=None)), (mask, dict(theta=None))):
        assert f(**kw) == null and f(dtype=7, **kw) == null and f(h=1 << 18, ld=1 << 18, **kw) == null
        assert f(acts=p + 4, **kw) == null and f(B=0, **kw) == shape
    assert call(ws=p + 2) == align and mask(theta=p + 2) == align and call(info=p + 2) == align
    assert call(ws_bytes=64) == shape  # last: a workspace below cc_batch_topk_ws_bytes
    assert call(ws=p + 2, ws_bytes=64) == align


def cfg_for(**kw):
    cfg = {"seed": 49, "batch_size": 64, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 6400, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": 256, "seq_len": 1024, "enc_dtype": "bf16", "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": 32, "log_every": 100, "save_every": 30000}
    cfg.update(kw)
    return cfg


def test_cfg_validation():
    assert activation_of(cfg_for(activation="batch_topk", k=1)) == ("batch_topk", 1)
    assert activation_of(cfg_for(activation="batch_topk", k=256)) == ("batch_topk", 256)
    assert batch_topk_options(cfg_for(activation="batch_topk", k=4)) == ("decoder_norm", 0.999)
    assert batch_topk_options(cfg_for(topk_weight="none", threshold_beta=0)) == ("none", 0.0)
    assert activation_of(cfg_for(activation="batch_topk", k=4, topk_weight="none", threshold_beta=0.5))[1] == 4
    assert activation_of(cfg_for(activation="relu", topk_weight="bogus")) == ("relu", None)  # keys of another mode
    for bad in (dict(activation="batchtopk", k=4), dict(activation="batch_topk"), dict(activation="batch_topk", k=0),
                dict(activation="batch_topk", k=257), dict(activation="batch_topk", k=4.0),
                dict(activation="batch_topk", k=True), dict(activation="batch_topk", k=4, topk_weight="l2"),
                dict(activation="batch_topk", k=4, topk_weight=None),
                dict(activation="batch_topk", k=4, threshold_beta=1.0),
                dict(activation="batch_topk", k=4, threshold_beta=-0.1),
                dict(activation="batch_topk", k=4, threshold_beta="0.9"),
                dict(activation="batch_topk", k=4, threshold_beta=True)):
        with pytest.raises(ValueError):
            activation_of(cfg_for(**bad))
        with pytest.raises(ValueError):  # at construction, before anything touches the device
            ca.CrossCoder(cfg_for(**bad))


def test_sharded_trainer_refuses_batch_topk():
    with pytest.raises(ValueError, match="batch_topk"):
        sharded.ShardedTrainer(cfg_for(activation="batch_topk", k=8), buffer=None)


def test_state_dict_keys():
    """The threshold buffer belongs to BatchTopK crosscoders alone: ReLU and TopK keep the reference's four keys."""
    ref_keys = ["W_enc", "W_dec", "b_enc", "b_dec"]
    assert list(ca.CrossCoder(cfg_for(device="cpu")).state_dict().keys()) == ref_keys
    assert list(ca.CrossCoder(cfg_for(device="cpu", activation="topk", k=8)).state_dict().keys()) == ref_keys
    cc = ca.CrossCoder(cfg_for(device="cpu", activation="batch_topk", k=8, topk_weight="none"))
    sd = cc.state_dict()
    assert list(sd.keys()) == ref_keys + ["threshold"]
    assert sd["threshold"].dtype == torch.float32 and sd["threshold"].shape == () and sd["threshold"].item() == -1.0
    assert cc.k == 8 and cc.topk_weight == "none" and cc.threshold_beta == 0.999
    with pytest.raises(ValueError):
        cc.batch_topk_info()  # no forward has run
    # the reference's four tensors load as they are (a ReLU checkpoint to train on); the threshold stays
    relu_sd = ca.CrossCoder(cfg_for(device="cpu", seed=7)).state_dict()
    with torch.no_grad():
        cc.threshold.fill_(0.25)
    cc.load_state_dict(relu_sd)
    assert cc.threshold.item() == 0.25 and torch.equal(cc.W_dec, relu_sd["W_dec"])
    cc.load_state_dict(dict(relu_sd, threshold=torch.tensor(0.5)))
    assert cc.threshold.item() == 0.5
    with pytest.raises(RuntimeError):  # the other way round stays strict
        ca.CrossCoder(cfg_for(device="cpu")).load_state_dict(cc.state_dict())
