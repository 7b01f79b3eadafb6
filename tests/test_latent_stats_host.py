"""LatentStats, the parts that need no GPU: the public name, the C ABI's declarations and the host-side
histograms."""
import os
import re
import shutil
import subprocess

import numpy as np
import torch

import crosscoder_amd as ca
from crosscoder_amd import _lib, latent_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cc_latent_stats_update", "cc_latent_stats_max_k")


def test_public_name():
    assert ca.LatentStats is latent_stats.LatentStats
    for method in ("update", "update_from_acts", "result", "reset"):
        assert callable(getattr(ca.LatentStats, method))


def test_entry_points_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "crosscoder_hip.h")).read()
    lib = _lib.load()
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    exported = {path: {ln.split()[-1] for ln in subprocess.run([nm, "-D", "--defined-only", path], check=True,
                                                                capture_output=True, text=True).stdout.splitlines()
                       if ln.strip()} for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH)}
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        for path, syms in exported.items():  # (exports.map's cc_* pattern lets them through)
            assert name in syms, (name, path)
        assert name in _lib.SIGNATURES
        getattr(lib, name)
    assert lib.cc_latent_stats_max_k() == 16
    assert len(_lib.SIGNATURES["cc_latent_stats_update"][1]) == 14


def test_argument_validation_needs_no_gpu():
    """Shape / dtype / NULL errors are returned before any launch (host pointers are never touched)."""
    lib = _lib.load()
    buf = (torch.zeros(64, dtype=torch.int64), torch.zeros(64))
    p = buf[0].data_ptr()

    def call(acts=p, ld=8, B=4, h=8, dtype=_lib.CC_F32, k=4, count=p):
        return lib.cc_latent_stats_update(acts, ld, B, h, dtype, None, 0, k, count, p, None, p, p, None)

    assert call(k=0) == 3 and call(k=17) == 3 and call(ld=6) == 3 and call(B=0) == 3 and call(ld=9, h=8) == 3
    assert call(acts=None) == 1 and call(count=None) == 1
    assert call(dtype=7) == 2


def test_hist_edges_are_the_powers_of_two():
    e = latent_stats.hist_edges()
    assert e.dtype == torch.float32 and e.shape == (33,)
    assert e.tolist() == [2.0 ** i for i in range(-16, 17)]


def test_log10_frequency_hist_matches_numpy():
    count = torch.tensor([0, 1, 1, 10, 250, 999, 1000, 1000, 0, 37, 500, 3])
    rows = 1000
    hist, edges = latent_stats.log10_frequency_hist(count, rows)
    c = count.numpy().astype(np.float64)
    want, want_edges = np.histogram(np.log10(c[c > 0] / rows), bins=50, range=(-10.0, 0.0))
    assert hist.dtype == torch.int64 and hist.tolist() == want.tolist()
    assert np.allclose(edges.numpy(), want_edges, rtol=0, atol=1e-12)
    assert int(hist.sum()) == int((count > 0).sum())  # (a latent firing on every row lands in the last bin)
    empty, _ = latent_stats.log10_frequency_hist(torch.zeros(5, dtype=torch.int64), 0)
    assert empty.tolist() == [0] * 50
