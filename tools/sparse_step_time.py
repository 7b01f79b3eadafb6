#!/usr/bin/env python3
"""Times Trainer.step of a TopK crosscoder, the dense step against cfg["sparse_step"], bf16,
l1_coeff 0, at config 2's shape (B 4096, 2 x 2304 -> 16384) and config 3's (-> 2^17), k = 32 and k = 128.

Per (shape, k) both trainers live in one process and the arms alternate: after `--warmup` steps each, `--steps` rounds
of one dense step, then one sparse step, each timed on the host clock from the call to a device synchronise (the
step's own host read of the loss scalars included, as in section 3.8); the figure is the median.  Then the sparse arm
alone once more under engine.TIMER: device events around every launch of the step, medians over the same number of
steps (the launches of the side stream -- the loss tail, the decoder-half Adam -- overlap the main stream's, so the
spans do not add up to the step).

    python tools/sparse_step_time.py [--out profiles/sparse_step_time.txt]
"""
import argparse
import contextlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402
from crosscoder_amd import engine  # noqa: E402

LINES = []
SHAPES = {"config 2": (4096, 2, 2304, 16384), "config 3's shape": (4096, 2, 2304, 131072)}


def say(s):
    print(s, flush=True)
    LINES.append(s)


class SpanTimer:
    """engine.TIMER: device events around every launch, on the stream the launch runs on"""

    def __init__(self):
        self.spans = []

    @contextlib.contextmanager
    def span(self, name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        try:
            yield
        finally:
            e1.record()
            self.spans.append((name, e0, e1))

    def drain(self):
        torch.cuda.synchronize()
        out = [(name, e0.elapsed_time(e1)) for name, e0, e1 in self.spans]
        self.spans = []
        return out


def timed_step(tr):
    t0 = time.perf_counter()
    tr.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def trainer(B, n, d, h, k, sparse, dev):
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 0.0,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000, "activation": "topk", "k": k}
    if sparse:
        cfg["sparse_step"] = True
    return ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=4 * B, n_models=n, seed=0),
                      crosscoder=ca.CrossCoder(cfg, n_models=n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sparse_step_time: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    say(f"sparse_step_time: {torch.cuda.get_device_name(0)}; TopK Trainer.step, bf16, l1_coeff 0; medians of {a.steps} "
        f"steps after {a.warmup} warm-up steps, arms alternating; host clock to a device synchronise")
    for label, (B, n, d, h) in SHAPES.items():
        for k in a.ks:
            dense, sparse = trainer(B, n, d, h, k, False, dev), trainer(B, n, d, h, k, True, dev)
            assert sparse.sparse_step and not dense.sparse_step
            for _ in range(a.warmup):
                dense.step()
                sparse.step()
            torch.cuda.synchronize()
            td, ts = [], []
            for _ in range(a.steps):
                td.append(timed_step(dense))
                ts.append(timed_step(sparse))
            md, ms = statistics.median(td), statistics.median(ts)
            say(f"{label}, B {B}, {n} x {d} -> {h}, k {k}:")
            say(f"  dense  step median {md:8.3f} ms  min {min(td):8.3f}  max {max(td):8.3f}")
            say(f"  sparse step median {ms:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}   sparse / dense = {ms / md:.3f}")
            timer = SpanTimer()
            engine.TIMER = timer
            try:
                per = {}
                for _ in range(a.steps):
                    sparse.step()
                    for name, ms_ in timer.drain():
                        per.setdefault(name, []).append(ms_)
            finally:
                engine.TIMER = None
            say("  sparse arm, per launch (device events, median ms): "
                + ", ".join(f"{name} {statistics.median(v):.3f}" for name, v in per.items()))
            del dense, sparse
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
