#!/usr/bin/env python3
"""Times Trainer.step of a TopK crosscoder with the AuxK dead-latent loss under the sparse step (cfg["auxk_compact"],
DESIGN.md section 3.22), bf16, l1_coeff 0, k = 32, at config 2's shape (B 4096, 2 x 2304 -> 16384) and config 3's
(-> 2^17).  Three arms in one process, single steps alternating:
  (a) the sparse step without the aux keys
  (b) the sparse step with the aux loss on the compacted dead set
  (c) the dense TopK + AuxK step
Two dead sets: about 5 % dead, made as section 3.11 made it (every 20th latent's encoder row scaled by 1/64 in all three
arms, dead_tokens = batch: those latents are positive yet never in a row's top k, so they are dead from the second step
on), and nothing dead (the same trainers with dead_tokens raised to 10^12 and tokens_since_fired zeroed).  After
`--warmup` steps each, `--steps` rounds of one step per arm, each timed on the host clock from the call to a device
synchronise; medians, min, max.  Then arm (b) alone under engine.TIMER: device events around every launch, medians over
the same number of steps; the column gather is set against its bytes model at 4 TB/s.  `--granules` repeats arm (b)
with engine.AUX_GRANULE set to each value (the A/B of the compact extent's padding).

    python tools/sparse_auxk_time.py [--out profiles/sparse_auxk_time.txt]
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
FLOOR_TBS = 4.0
LINE_BYTES = 128


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
    d = tr.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, d


def trainer(B, n, d, h, k, arm, dev):
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 0.0,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000, "activation": "topk", "k": k}
    if arm in "ab":
        cfg["sparse_step"] = True
    if arm in "bc":
        cfg.update(auxk_coeff=1.0 / 32, dead_tokens=B)
    if arm == "b":
        cfg["auxk_compact"] = True
    cc = ca.CrossCoder(cfg, n_models=n)
    with torch.no_grad():
        cc.W_enc[:, :, ::20] *= 1.0 / 64
    return ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=4 * B, n_models=n, seed=0), crosscoder=cc)


def nothing_dead(tr):
    """the same trainer with dead_tokens out of reach: its steps issue no aux launch from here on"""
    if tr.auxk is not None:
        tr.synchronize()
        tr.auxk = (tr.auxk[0], tr.auxk[1], 10 ** 12)
        tr.tokens_since_fired = torch.zeros_like(tr.tokens_since_fired)


def rounds(arms, warmup, steps):
    for _ in range(warmup):
        for tr in arms.values():
            tr.step()
    torch.cuda.synchronize()
    t, last = {name: [] for name in arms}, {}
    for _ in range(steps):
        for name, tr in arms.items():
            ms, last[name] = timed_step(tr)
            t[name].append(ms)
    return t, last


def report(t, last):
    med = {}
    for name, v in t.items():
        med[name] = statistics.median(v)
        dead = last[name].get("dead_latents")
        say(f"  ({name}) median {med[name]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}"
            + ("" if dead is None else f"   dead_latents {dead}  auxk_loss {last[name]['auxk_loss']:.4g}"))
    return med


def spans(tr, steps):
    timer = SpanTimer()
    engine.TIMER = timer
    per = {}
    try:
        for _ in range(steps):
            tr.step()
            for name, ms in timer.drain():
                per.setdefault(name, []).append(ms)
    finally:
        engine.TIMER = None
    return {name: statistics.median(v) for name, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--granules", type=int, nargs="*", default=[8, 256])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sparse_auxk_time: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    say(f"sparse_auxk_time: {torch.cuda.get_device_name(0)}; TopK Trainer.step, bf16, l1_coeff 0, k {a.k}; medians of "
        f"{a.steps} steps after {a.warmup} warm-up steps, arms alternating; host clock to a device synchronise; "
        f"AUX_GRANULE {engine.AUX_GRANULE}")
    for label in a.shapes:
        B, n, d, h = SHAPES[label]
        arms = {arm: trainer(B, n, d, h, a.k, arm, dev) for arm in "abc"}
        say(f"{label}, B {B}, {n} x {d} -> {h}, k {a.k}, k_aux {arms['b'].auxk[1]}:")
        say(" about 5 % dead (every 20th encoder row / 64, dead_tokens = batch):")
        t, last = rounds(arms, a.warmup, a.steps)
        med = report(t, last)
        say(f"  (b) - (a) = {med['b'] - med['a']:+.3f} ms   (c) - (b) = {med['c'] - med['b']:+.3f} ms   "
            f"(b) / (c) = {med['b'] / med['c']:.3f}")
        ws = arms["b"]._last_ws
        D, Dp = ws.aux_D, ws.aux_Dp
        per = spans(arms["b"], a.steps)
        say(f"  (b) per launch, D {D}, D_pad {Dp}, capacity {ws.aux_cap} (device events, median ms): "
            + ", ".join(f"{name} {ms:.3f}" for name, ms in per.items()))
        # the column gather's bytes: every cache line of G1's activations that holds a dead latent's element is read
        # once -- at most one line per element, at most the whole matrix -- and the compact matrix is written
        read = min(B * D * LINE_BYTES, B * h * 2)
        nbytes = read + B * Dp * 2
        floor = nbytes / (FLOOR_TBS * 1e9)
        say(f"  compact_cols: model {nbytes / 1e6:.1f} MB (read {read / 1e6:.1f}, write {B * Dp * 2 / 1e6:.1f}), floor "
            f"{floor:.4f} ms at {FLOOR_TBS} TB/s; measured {per['compact_cols']:.4f} ms = "
            f"{per['compact_cols'] / floor:.2f} x floor, {nbytes / per['compact_cols'] / 1e6:.0f} GB/s")
        for g in a.granules:
            if g == engine.AUX_GRANULE:
                continue
            keep = engine.AUX_GRANULE
            engine.AUX_GRANULE = g
            try:
                tb, lb = rounds({"b": arms["b"], "a": arms["a"]}, 2, a.steps)
            finally:
                engine.AUX_GRANULE = keep
            say(f"  granule {g} (D_pad {arms['b']._last_ws.aux_Dp}): (b) median {statistics.median(tb['b']):8.3f} ms  "
                f"min {min(tb['b']):8.3f}  max {max(tb['b']):8.3f};  (a) in the same rounds {statistics.median(tb['a']):8.3f}")
        say(" nothing dead (dead_tokens 10^12, tokens_since_fired zeroed):")
        for tr in arms.values():
            nothing_dead(tr)
        t, last = rounds(arms, 2, a.steps)
        med = report(t, last)
        spread = max(t["a"]) - min(t["a"])
        per = spans(arms["b"], a.steps)
        say(f"  (b) - (a) = {med['b'] - med['a']:+.3f} ms; (a)'s own min-max spread {spread:.3f} ms; dead_update "
            f"{per.get('dead_update', float('nan')):.4f} ms; launches of (b): {', '.join(per)}")
        del arms
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
