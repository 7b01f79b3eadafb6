#!/usr/bin/env python3
"""Times the per-row top-k kernel (cc_topk_rows) at config 2's activation shape (4096 x 16384 bf16), k in
{32, 128}, against the torch composition that yields the same dense output, and the cost of the TopK step.

Two inputs: the seed-49 initialisation (about half of the activations positive) and a "trained-like" set
(b_enc shifted so that 1-2 % fire).  Per input and k:
  in place  the step's launch: the mask written over the activations, column-sum partials and counts
  pairs     encode_topk's launch: only the k (latent, value) pairs per row
  torch     torch.topk on the fp32 copy of the same tensor, then a scatter into zeros (the same dense output
            wherever no tie straddles position k; the count of rows where it differs is printed)
Times are hip events around each launch (median of `--launches`); GB/s counts one read and one write of the
activations (2 * B * h * 2 bytes) for the dense forms.  The step A/B alternates single Trainer.step calls of three
trainers -- ReLU, ReLU forced to the batch-major step form, TopK (batch-major) -- each timed on the host clock up
to a device synchronise.

    python tools/topk_bench.py [--out profiles/topk_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402
from crosscoder_amd import engine, ops  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, n):
    """ms per call of fn(), one event pair per call."""
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def report(name, ms, nbytes):
    med = statistics.median(ms)
    say(f"    {name:<9} median {med:8.3f} ms  mean {statistics.fmean(ms):8.3f} ms  min {min(ms):8.3f} ms  "
        f"{nbytes / med / 1e6:8.1f} GB/s (median)")
    return med


def torch_composition(acts, k):
    vals, idx = torch.topk(acts.float(), k, dim=1)
    return torch.zeros_like(acts).scatter_(1, idx, torch.where(vals > 0, vals, torch.zeros_like(vals)).to(acts.dtype))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--dict-size", type=int, default=16384)
    ap.add_argument("--d-in", type=int, default=2304)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20, help="Trainer.step calls per arm of the step A/B (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_bench: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, h, d, L = a.rows, a.dict_size, a.d_in, a.launches
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    nbytes = 2 * B * h * 2
    say(f"topk_bench: {torch.cuda.get_device_name(0)}; acts {B} x {h} bf16 ({B * h * 2 / 1e6:.0f} MB), "
        f"{L} launches per figure")
    cc = ca.CrossCoder(cfg)
    x = ca.SyntheticBuffer(cfg, rows=B, seed=0).next()
    for label in ("seed-49 init", "trained-like"):
        if label == "trained-like":  # shift b_enc to the 98.5 % quantile of a sample of pre-activations
            pre = cc.encode(x[:256], apply_relu=False).float().flatten()
            q = torch.quantile(pre[torch.randperm(pre.numel(), device=dev)[:1 << 22]], 0.985).item()
            with torch.no_grad():
                cc.b_enc.sub_(q)
        acts = cc.encode(x)
        say(f"{label}: {100 * (acts > 0).float().mean().item():.2f} % of the activations positive")
        for k in (32, 128):
            work = torch.empty_like(acts)
            part = torch.empty(ops.topk_part_rows(B, h), h, device=dev)
            l0 = torch.empty(ops.topk_l0_parts(B, h), device=dev)
            idx = torch.empty(B, k, dtype=torch.int32, device=dev)
            val = torch.empty(B, k, dtype=acts.dtype, device=dev)

            def in_place():
                ops.topk_rows(work, h, k, out=work, colsum_part=part, l0_part=l0)

            def pairs():
                ops.topk_rows(acts, h, k, idx_out=idx, val_out=val)

            work.copy_(acts)
            in_place()  # (code object load)
            ref = torch_composition(acts, k)
            differ = int((work != ref).any(1).sum())
            assert int((work > 0).sum(1).max()) <= k and torch.equal((work > 0).sum(1), (ref > 0).sum(1))
            torch.cuda.synchronize()
            say(f"  k = {k}: rows where torch.topk broke a tie at position k differently: {differ} of {B}")
            ms = []
            for _ in range(L):  # the mask is idempotent but a masked row is cheaper to select from: restore it
                work.copy_(acts)
                torch.cuda.synchronize()
                ms += timed(in_place, 1)
            kern = report("in place", ms, nbytes)
            report("pairs", timed(pairs, L), nbytes // 2)
            tor = report("torch", timed(lambda: torch_composition(acts, k), L), nbytes)
            say(f"    kernel / torch: {kern / tor:.3f}")
            del work, ref
    del cc, acts
    if a.steps:
        arms = {}
        real = engine.transposed_wgrad
        for name, kw in (("relu", {}), ("relu bm", {}), ("topk 32", {"activation": "topk", "k": 32})):
            c = ca.CrossCoder(dict(cfg, **kw))
            engine.transposed_wgrad = (lambda *s: False) if name == "relu bm" else real
            tr = ca.Trainer(dict(cfg, **kw), buffer=ca.SyntheticBuffer(cfg, rows=B * 4, seed=0), crosscoder=c)
            tr.step_counter = 10_000  # past the l1 warm-up
            tr.step()  # (allocates the workspace in this arm's step form)
            tr.synchronize()
            say(f"  {name:<8} step form: {'transposed' if c._ws.tr else 'batch-major'}")
            arms[name] = (tr, [])
        engine.transposed_wgrad = real
        for i in range(a.steps + 5):
            for name, (tr, ms) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.step()
                tr.synchronize()
                torch.cuda.synchronize()
                if i >= 5:
                    ms.append(1e3 * (time.perf_counter() - t0))
        say(f"Trainer.step at config 2, {a.steps} steps per arm, alternating (host clock to a device synchronise):")
        med = {}
        for name, (tr, ms) in arms.items():
            med[name] = statistics.median(ms)
            say(f"  {name:<8} median {med[name]:8.3f} ms  mean {statistics.fmean(ms):8.3f} ms  "
                f"min {min(ms):8.3f} ms  max {max(ms):8.3f} ms")
        say(f"  topk over the batch-major relu step (medians): {med['topk 32'] - med['relu bm']:+.3f} ms; "
            f"batch-major over transposed relu: {med['relu bm'] - med['relu']:+.3f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
