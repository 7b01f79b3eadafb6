#!/usr/bin/env python3
"""Times the two JumpReLU kernels (cc_jumprelu_mask, cc_jumprelu_bwd) at config 2's activation shape
(4096 x 16384 bf16) beside cc_threshold_mask, the closest existing kernel (one read, one write, the same side
outputs), and the cost of the JumpReLU step.

Two inputs: the seed-49 initialisation (about half of the activations positive) and a "trained-like" set (b_enc
shifted so that 1-2 % fire).  The thresholds are one value for all latents, the median of the positive activations,
and the bandwidth a quarter of it, so the window is populated.  Per input:
  mask       the step's launch: the mask written over the activations, the gate, column-sum partials and counts
             (1 read + 2 writes of the activations)
  mask enc   encode's launch: the mask in place, no gate, no side outputs (1 read + 1 write)
  bwd        the backward pass: g_pre and the gate read, g_pre rewritten where an element is dropped, the threshold
             gradient's and g_pre's column partial slabs (2 reads + 1 write + 2 slabs)
  thr mask   cc_threshold_mask in place with its side outputs, at the same threshold (1 read + 1 write)
Times are hip events around each launch (median of `--launches`).  Each figure comes with its traffic floor at 4 TB/s
(DESIGN.md section 3.8's rate) and the time as a multiple of that floor.  The step A/B alternates single Trainer.step
calls of four trainers -- ReLU, ReLU forced to the batch-major step form, TopK (k = 32), JumpReLU -- each timed on the
host clock up to a device synchronise.

    python tools/jumprelu_bench.py [--out profiles/jumprelu_bench.txt]
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
FLOOR_RATE = 4.0e12  # bytes / s


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, n, before=None):
    """ms per call of fn(), one event pair per call; before(): restores the inputs, outside the timed span."""
    out = []
    for _ in range(n):
        if before is not None:
            before()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def report(name, ms, nbytes):
    med = statistics.median(ms)
    floor = 1e3 * nbytes / FLOOR_RATE
    say(f"    {name:<9} median {med:8.3f} ms  mean {statistics.fmean(ms):8.3f} ms  min {min(ms):8.3f} ms  "
        f"{nbytes / med / 1e6:8.1f} GB/s  floor {floor:6.3f} ms  x{med / floor:5.2f}")
    return med / floor


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
        sys.exit("jumprelu_bench: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, h, d, L = a.rows, a.dict_size, a.d_in, a.launches
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    ab = B * h * 2  # bytes of the activations
    say(f"jumprelu_bench: {torch.cuda.get_device_name(0)}; acts {B} x {h} bf16 ({ab / 1e6:.0f} MB), "
        f"{L} launches per figure, floors at {FLOOR_RATE / 1e12:.0f} TB/s")
    cc = ca.CrossCoder(cfg)
    x = ca.SyntheticBuffer(cfg, rows=B, seed=0).next()
    rows = ops.jumprelu_part_rows(B, h)
    slab = rows * h * 4
    for label in ("seed-49 init", "trained-like"):
        if label == "trained-like":  # shift b_enc to the 98.5 % quantile of a sample of pre-activations
            pre = cc.encode(x[:256], apply_relu=False).float().flatten()
            q = torch.quantile(pre[torch.randperm(pre.numel(), device=dev)[:1 << 22]], 0.985).item()
            with torch.no_grad():
                cc.b_enc.sub_(q)
        acts = cc.encode(x)
        pos = acts[acts > 0].float()
        t = torch.quantile(pos[torch.randperm(pos.numel(), device=dev)[:1 << 22]], 0.5).item()
        eps = t / 4
        theta = torch.full((h,), t, device=dev)
        work, gate = torch.empty_like(acts), torch.empty_like(acts)
        part, l0 = torch.empty(rows, h, device=dev), torch.empty(ops.jumprelu_l0_parts(B, h), device=dev)
        ops.jumprelu_mask(acts, h, theta, eps, out=work, gate=gate, colsum_part=part, l0_part=l0)
        kept, gated = (work > 0).float().mean().item(), (gate > 0).float().mean().item()
        say(f"{label}: {100 * (acts > 0).float().mean().item():.2f} % of the activations positive; theta {t:.4g}, "
            f"eps {eps:.4g}: {100 * kept:.2f} % kept, {100 * (gated - kept):.2f} % gated below theta")
        restore = lambda: work.copy_(acts)  # noqa: E731

        def mask():
            ops.jumprelu_mask(work, h, theta, eps, out=work, gate=gate, colsum_part=part, l0_part=l0)

        def mask_enc():
            ops.jumprelu_mask(work, h, theta, eps, out=work)

        g0 = torch.where(gate > 0, torch.randn(B, h, device=dev).to(acts.dtype), torch.zeros_like(gate))
        g = torch.empty_like(g0)
        thr, col = torch.empty(rows, h, device=dev), torch.empty(rows, h, device=dev)

        def bwd():
            ops.jumprelu_bwd(g, gate, h, theta, eps, 0.5 / B, gpre_colsum_part=col, thr_part=thr)

        tpart = torch.empty(ops.batch_topk_part_rows(B, h), h, device=dev)
        tl0 = torch.empty(ops.batch_topk_l0_parts(B, h), device=dev)
        th1 = torch.full((1,), t, device=dev)

        def thr_mask():
            ops.threshold_mask(work, h, th1, out=work, colsum_part=tpart, l0_part=tl0)

        x_mask = report("mask", timed(mask, L, restore), 3 * ab + slab)
        report("mask enc", timed(mask_enc, L, restore), 2 * ab)
        x_bwd = report("bwd", timed(bwd, L, lambda: g.copy_(g0)), 3 * ab + 2 * slab)
        x_thr = report("thr mask", timed(thr_mask, L, restore), 2 * ab + tpart.numel() * 4)
        say(f"    multiples of the own floor over cc_threshold_mask's: mask {x_mask / x_thr:.2f}, bwd {x_bwd / x_thr:.2f}")
        del work, gate, g, g0
    del cc, acts
    if a.steps:
        arms = {}
        real = engine.transposed_wgrad
        jr = {"activation": "jumprelu", "l0_coeff": 0.01}
        for name, kw in (("relu", {}), ("relu bm", {}), ("topk 32", {"activation": "topk", "k": 32}), ("jumprelu", jr)):
            c = ca.CrossCoder(dict(cfg, **kw))
            engine.transposed_wgrad = (lambda *s: False) if name == "relu bm" else real
            tr = ca.Trainer(dict(cfg, **kw), buffer=ca.SyntheticBuffer(cfg, rows=B * 4, seed=0), crosscoder=c)
            tr.step_counter = 10_000  # past the warm-up
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
        say(f"  jumprelu over the batch-major relu step (medians): {med['jumprelu'] - med['relu bm']:+.3f} ms; "
            f"over the topk step: {med['jumprelu'] - med['topk 32']:+.3f} ms; "
            f"batch-major over transposed relu: {med['relu bm'] - med['relu']:+.3f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
