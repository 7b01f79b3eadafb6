#!/usr/bin/env python3
"""Times the BatchTopK selection (cc_batch_topk, cc_threshold_mask) at config 2's activation shape (4096 x 16384
bf16), k in {32, 128}, against the per-row kernel (cc_topk_rows) and the torch composition on the same box, and the
cost of the BatchTopK step.

Two inputs: the seed-49 initialisation (about half of the activations positive) and a "trained-like" set (b_enc
shifted so that 1-2 % fire).  Per input and k:
  weighted    the step's launches: scored with the decoder norms, the mask written over the activations, column-sum
              partials, counts, row counts and info (3 histogram reads + 1 mask read and write)
  unweighted  the same with the activation itself as the score (2 histogram reads + 1 mask read and write)
  threshold   cc_threshold_mask at the weighted selection's threshold score (1 read and write)
  topk_rows   cc_topk_rows in place with its side outputs (1 read and write)
  torch       the fp32 score, torch.topk of B k out of the flattened tensor, scatter into zeros
Times are hip events around each call (median of `--launches`; a call is several launches for cc_batch_topk).  The
floor is the traffic of the passes built (reads + 1 write of the 134 MB of activations) at 4 TB/s.  The step A/B
alternates single Trainer.step calls of three trainers -- ReLU forced to the batch-major step form, TopK, BatchTopK
(weighted) -- each timed on the host clock up to a device synchronise.

    python tools/batch_topk_bench.py [--out profiles/batch_topk_bench.txt]
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
HBM = 4.0e12  # bytes / s, the rate DESIGN.md section 3.8 holds its kernel against


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def report(name, ms, passes, nbytes, tor=None):
    med = statistics.median(ms)
    floor = passes * nbytes / HBM * 1e3
    say(f"    {name:<10} median {med:8.3f} ms  mean {statistics.fmean(ms):8.3f} ms  min {min(ms):8.3f} ms  "
        f"floor ({passes} passes) {floor:6.3f} ms  x{med / floor:5.2f} of it"
        + (f"  {med / tor:7.4f} of torch" if tor else ""))
    return med


def torch_composition(acts, w, n_keep):
    score = acts.float() * w[None, :]
    vals, idx = torch.topk(score.flatten(), n_keep)
    keep = torch.zeros(acts.numel(), dtype=torch.bool, device=acts.device)
    keep[idx[vals > 0]] = True
    return torch.where(keep.view_as(acts), acts, torch.zeros((), dtype=acts.dtype, device=acts.device))


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
        sys.exit("batch_topk_bench: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, h, d, L = a.rows, a.dict_size, a.d_in, a.launches
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    nbytes = B * h * 2
    say(f"batch_topk_bench: {torch.cuda.get_device_name(0)}; acts {B} x {h} bf16 ({nbytes / 1e6:.0f} MB), "
        f"{L} calls per figure; floor at {HBM / 1e12:.0f} TB/s")
    cc = ca.CrossCoder(cfg)
    x = ca.SyntheticBuffer(cfg, rows=B, seed=0).next()
    w = ops.dec_norms(cc.arena().W_dec_hk, h, cc.n_models, d)[1]
    for label in ("seed-49 init", "trained-like"):
        if label == "trained-like":  # shift b_enc to the 98.5 % quantile of a sample of pre-activations
            pre = cc.encode(x[:256], apply_relu=False).float().flatten()
            q = torch.quantile(pre[torch.randperm(pre.numel(), device=dev)[:1 << 22]], 0.985).item()
            with torch.no_grad():
                cc.b_enc.sub_(q)
        acts = cc.encode(x)
        say(f"{label}: {100 * (acts > 0).float().mean().item():.2f} % of the activations positive")
        for k in (32, 128):
            n_keep = B * k
            work = torch.empty_like(acts)
            part = torch.empty(ops.batch_topk_part_rows(B, h), h, device=dev)
            l0 = torch.empty(ops.batch_topk_l0_parts(B, h), device=dev)
            rc = torch.empty(B, dtype=torch.int32, device=dev)
            info = torch.zeros(4, dtype=torch.int32, device=dev)
            ws = torch.empty(ops.batch_topk_ws_bytes(B, h, acts.dtype, True), dtype=torch.uint8, device=dev)
            tpart = torch.empty(ops.topk_part_rows(B, h), h, device=dev)
            tl0 = torch.empty(ops.topk_l0_parts(B, h), device=dev)
            theta = torch.zeros(1, device=dev)

            def batch(weight):
                return lambda: ops.batch_topk(work, h, n_keep, weight=weight, out=work, colsum_part=part, l0_part=l0,
                                              row_count=rc, info=info, ws=ws)

            arms = (("weighted", batch(w), 4), ("unweighted", batch(None), 3),
                    ("threshold", lambda: ops.threshold_mask(work, h, theta, weight=w, out=work, colsum_part=part,
                                                             l0_part=l0, row_count=rc), 2),
                    ("topk_rows", lambda: ops.topk_rows(work, h, k, out=work, colsum_part=tpart, l0_part=tl0), 2))
            work.copy_(acts)
            arms[0][1]()  # (code object load)
            ref = torch_composition(acts, w, n_keep)
            torch.cuda.synchronize()
            i4 = info.tolist()
            theta.copy_(info[0:1].view(torch.float32))
            say(f"  k = {k}: selected {i4[1]} of {i4[3]} eligible, threshold score {theta.item():.6g}, "
                f"{i4[2]} ties admitted; elements where the torch composition differs: {int((work != ref).sum())}; "
                f"rows' counts {int(rc.min())}..{int(rc.max())}")
            del ref
            tor = statistics.median([timed(lambda: torch_composition(acts, w, n_keep)) for _ in range(L)])
            say(f"    torch      median {tor:8.3f} ms")
            for name, fn, passes in arms:
                ms = []
                for _ in range(L):  # (a masked tensor is cheaper to select from: restore it)
                    work.copy_(acts)
                    torch.cuda.synchronize()
                    ms.append(timed(fn))
                report(name, ms, passes, nbytes, tor)
            del work
    del cc, acts
    if a.steps:
        arms = {}
        real = engine.transposed_wgrad
        for name, kw in (("relu bm", {}), ("topk 32", {"activation": "topk", "k": 32}),
                         ("batch 32", {"activation": "batch_topk", "k": 32})):
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
        say(f"  batch_topk over the batch-major relu step (medians): {med['batch 32'] - med['relu bm']:+.3f} ms; "
            f"over the topk step: {med['batch 32'] - med['topk 32']:+.3f} ms; "
            f"topk over the batch-major relu step: {med['topk 32'] - med['relu bm']:+.3f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
