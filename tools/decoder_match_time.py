#!/usr/bin/env python3
"""Times decoder matching (crosscoder_amd.match_decoders' one direction) against a chunked torch baseline, on two
random bf16 decoders of h latents and n * d = 4608 columns, matched over the concatenated vectors (K = 4608), at
h = 16384 (config 2) and h = 2^17 (config 3):

  (a) one direction as match_decoders runs it: the inverse norms of both decoders (cc_dec_norms), then per chunk of
      `--chunk-rows` candidates one cc_decoder_match launch into the reused key slab and one cc_match_reduce, then
      the key decoding
  (b) the launches of (a) alone (norms and decoding left out)
  (c) the torch baseline: normalised copies of both decoders, then per chunk `A_chunk @ B.T` (bf16 in, bf16 out, as
      torch.matmul gives it), `max(0)`, and the merge with the running best

Each figure: one warm-up call, then the median of `--reps` calls, each between its own pair of device events.  Peak
extra memory: torch's allocator high-water mark over one call above what was allocated before it.  The two forms
are compared before anything is timed (the baseline's cosines are rounded to bf16, so equal-looking neighbours may
swap).

    python tools/decoder_match_time.py [--out profiles/decoder_match_time.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from crosscoder_amd import decoder_match, ops  # noqa: E402

LINES = []


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


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def measure(h, n, d, chunk, reps, dev):
    g = torch.Generator(device=dev).manual_seed(h)
    K = n * d
    A = (0.02 * torch.randn(h, K, device=dev, generator=g)).to(torch.bfloat16)  # queries
    B = (0.02 * torch.randn(h, K, device=dev, generator=g)).to(torch.bfloat16)  # candidates
    B[: h // 2] = (A[torch.randperm(h, device=dev, generator=g)[: h // 2]].float()
                   * (1 + 0.3 * torch.randn(h // 2, K, device=dev, generator=g))).to(torch.bfloat16)
    R = ops.col_part_rows(min(chunk, h))
    slab = torch.empty(R, h, dtype=torch.int64, device=dev)

    def launches(sa, sb):
        return decoder_match.match_keys(B, sb, A, sa, chunk, slab=slab)

    def fused():
        sa, sb = (decoder_match.inverse_norms(W, n, d) for W in (A, B))
        return decoder_match.decode_keys(launches(sa, sb), sa)

    def baseline():
        An = (A.float() / A.float().norm(dim=1, keepdim=True)).to(torch.bfloat16)
        Bn = (B.float() / B.float().norm(dim=1, keepdim=True)).to(torch.bfloat16)
        best = torch.full((h,), -float("inf"), dtype=torch.bfloat16, device=dev)
        index = torch.full((h,), -1, dtype=torch.int64, device=dev)
        for r0 in range(0, h, chunk):
            v, i = (Bn[r0:r0 + chunk] @ An.t()).max(0)
            better = v > best
            best = torch.where(better, v, best)
            index = torch.where(better, i + r0, index)
        return index, best

    say(f"h {h} x {h} x K {K} bf16, chunk_rows {chunk}: key slab {R} x {h} x 8 B = {R * h * 8 / 2**20:.1f} MiB")
    index, cosine = fused()
    bi, bc = baseline()
    same = (index == bi).float().mean().item()
    say(f"  fused vs baseline: {100 * same:.2f} % of the indices equal, max |cosine diff| = "
        f"{(cosine - bc.float()).abs().max().item():.2e} (the baseline's cosines are bf16), "
        f"mean best cosine {cosine.double().mean().item():.4f}")
    sa, sb = (decoder_match.inverse_norms(W, n, d) for W in (A, B))
    arms = [("(a) one direction", fused), ("(b) its launches alone", lambda: launches(sa, sb)),
            ("(c) chunked torch baseline", baseline)]
    med = {}
    for name, fn in arms:
        fn()
        torch.cuda.synchronize()
        ms = [timed(fn) for _ in range(reps)]
        med[name] = statistics.median(ms)
        say(f"  {name:<28} median {med[name]:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({reps} calls)")
    flops = 2.0 * h * h * K
    a, b, c = (med[name] for name, _ in arms)
    say(f"  (b) {flops / b / 1e9:7.1f} TFLOP/s, (c) {flops / c / 1e9:7.1f} TFLOP/s;  (a) / (c) = {a / c:.3f}")
    pa, pc = peak_extra(fused), peak_extra(baseline)
    say(f"  peak extra memory: (a) {pa / 2**20:9.1f} MiB beside the {R * h * 8 / 2**20:.1f} MiB slab, "
        f"(c) {pc / 2**20:9.1f} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dict-sizes", type=int, nargs="+", default=[16384, 2 ** 17])
    ap.add_argument("--d-in", type=int, default=2304)
    ap.add_argument("--n-models", type=int, default=2)
    ap.add_argument("--chunk-rows", type=int, default=decoder_match.CHUNK_ROWS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decoder_match_time: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    say(f"decoder_match_time: {torch.cuda.get_device_name(0)}; median of {a.reps} calls after one warm-up call")
    with torch.no_grad():
        for h in a.dict_sizes:
            measure(h, a.n_models, a.d_in, a.chunk_rows, a.reps, dev)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
