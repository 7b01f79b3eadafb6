#!/usr/bin/env python3
"""Times latent scaling's fused GEMM (cc_latent_scaling) at config 2's shape (B 4096, d 2304, h 16384, bf16)
against what it replaces and against the floor its main loop sets:

  (a) one cc_latent_scaling launch (one model's slice of [B, n d] operands, the acts^2 sums on)
  (b) the unfused form: cc_gemm_f32out of the same operands into P [B, h] fp32, then torch's
      (acts.float() * P).sum(0)
  (c) cc_gemm_f32out alone
  (d) a whole LatentScaling.update of one B-row batch (encode, activation, decode, E, 2 n launches, reductions)

Each figure: `--warmup` calls, then `--rounds` windows of `--launches` calls between one pair of device events
(ms per call = window / launches; median and spread over the windows).  The arms alternate within a round.  Peak
extra memory: torch's allocator high-water mark over one call, above what was allocated before it (operands
excluded, the call's outputs and temporaries included).  The shader clock is read once (rocm-smi) while a burst of
(a) is queued.

    python tools/latent_scaling_time.py [--out profiles/latent_scaling_time.txt]
"""
import argparse
import ctypes
import os
import re
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402
from crosscoder_amd import _lib, ops  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


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


def sclk_mhz():
    try:
        s = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        c = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", s)
        return int(c.group(1)) if c else None
    except (OSError, subprocess.SubprocessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--dict-size", type=int, default=16384)
    ap.add_argument("--d-in", type=int, default=2304)
    ap.add_argument("--n-models", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("latent_scaling_time: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, h, d, n, m = a.rows, a.dict_size, a.d_in, a.n_models, a.n_models - 1
    dt = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    Y = torch.randn(B, n * d, device=dev, generator=g).to(dt)
    W = (0.02 * torch.randn(h, n * d, device=dev, generator=g)).to(dt)
    acts = torch.where(torch.rand(B, h, device=dev, generator=g) < 0.1,
                       torch.rand(B, h, device=dev, generator=g), torch.zeros((), device=dev)).to(dt)
    Ym, Wm = Y[:, m * d:(m + 1) * d], W[:, m * d:(m + 1) * d]
    R = ops.col_part_rows(B)
    dot_part = torch.empty(R, h, dtype=torch.float32, device=dev)
    sq_part = torch.empty(R, h, dtype=torch.float32, device=dev)
    S, Q = (torch.empty(h, dtype=torch.float32, device=dev) for _ in range(2))
    P = torch.empty(B, h, dtype=torch.float32, device=dev)
    lib = ops.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fused():
        ops.latent_scaling(Ym, Wm, acts, dot_part, sq_part)

    def gemm(out=P):
        ops.check(lib.cc_gemm_f32out(ptr(Ym), _lib.CC_LAYOUT_KC, n * d, ptr(Wm), _lib.CC_LAYOUT_KC, n * d, ptr(out), h,
                                     B, h, d, _lib.CC_BF16, stream()))

    def unfused():
        gemm()
        return (acts.float() * P).sum(0)

    say(f"latent_scaling_time: {torch.cuda.get_device_name(0)}; Y {B} x {d} (pitch {n * d}), W {h} x {d}, acts "
        f"{B} x {h}, bf16; {a.rounds} windows of {a.launches} calls per figure, {a.warmup} warm-up calls")

    # the two forms agree (fp32 reassociation) before anything is timed
    fused()
    ops.reduce_rows(dot_part, R, h, out_f32=S)
    ref = unfused().double()
    scale = (acts.double().abs() * (Ym.double().abs() @ Wm.double().abs().t())).sum(0)
    say(f"  fused vs unfused column sums: max |diff| / sum of magnitudes = "
        f"{((S.double() - ref).abs() / scale.clamp(min=1e-300)).max().item():.2e}")
    del ref, scale

    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    cc = ca.CrossCoder(cfg, n_models=n)
    x = torch.randn(B, n, d, device=dev, generator=g).to(dt)
    ls = ca.LatentScaling(cc, chunk_rows=B)
    arms = [("(a) cc_latent_scaling", fused, a.launches),
            ("(b) gemm_f32out + torch", unfused, a.launches),
            ("(c) gemm_f32out alone", gemm, a.launches),
            ("(d) LatentScaling.update", lambda: ls.update(x), max(1, a.launches // 4))]
    with torch.no_grad():
        for _, fn, _ in arms:
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in arms}
        for _ in range(a.rounds):
            for name, fn, launches in arms:
                ms[name].append(window(fn, launches))
        med = {}
        for name, _, launches in arms:
            v = ms[name]
            med[name] = statistics.median(v)
            say(f"  {name:<26} median {med[name]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  "
                f"({launches} calls per window)")
        flops = 2.0 * B * h * d
        ka, kb, kc, kd = (med[name] for name, _, _ in arms)
        say(f"  (a) {flops / ka / 1e9:7.1f} TFLOP/s, (c) {flops / kc / 1e9:7.1f} TFLOP/s;  (a) / (c) = {ka / kc:.3f}, "
            f"(a) / (b) = {ka / kb:.3f};  the epilogue costs {ka - kc:+.3f} ms over the plain fp32 store")
        say(f"  (d) per row: {kd / B * 1e3:.3f} us; its {2 * n} launches at (a)'s time: {2 * n * ka:.3f} ms")

        def fused_fresh():
            p = torch.empty(2, R, h, dtype=torch.float32, device=dev)
            ops.latent_scaling(Ym, Wm, acts, p[0], p[1])
            return p

        def unfused_fresh():
            p = torch.empty(B, h, dtype=torch.float32, device=dev)
            gemm(p)
            return (acts.float() * p).sum(0)

        say(f"  peak extra memory: (a) {peak_extra(fused_fresh) / 2**20:8.1f} MiB (the two slabs), "
            f"(b) {peak_extra(unfused_fresh) / 2**20:8.1f} MiB (P, acts.float() and their product)")
        for _ in range(40 * a.launches):  # a queued burst of (a) for the clock to be read under load
            fused()
        clk = sclk_mhz()
        torch.cuda.synchronize()
        say(f"  shader clock while a burst of (a) was queued: {clk if clk is not None else 'not read'} MHz")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
