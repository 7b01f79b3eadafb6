#!/usr/bin/env python3
"""Times the master-weight Adam (cc_adam_master_step, cfg["master_weights"]) against the default bf16 update at
config 2's shape (B 4096, 2 x 2304 -> 16384, bf16; the arena is 151 M elements), on the operands a few training steps
leave behind:

  (a) the encoder-half launch, default mode: cc_adam_step over bf16 p / g / m / v (one pass)
  (b) the encoder-half launch, master mode: cc_adam_master_step over fp32 p32 / m32 / v32, bf16 g and p16
  (c) the decoder-half launch alone, default: cc_adam_dec_norms, capped to engine.DEC_ADAM_BLOCKS workgroups
  (d) the decoder-half launch alone, master: cc_adam_master_step, capped the same (the launch only, no norms pass)
  (e) G1 (cc_encode_fwd_t) alone
  (f) G1 with (c) on a second stream, started together: the pair's time
  (g) G1 with (d) on a second stream
  (h) Trainer.step, default mode      (i) Trainer.step, master mode
  (j) what the master step runs for its Adam: cc_adam_master_step over the whole arena, then the decoder norms
      (/ W_dec^T) pass over the bf16 W_dec, on one stream

(d) and (g) time the capped form beside G1, an arrangement the step does not use: they say
what the side stream would cost, not what Trainer.step does.

Each figure: `--warmup` calls, then `--rounds` windows of `--launches` calls between one pair of device events (ms per
call = window / launches; median and spread over the windows).  The arms alternate within a round.  The shader clock
is read once (rocm-smi) while a burst of (b) is queued.

    python tools/master_adam_time.py [--out profiles/master_adam_time.txt]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402
from crosscoder_amd import engine, ops  # noqa: E402

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


def sclk_mhz():
    try:
        s = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        c = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", s)
        return int(c.group(1)) if c else None
    except (OSError, subprocess.SubprocessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dict-size", type=int, default=16384)
    ap.add_argument("--d-in", type=int, default=2304)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("master_adam_time: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, h, d, n = a.batch, a.dict_size, a.d_in, 2
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    trs = {}
    for mode in ("default", "master"):
        c = dict(cfg, master_weights=(mode == "master"))
        tr = ca.Trainer(c, buffer=ca.SyntheticBuffer(c, rows=4 * B, seed=0), crosscoder=ca.CrossCoder(c))
        for _ in range(3):
            tr.step()
        tr.synchronize()
        trs[mode] = tr
    torch.cuda.synchronize()
    td, tm = trs["default"], trs["master"]
    od, om = td.optimizer, tm.optimizer
    Pd, Pm = td.crosscoder.arena(), tm.crosscoder.arena()
    K = n * d
    numel = Pd.numel
    say(f"master_adam_time: {torch.cuda.get_device_name(0)}; B {B}, {n} x {d} -> {h}, bf16; arena {numel} elements "
        f"(encoder half {Pd.split}); {a.rounds} windows of {a.launches} calls per figure, {a.warmup} warm-up calls")
    say(f"  bytes per step from the operand sizes: default {numel * 14 / 1e9:.2f} GB (2-byte p, g, m, v read; p, m, v "
        f"written), master {numel * 28 / 1e9:.2f} GB (g 2 B and p32, m32, v32 4 B read; 3 x 4 B and p16 written)")
    hp = (5e-5, 0.9, 0.999, 1e-8, 4)
    coef = torch.ones(1, dtype=torch.float32, device=dev)
    part = torch.empty(int(ops.lib().cc_dec_norms_part_floats(h, n, d)), dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    ws = td.crosscoder._ws
    blocks = engine.DEC_ADAM_BLOCKS

    # the isolated launches update copies of the trainers' arenas (the trainers' own state stays a training run's)
    sp = Pd.split
    dp, dg, dm, dv = (t.data.clone() for t in (Pd, od.grads, od.exp_avg, od.exp_avg_sq))
    mp, mg, mm, mv, m16 = (t.data.clone() for t in (om.master, om.grads, om.exp_avg, om.exp_avg_sq, Pm))

    def enc_default():
        ops.adam_step(dp[:sp], dg[:sp], dm[:sp], dv[:sp], coef, *hp)

    def enc_master():
        ops.adam_master_step(mp[:sp], mg[:sp], mm[:sp], mv[:sp], m16[:sp], coef, *hp)

    def dec_default():
        ops.adam_dec_norms(dp[sp:], dg[sp:], dm[sp:], dv[sp:], h, K, *hp, part, coef=coef, max_blocks=blocks)

    def dec_master():
        ops.adam_master_step(mp[sp:], mg[sp:], mm[sp:], mv[sp:], m16[sp:], coef, *hp, max_blocks=blocks)

    wsm = tm.crosscoder._ws

    def whole_master():
        ops.adam_master_step(mp, mg, mm, mv, m16, coef, *hp)
        engine._decoder_derived(wsm, Pm)  # (reads the trainer's own W_dec, which no arm changes)

    def g1():
        ops.encode_fwd_t(ws.x, Pd.W_enc_hk, Pd.b_enc, ws.acts, ws.acts_t, True, colsum_part=ws.acts_colpart,
                         l0_part=ws.l0_part, mask_bits=ws.mask_bits)

    def beside(dec):
        def run():
            main_stream = torch.cuda.current_stream(dev)
            fork = torch.cuda.Event()
            fork.record(main_stream)
            with torch.cuda.stream(side):
                side.wait_event(fork)
                dec()
                done = torch.cuda.Event()
                done.record(side)
            g1()
            main_stream.wait_event(done)
        return run

    if not ws.tr:
        sys.exit("master_adam_time: this shape does not run the transposed-operand step whose G1 is timed")
    arms = [("(a) enc half, default", enc_default, a.launches),
            ("(b) enc half, master", enc_master, a.launches),
            ("(c) dec half alone, default", dec_default, a.launches),
            ("(d) dec half alone, master", dec_master, a.launches),
            ("(e) G1 alone", g1, a.launches),
            ("(f) G1 beside (c)", beside(dec_default), a.launches),
            ("(g) G1 beside (d)", beside(dec_master), a.launches),
            ("(h) Trainer.step, default", td.step, a.launches),
            ("(i) Trainer.step, master", tm.step, a.launches),
            ("(j) whole arena + norms, master", whole_master, a.launches)]
    for _, fn, _ in arms:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in arms}
    for _ in range(a.rounds):
        for name, fn, launches in arms:
            ms[name].append(window(fn, launches))
            torch.cuda.synchronize()
    med = {}
    for name, _, launches in arms:
        v = ms[name]
        med[name] = statistics.median(v)
        say(f"  {name:<32} median {med[name]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  "
            f"({launches} calls per window)")
    ka, kb, kc, kd, ke, kf, kg, kh, ki, kj = (med[name] for name, _, _ in arms)
    enc, dec = Pd.split, numel - Pd.split
    say(f"  enc half: default {enc * 14 / ka / 1e9:.2f} TB/s, master {enc * 28 / kb / 1e9:.2f} TB/s; master - default = "
        f"{kb - ka:+.3f} ms")
    say(f"  dec half alone ({blocks} workgroups): default {dec * 14 / kc / 1e9:.2f} TB/s, master "
        f"{dec * 28 / kd / 1e9:.2f} TB/s")
    say(f"  beside G1: the pair outlasts G1 alone by {kf - ke:+.3f} ms (default), {kg - ke:+.3f} ms (master; not the "
        f"step's arrangement)")
    say(f"  the master step's Adam, one stream: {kj:.3f} ms ({numel * 28 / kj / 1e9:.2f} TB/s over the Adam bytes alone); "
        f"the default step exposes (a) + (f) - (e) = {ka + kf - ke:.3f} ms")
    say(f"  Trainer.step: master - default = {ki - kh:+.3f} ms ({(ki / kh - 1) * 100:+.1f} %)")
    for _ in range(40 * a.launches):  # a queued burst of (b) for the clock to be read under load
        enc_master()
    clk = sclk_mhz()
    torch.cuda.synchronize()
    say(f"  shader clock while a burst of (b) was queued: {clk if clk is not None else 'not read'} MHz")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
