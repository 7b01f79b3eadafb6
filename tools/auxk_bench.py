#!/usr/bin/env python3
"""Times the AuxK dead-latent loss at config 2 (2 x 2304 -> 16384, batch 4096, bf16): the aux selection
(cc_auxk_rows) against cc_topk_rows out of place in the same run, the three small kernels (cc_dead_update,
cc_auxk_loss, cc_add_rows) against their traffic floors at 4 TB/s, and Trainer.step in three arms.

  rows    cc_topk_rows(k = k_aux, out of place, dense output only) and cc_auxk_rows(k_aux) on the same activations,
          alternating single launches: with every latent dead (the same selection, plus the predicate's one int64
          load per owned column) and with 5 % of the latents dead (what the step sees).
  small   each small entry alone; GB/s counts the bytes the algorithm has to move (stated per line).
  step    (i) TopK k = 32 without the aux keys, (ii) aux on with nothing dead (dead_tokens huge), (iii) aux on with
          every 20th latent's encoder row scaled by 1/64 and dead_tokens = batch: those latents are positive yet
          never in a row's top 32, so about 5 % of the dictionary is dead from the second step on.  Single
          Trainer.step calls alternate between the arms, each timed on the host clock up to a device synchronise.
Times are hip events around each launch; medians of `--launches`.

    python tools/auxk_bench.py [--out profiles/auxk_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402
from crosscoder_amd import ops  # noqa: E402

LINES = []
FLOOR_TBS = 4.0  # the HBM rate DESIGN.md section 3.8 measures its kernels against


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


def alternate(arms, n):
    """{name: fn} -> {name: [ms] * n}, single launches of the arms in turn (after one warm-up round)."""
    out = {name: [] for name in arms}
    for i in range(n + 1):
        for name, fn in arms.items():
            ms = timed(fn)
            if i:
                out[name].append(ms)
    return out


def line(name, ms, nbytes=None):
    med = statistics.median(ms)
    s = f"    {name:<26} median {med:8.4f} ms  min {min(ms):8.4f} ms  max {max(ms):8.4f} ms"
    if nbytes is not None:
        floor = nbytes / (FLOOR_TBS * 1e9)
        s += f"  {nbytes / 1e6:8.1f} MB  floor {floor:7.4f} ms  {nbytes / med / 1e6:8.1f} GB/s  ({med / floor:5.2f} x floor)"
    say(s)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--dict-size", type=int, default=16384)
    ap.add_argument("--d-in", type=int, default=2304)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20, help="Trainer.step calls per arm (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("auxk_bench: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, h, d, L = a.rows, a.dict_size, a.d_in, a.launches
    K = 2 * d
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000, "activation": "topk", "k": 32}
    k_aux = min(h, max(1, K // 2))
    say(f"auxk_bench: {torch.cuda.get_device_name(0)}; acts {B} x {h} bf16, K = {K}, k_aux = {k_aux}, "
        f"{L} launches per figure, floors at {FLOOR_TBS} TB/s")

    # ---- the aux selection against the plain one
    cc = ca.CrossCoder(cfg)
    x = ca.SyntheticBuffer(cfg, rows=B, seed=0).next()
    acts = torch.empty(B, h, dtype=torch.bfloat16, device=dev)
    ops.encode_fwd(cc._flat_x(x), cc.arena().W_enc_hk, cc.arena().b_enc, acts, True)
    out = torch.empty_like(acts)
    rc = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = 2 * B * h * 2
    say(f"rows: {100 * (acts > 0).float().mean().item():.1f} % of the activations positive; bytes: one read and one "
        f"write of the activations")
    for label, tsf in (("every latent dead", torch.full((h,), 10, dtype=torch.int64, device=dev)),
                       ("5 % dead", (torch.arange(h, device=dev) % 20 == 0).to(torch.int64) * 10)):
        ms = alternate({"topk": lambda: ops.topk_rows(acts, h, k_aux, out=out),
                        "auxk": lambda: ops.auxk_rows(acts, h, k_aux, tsf, 10, out=out, row_count=rc)}, L)
        say(f"  {label} (mean selected per row {rc.float().mean().item():.1f}):")
        t = line(f"cc_topk_rows k={k_aux}", ms["topk"], nbytes)
        u = line(f"cc_auxk_rows k_aux={k_aux}", ms["auxk"], nbytes)
        say(f"    auxk - topk (medians): {u - t:+.4f} ms")
    del cc

    # ---- the small kernels
    say("small:")
    colsum = torch.rand(h, device=dev)
    tsf = torch.zeros(h, dtype=torch.int64, device=dev)
    was = torch.empty(h, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ms = alternate({"d": lambda: ops.dead_update(colsum, tsf, h, B, 10 ** 9, cnt, was_dead=was)}, L)
    line("cc_dead_update", ms["d"], h * (4 + 8 + 8 + 1))
    recon = torch.randn(B, K, device=dev)
    ehat = torch.randn(B, K, device=dev)
    xx = torch.randn(B, K, device=dev).to(torch.bfloat16)
    b_dec = torch.zeros(K, dtype=torch.bfloat16, device=dev)
    g_aux = torch.empty_like(xx)
    part = torch.empty(ops.auxk_part_floats(B, K), device=dev)
    sc = torch.zeros(4, device=dev)
    ms = alternate({"l": lambda: ops.auxk_loss(recon, b_dec, xx, ehat, g_aux, part, sc, 1.0 / 32)}, L)
    line("cc_auxk_loss (4 launches)", ms["l"], B * K * (2 * (4 + 2 + 4) + 2))
    full = torch.randn(2 * B, h, device=dev).to(torch.bfloat16)
    ms = alternate({"a": lambda: ops.add_rows(full[:B], full[B:])}, L)
    line("cc_add_rows", ms["a"], B * h * 2 * 3)
    del recon, ehat, xx, g_aux, full, acts, out

    # ---- the step
    if a.steps:
        arms = {}
        for name, kw in (("(i) no aux keys", {}), ("(ii) aux, none dead", {"auxk_coeff": 1.0 / 32, "dead_tokens": 10 ** 15}),
                         ("(iii) aux, 5 % dead", {"auxk_coeff": 1.0 / 32, "dead_tokens": B})):
            c = ca.CrossCoder(dict(cfg, **kw))
            if name.startswith("(iii)"):
                with torch.no_grad():
                    c.W_enc[:, :, ::20] *= 1.0 / 64
            tr = ca.Trainer(dict(cfg, **kw), buffer=ca.SyntheticBuffer(cfg, rows=B * 4, seed=0), crosscoder=c)
            tr.step_counter = 10_000  # past the l1 warm-up
            tr.step()
            tr.synchronize()
            arms[name] = (tr, [], [])
        for i in range(a.steps + 5):
            for name, (tr, ms, dicts) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dct = tr.step()
                tr.synchronize()
                torch.cuda.synchronize()
                if i >= 5:
                    ms.append(1e3 * (time.perf_counter() - t0))
                    dicts.append(dct)
        say(f"Trainer.step at config 2, TopK k = 32, {a.steps} steps per arm, alternating (host clock to a device "
            f"synchronise):")
        med = {}
        for name, (tr, ms, dicts) in arms.items():
            med[name] = line(name, ms)
            if "auxk_loss" in dicts[-1]:
                say(f"      last step: auxk_loss {dicts[-1]['auxk_loss']:.6f}, dead_latents {dicts[-1]['dead_latents']} "
                    f"of {h}, aux launches issued: {tr._last_aux_on}")
        names = list(arms)
        say(f"  (ii) - (i) (medians): {med[names[1]] - med[names[0]]:+.4f} ms;  (iii) - (i): "
            f"{med[names[2]] - med[names[0]]:+.4f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
