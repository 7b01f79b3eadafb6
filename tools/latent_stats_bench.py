#!/usr/bin/env python3
"""Times the latent-statistics update kernel (cc_latent_stats_update) at config 2 (4096 x 16384 bf16
activations, k = 16, histogram on) against the torch composition that yields the same outputs, and the
cost of the Trainer's latent_stats hook.

Two inputs: the seed-49 initialisation (about half of the activations positive) and a "trained-like" set
(b_enc shifted so that 1-2 % fire).  Per input:
  fresh    the state is reset before every launch (each lane fills its lists from nothing: the worst case)
  steady   the state has seen `--launches` other batches first; the timed batches are new ones
  torch    (acts > 0).sum(0), acts.float().sum(0), torch.topk(acts.T.float(), k) on the same batches
Times are hip events around each launch (median and mean of `--launches`); GB/s counts the B * h * 2 bytes
of activations.  The hook A/B alternates single Trainer.step calls of two trainers (hook on / off), each
timed on the host clock up to a device synchronise.

    python tools/latent_stats_bench.py [--out profiles/latent_stats_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, items):
    """ms per call of fn(item), one event pair per call."""
    out = []
    for it in items:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(it)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def report(name, ms, nbytes):
    med, mean = statistics.median(ms), statistics.fmean(ms)
    say(f"  {name:<8} median {med:8.3f} ms  mean {mean:8.3f} ms  min {min(ms):8.3f} ms  "
        f"{nbytes / med / 1e6:8.1f} GB/s (median)")
    return med


def torch_composition(acts, k):
    return (acts > 0).sum(0), acts.float().sum(0), torch.topk(acts.t().float(), k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--dict-size", type=int, default=16384)
    ap.add_argument("--d-in", type=int, default=2304)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20, help="Trainer.step calls per arm of the hook A/B (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("latent_stats_bench: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, h, d, k, L = a.rows, a.dict_size, a.d_in, a.k, a.launches
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": str(dev),
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
    nbytes = B * h * 2
    say(f"latent_stats_bench: {torch.cuda.get_device_name(0)}; acts {B} x {h} bf16 ({nbytes / 1e6:.0f} MB), k {k}, "
        f"hist on, {L} launches per figure")
    cc = ca.CrossCoder(cfg)
    buf = ca.SyntheticBuffer(cfg, rows=B * 2 * L, seed=0)
    xs = [buf.next() for _ in range(2 * L)]
    for label in ("seed-49 init", "trained-like"):
        if label == "trained-like":  # shift b_enc to the 98.5 % quantile of a sample of pre-activations
            pre = cc.encode(xs[0][:256], apply_relu=False).float().flatten()
            q = torch.quantile(pre[torch.randperm(pre.numel(), device=dev)[:1 << 22]], 0.985).item()
            with torch.no_grad():
                cc.b_enc.sub_(q)
        pool = [cc.encode(x) for x in xs]
        frac = sum((p > 0).float().mean().item() for p in pool[:4]) / 4
        say(f"{label}: {100 * frac:.2f} % of the activations positive")
        st = ca.LatentStats(cc, k=k, hist=True)
        st.update_from_acts(pool[0])  # (code object load)
        torch_composition(pool[0], k)
        torch.cuda.synchronize()

        def fresh(p):
            st.update_from_acts(p)

        ms = []
        for p in pool[:L]:
            st.reset()
            torch.cuda.synchronize()
            ms += timed(fresh, [p])
        fresh_ms = report("fresh", ms, nbytes)
        st.reset()
        for p in pool[:L]:
            st.update_from_acts(p)
        torch.cuda.synchronize()
        steady_ms = report("steady", timed(fresh, pool[L:]), nbytes)
        torch_ms = report("torch", timed(lambda p: torch_composition(p, k), pool[L:]), nbytes)
        say(f"  kernel / torch: fresh {fresh_ms / torch_ms:.3f}, steady {steady_ms / torch_ms:.3f}")
        r = st.result()
        top = torch.topk(torch.cat([p[:, :64] for p in pool]).t().float(), k).values
        assert torch.equal(r["topk_values"][:64], torch.where(top > 0, top, torch.zeros_like(top)))
        assert torch.equal(r["count"], sum((p > 0).sum(0) for p in pool))
        del pool, st
    del cc, xs, buf
    if a.steps:
        arms = {}
        for name in ("hook off", "hook on"):
            c = ca.CrossCoder(cfg)
            st = ca.LatentStats(c, k=k, hist=True) if name == "hook on" else None
            tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * 4, seed=0), crosscoder=c, latent_stats=st)
            tr.step_counter = 10_000  # past the l1 warm-up
            arms[name] = (tr, [])
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
        say(f"  hook overhead (medians): {med['hook on'] - med['hook off']:+.3f} ms "
            f"({100 * (med['hook on'] / med['hook off'] - 1):+.2f} %)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
