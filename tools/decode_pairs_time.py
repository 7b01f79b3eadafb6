#!/usr/bin/env python3
"""Times the sparse decode from (value, latent) pairs (cc_decode_pairs: CrossCoder.decode_pairs / pairs_sq_err) against
the dense decode of the same activations, on a seeded-init bf16 crosscoder of n * d = 2 * 2304 columns and 4096 rows:
h = 16384 (config 2) at k = 32 and 128, h = 2^17 (config 3's dictionary) at k = 32.  Two sets of pairs per case: the
seeded-init encode_topk of random tokens, and uniformly random latents (every slot valid in both).

  (a) decode_pairs     ops.decode_pairs -> recon [rows, n d]                   (one launch, output preallocated)
  (b) pairs_sq_err     ops.decode_pairs with x -> sq_err [rows, n], no recon   (one launch)
  (c) dense decode     ops.decode_fwd of the pairs scattered into a zero [rows, h] matrix (the GEMM alone)
  (d) scatter + dense  zeros [rows, h], scatter_ of the pairs, then (c): what the dense path costs from the pairs

Each figure: `--reps` launches after one warm-up, each between its own pair of device events; median, min and max.
The gather rate is rows * k * n d * 2 bytes of W_dec rows over (a)'s median.  (a) and (c) are compared before
anything is timed (both round an fp32 sum once; the sums differ in order).

    python tools/decode_pairs_time.py [--out profiles/decode_pairs_time.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402
from crosscoder_amd import ops  # noqa: E402

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


def measure(cc, x, k, source, reps):
    a = cc.arena()
    a.wait_pending()
    rows, n, dp, h, hp = x.shape[0], cc.n_models, cc._dp, cc.d_hidden, cc._hp
    K, dev = n * dp, x.device
    xf = cc._flat_x(x)
    if source == "encode_topk":
        vals, idx = cc.encode_topk(x, k)
    else:
        g = torch.Generator(device=dev).manual_seed(k)
        idx = torch.randint(0, h, (rows, k), device=dev, generator=g, dtype=torch.int32)
        vals = torch.rand(rows, k, device=dev, generator=g).to(cc.dtype)
    valid = int((idx >= 0).sum())
    recon = torch.empty(rows, K, dtype=cc.dtype, device=dev)
    dense_out = torch.empty_like(recon)
    sq = torch.empty(rows, n, dtype=torch.float32, device=dev)

    def scatter():
        acts = torch.zeros(rows, hp, dtype=cc.dtype, device=dev)
        # (duplicate random latents: the dense form adds them like the sparse one)
        return acts.scatter_add_(1, idx.clamp(min=0).long(), vals)

    acts = scatter()
    arms = [("(a) decode_pairs", lambda: ops.decode_pairs(vals, idx, a.W_dec_hk, a.b_dec_flat, n, dp, h=h, recon=recon)),
            ("(b) pairs_sq_err", lambda: ops.decode_pairs(vals, idx, a.W_dec_hk, a.b_dec_flat, n, dp, h=h, x=xf,
                                                          sq_err=sq)),
            ("(c) dense decode", lambda: ops.decode_fwd(acts, a.W_dec_hk, a.b_dec_flat, recon_t=dense_out)),
            ("(d) scatter + dense", lambda: ops.decode_fwd(scatter(), a.W_dec_hk, a.b_dec_flat, recon_t=dense_out))]
    gather = valid * K * recon.element_size()
    say(f"h {h}, rows {rows}, K {K} bf16, k {k}, pairs from {source}: {valid} valid pairs, "
        f"{gather / 1e9:.2f} GB of W_dec rows; dense activations {rows * hp * 2 / 2**20:.0f} MiB")
    arms[0][1]()
    arms[2][1]()
    diff = (recon.float() - dense_out.float()).abs().max().item()
    say(f"  sparse vs dense reconstruction: max |diff| = {diff:.3e} (max |recon| = {recon.float().abs().max().item():.3e})")
    med = {}
    for name, fn in arms:
        fn()
        torch.cuda.synchronize()
        ms = [timed(fn) for _ in range(reps)]
        med[name] = statistics.median(ms)
        say(f"  {name:<22} median {med[name]:8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  ({reps} launches)")
    ta, tb, tc, td = (med[name] for name, _ in arms)
    say(f"  (a) gathers {gather / ta / 1e9:6.2f} TB/s;  (a) / (c) = {ta / tc:.3f}, (a) / (d) = {ta / td:.3f}, "
        f"(b) / (a) = {tb / ta:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["16384:32", "16384:128", "131072:32"], help="dict_size:k")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--d-in", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_pairs_time: no ROCm device (nothing is measured without one)")
    say(f"decode_pairs_time: {torch.cuda.get_device_name(0)}; median of {a.reps} launches after one warm-up")
    cases = [tuple(int(v) for v in c.split(":")) for c in a.cases]
    with torch.no_grad():
        for h in sorted({h for h, _ in cases}):
            cfg = {"seed": 49, "batch_size": a.rows, "buffer_mult": 128, "lr": 5e-5, "num_tokens": a.rows, "l1_coeff": 2,
                   "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16",
                   "device": "cuda:0", "dec_init_norm": 0.08, "d_in": a.d_in, "log_every": 100, "save_every": 30000}
            # the reference's init distribution (Gaussian rows scaled to dec_init_norm, W_enc its transpose), drawn
            # on the device from a seed: the CPU draw of 2^17 x 4608 elements takes longer than everything timed here
            g = torch.Generator(device="cuda:0").manual_seed(h)
            W = torch.randn(h, 2, a.d_in, device="cuda:0", generator=g)
            cc = ca.CrossCoder(cfg, init_W_dec=W / W.norm(dim=-1, keepdim=True) * cfg["dec_init_norm"])
            del W
            x = torch.randn(a.rows, 2, a.d_in, device="cuda:0", generator=g).to(torch.bfloat16)
            for k in [k for hh, k in cases if hh == h]:
                for source in ("encode_topk", "uniform random"):
                    measure(cc, x, k, source, a.reps)
            del cc
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
