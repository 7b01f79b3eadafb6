#!/usr/bin/env python3
"""Times the sparse decode's backward (cc_pairs_grad_values, cc_pairs_grad_decoder, cc_pairs_latent_sums and
ops.pairs_by_latent) against the dense routes on the same rows, on a seeded-init bf16 crosscoder of n * d = 2 * 2304
columns and 4096 rows: h = 16384 (config 2) and h = 2^17 at k = 32 and 128.  Pairs per case: the seeded-init
encode_topk of random tokens, and uniformly random latents; one extra case (h = 16384, k = 32, uniform) puts one latent
into slot 0 of every row -- a segment of 4096 pairs, which cc_pairs_grad_decoder splits.

  (a) grad_values      ops.pairs_grad_values with val -> dot [rows, k, n] and total     (one launch)
  (b) by_latent        ops.pairs_by_latent (torch: a sort, a count, a cumsum)
  (c) grad_decoder     ops.pairs_grad_decoder -> dW [h, n d]                            (two launches, scratch preallocated)
  (d) latent_sums      ops.pairs_latent_sums of (a)'s dot                               (one launch)
  (e) dense d_acts     cc_dacts_bwd on the pairs scattered into a zero [rows, h] matrix: the GEMM g . W_dec^T that
                       (a) samples
  (f) dense wgrad_dec  cc_wgrad_dec on the same matrix: the GEMM acts^T . g that (c) replaces

Each figure: `--reps` launches after one warm-up, each between its own pair of device events; median, min and max.

    python tools/pairs_grad_time.py [--out profiles/pairs_grad_time.txt]
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


def measure(cc, x, gr, k, source, reps):
    a = cc.arena()
    a.wait_pending()
    rows, n, dp, h, hp = x.shape[0], cc.n_models, cc._dp, cc.d_hidden, cc._hp
    K, dev, dt = n * dp, x.device, cc.dtype
    gf = cc._flat_x(gr)
    if source == "encode_topk":
        vals, idx = cc.encode_topk(x, k)
    else:
        g = torch.Generator(device=dev).manual_seed(k)
        idx = torch.randint(0, h, (rows, k), device=dev, generator=g, dtype=torch.int32)
        vals = torch.rand(rows, k, device=dev, generator=g).to(dt)
        if source == "uniform random + one latent in every row":
            idx[:, 0] = 7
    valid = int((idx >= 0).sum())
    perm, seg = ops.pairs_by_latent(idx, h)
    longest = int((seg[1:] - seg[:-1]).max())
    dot = torch.empty(rows, k, n, dtype=torch.float32, device=dev)
    total = torch.empty(rows, k, dtype=torch.float32, device=dev)
    dW = torch.empty(h, K, dtype=dt, device=dev)
    ws = torch.empty(max(1, ops.pairs_grad_decoder_ws_floats(rows * k, K)), dtype=torch.float32, device=dev)
    s, sa = (torch.zeros(h, n, dtype=torch.float64, device=dev) for _ in range(2))
    cnt = torch.zeros(h, dtype=torch.int64, device=dev)
    # the dense routes' operands: the pairs scattered into a zero matrix, no L1 term
    acts = torch.zeros(rows, hp, dtype=dt, device=dev).scatter_add_(1, idx.clamp(min=0).long(), vals)
    tn = torch.zeros(hp, dtype=torch.float32, device=dev)
    inv_norms = torch.zeros(hp, n, dtype=torch.float32, device=dev)
    g_pre = torch.empty(rows, hp, dtype=dt, device=dev)
    colpart = torch.empty(ops.col_part_rows(rows), hp, dtype=torch.float32, device=dev)
    dW_dense = torch.empty(hp, K, dtype=dt, device=dev)
    sq_part = torch.empty(ops.wgrad_parts(hp, K, dt), dtype=torch.float32, device=dev)
    arms = [("(a) grad_values", lambda: ops.pairs_grad_values(idx, a.W_dec_hk, gf, n, dp, val=vals, h=h, dot=dot,
                                                              total=total)),
            ("(b) by_latent", lambda: ops.pairs_by_latent(idx, h)),
            ("(c) grad_decoder", lambda: ops.pairs_grad_decoder(perm, seg, vals, gf, K, out=dW, ws=ws)),
            ("(d) latent_sums", lambda: ops.pairs_latent_sums(dot, perm, seg, s, sa, cnt)),
            ("(e) dense d_acts", lambda: ops.dacts_bwd(gf, a.W_dec_hk, acts, tn, 0.0, g_pre, colsum_part=colpart)),
            ("(f) dense wgrad_dec", lambda: ops.wgrad_dec(acts, gf, a.W_dec_hk, inv_norms, tn, 0.0, dW_dense, sq_part,
                                                          n, dp))]
    gather = valid * K * dW.element_size()
    say(f"h {h}, rows {rows}, K {K} bf16, k {k}, pairs from {source}: {valid} valid pairs, longest segment {longest}, "
        f"{gather / 1e9:.2f} GB of gathered rows; dW {h * K * 2 / 2**20:.0f} MiB, scratch {ws.numel() * 4 / 2**20:.0f} MiB")
    arms[2][1]()
    arms[5][1]()
    diff = (dW.float() - dW_dense[:h].float()).abs().max().item()
    say(f"  sparse vs dense dW: max |diff| = {diff:.3e} (max |dW| = {dW.float().abs().max().item():.3e})")
    med = {}
    for name, fn in arms:
        fn()
        torch.cuda.synchronize()
        ms = [timed(fn) for _ in range(reps)]
        med[name] = statistics.median(ms)
        say(f"  {name:<22} median {med[name]:8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  ({reps} launches)")
    ta, tb, tc, td, te, tf = (med[name] for name, _ in arms)
    say(f"  (a) gathers {gather / ta / 1e9:6.2f} TB/s, (c) reads and writes {(gather + h * K * 2) / tc / 1e9:6.2f} TB/s;  "
        f"(a) / (e) = {ta / te:.3f}, (c) / (f) = {tc / tf:.3f}, (b + c) / (f) = {(tb + tc) / tf:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["16384:32", "16384:128", "131072:32", "131072:128"], help="dict_size:k")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--d-in", type=int, default=2304)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pairs_grad_time: no ROCm device (nothing is measured without one)")
    say(f"pairs_grad_time: {torch.cuda.get_device_name(0)}; median of {a.reps} launches after one warm-up")
    cases = [tuple(int(v) for v in c.split(":")) for c in a.cases]
    with torch.no_grad():
        for i, h in enumerate(sorted({h for h, _ in cases})):
            cfg = {"seed": 49, "batch_size": a.rows, "buffer_mult": 128, "lr": 5e-5, "num_tokens": a.rows, "l1_coeff": 2,
                   "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16",
                   "device": "cuda:0", "dec_init_norm": 0.08, "d_in": a.d_in, "log_every": 100, "save_every": 30000}
            # the reference's init distribution, drawn on the device from a seed (tools/decode_pairs_time.py)
            g = torch.Generator(device="cuda:0").manual_seed(h)
            W = torch.randn(h, 2, a.d_in, device="cuda:0", generator=g)
            cc = ca.CrossCoder(cfg, init_W_dec=W / W.norm(dim=-1, keepdim=True) * cfg["dec_init_norm"])
            del W
            x = torch.randn(a.rows, 2, a.d_in, device="cuda:0", generator=g).to(torch.bfloat16)
            gr = torch.randn(a.rows, 2, a.d_in, device="cuda:0", generator=g).to(torch.bfloat16)
            ks = [k for hh, k in cases if hh == h]
            for k in ks:
                for source in ("encode_topk", "uniform random"):
                    measure(cc, x, gr, k, source, a.reps)
            if i == 0:
                measure(cc, x, gr, ks[0], "uniform random + one latent in every row", a.reps)
            del cc
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
