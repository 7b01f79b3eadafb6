#!/usr/bin/env python3
"""Times dead-latent resampling at config 2 (B 4096, n 2, d 2304, h 16384, bf16, seeded init):

  get_losses_fwd / rs_add   a plain get_losses forward of one 4096-row batch against LatentResampler.add of the same
                            batch (reset() before each add, timed apart as rs_reset), alternated twice: the difference
                            is what the pool adds (the row copy, the per-row loss reduction, the firing counts)
  pick_*                    cc_resample_pick (all of its launches) at R = 819 200, 65 536 and 4096, J = 1024
  write_*                   cc_resample_write at J = 1024 on config 2's arenas: bf16 moments; fp32 masters with fp32
                            moments; the parameters alone.  bytes = J rows x K x the arenas touched (the source row
                            counted once: its second read hits the cache)
  row_norms_*               cc_row_norms over config 2's W_dec

Each figure: launches after 5 warm-ups, each between its own pair of device events; median, min and max in us.

    python tools/resample_time.py [--out profiles/resample_time.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402
from crosscoder_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the JSON result here")
args = ap.parse_args()
dev = torch.device("cuda:0")
B, n, d, h = 4096, 2, 2304, 16384
K = n * d
cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": B * 1000, "l1_coeff": 2,
       "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": "cuda:0",
       "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000}
out = {}


def timed(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1),
            "reps": reps}


cc = ca.CrossCoder(cfg)
buf = ca.SyntheticBuffer(cfg, rows=B * 2, seed=0)
x = buf.next()
rs = ca.LatentResampler(cc, rows=B * 4)


def add():
    rs.reset()  # (4 small memsets; timed apart below)
    rs.add(x)


def fwd():
    with torch.no_grad():
        cc.get_losses(x)


# alternate the two, twice
for rnd in range(2):
    out[f"get_losses_fwd_{rnd}"] = timed(fwd)
    out[f"rs_add_{rnd}"] = timed(add)
out["rs_reset"] = timed(rs.reset)

# pick
R, J = 819200, 1024
g = torch.Generator().manual_seed(0)
loss = (torch.rand(R, generator=g) * 3).to(dev)
u = torch.rand(J, dtype=torch.float64, generator=g).to(dev)
cdf = torch.empty(R, dtype=torch.float64, device=dev)
rows = torch.empty(J, dtype=torch.int64, device=dev)
out["pick_R819200_J1024"] = timed(lambda: ops.resample_pick(loss, u, cdf=cdf, rows_out=rows), reps=50)
for Rs in (4096, 65536):
    out[f"pick_R{Rs}_J1024"] = timed(lambda: ops.resample_pick(loss[:Rs], u, cdf=cdf[:Rs], rows_out=rows), reps=50)

# write, J = 1024, the trainer's arenas (bf16 moments; then fp32 masters + fp32 moments)
Rp = B * 4
X = torch.randn(Rp, K, generator=g).to(torch.bfloat16).to(dev)
lat = torch.randperm(h, generator=g)[:J].sort().values.to(dev)
prow = torch.randint(Rp, (J,), generator=g).to(dev)
N = 2 * h * K + h + K
P = torch.zeros(N, dtype=torch.bfloat16, device=dev)
for name, sdt, master in (("write_bf16_state", torch.bfloat16, False), ("write_master_f32_state", torch.float32, True),
                          ("write_params_only", None, False)):
    M = V = W = None
    if sdt is not None:
        M, V = torch.zeros(N, dtype=sdt, device=dev), torch.zeros(N, dtype=sdt, device=dev)
    if master:
        W = torch.zeros(N, dtype=torch.float32, device=dev)
    done = torch.empty(J, dtype=torch.int32, device=dev)
    t = timed(lambda: ops.resample_write(X, prow, lat, h, 0.1, 1.0, P, master=W, exp_avg=M, exp_avg_sq=V, done=done),
              reps=50)
    es, ss = 2, (0 if sdt is None else (2 if sdt == torch.bfloat16 else 4))
    # bytes that must move: the source row read once (the second read is cache-resident), 2 parameter rows, 4 moment
    # rows, 2 master rows
    byts = J * K * (es + 2 * es + 4 * ss + (8 if master else 0))
    t["bytes"] = byts
    t["GBps_at_median"] = round(byts / t["median_us"] / 1e3, 1)
    out[name] = t
    del M, V, W

# row norms over W_dec at config 2
a = cc.arena()
nrm = torch.empty(h, dtype=torch.float32, device=dev)
t = timed(lambda: ops.row_norms(a.W_dec_hk, out=nrm), reps=50)
t["bytes"] = h * K * 2
t["GBps_at_median"] = round(t["bytes"] / t["median_us"] / 1e3, 1)
out["row_norms_h16384_K4608_bf16"] = t

out["device"] = torch.cuda.get_device_name(0)
txt = json.dumps(out, indent=1)
print(txt)
if args.out:
    with open(args.out, "w") as f:
        f.write(txt + "\n")
