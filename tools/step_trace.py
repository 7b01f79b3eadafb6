#!/usr/bin/env python3
"""Runs 14 Trainer.step calls at config 2 (2 x 2304 -> 16384, batch 4096, bf16, synthetic data) for one arm --
relu, topk (k = 32), batch (batch_topk, k = 32, weighted by the decoder norms) or auxk (topk with the AuxK dead-latent
loss on and about 5 % of the dictionary dead: every 20th latent's encoder row scaled by 1/64, dead_tokens = batch) -- as
the program of a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o ARM -- python tools/step_trace.py ARM
    python tools/step_timeline.py OUT/.../ARM_kernel_trace.csv 10

(profiles/batch_topk_timeline.txt holds step 10 of the three arms.)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import crosscoder_amd as ca  # noqa: E402

ARMS = {"relu": {}, "topk": {"activation": "topk", "k": 32}, "batch": {"activation": "batch_topk", "k": 32},
        "auxk": {"activation": "topk", "k": 32, "auxk_coeff": 1.0 / 32, "dead_tokens": 4096}}


def main():
    if len(sys.argv) != 2 or sys.argv[1] not in ARMS:
        sys.exit(f"usage: step_trace.py {{{'|'.join(ARMS)}}}")
    if not torch.cuda.is_available():
        sys.exit("step_trace: no ROCm device")
    B, h, d = 4096, 16384, 2304
    cfg = {"seed": 49, "batch_size": B, "buffer_mult": 128, "lr": 5e-5, "num_tokens": 400_000_000, "l1_coeff": 2,
           "beta1": 0.9, "beta2": 0.999, "dict_size": h, "seq_len": 1024, "enc_dtype": "bf16", "device": "cuda:0",
           "dec_init_norm": 0.08, "d_in": d, "log_every": 100, "save_every": 30000, **ARMS[sys.argv[1]]}
    cc = ca.CrossCoder(cfg)
    if sys.argv[1] == "auxk":
        with torch.no_grad():
            cc.W_enc[:, :, ::20] *= 1.0 / 64  # positive, never in a row's top 32: dead from the second step on
    tr = ca.Trainer(cfg, buffer=ca.SyntheticBuffer(cfg, rows=B * 4, seed=0), crosscoder=cc)
    tr.step_counter = 10_000  # past the l1 warm-up
    for _ in range(14):
        tr.step()
    tr.synchronize()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
