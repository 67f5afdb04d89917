#!/usr/bin/env python3
"""Integrated loudness (csrc/loudness.hip, ``ops.loudness``) at three shapes, in ONE process, event-timed after warm-up:

  (a) bank-shaped:   2000 segments of 0.2 .. 3 s plus 50 of 30 s, back to back in one flat buffer, 32 kHz
  (b) batch-shaped:  256 clips of 320 000 samples
  (c) one segment:   S = 1, 320 000 samples -- beside (b) it shows whether one long segment is spread over the device

Per case: the median (min - max) of ``--reps`` calls in microseconds (each call = the hop-sum launch and the gate launch,
timed by device events around the call), and the achieved rate against the 4 bytes per effective sample the kernel must
read, also as a share of the 6.3 TB/s a streaming float4 copy reaches on an MI355X.  The kernel filters every sample
twice in float64 (about 10 multiply-adds per sample and pass), so the rate says how far the arithmetic is from the memory roof.

    python tools/loudness_bench.py [--reps 30] [--out FILE.json]

Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsed_amd import ops  # noqa: E402

HBM_STREAM = 6.3e12      # bytes / s
SR = 32000


def effective_samples(lengths, sr=SR):
    half = (sr + 1) // 2
    return int(sum(n if n >= half else n * -(-half // n) for n in lengths))


def cases():
    rng = np.random.default_rng(1)
    bank = [int(rng.uniform(0.2, 3.0) * SR) for _ in range(2000)] + [30 * SR] * 50
    return [("bank: 2000 x 0.2-3 s + 50 x 30 s", bank), ("batch: 256 x 320000", [320000] * 256), ("one segment: 320000", [320000])]


def time_case(name, lengths, reps):
    total = int(sum(lengths))
    g = torch.Generator(device="cuda").manual_seed(3)
    x = 0.1 * torch.randn(total, device="cuda", generator=g)
    ln = torch.tensor(lengths, dtype=torch.int64)
    off = (torch.cumsum(ln, 0) - ln).cuda()
    ln = ln.cuda()
    max_len = max(lengths)
    n_eff = effective_samples(lengths)
    for _ in range(3):
        loud = ops.loudness(x, off, ln, SR, max_len, samples=n_eff)
    torch.cuda.synchronize()
    assert torch.isfinite(loud).all()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.loudness(x, off, ln, SR, max_len, samples=n_eff)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e-3)
    t = float(np.median(times))
    nbytes = 4.0 * n_eff
    return dict(case=name, S=len(lengths), max_len=max_len, effective_samples=n_eff, us=t * 1e6, us_min=min(times) * 1e6,
                us_max=max(times) * 1e6, bytes=nbytes, GBps=nbytes / t / 1e9, fraction_of_hbm_stream=nbytes / t / HBM_STREAM,
                mean_lufs=float(loud.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="timed calls per case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_bench needs the GPU: a CPU run says nothing about time")
    results = []
    for name, lengths in cases():
        res = time_case(name, lengths, args.reps)
        print(json.dumps(res), flush=True)
        results.append(res)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
