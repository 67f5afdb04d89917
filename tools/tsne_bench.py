#!/usr/bin/env python3
"""Exact t-SNE on the GPU (csrc/tsne.hip, ``bsed_amd.tsne``) at the two sizes it is for, in ONE process, event-timed
after warm-up:

  the reference's sample:  N = 2000 points (1000 synth + 1000 real frames) of D = 256 features
  every frame:             N = 20 000 points of D = 256 features (the affinities are 1.6 GB)

Per case: the median (min - max) over ``--reps`` calls of ``bsed_tsne_affinities`` itself, of one gradient + update
iteration (the four launches ``tsne`` makes, device events around them, every buffer allocated before) and of the
gradient with the error (every 50th iteration); the bytes the pairs pass streams (the N x N float32 affinities, once)
divided by the iteration's time, beside what a float4 copy reaches on this chip (6.29 TB/s of HBM; at N = 2000 the 16 MB
of affinities stay in the cache, so that figure is no bound there); and the wall time of ``tsne`` with its default
1000 iterations, host reads included.  No pass mark is attached: there is no earlier version to compare with.

    python tools/tsne_bench.py [--reps 20] [--out profiles/tsne.json] [--small]

Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bsed_amd import tsne as T  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return float(np.median(times)), min(times), max(times)


def time_case(name, N, D, reps):
    L = T.L
    gen = torch.Generator(device="cuda").manual_seed(N + D)
    x = 5.0 + 0.05 * torch.randn((N, D), device="cuda", generator=gen)
    x[N // 2:, 0] += 0.3                                             # two domains
    aff_ms, aff_lo, aff_hi = timed(lambda: T.tsne_affinities_gpu(x, 30.0), max(reps // 4, 3), warm=1)
    aff = T.tsne_affinities_gpu(x, 30.0)
    g = T._Gradient(aff, 0, "tsne_bench")
    y = T.pca_init(x).contiguous()
    velocity, gains = torch.zeros_like(y), torch.ones_like(y)
    lr = max(N / 12.0 / 4.0, 50.0)

    def iteration(error=False):
        g.launch(y, 12.0, error)
        L.call("bsed_tsne_update", L.ptr(y), L.ptr(g.grad), L.ptr(velocity), L.ptr(gains), 2 * N, 0.5, lr, T.MIN_GAIN,
               L.stream())
    it_ms, it_lo, it_hi = timed(iteration, reps)
    err_ms, _, _ = timed(lambda: iteration(True), reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = T.tsne(x, perplexity=30.0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    streamed = 4.0 * N * N
    return dict(case=name, N=N, D=D, splits=L.lib().bsed_tsne_gradient_splits(N), affinities_ms=aff_ms,
                affinities_ms_min=aff_lo, affinities_ms_max=aff_hi, iteration_ms=it_ms, iteration_ms_min=it_lo,
                iteration_ms_max=it_hi, iteration_with_error_ms=err_ms, affinity_bytes=streamed,
                pairs_bytes_per_s=streamed / (it_ms * 1e-3), hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S,
                share_of_hbm_copy=streamed / (it_ms * 1e-3) / HBM_COPY_BYTES_PER_S, tsne_1000_iterations_s=wall,
                n_iter=res.n_iter, kl_divergence=res.kl_divergence)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per case")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a quarter of each N (a quick look; not the figures of DESIGN.md)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench needs the GPU: a CPU run says nothing about time")
    div = 4 if args.small else 1
    results = [{"tool": "tools/tsne_bench.py", "device": torch.cuda.get_device_name(0), "abi": T.L.lib().bsed_abi_version(),
                "reps": args.reps}]
    for name, N in (("the reference's sample", 2000 // div), ("every frame", 20000 // div)):
        res = time_case(name, N, 256, args.reps)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
