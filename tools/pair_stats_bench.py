#!/usr/bin/env python3
"""The all-pairs pass of the domain gap (csrc/pair_stats.hip, ``domain_gap.pair_stats_gpu``) at the two shapes it is for,
in ONE process, event-timed after warm-up, beside a plain-torch baseline (``torch.cdist`` + masked sums + ``exp``):

  frame level:  N = 4096 points of D = 256 features, two groups, S = 5 scales
  clip level:   N = 2048 points of D = 80128 = 313 x 256 features, two groups, S = 5 scales

Per case: the median (min - max) of ``--reps`` calls of ``bsed_pair_stats`` itself in milliseconds (device events around
the two launches, every buffer allocated before; ``wrapper_ms`` is ``pair_stats_gpu`` with its allocations and its count
of the groups, which reads a size back), the arithmetic of the distances alone
(3 N^2 D: a subtraction, a multiplication and an addition per pair and feature, every ordered pair), what share of the
fp32 vector peak (157.3 TFLOP/s) that is, and the largest relative difference of the two routes' distance sums (the
baseline's distances come from the Gram form in float32, so they differ far more than the kernel's bound).

    python tools/pair_stats_bench.py [--reps 20] [--out FILE.json] [--small]

Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bsed_amd import domain_gap as DG  # noqa: E402

PEAK_FP32_VECTOR = 157.3e12


def torch_baseline(x, groups, G, scales):
    d = torch.cdist(x, x)
    d2 = d * d
    eye = torch.eye(x.shape[0], device=x.device, dtype=torch.bool)
    sel = [((groups == g)[None, :] & ~eye) for g in range(G)]
    dist_sum = torch.stack([(d.double() * m).sum(1) for m in sel], 1)
    kern_sum = torch.stack([torch.stack([(torch.exp(-(d2 * s)).double() * m).sum(1) for s in scales], 1) for m in sel], 1)
    nn = torch.where(eye, torch.inf, d2).min(1)
    return dist_sum, kern_sum, nn.values, nn.indices


def timed(fn, reps):
    for _ in range(3):
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


def entry_point(x, groups, G, scales):
    """``bsed_pair_stats`` on buffers allocated once -> a function that makes the two launches"""
    import ctypes
    L = DG.L
    lib = L.lib()
    N, D = x.shape
    S = scales.numel()
    nbytes = lib.bsed_pair_stats_workspace(N, G, S, 0)
    ws = torch.empty(nbytes // 8, device="cuda", dtype=torch.float64)
    dist_sum = torch.empty((N, G), device="cuda", dtype=torch.float64)
    kern_sum = torch.empty((N, G, S), device="cuda", dtype=torch.float64)
    nn_d2, nn_index = torch.empty(N, device="cuda"), torch.empty(N, device="cuda", dtype=torch.int32)
    args = (ctypes.c_void_p(x.data_ptr()), x.stride(0), N, D, L.ptr(groups, torch.int32), G, L.ptr(scales), S, 0,
            L.ptr(dist_sum, torch.float64), L.ptr(kern_sum, torch.float64), L.ptr(nn_d2), L.ptr(nn_index, torch.int32),
            L.ptr(ws, torch.float64), nbytes)
    keep = (ws, dist_sum, kern_sum, nn_d2, nn_index)

    def go(_keep=keep):
        L.check(lib.bsed_pair_stats(*args, L.stream()), "bsed_pair_stats")
    return go, dist_sum


def time_case(name, N, D, reps):
    gen = torch.Generator(device="cuda").manual_seed(N + D)
    x = 5.0 + 0.05 * torch.randn((N, D), device="cuda", generator=gen)
    groups = (torch.arange(N, device="cuda") % 2).int()
    scales = torch.from_numpy(DG.mmd_scales(DG.mean_sq_distance(x))).cuda()
    st = DG.pair_stats_gpu(x, groups, 2, scales)
    base = torch_baseline(x, groups, 2, scales)
    rel = float(((st.dist_sum - base[0]).abs() / base[0]).max())
    go, dist_sum = entry_point(x, groups, 2, scales)
    go()
    assert torch.equal(dist_sum, st.dist_sum)
    ms, lo, hi = timed(go, reps)
    wms, _, _ = timed(lambda: DG.pair_stats_gpu(x, groups, 2, scales), reps)
    bms, blo, bhi = timed(lambda: torch_baseline(x, groups, 2, scales), max(reps // 4, 3))
    flop = 3.0 * N * N * D
    return dict(case=name, N=N, D=D, S=int(scales.numel()), splits=DG.L.lib().bsed_pair_stats_splits(N, D), ms=ms, ms_min=lo,
                ms_max=hi, wrapper_ms=wms, torch_ms=bms, torch_ms_min=blo, torch_ms_max=bhi, distance_tflops=flop / (ms * 1e-3) / 1e12,
                share_of_fp32_vector_peak=flop / (ms * 1e-3) / PEAK_FP32_VECTOR, dist_sum_max_rel_diff_to_torch=rel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per case")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a quarter of each N (a quick look; not the figures of DESIGN.md)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_stats_bench needs the GPU: a CPU run says nothing about time")
    div = 4 if args.small else 1
    results = []
    for name, N, D in (("frame level", 4096 // div, 256), ("clip level", 2048 // div, 313 * 256)):
        res = time_case(name, N, D, args.reps)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
