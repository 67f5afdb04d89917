"""Measures the dataset scaler's two kernels on the benchmark's own shape (B = 256, 22.05 kHz, T = T_out = 865,
n_mels = 128), one process, one call:

  1. does fusing pay?   normalised ``to_db`` (one launch) against what a user would otherwise run: unnormalised
                        ``to_db`` followed by the torch broadcast ``(x - mean) / std``; unnormalised ``to_db`` alone is
                        recorded beside them for scale.
  2. is the statistics pass a single read?   ``Scaler.update`` from linear mel against ``to_db`` followed by float64 torch
                        reductions of x and x^2; its achieved bytes per second against the bytes it must read (the linear
                        mel).

Method: warm-up, then ``--rounds`` rounds in which the variants ALTERNATE (each timed with device events over
``--iters`` back-to-back calls), the median over rounds and the spread (min .. max) reported per variant.  Prints one
JSON line.

  python tools/scaler_bench.py [--rounds 15] [--iters 50]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from bsed_amd.features import MelConfig, MelFrontEnd
    from bsed_amd.scaler import Scaler
    cfg = MelConfig(sr=22050)
    B, T, M = args.batch, cfg.max_frames, cfg.n_mels
    assert (T, M) == (865, 128)
    g = torch.Generator(device="cuda").manual_seed(0)
    mel = torch.exp(torch.randn(B, T, M, device="cuda", generator=g) * 3.0 - 4.0)
    plain = MelFrontEnd(cfg)
    cmax, _ = plain.stats(mel)
    sc = Scaler().update(mel, cmax, top_db=cfg.top_db)
    sc.finish()
    fused = MelFrontEnd(cfg, scaler=sc)
    mean32 = torch.from_numpy(sc.mean_.astype(np.float32)).cuda()
    std32 = torch.from_numpy(sc.std_.astype(np.float32)).cuda()
    acc = Scaler()

    def torch_stats():
        x = plain.to_db(mel, cmax).double()
        return x.sum(dim=(0, 1, 2)), (x * x).sum(dim=(0, 1, 2))

    variants = {
        "to_db": lambda: plain.to_db(mel, cmax),
        "to_db_then_torch_normalize": lambda: (plain.to_db(mel, cmax) - mean32) / std32,
        "to_db_normalised_fused": lambda: fused.to_db(mel, cmax),
        "to_db_then_torch_float64_sums": torch_stats,
        "scaler_update": lambda: acc.update(mel, cmax, top_db=cfg.top_db),
    }
    # the fused kernel computes what it should before it is timed
    want = torch.from_numpy(((plain.to_db(mel[:2], cmax[:2]).cpu().numpy().astype(np.float64) - sc.mean_) / sc.std_)
                            .astype(np.float32)).cuda()
    assert torch.equal(fused.to_db(mel[:2].contiguous(), cmax[:2].contiguous()), want)
    for f in variants.values():
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / args.iters)
    res = {"shape": [B, T, M], "rounds": args.rounds, "iters": args.iters, "unit": "ms per call"}
    for k, v in times.items():
        res[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    lin_bytes = 4.0 * B * T * M
    res["scaler_update_GBps_of_linear_mel"] = round(lin_bytes / (res["scaler_update"]["median"] * 1e-3) / 1e9, 1)
    res["to_db_normalised_fused_GBps"] = round(2 * lin_bytes / (res["to_db_normalised_fused"]["median"] * 1e-3) / 1e9, 1)
    res["to_db_GBps"] = round(2 * lin_bytes / (res["to_db"]["median"] * 1e-3) / 1e9, 1)

    def beats(a, b):          # a faster than b by more than both spreads
        return res[a]["max"] < res[b]["min"]
    res["fused_beats_pair_beyond_spread"] = beats("to_db_normalised_fused", "to_db_then_torch_normalize")
    res["update_beats_torch_sums_beyond_spread"] = beats("scaler_update", "to_db_then_torch_float64_sums")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
