#!/usr/bin/env python3
"""python tools/tagging_bench.py [out.json] -- timings of the clip-level (weak) scoring, one JSON line.

At a validation-sized problem (3008 clips in 47 batches of 64, C = 20 classes, S = 50 thresholds):
  counting   the counting stage of ``validate_weak``: one ``tag_counts_gpu`` launch per batch into one device accumulator,
             one copy of the (S, C, 4) counts at the end;
  host       the route the reference takes: ``.cpu()`` of every batch's weak output, then per threshold the numpy
             binarisation and the four compares of ``intermediate_at_measures``;
  strong     ``bsed_tag_counts`` alone on (64, 313, 20) scores AND targets, set against the bytes it must read,
             2 * B * T * C * 4;
  pass       ``validate_weak``'s loop on a CRNN + Predictor at the product shape, the forward and the counting of every
             batch bracketed by events: the share of the device time that is the forward.
Warm-up first, device time from events (the host route: a host clock, it ends on the host), medians over the rounds.
The counts of the two routes are compared before anything is timed.

python tools/tagging_bench.py --trace-pass runs only the counting loop once (47 launches, one read-back), for a kernel /
memory-copy trace collected around it."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsed_amd.evaluation import TagThresholds, _forward, tag_counts_gpu  # noqa: E402

CLIPS, BATCH, C, S, T = 3008, 64, 20, 50, 313
ROUNDS, WARMUP, REPEAT = 9, 3, 20


def _spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def host_counts(batches, thresholds):
    """.cpu() per batch + the reference's arithmetic per threshold (src/evaluation_measures.py:386-446) -> (S,C,4)"""
    out = np.zeros((len(thresholds), C, 4), np.int64)
    for weak, y in batches:
        p, ref = weak.cpu().numpy(), y.cpu().numpy()
        for s, t in enumerate(thresholds):
            est = (p > np.float32(t)).astype(np.float64)
            out[s, :, 0] += (est + ref == 2).sum(0)
            out[s, :, 1] += (est - ref == 1).sum(0)
            out[s, :, 2] += (ref - est == 1).sum(0)
            out[s, :, 3] += (est + ref == 0).sum(0)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/tagging_bench.py times kernels on the GPU: no device found")
    rng = np.random.default_rng(0)
    thresholds = [float(v) for v in np.linspace(0.02, 0.98, S).astype(np.float32)]
    thr = TagThresholds(thresholds)
    batches = [(torch.from_numpy(rng.random((BATCH, C)).astype(np.float32)).cuda(),
                torch.from_numpy((rng.random((BATCH, C)) < 0.3).astype(np.float32)).cuda()) for _ in range(CLIPS // BATCH)]

    def counting():
        acc = None
        for weak, y in batches:
            acc = tag_counts_gpu(weak, y, thr, out=acc)
        return acc.cpu().numpy()

    if "--trace-pass" in sys.argv:
        counting()
        torch.cuda.synchronize()
        print("trace pass done:", len(batches), "batches")
        return
    assert np.array_equal(counting(), host_counts(batches, thresholds)), "the two routes disagree"
    for _ in range(WARMUP):
        counting(); host_counts(batches, thresholds)
    t_count, t_wall, t_host = [], [], []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms, _ = _events(counting)
        t_wall.append((time.perf_counter() - t0) * 1e3)
        t_count.append(ms)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_counts(batches, thresholds)
        t_host.append((time.perf_counter() - t0) * 1e3)

    # the strong form: scores and targets (64, 313, 20), REPEAT launches per timed window
    xs = torch.from_numpy(rng.random((BATCH, T, C)).astype(np.float32)).cuda()
    ys = torch.from_numpy((rng.random((BATCH, T, C)) < 0.01).astype(np.float32)).cuda()
    acc = tag_counts_gpu(xs, ys, thr)
    want = host_counts([(xs.max(1)[0], (ys.max(1)[0] > 0.5).float())], thresholds)
    assert np.array_equal(acc.cpu().numpy(), want), "the strong form disagrees with the host"

    def strong():
        for _ in range(REPEAT):
            tag_counts_gpu(xs, ys, thr, out=acc)

    for _ in range(WARMUP):
        strong()
    t_strong = [_events(strong)[0] / REPEAT * 1e3 for _ in range(ROUNDS)]          # microseconds per launch
    nbytes = 2 * BATCH * T * C * 4

    # the whole pass: forward + counting per batch, bracketed by events
    from bsed_amd.models import CRNN, Predictor
    from oracle import crnn_oracle as co
    crnn, pred = CRNN(**co.CRNN_KWARGS).eval(), Predictor(**co.PREDICTOR_KWARGS).eval()
    x = torch.from_numpy(rng.standard_normal((BATCH, 1, 4 * T, 128)).astype(np.float32) * 10 - 40).cuda()
    y = batches[0][1]

    def whole_pass():
        marks, out = [], None
        with torch.no_grad():
            for _ in range(CLIPS // BATCH):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                weak = _forward(crnn, pred, False, x, weak=True)[1]
                e[1].record()
                out = tag_counts_gpu(weak, y, thr, out=out)
                e[2].record()
                marks.append(e)
        out.cpu()
        return (sum(a.elapsed_time(b) for a, b, _ in marks), sum(b.elapsed_time(c) for _, b, c in marks))

    for _ in range(2):
        whole_pass()
    passes = [whole_pass() for _ in range(5)]
    fwd, cnt = [p[0] for p in passes], [p[1] for p in passes]
    res = {"tool": "tools/tagging_bench.py", "device": torch.cuda.get_device_name(0), "clips": CLIPS, "batch": BATCH, "C": C,
           "S": S, "rounds": ROUNDS,
           "counting_stage_device_ms": _spread(t_count), "counting_stage_wall_ms": _spread(t_wall),
           "counting_us_per_batch": round(statistics.median(t_count) / len(batches) * 1e3, 2),
           "host_route_wall_ms": _spread(t_host),
           "host_over_counting_wall": round(statistics.median(t_host) / statistics.median(t_wall), 1),
           "counting_slower_in_rounds": sum(a > b for a, b in zip(t_wall, t_host)),
           "strong_form": {"shape": [BATCH, T, C], "launches_per_window": REPEAT, "us_per_launch": _spread(t_strong),
                           "bytes_read": nbytes,
                           "achieved_GB_per_s": round(nbytes / (statistics.median(t_strong) * 1e-6) / 1e9, 1)},
           "pass": {"input": list(x.shape), "batches": CLIPS // BATCH, "forward_device_ms": _spread(fwd),
                    "counting_device_ms": _spread(cnt),
                    "forward_share": round(statistics.median(fwd) / (statistics.median(fwd) + statistics.median(cnt)), 4)}}
    line = json.dumps(res)
    print(line)
    out = [a for a in sys.argv[1:] if not a.startswith("--")]
    if out:
        with open(out[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
