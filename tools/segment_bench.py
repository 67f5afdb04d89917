#!/usr/bin/env python3
"""Segment-based counts (csrc/segment_metrics.hip, ``segment_metrics.segment_counts_gpu``) at the two ends of its
workload, in ONE process, event-timed after warm-up:

  (a) validation-shaped:  S = 50 thresholds x B = 24 clips x C = 20 classes, 10 s clips, resolution 1.0, no evaluated length
  (b) one recording:      B = 1, 12 h, C = 20, ``--events`` events per class and side; S = 1 and S = 50, resolution 1.0,
                          the recording's length as the evaluated length -- beside (a) it shows whether one long clip is
                          spread over the device (the grid's tile dimension) or is one workgroup's loop

Per case: the median (min - max) of ``--reps`` calls in microseconds (device events around the call: one launch, the
accumulators allocated before), the workgroups of the launch, and the host's time for the numpy restatement of the tests
(tests/segment_reference.py) on the same lists, whose counts the first call must equal.

    python tools/segment_bench.py [--reps 30] [--events 2000] [--out FILE.json]

Prints one JSON line per case."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segment_reference as R  # noqa: E402
from bsed_amd.evaluation import EventLists, EventReference  # noqa: E402
from bsed_amd.segment_metrics import segment_counts_gpu  # noqa: E402

TILE, MAX_TILES, MAX_Z, MAX_WG = 1024, 1024, 1024, 16384       # the launch geometry of csrc/segment_metrics.hip


def workgroups(S, B, resolution, expected_seconds):
    gx = min(max(math.ceil(math.ceil(expected_seconds / resolution) / TILE), 1), MAX_TILES)
    gz = min(S, MAX_Z)
    return gx * min(B, max(MAX_WG // (gx * gz), 1)) * gz


def lists(rng, n, span, longest):
    on = np.round(rng.uniform(0, span - longest, n) * 8) / 8
    return np.stack([on, on + rng.uniform(0.05, longest, n)], 1)


def cases(events):
    rng = np.random.default_rng(1)
    S, B, C = 50, 24, 20
    ref = [[lists(rng, int(rng.integers(0, 4)), 10.0, 3.0) for _ in range(C)] for _ in range(B)]
    est = [[[lists(rng, int(rng.integers(0, 5)), 10.0, 3.0) for _ in range(C)] for _ in range(B)] for _ in range(S)]
    yield "validation: S=50 B=24 C=20, 10 s clips", est, ref, None, 10.0
    span = 12 * 3600.0
    ref = [[lists(rng, events, span, 20.0) for _ in range(C)]]
    for S in (1, 50):
        est = [[[lists(rng, events, span, 20.0) for _ in range(C)]] for _ in range(S)]
        yield f"recording: S={S} B=1 C=20, 12 h, {events} events per class", est, ref, span, span


def to_gpu(est, ref):
    S, B, C = len(est), len(ref), len(ref[0])
    counts = np.asarray([[[len(est[s][b][c]) for c in range(C)] for b in range(B)] for s in range(S)])
    flat = np.concatenate([est[s][b][c] for s in range(S) for b in range(B) for c in range(C)]).reshape(-1, 2)
    rcounts = np.asarray([[len(ref[b][c]) for c in range(C)] for b in range(B)])
    rflat = np.concatenate([ref[b][c] for b in range(B) for c in range(C)]).reshape(-1, 2)
    return EventLists.from_host(counts, flat), EventReference(rcounts, rflat, [f"clip{b}" for b in range(B)], list(range(C)))


def time_case(name, est, ref, length, expected, reps):
    events, reference = to_gpu(est, ref)
    S, B, C = events.S, events.B, events.C
    t0 = time.perf_counter()
    want = R.segment_counts_np(est, ref, 1.0, length)
    host_s = time.perf_counter() - t0
    got = segment_counts_gpu(events, reference, 1.0, length, expected_seconds=expected)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]), name
    out = (torch.zeros_like(got[0]), torch.zeros_like(got[1]))
    for _ in range(3):
        segment_counts_gpu(events, reference, 1.0, length, out=out, expected_seconds=expected)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        segment_counts_gpu(events, reference, 1.0, length, out=out, expected_seconds=expected)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e-3)
    t = float(np.median(times))
    return dict(case=name, S=S, B=B, C=C, estimated_events=events.total, reference_events=len(reference.seconds),
                segments=int(want[1][0, 3]), workgroups=workgroups(S, B, 1.0, expected), us=t * 1e6, us_min=min(times) * 1e6,
                us_max=max(times) * 1e6, numpy_reference_s=host_s, f1=float(R.segment_metrics_np(*want)["f1"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="timed calls per case")
    ap.add_argument("--events", type=int, default=2000, help="events per class and side of the recording")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_bench needs the GPU: a CPU run says nothing about time")
    results = []
    for name, est, ref, length, expected in cases(args.events):
        res = time_case(name, est, ref, length, expected, args.reps)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
