#!/usr/bin/env python3
"""python tools/intersection_bench.py [out.json] -- what ``validate(intersection=True)`` adds to the scoring of a pass, one
JSON line.  The shapes, batches, thresholds and round counts of tools/validate_bench.py (its ``make_batch``): (B, 313, 20)
synthetic probabilities, class-wise median windows, S = 1, 10 and 50 thresholds, one batch of 64 clips and a 1000-clip
pass (15 batches of 64 and one of 40).

  off    per batch ``sweep_events_gpu`` -> ``event_counts_gpu``, the counts copied once at the end of the pass: what
         ``validate`` does without the argument, the baseline;
  on     the same plus ``intersection_counts_gpu`` per batch and its two accumulators copied at the end;
  sweep  ``sweep_events_gpu`` alone, the stage the addition is set against;
  device the two launches of ``bsed_intersection_counts`` between two events on the stream, summed over the batches of a
         pass, on event lists made beforehand.
off / on / sweep are host clocks around work that ends in a device synchronise and alternate inside one process; median,
min and max over the rounds, in milliseconds.  Before anything is timed the counts of the 64-clip batch are compared with
the plain-loop restatement of tests/intersection_reference.py.
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
from bsed_amd.evaluation import EventReference, event_counts_gpu, intersection_counts_gpu, sweep_events_gpu  # noqa: E402
from validate_bench import COLLAR, PCT, ROUNDS, SCALE, WARMUP, WINDOWS, C, T, _clock, _spread, make_batch  # noqa: E402


def bench(clips, S):
    sizes = [64] * (clips // 64) + ([clips % 64] if clips % 64 else [])
    thresholds = [float(v) for v in np.linspace(0.1, 0.9, S).astype(np.float32)] if S > 1 else [0.5]
    thr = torch.tensor(thresholds, dtype=torch.float32).cuda()
    batches = []
    for i, B in enumerate(sizes):
        x, ref = make_batch(1000 * clips + i, B)
        counts = np.asarray([[len(ref[b][c]) for c in range(C)] for b in range(B)])
        reference = EventReference(counts, np.concatenate([ref[b][c] for b in range(B) for c in range(C)]).reshape(-1, 2),
                                   [f"clip{i}_{b}" for b in range(B)], [f"class{c}" for c in range(C)])
        reference.device()
        batches.append((torch.from_numpy(x).cuda(), ref, reference))

    def sweep():
        return [sweep_events_gpu(x, thr, classwise_median_window=WINDOWS, scale=SCALE) for x, _, _ in batches]

    def off():
        acc = None
        for x, _, reference in batches:
            ev = sweep_events_gpu(x, thr, classwise_median_window=WINDOWS, scale=SCALE)
            acc = event_counts_gpu(ev, reference, COLLAR, PCT, out=acc)
        return acc.cpu().numpy()

    def on():
        acc = out = None
        for x, _, reference in batches:
            ev = sweep_events_gpu(x, thr, classwise_median_window=WINDOWS, scale=SCALE)
            acc = event_counts_gpu(ev, reference, COLLAR, PCT, out=acc)
            out = intersection_counts_gpu(ev, reference, out=out)
        return acc.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()

    def device(events):
        marks, out = [], None
        for ev, (_, _, reference) in zip(events, batches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = intersection_counts_gpu(ev, reference, out=out)
            b.record()
            marks.append((a, b))
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in marks)

    counts_off, (counts_on, acc, ct) = off(), on()
    assert np.array_equal(counts_off, counts_on), "the collar-based counts changed with the argument on"
    if clips == 64:
        import intersection_reference as R
        ev = sweep()[0]
        n, _, sec = ev.host()
        at = np.concatenate([[0], np.cumsum(n.ravel())])
        est = [[[sec[at[(s * 64 + b) * C + c]:at[(s * 64 + b) * C + c + 1]] for c in range(C)] for b in range(64)] for s in range(S)]
        want = R.intersection_counts_np(est, batches[0][1])
        assert np.array_equal(acc, want[0]) and np.array_equal(ct, want[1]), "the counts differ from the restatement"
    for _ in range(WARMUP):
        off(); on()
    t = {k: [] for k in ("off", "on", "sweep", "device")}
    for _ in range(ROUNDS[clips]):
        t["off"].append(_clock(off)[0])
        t["on"].append(_clock(on)[0])
        ms, events = _clock(sweep)
        t["sweep"].append(ms)
        t["device"].append(device(events))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"clips": clips, "batches": len(sizes), "S": S, "events": int(sum(e.total for e in sweep())),
            "counts_sum_ntp_nfp_nsys_nref": [int(v) for v in acc.sum((0, 1))], "cross_triggers": int(ct.sum()),
            "off_ms": _spread(t["off"]), "on_ms": _spread(t["on"]), "sweep_ms": _spread(t["sweep"]),
            "intersection_device_ms": _spread(t["device"]),
            "added_ms_median": round(med["on"] - med["off"], 3),
            "added_per_batch_ms_median": round((med["on"] - med["off"]) / len(sizes), 4),
            "device_per_batch_ms_median": round(med["device"] / len(sizes), 4),
            "sweep_per_batch_ms_median": round(med["sweep"] / len(sizes), 4),
            "added_below_sweep": bool(med["on"] - med["off"] < med["sweep"]), "rounds": ROUNDS[clips]}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/intersection_bench.py times kernels on the GPU: no device found")
    res = {"tool": "tools/intersection_bench.py", "device": torch.cuda.get_device_name(0), "T": T, "C": C, "windows": WINDOWS,
           "criteria": [0.5, 0.5, 0.3], "results": [bench(clips, S) for clips in (64, 1000) for S in (1, 10, 50)]}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
