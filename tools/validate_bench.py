#!/usr/bin/env python3
"""python tools/validate_bench.py [out.json] -- timings of the validation post-processing, one JSON line.

Two routes from the same (B, 313, 20) GPU probabilities and the same reference events to the same (S, 20, 3) event counts
(Ntp, Nsys, Nref), for S = 1, 10 and 50 thresholds, on one batch of 64 clips and on a 1000-clip pass (15 batches of 64
and one of 40):
  new  ``sweep_events_gpu`` (one count launch, one prefix, ONE host sync, one write launch for all thresholds) ->
       ``event_counts_gpu`` (one launch, counts accumulated on the device), one copy of the counts at the end of the pass;
  old  per threshold ``binarize_median_classwise_gpu`` -> ``decode_regions_gpu`` (the event list copied to the host), then
       the metric on the host in numpy / scipy: list lengths by bincount, a maximum bipartite matching
       (scipy.sparse.csgraph) for every (threshold, clip, class) that has events on both sides.
Class-wise median windows of 14 and 84 frames (the reference's 0.45 s and 2.7 s) over all 20 classes.  The probabilities
are synthetic: low noise plus two to five plateaus per clip; the reference events are the plateaus, moved by up to 0.3 s.
Both routes alternate inside one process; every timed window is a host clock around work that ends in a device
synchronise; median, min and max over the rounds, in milliseconds.  The stages (sweep / match, decode / metric) are timed
in rounds of their own, each stage closed by a synchronise, so their sum exceeds the pipelined total.  The counts of the
two routes are compared before anything is timed.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsed_amd.evaluation import (EventReference, binarize_median_classwise_gpu, decode_regions_gpu, event_counts_gpu,  # noqa: E402
                                 sweep_events_gpu)

T, C = 313, 20
SCALE = 4 / (32000 / 255)
WINDOWS = [14, 14, 14, 14, 14, 84, 84, 84, 14, 84] * 2
COLLAR, PCT = 0.2, 0.2
ROUNDS = {64: 7, 1000: 3}
WARMUP = 2


def make_batch(seed, B):
    """-> ((B,T,C) float32 probabilities, reference lists ref[b][c] of (n,2) seconds)"""
    rng = np.random.default_rng(seed)
    x = (0.08 * rng.random((B, T, C))).astype(np.float32)
    ref = [[[] for _ in range(C)] for _ in range(B)]
    for b in range(B):
        for _ in range(int(rng.integers(2, 6))):
            c, n = int(rng.integers(0, C)), int(rng.integers(20, 140))
            on = int(rng.integers(0, T - n))
            level = rng.uniform(0.3, 0.98)
            x[b, on:on + n, c] = np.maximum(x[b, on:on + n, c], level * (0.75 + 0.25 * rng.random(n)))
            ref[b][c].append((max(on * SCALE + rng.uniform(-0.3, 0.3), 0.0), (on + n) * SCALE + rng.uniform(-0.3, 0.3)))
    return x, [[np.asarray(sorted(ref[b][c]), np.float64).reshape(-1, 2) for c in range(C)] for b in range(B)]


def host_metric(decoded, ref, S, B):
    """the parent commit's way to the counts: event lists on the host -> (S,C,3)"""
    out = np.zeros((S, C, 3), np.int64)
    nref = np.asarray([[len(ref[b][c]) for c in range(C)] for b in range(B)])
    out[:, :, 2] = nref.sum(0)
    for s, (ev_clip, ev_class, _, ev_sec) in enumerate(decoded):
        group = ev_clip.astype(np.int64) * C + ev_class
        n = np.bincount(group, minlength=B * C)
        out[s, :, 1] = n.reshape(B, C).sum(0)
        start = np.concatenate([[0], np.cumsum(n)])
        for g in np.nonzero((n > 0) & (nref.ravel() > 0))[0]:
            r, e = ref[g // C][g % C], ev_sec[start[g]:start[g + 1]]
            hit = (np.abs(r[:, None, 0] - e[None, :, 0]) <= COLLAR) & \
                (np.abs(r[:, None, 1] - e[None, :, 1]) <= np.maximum(COLLAR, PCT * (r[:, 1] - r[:, 0]))[:, None])
            if hit.any():
                out[s, g % C, 0] += int((maximum_bipartite_matching(csr_matrix(hit.astype(np.int8)), perm_type="column") >= 0).sum())
    return out


def _spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


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

    def new_sweep():
        return [sweep_events_gpu(x, thr, classwise_median_window=WINDOWS, scale=SCALE) for x, _, _ in batches]

    def new_match(events):
        acc = None
        for ev, (_, _, reference) in zip(events, batches):
            acc = event_counts_gpu(ev, reference, COLLAR, PCT, out=acc)
        return acc.cpu().numpy()

    def new():
        acc = None
        for x, _, reference in batches:
            ev = sweep_events_gpu(x, thr, classwise_median_window=WINDOWS, scale=SCALE)
            acc = event_counts_gpu(ev, reference, COLLAR, PCT, out=acc)
        return acc.cpu().numpy()

    def old_decode():
        return [[decode_regions_gpu(binarize_median_classwise_gpu(x, t, WINDOWS), SCALE, 10.0) for t in thresholds]
                for x, _, _ in batches]

    def old_metric(decoded):
        return sum(host_metric(d, ref, S, x.shape[0]) for d, (x, ref, _) in zip(decoded, batches))

    def old():
        return old_metric(old_decode())

    a, b = new(), old()
    assert np.array_equal(a, b), "the two routes disagree"
    for _ in range(WARMUP):
        new(); old()
    t = {k: [] for k in ("new", "old", "sweep", "match", "decode", "metric")}
    for _ in range(ROUNDS[clips]):
        t["new"].append(_clock(new)[0])
        t["old"].append(_clock(old)[0])
        ms, ev = _clock(new_sweep)
        t["sweep"].append(ms)
        t["match"].append(_clock(lambda: new_match(ev))[0])
        ms, dec = _clock(old_decode)
        t["decode"].append(ms)
        t["metric"].append(_clock(lambda: old_metric(dec))[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"clips": clips, "batches": len(sizes), "S": S, "events_new_route": int(sum(e.total for e in new_sweep())),
            "counts_sum_ntp_nsys_nref": [int(v) for v in a.sum((0, 1))],
            "new_ms": {"total": _spread(t["new"]), "sweep": _spread(t["sweep"]), "match": _spread(t["match"])},
            "old_ms": {"total": _spread(t["old"]), "decode": _spread(t["decode"]), "metric_host": _spread(t["metric"])},
            "old_over_new": round(med["old"] / med["new"], 2), "decode_over_sweep": round(med["decode"] / med["sweep"], 2),
            "metric_over_match": round(med["metric"] / med["match"], 2),
            "new_slower_in_rounds": sum(x > y for x, y in zip(t["new"], t["old"])), "rounds": ROUNDS[clips]}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/validate_bench.py times kernels on the GPU: no device found")
    res = {"tool": "tools/validate_bench.py", "device": torch.cuda.get_device_name(0), "T": T, "C": C, "windows": WINDOWS,
           "t_collar": COLLAR, "percentage_of_length": PCT,
           "results": [bench(clips, S) for clips in (64, 1000) for S in (1, 10, 50)]}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
