#!/usr/bin/env python3
"""python tools/detect_bench.py [out.json] -- timings of recording-level detection, one JSON line.

(a) "decode": ``decode_long_gpu`` (time-parallel ``bsed_decode_long_count`` / ``_write``) against ``decode_regions_gpu``
    (one thread per column, ``bsed_decode_count`` / ``_write``) on the same (1, T, 20) mask with 1 % of the frames on:
    T = 313 (one clip), 11 300 (6 min) and 113 000 (1 h at 32 kHz).  Both are whole calls: count, prefix, the host sync
    on the event count, write, copies of the event list to the host.  The two sides alternate inside one process; each
    round times ITERS back-to-back calls between two device events; median, min and max over ROUNDS rounds of the
    per-call time in microseconds, and in how many rounds the new pair was the slower side.
(b) "detect": ``detect_recording`` on 6 min and 1 h of synthetic audio at 32 kHz, hop_frames = Tp // 2, batch_windows 64,
    default conv_mode, initialised (untrained) weights: wall seconds per call (host clock around a synchronised call),
    seconds of audio per second, and the device time of the stages (front end = gather + mel, forward, stitch,
    post = threshold / median / decode) from event pairs around each stage.
Every timed window ends in a synchronise before its events are read.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsed_amd.evaluation import decode_long_gpu, decode_regions_gpu, detect_recording, window_plan  # noqa: E402
from bsed_amd.features import MelFrontEnd  # noqa: E402
from bsed_amd.labels import BIRD_LIST, ManyHotEncoder  # noqa: E402
from bsed_amd.models import CRNN, Predictor, weights_init  # noqa: E402

ROUNDS, ITERS, WARMUP = 9, 30, 3
DETECT_ROUNDS = 3
SCALE = 4 / (32000 / 255)


def _timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _spread(v, scale=1.0, nd=2):
    return {"median": round(statistics.median(v) * scale, nd), "min": round(min(v) * scale, nd),
            "max": round(max(v) * scale, nd)}


def bench_decode(T, C=20, density=0.01):
    mask = torch.from_numpy((np.random.default_rng(T).random((T, C)) < density).astype(np.float32)).cuda()
    mask3 = mask[None].contiguous()

    def new():
        return decode_long_gpu(mask, SCALE, T * SCALE)

    def old():
        return decode_regions_gpu(mask3, SCALE, T * SCALE)

    assert all(np.array_equal(a, b) for a, b in zip(new(), old()))
    for _ in range(WARMUP):
        new(); old()
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(ROUNDS):
        tn.append(_timed(new, ITERS))
        to.append(_timed(old, ITERS))
    return {"T": T, "C": C, "events": int(len(new()[0])), "decode_long_us": _spread(tn, 1e3), "decode_regions_us": _spread(to, 1e3),
            "speedup_median": round(statistics.median(to) / statistics.median(tn), 2),
            "long_slower_in_rounds": sum(a > b for a, b in zip(tn, to))}


def bench_detect(seconds, fe, crnn, pred, enc):
    sr = fe.cfg.sr
    n = int(seconds * sr)
    g = torch.Generator(device="cuda").manual_seed(int(seconds))
    wave = (torch.rand(n, device="cuda", generator=g) - 0.5) * 0.2
    t = torch.arange(n, device="cuda", dtype=torch.float32) / sr
    wave += 0.2 * torch.sin(2 * np.pi * 1500.0 * t) * (torch.sin(2 * np.pi * 0.05 * t) > 0)
    del t
    starts, Tp, T_total = window_plan(n, sr, fe.cfg.hop_size)

    def run(events=None):
        return detect_recording(crnn, wave, enc.decode_strong, predictor=pred, mel=fe, median_window=14,
                                batch_windows=64, stage_events=events)

    df = run()
    torch.cuda.synchronize()
    wall, stages = [], {}
    for _ in range(DETECT_ROUNDS):
        events = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(events)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        tot = {}
        for name, s, e in events:
            tot[name] = tot.get(name, 0.0) + s.elapsed_time(e)
        for k, v in tot.items():
            stages.setdefault(k, []).append(v)
    med = statistics.median(wall)
    return {"seconds_of_audio": seconds, "windows": int(len(starts)), "output_frames": int(T_total), "events": int(len(df)),
            "wall_s": _spread(wall, 1.0, 4), "audio_seconds_per_second": round(seconds / med, 0),
            "stage_device_ms": {k: _spread(v, 1.0, 2) for k, v in stages.items()}}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/detect_bench.py times kernels on the GPU: no device found")
    kw = dict(n_in_channel=1, activation="glu", dropout=0.5, kernel_size=7 * [3], padding=7 * [1], stride=7 * [1],
              nb_filters=[16, 32, 64, 128, 128, 128, 128],
              pooling=[[2, 2], [2, 2], [1, 2], [1, 2], [1, 2], [1, 2], [1, 2]], nclass=20, attention=True, n_RNN_cell=128,
              n_layers_RNN=2)
    torch.manual_seed(2023)
    fe = MelFrontEnd()
    crnn, pred = CRNN(**kw), Predictor(nclass=20, attention=True, n_RNN_cell=128)
    weights_init(crnn); weights_init(pred)
    enc = ManyHotEncoder(BIRD_LIST, n_frames=313)
    res = {"tool": "tools/detect_bench.py", "device": torch.cuda.get_device_name(0), "conv_mode": crnn.conv_mode,
           "decode": [bench_decode(T) for T in (313, 11300, 113000)], "decode_rounds_x_iters": [ROUNDS, ITERS],
           "detect": [bench_detect(s, fe, crnn, pred, enc) for s in (360.0, 3600.0)], "detect_rounds": DETECT_ROUNDS}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
