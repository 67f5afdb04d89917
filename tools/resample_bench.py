#!/usr/bin/env python3
"""python tools/resample_bench.py [out.json] -- timings of the GPU resampler (csrc/resample.hip), one JSON line.

(a) "kernel": ``features.Resampler`` on 1 minute, 10 minutes and 1 hour of audio for stereo int16 48 k -> 32 k, stereo
    int16 44.1 k -> 32 k and mono float32 48 k -> 22.05 k.  Each round times ITERS back-to-back launches between two
    device events, every launch on another input buffer: the buffers of a case add up to at least COLD_BYTES (or two of
    them for the hour), so a launch never finds its input in L2 or the 256 MB Infinity Cache.  (The outputs land in the
    allocator's recycled block; the tap table, at most 356 KB, is meant to stay in L2.)  Per launch: median, min and max
    over ROUNDS rounds in milliseconds; bytes per second for input + output + one read of the table against the 6.3 TB/s
    a streaming kernel reaches on this device; multiply-adds per second (n_out * taps per phase).
(b) "host": ``scipy.signal.resample_poly`` with the same taps on one minute of mono float32, best of HOST_REPEATS, on the
    CPU of the same machine: the route a user had before.
(c) "detect": ``detect_recording`` on one hour of stereo int16 at 48 kHz with ``sr=48000`` against the same call on the
    resampled waveform (``sr=None``), alternating, wall seconds and device milliseconds per stage.
Every timed window ends in a synchronise before its events are read.
"""
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsed_amd.evaluation import detect_recording  # noqa: E402
from bsed_amd.features import MelFrontEnd, resampler  # noqa: E402
from bsed_amd.labels import BIRD_LIST, ManyHotEncoder  # noqa: E402
from bsed_amd.models import CRNN, Predictor, weights_init  # noqa: E402

ROUNDS, WARMUP_ROUNDS, HOST_REPEATS, DETECT_ROUNDS = 9, 2, 3, 3
COLD_BYTES = 600e6
STREAM_PEAK = 6.3e12
CASES = [("int16", 2, 48000, 32000), ("int16", 2, 44100, 32000), ("float32", 1, 48000, 22050)]
SECONDS = (60, 600, 3600)


def _spread(v, scale=1.0, nd=4):
    return {"median": round(statistics.median(v) * scale, nd), "min": round(min(v) * scale, nd), "max": round(max(v) * scale, nd)}


def _input(fmt, n, channels, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (n, channels) if channels > 1 else (n,)
    if fmt == "int16":
        return torch.randint(-32768, 32768, shape, device="cuda", generator=g, dtype=torch.int16)
    return torch.rand(shape, device="cuda", generator=g) - 0.5


def bench_kernel(fmt, channels, sr_in, sr_out, seconds):
    rs = resampler(sr_in, sr_out)
    n = seconds * sr_in
    in_bytes = n * channels * (2 if fmt == "int16" else 4)
    nbuf = max(2, math.ceil(COLD_BYTES / in_bytes))
    bufs = [_input(fmt, n, channels, 1000 * seconds + i) for i in range(nbuf)]
    iters = nbuf
    n_out = rs.n_out(n)
    times = []
    for r in range(WARMUP_ROUNDS + ROUNDS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for i in range(iters):
            y = rs(bufs[i])
        e.record()
        torch.cuda.synchronize()
        if r >= WARMUP_ROUNDS:
            times.append(s.elapsed_time(e) / iters)
    assert y.shape == (n_out,)
    med = statistics.median(times) * 1e-3
    nbytes = in_bytes + 4 * n_out + 4 * rs.table.size
    macs = n_out * rs.taps_per_phase
    return {"format": fmt, "channels": channels, "sr_in": sr_in, "sr_out": sr_out, "up": rs.up, "down": rs.down,
            "taps_per_phase": rs.taps_per_phase, "seconds_of_audio": seconds, "n_in": n, "n_out": n_out,
            "launches_per_round": iters, "input_buffers": nbuf, "ms": _spread(times), "bytes": nbytes,
            "TB_per_s": round(nbytes / med / 1e12, 3), "share_of_6.3_TB_per_s": round(nbytes / med / STREAM_PEAK, 4),
            "TMAC_per_s": round(macs / med / 1e12, 3), "ns_per_output": round(med / n_out * 1e9, 4)}


def bench_host(sr_in, sr_out, seconds=60):
    from scipy.signal import resample_poly
    rs = resampler(sr_in, sr_out)
    x = (np.random.default_rng(sr_in).random(seconds * sr_in, dtype=np.float32) - 0.5)
    win = (rs.taps / rs.up).astype(np.float32)
    best = math.inf
    for _ in range(HOST_REPEATS):
        t0 = time.perf_counter()
        y = resample_poly(x, rs.up, rs.down, window=win, padtype="constant")
        best = min(best, time.perf_counter() - t0)
    assert y.dtype == np.float32 and len(y) == rs.n_out(len(x))
    return {"sr_in": sr_in, "sr_out": sr_out, "dtype": "float32", "seconds_per_minute_of_audio": round(best * 60 / seconds, 4),
            "repeats": HOST_REPEATS, "threads": "scipy.signal.resample_poly is single-threaded"}


def bench_detect(seconds=3600, sr_in=48000):
    kw = dict(n_in_channel=1, activation="glu", dropout=0.5, kernel_size=7 * [3], padding=7 * [1], stride=7 * [1],
              nb_filters=[16, 32, 64, 128, 128, 128, 128],
              pooling=[[2, 2], [2, 2], [1, 2], [1, 2], [1, 2], [1, 2], [1, 2]], nclass=20, attention=True, n_RNN_cell=128,
              n_layers_RNN=2)
    torch.manual_seed(2023)
    fe = MelFrontEnd()
    crnn, pred = CRNN(**kw), Predictor(nclass=20, attention=True, n_RNN_cell=128)
    weights_init(crnn); weights_init(pred)
    enc = ManyHotEncoder(BIRD_LIST, n_frames=313)
    n = seconds * sr_in
    t = torch.arange(n, device="cuda", dtype=torch.float32) / sr_in
    g = torch.Generator(device="cuda").manual_seed(seconds)
    w = (torch.rand(n, device="cuda", generator=g) - 0.5) * 0.2
    w += 0.2 * torch.sin(2 * np.pi * 1500.0 * t) * (torch.sin(2 * np.pi * 0.05 * t) > 0)
    raw = torch.stack([(w * 30000).round().to(torch.int16), (w * 20000).round().to(torch.int16)], dim=1).contiguous()
    del t, w
    wave = resampler(sr_in, fe.cfg.sr)(raw)

    def run(with_sr, events=None):
        if with_sr:
            return detect_recording(crnn, raw, enc.decode_strong, predictor=pred, mel=fe, median_window=14, batch_windows=64,
                                    stage_events=events, sr=sr_in)
        return detect_recording(crnn, wave, enc.decode_strong, predictor=pred, mel=fe, median_window=14, batch_windows=64,
                                stage_events=events)

    assert run(True).equals(run(False))
    torch.cuda.synchronize()
    out = {}
    wall, stages = {True: [], False: []}, {True: {}, False: {}}
    for _ in range(DETECT_ROUNDS):
        for with_sr in (True, False):
            events = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(with_sr, events)
            torch.cuda.synchronize()
            wall[with_sr].append(time.perf_counter() - t0)
            tot = {}
            for name, s, e in events:
                tot[name] = tot.get(name, 0.0) + s.elapsed_time(e)
            for k, v in tot.items():
                stages[with_sr].setdefault(k, []).append(v)
    for with_sr, key in ((True, "sr=48000 (stereo int16 in)"), (False, "sr=None (resampled float32 in)")):
        out[key] = {"wall_s": _spread(wall[with_sr]), "stage_device_ms": {k: _spread(v, 1.0, 2) for k, v in stages[with_sr].items()}}
    out.update({"seconds_of_audio": seconds, "rounds": DETECT_ROUNDS,
                "committed_sr_none_wall_ms_profiles_detect_recording_json": 21.6})
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/resample_bench.py times kernels on the GPU: no device found")
    res = {"tool": "tools/resample_bench.py", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
           "warmup_rounds": WARMUP_ROUNDS, "kernel": [], "host": [], "detect": None}
    for fmt, ch, a, b in CASES:
        for sec in SECONDS:
            res["kernel"].append(bench_kernel(fmt, ch, a, b, sec))
            torch.cuda.empty_cache()
    res["host"] = [bench_host(a, b) for _, _, a, b in CASES]
    res["detect"] = bench_detect()
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
