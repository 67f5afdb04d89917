#!/usr/bin/env python3
"""Soundscape synthesis (csrc/synth.hip, bsed_amd.synth) at the bench shapes, in ONE process, the compared runs alternating:

  1. ``bsed_synth_mix`` alone, event-timed after warm-up: time, algorithmic bytes 4 * B * n * (2 + mean coverage) over
     time, and that rate as a fraction of the 6.3 TB/s a streaming kernel reaches on an MI355X (float4 copy).
  2. the ``from_wave`` train step fed by ``Synthesizer.batch`` one step ahead, against the same step fed from two fixed,
     pre-made waveform batches with fixed targets (bench.py's path): ms per step of each run, the difference of the
     means, and the spread of the repeated identical runs.  Also the host time of drawing and uploading one plan.

    python tools/synth_bench.py [--batch 256] [--steps 30] [--runs 4] [--out FILE.json]

Prints one JSON line per shape (n = 220500 at 22.05 kHz, n = 320000 at 32 kHz)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsed_amd import synth  # noqa: E402
from bsed_amd.engine import FlatAdam, SEDTrainer  # noqa: E402
from bsed_amd.features import MelConfig, MelFrontEnd  # noqa: E402
from bsed_amd.labels import BIRD_LIST, ManyHotEncoder  # noqa: E402
from bsed_amd.models import CRNN, Predictor, weights_init  # noqa: E402

HBM_STREAM = 6.3e12      # bytes / s


def make_bank(sr, seed=1):
    """200 snippets of 0.3 .. 4 s over the 20 labels and 20 backgrounds of 10 s: 60-80 MB, beyond the 32 MiB of L2 but inside
    the 256 MiB Infinity Cache (as a real bank of a few hundred snippets is)"""
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    ev = [(BIRD_LIST[k % 20], 0.1 * torch.randn(int(rng.uniform(0.3, 4.0) * sr), device="cuda", generator=g))
          for k in range(200)]
    bg = [0.02 * torch.randn(10 * sr, device="cuda", generator=g) for _ in range(20)]
    return synth.SoundBank(ev, bg, BIRD_LIST, sr=sr)


def time_mix(bank, syn, B, reps):
    plan = syn.plan(B, 0)
    tables = synth.PlanTables(plan, bank.flat.device)
    out = torch.empty((B, plan.n), device="cuda")
    for _ in range(3):
        synth.mix(bank, plan, tables, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        synth.mix(bank, plan, tables, out=out)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e-3)
    t = float(np.median(times))
    nbytes = 4.0 * B * plan.n * (2.0 + plan.coverage)
    return dict(mix_us=t * 1e6, mix_us_min=min(times) * 1e6, mix_us_max=max(times) * 1e6, coverage=plan.coverage,
                mix_bytes=nbytes, mix_TBps=nbytes / t / 1e12, mix_fraction_of_hbm_stream=nbytes / t / HBM_STREAM)


def make_trainer(fe):
    kw = dict(n_in_channel=1, nclass=20, attention=True, n_RNN_cell=128, n_layers_RNN=2, activation="glu", dropout=0.5,
              kernel_size=7 * [3], padding=7 * [1], stride=7 * [1], nb_filters=[16, 32, 64, 128, 128, 128, 128],
              pooling=[[2, 2], [2, 2], [1, 2], [1, 2], [1, 2], [1, 2], [1, 2]])
    torch.manual_seed(2023)
    crnn, pred = CRNN(**kw), Predictor(nclass=20, attention=True, n_RNN_cell=128)
    weights_init(crnn); weights_init(pred)
    return SEDTrainer(crnn, pred, optimizer=FlatAdam([crnn, pred], lr=1e-3), frontend=fe, seed=2023)


def run_steps(tr, feed, steps):
    """ms per step over `steps` steps: device events around the block AND the host clock to the final synchronise"""
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    w0, y0 = feed(0)
    for k in range(steps):
        w1, y1 = feed(k + 1)
        tr.train_step(w0, y0, from_wave=True, next_waves=(w1, None))
        w0, y0 = w1, y1
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps, (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=4, help="runs of each feed, alternating")
    ap.add_argument("--reps", type=int, default=30, help="timed launches of the mix kernel")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B = args.batch
    results = []
    for sr in (22050, 32000):
        n = 10 * sr
        fe = MelFrontEnd(MelConfig(sr=sr))
        enc = ManyHotEncoder(BIRD_LIST, n_frames=fe.num_frames(n) // 4, sr=sr)
        bank = make_bank(sr)
        syn = synth.Synthesizer(bank, enc, n)
        res = dict(sr=sr, n=n, B=B, bank_MB=4e-6 * bank.total_samples)
        res.update(time_mix(bank, syn, B, args.reps))
        t0 = time.perf_counter()
        for k in range(5):
            synth.PlanTables(syn.plan(B, 100 + k), "cuda")
        res["plan_host_ms"] = (time.perf_counter() - t0) * 1e3 / 5
        fixed = [syn.batch(B, 1000 + i)[:2] for i in range(2)]          # the parent's path: resident, pre-made batches
        tr = make_trainer(fe)
        count = [0]

        def feed_fixed(k):
            return fixed[k % 2]

        def feed_synth(k):
            count[0] += 1
            return syn.batch(B, count[0])[:2]
        run_steps(tr, feed_fixed, 3)
        run_steps(tr, feed_synth, 3)                                     # warm-up of both feeds
        runs = {"fixed": [], "synth": []}
        for _ in range(args.runs):
            for name, feed in (("fixed", feed_fixed), ("synth", feed_synth)):
                runs[name].append(run_steps(tr, feed, args.steps))
        for name, r in runs.items():
            dev = [a for a, _ in r]
            res[f"step_ms_{name}"] = dev
            res[f"step_ms_{name}_host_clock"] = [b for _, b in r]
            res[f"step_ms_{name}_mean"] = float(np.mean(dev))
            res[f"step_ms_{name}_spread"] = float(max(dev) - min(dev))
        res["step_ms_difference"] = res["step_ms_synth_mean"] - res["step_ms_fixed_mean"]
        print(json.dumps(res), flush=True)
        results.append(res)
        del tr, fixed, bank, syn
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
