#!/usr/bin/env python3
"""python tools/isp_bench.py [out.json] -- timings of the ISP (shift-consistency) input path and step, one JSON line.

(a) "views": ``mel_db_views_kernel`` (dB-mel + time-rolled + frequency-rolled view in one pass) against the sequence it
    replaces, ``to_db`` + 2 x ``ops.roll``, on the same linear-mel batch: B = 24 and 128 clips of 10 s at 32 kHz
    (T = 1255) and 22.05 kHz (T = 865).  The two sides alternate inside one process; each round times ITERS
    back-to-back calls between two device events, and the spread over the ROUNDS rounds is reported (median, min, max
    of the per-call time in microseconds).  Algorithmic bytes: 4 B 128 (T + 3 T_out) for the fused kernel.
(b) "step": ms per full ISP + adversarial ``train_step_isp(from_wave=True)`` from device waveforms, dropout 0.5,
    SGD-Nesterov(0.9, 1e-4) on both optimizers as ``bench.py --mode ada``: the reference batch (24 synthetic + 24 real,
    src/data/config.py:70) at 32 kHz and 128 + 128 at 22.05 kHz; per-step shifts drawn as the reference does
    (randint(-64, 64) * 4 frames, randint(-4, 4) bins).  WARMUP steps, then STEP_ROUNDS rounds of STEP_ITERS steps.
Every timed window ends in a synchronise before its events are read.
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsed_amd import ops  # noqa: E402
from bsed_amd.disc import Clip_Discriminator, ConditionalDomainAdversarialLoss  # noqa: E402
from bsed_amd.engine import FlatSGD, SEDTrainer  # noqa: E402
from bsed_amd.features import MelConfig, MelFrontEnd  # noqa: E402
from bsed_amd.models import CRNN, Predictor, weights_init  # noqa: E402

ROUNDS, ITERS, WARMUP = 9, 30, 3
STEP_ROUNDS, STEP_ITERS = 3, 10


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


def bench_views(fe, B, T):
    g = torch.Generator(device="cuda").manual_seed(B + T)
    mel = torch.rand(B, T, 128, device="cuda", generator=g) * torch.exp(8.0 * torch.rand(B, T, 128, device="cuda", generator=g) - 8.0)
    cmax = mel.amax(dim=(1, 2)).contiguous()
    rng = np.random.default_rng(T)
    sh = torch.tensor([int(v) * 4 for v in rng.integers(-64, 65, B)], dtype=torch.int32, device="cuda")
    sw = torch.tensor([int(v) for v in rng.integers(-4, 5, B)], dtype=torch.int32, device="cuda")

    def fused():
        return fe.to_db_views(mel, cmax, sh, sw, T)

    def sequence():
        x = fe.to_db(mel, cmax, T)
        return x, ops.roll(x, B, T, 128, sh=sh), ops.roll(x, B, T, 128, sw=sw)

    assert all(torch.equal(a, b) for a, b in zip(fused(), sequence()))
    for _ in range(WARMUP):
        fused(); sequence()
    torch.cuda.synchronize()
    tf, ts = [], []
    for _ in range(ROUNDS):
        tf.append(_timed(fused, ITERS))
        ts.append(_timed(sequence, ITERS))
    nbytes = 4.0 * B * 128 * (T + 3 * T)
    mf = statistics.median(tf)
    return {"B": B, "T": T, "fused_us": _spread(tf, 1e3), "to_db_2roll_us": _spread(ts, 1e3),
            "speedup_median": round(statistics.median(ts) / mf, 2), "fused_slower_in_rounds": sum(a > b for a, b in zip(tf, ts)),
            "fused_GBps_algorithmic": round(nbytes / (mf * 1e-3) / 1e9, 0)}


def bench_step(sr, B):
    kw = dict(n_in_channel=1, activation="glu", dropout=0.5, kernel_size=7 * [3], padding=7 * [1], stride=7 * [1],
              nb_filters=[16, 32, 64, 128, 128, 128, 128],
              pooling=[[2, 2], [2, 2], [1, 2], [1, 2], [1, 2], [1, 2], [1, 2]], nclass=20, attention=True, n_RNN_cell=128,
              n_layers_RNN=2)
    torch.manual_seed(2023)
    fe = MelFrontEnd(MelConfig(sr=sr))
    crnn, pred = CRNN(**kw), Predictor(nclass=20, attention=True, n_RNN_cell=128)
    weights_init(crnn); weights_init(pred)
    ema_c, ema_p = CRNN(**kw), Predictor(nclass=20, attention=True, n_RNN_cell=128)
    ema_c.load_state_dict(crnn.state_dict()); ema_p.load_state_dict(pred.state_dict())
    disc = Clip_Discriminator()
    tr = SEDTrainer(crnn, pred, ema_c, ema_p, frontend=fe, seed=2023,
                    optimizer=FlatSGD([crnn, pred], lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True),
                    domain_loss=ConditionalDomainAdversarialLoss(disc),
                    optimizer_d=FlatSGD([disc], lr=1e-4, momentum=0.9, weight_decay=1e-4, nesterov=True))
    n = 10 * sr
    g = torch.Generator(device="cuda").manual_seed(sr + B)
    wav_s = (torch.rand(B, n, device="cuda", generator=g) - 0.5) * 0.2
    wav_r = (torch.rand(B, n, device="cuda", generator=g) - 0.5) * 0.2
    Tp = fe.num_frames(n) // 4
    y = (torch.rand(B, Tp, 20, device="cuda", generator=g) < 0.1).float()
    yw = y.max(1)[0].contiguous()
    rng = np.random.default_rng(B)

    def step():
        frames = [int(v) * 4 for v in rng.integers(-64, 65, B)]
        bins = [int(v) for v in rng.integers(-4, 5, B)]
        return tr.train_step_isp(wav_s, y, wav_r, yw, shift_frames=frames, shift_bins=bins, from_wave=True)

    for _ in range(WARMUP):
        out = step()
    torch.cuda.synchronize()
    ms = [_timed(step, STEP_ITERS) for _ in range(STEP_ROUNDS)]
    loss = SEDTrainer.isp_loss_value(out)
    assert np.isfinite(loss), loss
    med = statistics.median(ms)
    return {"sr": sr, "batch": f"{B}+{B}", "frames": fe.num_frames(n), "ms_per_step": _spread(ms, 1.0, 3),
            "clips_per_s": round(2 * B / (med * 1e-3), 0), "steps_timed": STEP_ROUNDS * STEP_ITERS}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/isp_bench.py times kernels on the GPU: no device found")
    fe = MelFrontEnd(MelConfig(sr=22050))      # to_db / to_db_views use the plan's top_db only: one front end serves both T
    res = {"tool": "tools/isp_bench.py", "device": torch.cuda.get_device_name(0),
           "views": [bench_views(fe, B, T) for T in (1255, 865) for B in (24, 128)],
           "views_rounds_x_iters": [ROUNDS, ITERS],
           "step": [bench_step(32000, 24), bench_step(22050, 128)]}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
