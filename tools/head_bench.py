#!/usr/bin/env python3
"""python tools/head_bench.py [out.json] [--classes 20,33,...] -- device time of the Predictor head by class count, one
JSON line (default output: profiles/head_classes.json).

``bsed_head_fwd`` and ``bsed_head_bwd`` (csrc/head.hip) at the bench shape, B = 256 clips of T = 216 frames, K = 256, for
C in {1, 10, 20, 32, 33, 48, 64}: one and two 32-column tiles with the weights in LDS, the 20-class build, and three
and four tiles with the weights read from L2.  The backward carries the terms of the plain train step (BCE on strong and
weak).  All buffers are allocated once; each round times ITERS back-to-back calls between two device events (the forward's
second launch, the sum over the time splits, included) and ends in a synchronise; per call: median, min and max over
ROUNDS rounds in microseconds, after WARMUP_ROUNDS untimed ones.  GFLOP/s counts 2 * B * T * K * 2C for the forward
and three such contractions for the backward, as the roofline notes of ops.py do.

The tool calls the C ABI directly and uses nothing newer than ``bsed_head_bwd`` itself, so ``--classes 20`` also runs
on a build from before the head took other class counts: the 20-class figures of two builds are compared that way,
against the spread between repeated runs of one build."""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bsed_amd import _lib as L  # noqa: E402
from bsed_amd import ops  # noqa: E402

B, T, K = 256, 216, 256
CLASSES = (1, 10, 20, 32, 33, 48, 64)
ROUNDS, WARMUP_ROUNDS, ITERS = 9, 2, 50


def _spread(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def _timed(fn):
    times = []
    for r in range(WARMUP_ROUNDS + ROUNDS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(ITERS):
            fn()
        e.record()
        torch.cuda.synchronize()
        if r >= WARMUP_ROUNDS:
            times.append(s.elapsed_time(e) / ITERS * 1e3)          # microseconds per call
    return times


def bench(C):
    g = torch.Generator(device="cuda").manual_seed(C)
    rnd = lambda *shape: torch.randn(shape, device="cuda", generator=g)
    x, w, b = rnd(B, T, K), rnd(2 * C, K) / 16, rnd(2 * C) / 16      # logits of order 1
    y = (torch.rand((B, T, C), device="cuda", generator=g) < 0.1).float()
    yw = y.max(1)[0].contiguous()
    S = L.lib().bsed_head_splits(B, T)
    empty = lambda *shape: torch.empty(shape, device="cuda", dtype=torch.float32)
    strong, sof, weak, den, part = empty(B, T, C), empty(B, T, C), empty(B, C), empty(B, C), empty(B, S, 2, C)
    dx, dw_part, db_part, loss_part = empty(B, T, K), empty(B * S, 2 * C, K), empty(B * S, 2 * C), empty(B * S, 6)
    d = ops.HeadBwdDesc()
    p = lambda t: t.data_ptr()
    d.x, d.w, d.strong, d.sof_raw, d.weak, d.den = p(x), p(w), p(strong), p(sof), p(weak), p(den)
    d.y_strong, d.y_weak = p(y), p(yw)
    d.w_strong = d.w_weak = 1.0
    d.inv_n_strong, d.inv_n_weak = 1.0 / (B * T * C), 1.0 / (B * C)
    d.dx, d.dw_part, d.db_part, d.loss_part = p(dx), p(dw_part), p(db_part), p(loss_part)
    d.B, d.T, d.K, d.C, d.attention = B, T, K, C, 1
    stream = L.stream()

    def fwd():
        L.call("bsed_head_fwd", p(x), p(w), p(b), p(strong), p(sof), p(weak), p(den), p(part), B, T, K, C, 1, stream)

    def bwd():
        L.call("bsed_head_bwd", ctypes.byref(d), stream)

    fwd(); bwd()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(weak).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dw_part).all())
    t_f, t_b = _timed(fwd), _timed(bwd)
    flop = 2.0 * B * T * K * 2 * C
    return {"C": C, "time_splits": S, "forward_us": _spread(t_f), "backward_us": _spread(t_b),
            "forward_GFLOP_per_s": round(flop / statistics.median(t_f) / 1e3, 1),
            "backward_GFLOP_per_s": round(3 * flop / statistics.median(t_b) / 1e3, 1)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/head_bench.py times kernels on the GPU: no device found")
    args = sys.argv[1:]
    classes = CLASSES
    if "--classes" in args:
        i = args.index("--classes")
        classes = tuple(int(v) for v in args[i + 1].split(","))
        del args[i:i + 2]
    res = {"tool": "tools/head_bench.py", "device": torch.cuda.get_device_name(0), "abi": L.lib().bsed_abi_version(),
           "B": B, "T": T, "K": K, "rounds": ROUNDS, "warmup_rounds": WARMUP_ROUNDS, "calls_per_round": ITERS,
           "cases": [bench(C) for C in classes]}
    line = json.dumps(res)
    print(line)
    out = args[0] if args else os.path.join(ROOT, "profiles", "head_classes.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
