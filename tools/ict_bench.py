"""The measurements of DESIGN.md section 5 "Interpolation consistency": ``ops.mix_rows`` at the sizes of a B = 256 step
against the torch composition it replaces (device events, median of 20 launches after warm-up, and 20 launches back to
back), and the ISP + adversarial step from waveforms with and without an ``IctPlan`` at 12 + 12 clips of 10 s.  Needs
the MI355X; prints one JSON line.   python tools/ict_bench.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bsed_amd import ops  # noqa: E402


def event_times(fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def batch_time(fn, n=20, reps=5):
    """n launches back to back between two events (the host's enqueue time hides behind the kernels), median of reps"""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / n)
    return float(np.median(ts))


res = {}
g = torch.Generator(device="cuda").manual_seed(1)
shapes = [(256, 1, 865, 128), (128, 1, 865, 128), (128, 1, 865, 128), (256, 216, 20), (128, 20)]
xs = [torch.randn(s, device="cuda", generator=g) for s in shapes]
perms = [torch.randperm(s[0], device="cuda") for s in shapes]
p32 = [p.to(torch.int32) for p in perms]
lams = [0.3137, 0.7, 0.55, 0.7, 0.3137]
elements = sum(x.numel() for x in xs)
jobs = [(x, p, l) for x, p, l in zip(xs, p32, lams)]
med, lo, hi = event_times(lambda: ops.mix_rows(jobs))
res["mix_rows_ms"] = (med, lo, hi)
res["mix_rows_TBps"] = 12.0 * elements / (med * 1e-3) / 1e12
med, lo, hi = event_times(lambda: [l * x + (1 - l) * x[p] for x, p, l in zip(xs, perms, lams)])
res["torch_ms"] = (med, lo, hi)
res["torch_TBps_same_bytes"] = 12.0 * elements / (med * 1e-3) / 1e12
res["elements"] = elements
res["mix_rows_back_to_back_ms"] = batch_time(lambda: ops.mix_rows(jobs))
res["torch_back_to_back_ms"] = batch_time(lambda: [l * x + (1 - l) * x[p] for x, p, l in zip(xs, perms, lams)])
# the big job alone, and a plain copy of the same bytes for the day's yardstick
med, _, _ = event_times(lambda: ops.mix_rows(jobs[:1]))
res["mix_rows_big_job_ms"] = med
res["mix_rows_big_job_TBps"] = 12.0 * xs[0].numel() / (med * 1e-3) / 1e12
dst = torch.empty_like(xs[0])
med, _, _ = event_times(lambda: dst.copy_(xs[0]))
res["copy_big_ms"] = med
res["copy_big_TBps"] = 8.0 * xs[0].numel() / (med * 1e-3) / 1e12
got = ops.mix_rows(jobs)
want = [l * x + (1 - l) * x[p] for x, p, l in zip(xs, perms, lams)]
res["equal_to_torch_gpu"] = [bool(torch.equal(a, b)) for a, b in zip(got, want)]
del xs, got, want, dst, jobs
torch.cuda.empty_cache()

# ---- the ISP step at the size of the realistic test
from oracle import crnn_oracle as co  # noqa: E402
from oracle import seeded  # noqa: E402
from bsed_amd.disc import Clip_Discriminator, ConditionalDomainAdversarialLoss  # noqa: E402
from bsed_amd.engine import FlatSGD, SEDTrainer, draw_ict  # noqa: E402
from bsed_amd.features import MelConfig, MelFrontEnd  # noqa: E402
from bsed_amd.models import CRNN, Predictor, weights_init  # noqa: E402

B, sr = 12, 22050
kw = dict(co.CRNN_KWARGS); kw["dropout"] = 0.5
torch.manual_seed(5)
fe = MelFrontEnd(MelConfig(sr=sr))
g = torch.Generator(device="cuda").manual_seed(9)
wav_s = (torch.rand(B, 10 * sr, device="cuda", generator=g) - 0.5) * 0.2
wav_r = (torch.rand(B, 10 * sr, device="cuda", generator=g) - 0.5) * 0.2
T = fe.num_frames(10 * sr)
y = torch.from_numpy(seeded.strong_targets(3, B, T // 4)).cuda()
yw = y.max(1)[0].contiguous()
crnn, pred = CRNN(**kw), Predictor(**co.PREDICTOR_KWARGS)
ema_c, ema_p = CRNN(**kw), Predictor(**co.PREDICTOR_KWARGS)
weights_init(crnn); weights_init(pred)
ema_c.load_state_dict(crnn.state_dict()); ema_p.load_state_dict(pred.state_dict())
disc = Clip_Discriminator()
tr = SEDTrainer(crnn, pred, ema_c, ema_p, frontend=fe,
                optimizer=FlatSGD([crnn, pred], lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True),
                domain_loss=ConditionalDomainAdversarialLoss(disc),
                optimizer_d=FlatSGD([disc], lr=1e-4, momentum=0.9, weight_decay=1e-4, nesterov=True))
rng = np.random.default_rng(1)
frames = [int(v) * 4 for v in rng.integers(-64, 65, B)]
bins = [int(v) for v in rng.integers(-4, 5, B)]
plan = draw_ict(rng, B // 2, B, B - B // 2)
for name, ict in (("isp_step_ms", None), ("isp_ict_step_ms", plan), ("isp_step_again_ms", None)):
    step = lambda: tr.train_step_isp(wav_s, y, wav_r, yw, shift_frames=frames, shift_bins=bins, from_wave=True, ict=ict)
    res[name] = event_times(step, n=10, warm=3)
print(json.dumps(res), flush=True)
