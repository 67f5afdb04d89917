#!/usr/bin/env python3
"""The domain classifier on the GPU (csrc/svc.hip, ``bsed_amd.svc``) at the reference's size -- 1000 synthetic and 1000
real points, five folds -- in ONE process, event-timed after warm-up:

  frame level:  D = 256 features a point
  clip level:   D = 80 128 features a point (T' * F of a 10 s clip)

Per case: the wall time of ``domain_svc`` (host reads included), the median (min - max) over ``--reps`` calls of
``bsed_svc_d2``, of the ONE solve launch of the five folds, of five launches of one fold each (what the batch saves) and
of the decision launch; the pair updates each fold made.  Where sklearn can be imported the wall time of
``cross_val_score(SVC(), X, y, cv=5)`` on the same data (host threads as the environment sets them) and its scores are
added.  libsvm forms its kernel rows one dot product at a time on one thread: 2 n^2 D = 4e11 operations a fold at the clip
level, many minutes for the five folds; ``--sklearn frame`` leaves that case out and the result says so.  No pass mark is
attached: there is no earlier version to compare with.

    python tools/svc_bench.py [--reps 10] [--out profiles/svc.json] [--small] [--sklearn all|frame|none]

Prints one JSON line per case on stdout and the stage it is at on stderr."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bsed_amd import svc as S  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return dict(median=float(np.median(times)), min=min(times), max=max(times))


def stage(text):
    print(f"[svc_bench] {text}", file=sys.stderr, flush=True)


def time_case(name, n, D, reps, with_sklearn):
    stage(f"{name}: n = {n} per domain, D = {D}: domain_svc")
    gen = torch.Generator(device="cuda").manual_seed(n + D)
    x = 5.0 + 0.05 * torch.randn((2 * n, D), device="cuda", generator=gen)
    x[n:] += 0.05 * 1.5 / np.sqrt(D)                                 # two domains that overlap
    synth, real = x[:n], x[n:]
    S.domain_svc(synth, real)                                        # warm-up: the first launches, torch's allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = S.domain_svc(synth, real)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    # the launches by themselves, on the same folds
    target = np.concatenate([np.ones(n, np.int64), np.zeros(n, np.int64)])
    y = torch.from_numpy(np.where(target == 1, 1, -1).astype(np.int32)).cuda()
    train = [np.nonzero(res.fold != f)[0] for f in range(5)]
    test = [np.nonzero(res.fold == f)[0] for f in range(5)]
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in train])])
    test_offsets = np.concatenate([[0], np.cumsum([len(t) for t in test])])
    gammas = res.gamma.tolist()
    max_iter = S.default_max_iter(max(len(t) for t in train))
    stage(f"{name}: domain_svc took {wall:.3f} s, {res.iterations.tolist()} updates; timing the launches")
    d2_ms = timed(lambda: S.svc_d2_gpu(x), reps)
    d2 = S.svc_d2_gpu(x)
    train_gpu, test_gpu = torch.from_numpy(np.concatenate(train)).cuda(), torch.from_numpy(np.concatenate(test)).cuda()
    singles = [torch.from_numpy(t).cuda() for t in train]

    def together():
        return S.svc_solve_gpu(d2, y, offsets, train_gpu, gammas, 1.0, 1e-3, max_iter)

    def one_by_one():
        for f in range(5):
            S.svc_solve_gpu(d2, y, [0, len(train[f])], singles[f], gammas[f], 1.0, 1e-3, max_iter)
    solve_ms = timed(together, reps)
    stage(f"{name}: d2 {d2_ms['median']:.3f} ms, five folds in one launch {solve_ms['median']:.3f} ms")
    single_ms = timed(one_by_one, reps)
    fit = together()
    decision_ms = timed(lambda: S.svc_decision_gpu(d2, y, offsets, train_gpu, test_offsets, test_gpu, gammas, fit), reps)
    out = dict(case=name, n_per_domain=n, D=D, folds=5, domain_svc_wall_s=wall, d2_ms=d2_ms, solve_five_folds_one_launch_ms=solve_ms,
               solve_five_launches_of_one_fold_ms=single_ms, decision_ms=decision_ms, iterations=res.iterations.tolist(),
               n_support=res.n_support.tolist(), scores=res.scores.tolist(), accuracy=res.accuracy, gamma=gammas,
               max_iter=max_iter)
    if not with_sklearn:
        out["sklearn"] = "not run (--sklearn)"
    else:
        stage(f"{name}: sklearn's cross_val_score on the host")
        try:
            from sklearn.model_selection import cross_val_score
            from sklearn.svm import SVC
        except ImportError:
            out["sklearn"] = "not importable"
        else:
            xh = x.cpu().numpy()
            t0 = time.perf_counter()
            scores = cross_val_score(SVC(), xh, target, cv=5)
            out["sklearn_cross_val_score_wall_s"] = time.perf_counter() - t0
            out["sklearn_scores"] = scores.tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed calls per launch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a quarter of the points and of D (a quick look; not the figures "
                                                          "of DESIGN.md)")
    ap.add_argument("--sklearn", choices=("all", "frame", "none"), default="all",
                    help="the cases sklearn's cross_val_score is timed on (the clip level takes it many minutes)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svc_bench needs the GPU: a CPU run says nothing about time")
    div = 4 if args.small else 1
    results = [{"tool": "tools/svc_bench.py", "device": torch.cuda.get_device_name(0), "abi": S.L.lib().bsed_abi_version(),
                "reps": args.reps, "sklearn": args.sklearn}]
    for name, D in (("frame level", 256 // div), ("clip level", 80128 // div)):
        with_sklearn = args.sklearn == "all" or (args.sklearn == "frame" and name == "frame level")
        res = time_case(name, 1000 // div, D, args.reps, with_sklearn)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
