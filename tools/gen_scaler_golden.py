"""Writes tests/golden/scaler.npz and tests/golden/scaler_state.json: recorded results of the reference's own ``Scaler``
(src/utilities/Scaler.py) over seeded inputs.  The reference is imported at run time from the checkout given by
``--reference`` (its ``src`` directory goes on sys.path); nothing of it is copied.

  python tools/gen_scaler_golden.py --reference /path/to/bird-sound-event-detecion

Inputs: 6 clips shaped (1, 24, 128) float32, values in [-80, 0] on a 1/64 grid (the file compresses), the last 5 frames
0 as PadOrTrunc pads them.  Recorded: mean_, mean_of_square_, std_ of ``calculate_scaler`` over the items
``((features, target), path)``, ``normalize`` of the first clip as a CPU tensor, and the JSON ``save`` writes."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def inputs(seed=20240607, clips=6, frames=24, pad=5, n_mels=128):
    rng = np.random.RandomState(seed)
    x = -np.round(rng.uniform(0.0, 80.0, size=(clips, 1, frames, n_mels)) * 64.0) / 64.0
    x[:, :, frames - pad:, :] = 0.0
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "src"))
    from utilities.Scaler import Scaler
    x = inputs()
    items = [((torch.from_numpy(c), np.zeros(1, dtype=np.float32)), f"clip{i}") for i, c in enumerate(x)]
    sc = Scaler()
    mean, std = sc.calculate_scaler(items)
    norm0 = sc.normalize(torch.from_numpy(x[0])).numpy()
    assert norm0.dtype == np.float32
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "scaler.npz"), x=x, mean_=sc.mean_, mean_of_square_=sc.mean_of_square_,
                        std_=sc.std_, norm0=norm0)
    sc.save(os.path.join(GOLDEN, "scaler_state.json"))
    print("wrote", [(f, os.path.getsize(os.path.join(GOLDEN, f))) for f in ("scaler.npz", "scaler_state.json")])


if __name__ == "__main__":
    main()
