"""The order of the post-processing launches of every evaluation pass, recorded at ``_lib.call`` and held against
literal lists, and the training flags after a forward that raises.  The lists restate which kernels each pass launches
per batch and per threshold: a pass that launches one more, one fewer or in another order fails here."""
import numpy as np
import pytest
import torch

from oracle import seeded
from test_detect_gpu import _models as recording_models
from test_detect_gpu import recording
from test_event_metrics_gpu import _seeded_models

pytestmark = pytest.mark.gpu

POST = {"bsed_binarize_median", "bsed_decode_count", "bsed_decode_write", "bsed_decode_long_count",
        "bsed_decode_long_write", "bsed_sweep_count", "bsed_sweep_write", "bsed_event_match", "bsed_tag_counts",
        "bsed_tag_masks", "bsed_gather_windows", "bsed_stitch_windows", "bsed_resample_poly"}
SEED, B, T = 41, 6, 256                                 # every strong and weak output lies in 0.66 .. 0.77 (dense bias + 1)
BATCHES = 2


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """two batches of three clips, no annotation files; ``loader(targets)``"""
    from bsed_amd.labels import BIRD_LIST, ManyHotEncoder
    crnn, pred = _seeded_models(SEED)
    x = seeded.db_like_input(SEED + 2, B, T)
    root = tmp_path_factory.mktemp("routes")
    paths = [str(root / "wav" / f"clip{j}.npy") for j in range(B)]

    def loader(y=None):
        return [(((torch.from_numpy(x[i:i + 3]), torch.from_numpy(x[i:i + 3])), None if y is None else torch.from_numpy(y[i:i + 3])),
                 paths[i:i + 3]) for i in (0, 3)]

    return dict(crnn=crnn, pred=pred, loader=loader, enc=ManyHotEncoder(BIRD_LIST, n_frames=T // 4),
                y=np.zeros((B, 20), np.float32))


@pytest.fixture
def launches(monkeypatch):
    """the names of the post-processing entry points in the order they are called; everything is forwarded"""
    from bsed_amd import _lib as L
    seen, real = [], L.call

    def call(name, *args):
        if name in POST:
            seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(L, "call", call)
    return seen


def taken(launches):
    got = list(launches)
    launches.clear()
    return got


def test_launch_order_of_every_pass(clips, launches):
    from bsed_amd.evaluation import (classwise_median_windows, detect_recording, get_predictions, pseudo_label, validate,
                                     validate_weak)
    from bsed_amd.features import MelFrontEnd
    crnn, pred, loader, enc, y = clips["crnn"], clips["pred"], clips["loader"], clips["enc"], clips["y"]
    kw = dict(pooling_time_ratio=4, thresholds=[0.3, 0.5], predictor=pred)
    decode = ["bsed_decode_count", "bsed_decode_write"]

    # get_predictions: per batch, per threshold: the mask, then the two launches of the decode
    dfs, _, _ = get_predictions(crnn, loader(), enc.decode_strong, median_window=5, **kw)
    assert taken(launches) == (["bsed_binarize_median"] + decode) * 2 * BATCHES
    assert all(len(df) > 0 for df in dfs)

    # learned_post: one mask per DISTINCT window (14 and 84 at 32 kHz / 255 / 4) per threshold
    assert sorted(set(classwise_median_windows(32000, 255, 4))) == [14, 84]
    dfs, _, _ = get_predictions(crnn, loader(), enc.decode_strong, learned_post=True, **kw)
    assert taken(launches) == (["bsed_binarize_median"] * 2 + decode) * 2 * BATCHES
    assert all(len(df) > 0 for df in dfs)

    # validate: per batch one sweep over all thresholds and one match; with tagging_thresholds the tag counts first
    sweep = ["bsed_sweep_count", "bsed_sweep_write", "bsed_event_match"]
    res = validate(crnn, loader(), enc.decode_strong, median_window=5, **kw)
    assert taken(launches) == sweep * BATCHES
    assert res.counts[:, :, 1].sum() == 0 and res.tagging is None           # no clip has an annotation: nothing is scored
    res = validate(crnn, loader(y), enc.decode_strong, median_window=5, tagging_thresholds=[0.5, 0.9], **kw)
    assert taken(launches) == (["bsed_tag_counts"] + sweep) * BATCHES
    assert res.tagging.counts[0, :, 1].tolist() == [B] * 20 and res.tagging.counts[1].sum(0).tolist() == [0, 0, 0, 20 * B]

    # the clip-level passes: one launch per batch
    assert (validate_weak(crnn, loader(y), predictor=pred, thresholds=[0.5, 0.9]).counts == res.tagging.counts).all()
    assert taken(launches) == ["bsed_tag_counts"] * BATCHES
    assert len(pseudo_label(crnn, loader(), enc.decode_weak, predictor=pred)) == B
    assert taken(launches) == ["bsed_tag_masks"] * BATCHES

    # detect_recording: 12 s are two windows (0 and the end-aligned one); the seeded probabilities lie in 0.45 .. 0.57
    _, _, rcrnn, rpred = recording_models()
    df = detect_recording(rcrnn, recording(12.0), enc.decode_strong, predictor=rpred, mel=MelFrontEnd(), thresholds=(0.4,))
    assert taken(launches) == ["bsed_gather_windows", "bsed_stitch_windows", "bsed_binarize_median",
                               "bsed_decode_long_count", "bsed_decode_long_write"]
    assert len(df) == 20


class BrokenHead(torch.nn.Module):
    def forward(self, x, inference=False):
        raise RuntimeError("the head broke")


def test_get_predictions_restores_the_training_flags_when_the_forward_raises(clips):
    from bsed_amd.evaluation import get_predictions
    crnn, head = clips["crnn"], BrokenHead()
    for model_training in (True, False):
        crnn.train(model_training); head.train(not model_training)
        with pytest.raises(RuntimeError, match="the head broke"):
            get_predictions(crnn, clips["loader"](), clips["enc"].decode_strong, pooling_time_ratio=4, predictor=head)
        assert crnn.training is model_training and head.training is (not model_training)
    crnn.train()
