"""The whole model with a species list that is not 20 long: CRNN + Predictor at nclass 10 (one 32-column tile, weights in
LDS) and 48 (three tiles, weights read from L2) against the torch CPU oracle, with seeded weights as in
tests/test_crnn_gpu.py and the "small" shape of its golden file.

Bars (those of tests/test_crnn_gpu.py for these shapes: the head is 2 % of the arithmetic, the CNN / GRU path is the
same): enc 1e-4, strong / weak 2e-5 absolute, loss 2e-5 relative, every gradient tensor 2e-4 relative L2 (+1e-7), the
mean-teacher loss 1e-4 relative.

Then, with 10 classes, the plumbing around the model: checkpoint round trip, ``validate``, ``detect_recording`` and the
graph-replayed train step."""
import os

import numpy as np
import pytest
import torch

from oracle import crnn_oracle as co
from oracle import seeded
from test_crnn_gpu import _grad_check

pytestmark = pytest.mark.gpu

LABELS10 = ["EATO", "WOTH", "BCCH", "BTNW", "TUTI", "NOCA", "REVI", "AMCR", "BLJA", "OVEN"]


def _kwargs(nclass, dropout):
    ck, pk = dict(co.CRNN_KWARGS), dict(co.PREDICTOR_KWARGS)
    ck["nclass"] = pk["nclass"] = nclass
    ck["dropout"] = dropout
    return ck, pk


def _oracle(nclass, dropout, seed):
    ck, pk = _kwargs(nclass, dropout)
    crnn, pred = co.CRNN(**ck), co.Predictor(**pk)
    seeded.load_seeded(crnn, seed)
    seeded.load_seeded(pred, seed + 1)
    return crnn, pred


def _mine(nclass, dropout, ocrnn, opred):
    from bsed_amd.models import CRNN, Predictor
    ck, pk = _kwargs(nclass, dropout)
    crnn, pred = CRNN(**ck), Predictor(**pk)
    crnn.load_state_dict(ocrnn.state_dict())
    pred.load_state_dict(opred.state_dict())
    return crnn, pred


@pytest.fixture(scope="module")
def small(golden_dir):
    """(B, T, seed) of the "small" case of tests/golden/crnn_small.npz"""
    return tuple(int(v) for v in np.load(os.path.join(golden_dir, "crnn_small.npz"))["meta"])


@pytest.mark.parametrize("nclass", [10, 48])
def test_eval_forward_matches_oracle(small, nclass):
    B, T, seed = small
    x = torch.from_numpy(seeded.db_like_input(seed + 10, B, T))
    ocrnn, opred = _oracle(nclass, 0.5, seed)
    crnn, pred = _mine(nclass, 0.5, ocrnn, opred)
    assert set(pred.state_dict()) == set(opred.state_dict())
    for m in (ocrnn, opred, crnn, pred):
        m.eval()
    with torch.no_grad():
        enc_ref, _ = ocrnn(x)
        strong_ref, weak_ref = opred(enc_ref)
        enc, _ = crnn(x.cuda())
        strong, weak = pred(enc)
    assert strong.shape == (B, T // 4, nclass) and weak.shape == (B, nclass)
    assert float((enc.cpu() - enc_ref).abs().max()) < 1e-4
    assert float((strong.cpu() - strong_ref).abs().max()) < 2e-5
    assert float((weak.cpu() - weak_ref).abs().max()) < 2e-5


@pytest.mark.parametrize("nclass", [10, 48])
def test_train_step_loss_and_gradients_match_oracle(small, nclass):
    B, T, seed = small
    x = torch.from_numpy(seeded.db_like_input(seed + 10, B, T))
    y = torch.from_numpy(seeded.strong_targets(seed + 11, B, T // 4, C=nclass))
    ocrnn, opred = _oracle(nclass, 0.0, seed)
    crnn, pred = _mine(nclass, 0.0, ocrnn, opred)
    for m in (ocrnn, opred, crnn, pred):
        m.train()
    loss_ref, _ = co.train_losses(ocrnn, opred, x, y)
    loss_ref.backward()
    enc, ctx = crnn.run_forward(x.cuda(), save=True)
    saved = pred.run_forward(enc)
    crnn.zero_grad(); pred.zero_grad()
    dx, loss_part = pred.run_backward(enc, saved, y_strong=y.cuda(), y_weak=y.max(-2)[0].cuda())
    lp = loss_part.sum(0).cpu().double()
    loss = float(lp[0] / (B * (T // 4) * nclass) + lp[1] / (B * nclass))
    assert abs(loss - float(loss_ref)) < 2e-5 * abs(float(loss_ref)), (loss, float(loss_ref))
    crnn.run_backward(ctx, dx)
    bad = _grad_check(pred, {k: p.grad for k, p in opred.named_parameters()})
    assert not bad, bad
    bad = _grad_check(crnn, {k: p.grad for k, p in ocrnn.named_parameters()})
    assert not bad, bad


@pytest.mark.parametrize("nclass", [10, 48])
def test_mean_teacher_step_loss_matches_oracle(small, nclass):
    from bsed_amd.engine import FlatAdam, SEDTrainer
    B, T, seed = small
    tt = torch.from_numpy
    x = seeded.db_like_input(seed + 10, B, T)
    y = seeded.strong_targets(seed + 11, B, T // 4, C=nclass)
    xr = seeded.db_like_input(seed + 20, B, T)
    xe = xr + np.random.default_rng(seed + 21).normal(0, 1.0, xr.shape).astype(np.float32)
    yw = (np.random.default_rng(seed + 22).random((B, nclass)) < 0.2).astype(np.float32)
    ocrnn, opred = _oracle(nclass, 0.0, seed)
    oema_c, oema_p = _oracle(nclass, 0.0, seed + 5)
    crnn, pred = _mine(nclass, 0.0, ocrnn, opred)
    ema_c, ema_p = _mine(nclass, 0.0, oema_c, oema_p)
    for m in (ocrnn, opred, oema_c, oema_p):
        m.train()
    loss_ref, _ = co.train_losses(ocrnn, opred, tt(x), tt(y), tt(xr), tt(yw), (oema_c, oema_p), tt(xe),
                                  consistency_cost=0.7)
    tr = SEDTrainer(crnn, pred, ema_c, ema_p, optimizer=FlatAdam([crnn, pred], lr=1e-3))
    out = tr.train_step(tt(x).cuda(), tt(y).cuda(), tt(xr).cuda(), tt(yw).cuda(), tt(xe).cuda(), consistency_cost=0.7)
    loss = SEDTrainer.loss_value(out, consistency_cost=0.7)
    assert abs(loss - float(loss_ref)) < 1e-4 * abs(loss), (loss, float(loss_ref))


@pytest.mark.parametrize("nclass", [0, 65])
def test_predictor_refuses_a_class_count_outside_the_range(nclass):
    from bsed_amd.models import Predictor
    assert Predictor.MAX_CLASSES == 64
    with pytest.raises(NotImplementedError, match="nclass <= 64"):
        Predictor(nclass=nclass, attention=True, n_RNN_cell=128)


# ---- plumbing with a 10-species list ---------------------------------------------------------------------------------
def _pair10(seed=23, dropout=0.5, bias=0.0):
    ocrnn, opred = _oracle(10, dropout, seed)
    with torch.no_grad():
        opred.dense.bias += bias
    return _mine(10, dropout, ocrnn, opred)


def test_checkpoint_round_trip_with_10_classes(tmp_path):
    from bsed_amd import checkpoint
    from bsed_amd.labels import ManyHotEncoder
    crnn, pred = _pair10()
    ck, pk = _kwargs(10, 0.5)
    enc = ManyHotEncoder(LABELS10, n_frames=16)
    path = str(tmp_path / "ten.pt")
    checkpoint.save(checkpoint.build_state(crnn, pred, ck, pk, many_hot_encoder=enc), path)
    got = checkpoint.load_models(path)
    assert got["predictor"].nclass == 10 and got["state"]["many_hot_encoder"]["labels"] == LABELS10
    x = torch.from_numpy(seeded.db_like_input(5, 2, 64)).cuda()
    outs = []
    for c, p in ((crnn, pred), (got["crnn"], got["predictor"])):
        c.eval(); p.eval()
        with torch.no_grad():
            outs.append(p(c(x)[0]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_validate_counts_have_one_row_per_label_of_the_list(tmp_path):
    from bsed_amd.evaluation import validate
    from bsed_amd.labels import ManyHotEncoder
    B, T = 4, 128
    crnn, pred = _pair10(bias=1.0)                                  # some classes over the thresholds
    x = seeded.db_like_input(31, B, T)
    root = tmp_path / "d"
    (root / "wav").mkdir(parents=True); (root / "annotation").mkdir()
    for j in range(B):
        with open(root / "annotation" / f"clip{j}.txt", "w") as f:
            f.write("onset\toffset\tevent_label\n0.5\t1.5\tOVEN\n")
    loader = [(((torch.from_numpy(x[i:i + 2]), torch.from_numpy(x[i:i + 2])), None),
               [str(root / "wav" / f"clip{j}.npy") for j in range(i, i + 2)]) for i in (0, 2)]
    enc = ManyHotEncoder(LABELS10, n_frames=T // 4)
    res = validate(crnn, loader, enc.decode_strong, predictor=pred, pooling_time_ratio=4, thresholds=[0.3, 0.5, 0.7],
                   median_window=3)
    assert res.counts.shape == (3, 10, 3) and res.labels == LABELS10
    assert res.counts[:, 9, 2].tolist() == [B] * 3 and res.counts[:, :9, 2].sum() == 0      # Nref: one OVEN per clip
    assert res.counts[:, :, 1].sum() > 0                                                    # and something was detected


def test_detect_recording_returns_labels_of_the_list_only():
    from bsed_amd.evaluation import detect_recording
    from bsed_amd.labels import ManyHotEncoder
    from test_detect_gpu import recording
    crnn, pred = _pair10(bias=1.0)
    enc = ManyHotEncoder(LABELS10, n_frames=313)
    df, stitched, _ = detect_recording(crnn, recording(25.0), enc.decode_strong, predictor=pred, median_window=5,
                                       return_probabilities=True)
    assert stitched.shape[1] == 10
    assert len(df) > 0 and set(df.event_label) <= set(LABELS10)


def test_graph_replay_equals_the_eager_step_with_10_classes():
    from bsed_amd.engine import FlatAdam, SEDTrainer
    B, T = 4, 128
    xs = [torch.from_numpy(seeded.db_like_input(70 + k, B, T)).cuda() for k in range(2)]
    ys = [torch.from_numpy(seeded.strong_targets(80 + k, B, T // 4, C=10)).cuda() for k in range(2)]
    res = {}
    for how in ("eager", "graph"):
        crnn, pred = _pair10(seed=9)
        tr = SEDTrainer(crnn, pred, optimizer=FlatAdam([crnn, pred], lr=1e-3), seed=11)
        if how == "eager":
            for _ in range(3):
                tr.train_step(xs[0], ys[0])
            loss = SEDTrainer.loss_value(tr.train_step(xs[1], ys[1]))
        else:
            tr.capture_step(xs[0], ys[0], warmup=3)
            try:
                loss = SEDTrainer.loss_value(tr.replay_step(xs[1], ys[1]))
            finally:
                tr.release_graph()
        torch.cuda.synchronize()
        res[how] = (loss, pred.flat.clone())
    assert res["eager"][0] == res["graph"][0]
    assert torch.equal(res["eager"][1], res["graph"][1])
