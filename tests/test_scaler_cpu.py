"""Dataset scaler, host side: the numpy restatement against the reference's recorded results (tests/golden/scaler.npz,
written by tools/gen_scaler_golden.py from the reference's own Scaler), the Scaler class's persistence, CPU
normalisation and error checks, the ABI 10 entry points' argument checks (all before any HIP call) and the checkpoint
entry.  Nothing here needs a GPU."""
import json
import os

import numpy as np
import pytest
import torch

import scaler_reference as sref
from bsed_amd import _lib as L
from bsed_amd import checkpoint
from bsed_amd.scaler import Scaler
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "scaler.npz")))


STATE_JSON = os.path.join(GOLDEN, "scaler_state.json")


def test_fixture_is_what_the_issue_describes(gold):
    x = gold["x"]
    assert x.shape == (6, 1, 24, 128) and x.dtype == np.float32
    assert x.min() >= -80.0 and x.max() <= 0.0 and not x[:, :, -5:].any() and x[:, :, :-5].any()
    size = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in ("scaler.npz", "scaler_state.json"))
    assert size < 100 * 1024


def test_restatement_reproduces_the_reference(gold):
    mean, msq = sref.statistics(gold["x"])
    # only the order of the 144 float64 additions per band differs
    np.testing.assert_allclose(mean, gold["mean_"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(msq, gold["mean_of_square_"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(sref.std_of(gold["mean_"], gold["mean_of_square_"]), gold["std_"])
    got = sref.normalize(gold["x"][0], gold["mean_"], gold["std_"])
    assert got.dtype == np.float32 and got.tobytes() == gold["norm0"].tobytes()


def test_float64_square_is_seen(gold):
    """the check above is sharp enough to tell the float32 square from a float64 one"""
    x = gold["x"].astype(np.float64).reshape(-1, 128)
    msq64 = (x * x).sum(axis=0) / x.shape[0]
    rel = np.abs(msq64 - gold["mean_of_square_"]) / gold["mean_of_square_"]
    assert rel.max() > 1e-10


def test_scaler_loads_the_reference_json_and_round_trips(gold, tmp_path):
    s = Scaler()
    s.load(STATE_JSON)
    for name in ("mean_", "mean_of_square_", "std_"):
        a = getattr(s, name)
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (128,)
        np.testing.assert_array_equal(a, gold[name])
    assert s.state_dict() == json.load(open(STATE_JSON))
    p = str(tmp_path / "s.json")
    s.save(p)
    assert json.load(open(p)) == json.load(open(STATE_JSON))
    t = Scaler()
    t.load(p)
    u = Scaler().load_state_dict(t.state_dict())
    for name in ("mean_", "mean_of_square_", "std_"):
        np.testing.assert_array_equal(getattr(u, name), gold[name])


def test_normalize_on_the_cpu_is_bitwise_the_reference(gold):
    s = Scaler().load_state_dict(json.load(open(STATE_JSON)))
    x0 = gold["x"][0]
    t = s.normalize(torch.from_numpy(x0))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and not t.is_cuda
    assert t.numpy().tobytes() == gold["norm0"].tobytes()
    a = s.normalize(x0)                      # numpy in: the float64 array the reference returns
    assert isinstance(a, np.ndarray) and a.dtype == np.float64
    assert a.astype(np.float32).tobytes() == gold["norm0"].tobytes()
    # a pad row is -mean / std
    assert t.numpy()[0, -1].tobytes() == (-gold["mean_"] / gold["std_"]).astype(np.float32).tobytes()


@pytest.mark.parametrize("defect", ["zero", "nan", "negative variance", "inf mean"])
def test_unusable_statistics_raise_and_name_the_band(gold, defect):
    sd = {"mean_": gold["mean_"].copy(), "mean_of_square_": gold["mean_of_square_"].copy()}
    if defect == "zero":
        sd["mean_of_square_"][7] = sd["mean_"][7] ** 2
    elif defect == "nan":
        sd["mean_of_square_"][7] = np.nan
    elif defect == "negative variance":
        sd["mean_of_square_"][7] = sd["mean_"][7] ** 2 * 0.5
    else:
        sd["mean_"][7] = np.inf
    sd = {k: v.tolist() for k, v in sd.items()}
    with pytest.raises(L.BsedError, match=r"band\(s\) \[7\]"):
        Scaler().load_state_dict(sd)
    # statistics set behind the class's back are caught at use and at attachment (check is what set_scaler calls)
    s = Scaler().load_state_dict(json.load(open(STATE_JSON)))
    s.std_[3] = 0.0 if defect == "zero" else np.nan
    with pytest.raises(L.BsedError, match="3"):
        s.check(128, who="attach")
    with pytest.raises(L.BsedError, match="3"):
        s.normalize(gold["x"][0])


def test_wrong_width_and_missing_statistics_raise(gold):
    s = Scaler().load_state_dict(json.load(open(STATE_JSON)))
    with pytest.raises(L.BsedError, match="128 bands"):
        s.check(64, who="attach")
    with pytest.raises(L.BsedError, match="no statistics"):
        Scaler().check(128)
    with pytest.raises(L.BsedError):
        Scaler().state_dict()
    with pytest.raises(L.BsedError, match="nothing was accumulated"):
        Scaler().finish()


def test_second_update_of_another_shape_raises_on_the_host():
    """the first update asked for fixes (frames, n_mels); the shape check precedes everything that needs a GPU, so host
    tensors show it: they are refused as such after the check, a differing shape before"""
    s = Scaler()
    with pytest.raises(L.BsedError, match="GPU tensor"):
        s.update(torch.zeros(2, 24, 128))
    with pytest.raises(L.BsedError, match="same frame count and n_mels"):
        s.update(torch.zeros(2, 30, 128))
    with pytest.raises(L.BsedError, match="same frame count and n_mels"):
        s.update(torch.zeros(2, 30, 128), max_frames=25)
    with pytest.raises(L.BsedError, match="same frame count and n_mels"):
        s.update(torch.zeros(2, 24, 64))
    with pytest.raises(L.BsedError, match="same frame count and n_mels"):
        s.update_db(torch.zeros(2, 1, 24, 40))
    with pytest.raises(L.BsedError, match="GPU tensor"):          # the pinned shape is still accepted
        s.update_db(torch.zeros(2, 1, 24, 128))
    with pytest.raises(L.BsedError, match="GPU tensor"):
        s.update(torch.zeros(2, 30, 128), max_frames=24)


def test_abi_10_entry_points_check_their_arguments_before_any_hip_call():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 10
    for name in ("bsed_scaler_scratch_doubles", "bsed_scaler_accum", "bsed_scaler_accum_db", "bsed_scaler_normalize",
                 "bsed_mel_db_norm", "bsed_mel_db_views_norm"):
        assert name in L.FUNCTIONS
    d = 0x1000        # dummy non-null pointer, never dereferenced on the host
    assert lib.bsed_scaler_scratch_doubles(3, 37, 29, 128) == 3 * 1 * 2 * 128
    assert lib.bsed_scaler_scratch_doubles(2, 300, 300, 40) == 2 * 5 * 2 * 40
    assert lib.bsed_scaler_scratch_doubles(0, 37, 29, 128) < 0

    def bad(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    bad(lib.bsed_scaler_accum(None, d, 2, 37, 37, 128, 80.0, d, d, None), "null")
    bad(lib.bsed_scaler_accum(d, None, 2, 37, 37, 128, 80.0, d, d, None), "null")
    bad(lib.bsed_scaler_accum(d, d, 2, 37, 37, 128, 80.0, None, d, None), "null")
    bad(lib.bsed_scaler_accum(d, d, 2, 37, 37, 128, 80.0, d, None, None), "null")
    bad(lib.bsed_scaler_accum(d, d, 0, 37, 37, 128, 80.0, d, d, None), "B must be")
    bad(lib.bsed_scaler_accum(d, d, 65536, 37, 37, 128, 80.0, d, d, None), "B must be")
    bad(lib.bsed_scaler_accum(d, d, 2, 0, 37, 128, 80.0, d, d, None), "bad shape")
    bad(lib.bsed_scaler_accum(d, d, 2, 37, 0, 128, 80.0, d, d, None), "bad shape")
    bad(lib.bsed_scaler_accum(d, d, 2, 37, 37, 0, 80.0, d, d, None), "n_mels")
    bad(lib.bsed_scaler_accum(d, d, 2, 37, 37, 257, 80.0, d, d, None), "n_mels")
    bad(lib.bsed_scaler_accum(d, d, 2, 37, 37, 128, 80.0, d + 4, d, None), "aligned")
    bad(lib.bsed_scaler_accum_db(None, 2, 37, 128, d, d, None), "null")
    bad(lib.bsed_scaler_accum_db(d, 2, 37, 128, None, d, None), "null")
    bad(lib.bsed_scaler_accum_db(d, 2, 0, 128, d, d, None), "bad shape")
    bad(lib.bsed_scaler_accum_db(d, 2, 37, 300, d, d, None), "n_mels")
    bad(lib.bsed_scaler_normalize(d, 10, 128, None, d, d, None), "null")
    bad(lib.bsed_scaler_normalize(d, 0, 128, d, d, d, None), "bad shape")
    bad(lib.bsed_mel_db_norm(d, d, 2, 37, 37, 128, 80.0, None, d, d, None), "null")
    bad(lib.bsed_mel_db_norm(d, d, 2, 37, 37, 128, 80.0, d, None, d, None), "null")
    bad(lib.bsed_mel_db_norm(d, d, 2, 37, 0, 128, 80.0, d, d, d, None), "bad shape")
    bad(lib.bsed_mel_db_views_norm(d, d, 2, 37, 37, 128, 80.0, d, d, None, d, d, d + 16, d + 32, None), "null")
    bad(lib.bsed_mel_db_views_norm(d, d, 2, 37, 37, 40, 80.0, d, d, d, d, d, d + 16, d + 32, None), "n_mels = 128")
    bad(lib.bsed_mel_db_views_norm(d, d, 2, 37, 37, 128, 80.0, d, d, d, d, d, d, d + 32, None), "distinct")
    assert lib.bsed_last_error().decode().startswith("bsed_mel_db_views_norm:")


class _Module:
    """the little of a model that checkpoint._entry reads"""

    def __init__(self, n):
        self._sd = {"w": torch.arange(n, dtype=torch.float32)}

    def state_dict(self):
        return self._sd


def test_checkpoint_entry_is_the_reference_s(gold, tmp_path):
    s = Scaler().load_state_dict(json.load(open(STATE_JSON)))
    crnn, pred = _Module(3), _Module(2)
    without = checkpoint.build_state(crnn, pred, {"a": 1}, {"b": 2})
    assert set(without) == {"model", "model_p", "pooling_time_ratio", "median_window", "epoch"}
    st = checkpoint.build_state(crnn, pred, {"a": 1}, {"b": 2}, scaler=s)
    assert set(st) == set(without) | {"scaler"}
    assert st["scaler"] == {"type": "Scaler", "args": [], "state_dict": json.load(open(STATE_JSON))}
    p = str(tmp_path / "ck.pt")
    checkpoint.save(st, p)
    back = torch.load(p, map_location="cpu", weights_only=False)
    assert back["scaler"] == st["scaler"]
    r = Scaler().load_state_dict(back["scaler"]["state_dict"])
    for name in ("mean_", "mean_of_square_", "std_"):
        np.testing.assert_array_equal(getattr(r, name), gold[name])
