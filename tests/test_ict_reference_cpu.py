"""tests/ict_reference.py against the reference's own expressions, on the host: ``mix`` is bit for bit what
``lam * x + (1 - lam) * x[index, :]`` gives in torch float32 (mixup_data_sup, src/main.py:135) and in numpy float32
(mixup_data, src/main.py:152-154), and the reference's ``mixup_criterion`` equals BCE against the mixed target."""
import numpy as np
import pytest
import torch

import ict_reference as R

_RNG = np.random.default_rng(2024)
LAMS = [0.0, 1.0, 0.5, 0.3137, float(_RNG.beta(2, 2))]
PERMS = {"fixed point": [2, 1, 3, 0, 5, 4], "identity": [0, 1, 2, 3, 4, 5], "2-cycle": [1, 0, 3, 2, 5, 4]}


@pytest.mark.parametrize("row_len", [1, 3, 20, 257])
@pytest.mark.parametrize("perm", list(PERMS))
@pytest.mark.parametrize("lam", LAMS)
def test_mix_is_the_reference_expression_bit_for_bit(lam, perm, row_len):
    rng = np.random.default_rng(row_len)
    x = (rng.normal(0, 20, (6, row_len)) - 40).astype(np.float32)       # dB-mel sized values
    idx = np.array(PERMS[perm])
    got = R.mix(x, idx, lam)
    assert got.dtype == np.float32 and got.shape == x.shape
    xt = torch.from_numpy(x)
    want_torch = (lam * xt + (1 - lam) * xt[idx, :]).numpy()             # mixup_data_sup
    want_numpy = lam * x + (1 - lam) * x[idx, :]                         # mixup_data, after .cpu().numpy()
    assert want_torch.dtype == np.float32 and want_numpy.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want_torch.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), want_numpy.view(np.uint32))
    if lam == 1.0 or perm == "identity" and lam == 0.0:
        assert np.array_equal(got, x)


def test_mix_keeps_the_trailing_shape_and_takes_rows_along_axis_0():
    x = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    got = R.mix(x, [1, 0], 0.25)
    assert got.shape == x.shape and np.array_equal(got[0], np.float32(0.25) * x[0] + np.float32(0.75) * x[1])


def _bce(p, y):
    """nn.BCELoss(reduction='mean') in float64, with its clamp of the logs at -100"""
    return float(np.mean(-(y * np.maximum(np.log(p), -100.0) + (1.0 - y) * np.maximum(np.log1p(-p), -100.0))))


@pytest.mark.parametrize("lam", LAMS)
def test_mixup_criterion_equals_bce_against_the_mixed_target(lam):
    """BCE is linear in its target: lam * bce(p, ya) + (1 - lam) * bce(p, yb) == bce(p, lam * ya + (1 - lam) * yb), also
    where p is exactly 0 or 1 and the log is clamped (the clamped log is a constant of p, the linearity is in y)"""
    rng = np.random.default_rng(7)
    p = rng.random((6, 40, 20))
    p[0, :5] = 0.0
    p[1, :5] = 1.0
    ya = (rng.random(p.shape) < 0.3).astype(np.float64)
    ya[0, :5, :10] = 1.0                                                 # a target of 1 where p = 0: the clamp at work
    yb = ya[[2, 1, 3, 0, 5, 4]]
    with np.errstate(divide="ignore"):
        two = lam * _bce(p, ya) + (1 - lam) * _bce(p, yb)
        one = _bce(p, lam * ya + (1 - lam) * yb)
        plain = _bce(p, ya)
        torch_bce = float(torch.nn.BCELoss()(torch.from_numpy(p), torch.from_numpy(ya)))
    assert abs(plain - torch_bce) <= 1e-12 * abs(torch_bce)              # _bce is BCELoss
    assert abs(two - one) <= 1e-12 * abs(one), (two, one)
    assert one > 1.0                                                     # the clamped elements really weigh in
