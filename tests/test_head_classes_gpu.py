"""The Predictor head for any class count (1 .. 64) against float64 autograd on the reference's formulas (reference
src/models/CRNN_GRL.py:441-460 and the BCE / MSE assembly of main_baseline.py:431-498), with the recipe of
tests/test_head_gpu.py::test_head_forward_backward_vs_autograd: weights scaled so that the logits are of order 1, the
strong, weak and both consistency terms on.

Class counts: both sides of every 32-column tile edge of the 2C logits (16|17, 32|33, 48|49), both dispatch ranges
(weights in LDS up to 32 classes, read from L2 above), the single-class softmax and the top of the range.
Shapes: (1, 77) three chunks of 32 frames with a ragged last one, in two time splits; (3, 31) less than a chunk;
(2, 33) one frame into the second chunk; (1, 1) a single frame.

Bars: strong / weak 4e-6 absolute and the assembled loss 1e-5 relative (the same formulas in plain fp32 against
float64 over this grid: 1.1e-6 at C = 64 and 4.8e-6 at (2, 33), C = 33), gradients 2e-5 relative L2 (the project's bar;
1.2e-6 in that evaluation).  At T = 1 with attention on, weak == strong exactly and the attention-path gradient is pure
cancellation (2.4e-5 in the fp32 evaluation alone): there the forward is checked in both modes, the gradients with
attention off only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 256
ALL_C = [1, 2, 16, 17, 19, 21, 32, 33, 48, 49, 63, 64]
SHAPES = [(1, 77), (3, 31), (2, 33), (1, 1)]
CASES = [(C, 1, 77, True) for C in ALL_C]
CASES += [(C, B, T, att) for C in (1, 33, 64) for B, T in SHAPES for att in (True, False) if (C, B, T, att) not in CASES]


def _setup(C, B, T, attention):
    from bsed_amd import ops
    from bsed_amd.models import Predictor, weights_init
    torch.manual_seed(3)
    pred = Predictor(nclass=C, attention=attention, n_RNN_cell=128)
    weights_init(pred)
    with torch.no_grad():
        pred.flat.mul_(20.0)                                             # logits of order 1
    g = torch.Generator(device="cuda").manual_seed(17 + C)
    enc = torch.randn((B, T, K), device="cuda", generator=g)
    y = (torch.rand((B, T, C), device="cuda", generator=g) < 0.2).float()
    es = torch.rand((B, T, C), device="cuda", generator=g)
    ew = torch.rand((B, C), device="cuda", generator=g)
    pred.train()
    return pred, enc, dict(y_strong=y, y_weak=ops.max_over_time(y), ema_strong=es, ema_weak=ew, w_cons_s=0.7, w_cons_w=0.3)


def _run(pred, enc, kw):
    saved = pred.run_forward(enc)
    pred.flat_grad.zero_()
    dx, lp = pred.run_backward(enc, saved, **kw)
    return saved, dx, lp, pred.flat_grad.clone()


@pytest.mark.parametrize("C,B,T,attention", CASES)
def test_head_forward_backward_vs_autograd(C, B, T, attention):
    pred, enc, kw = _setup(C, B, T, attention)
    saved, dx, lp, grad = _run(pred, enc, kw)
    # float64 autograd on the reference's formulas
    w = pred.flat[:2 * C * K].detach().double().view(2 * C, K).requires_grad_(True)
    b = pred.flat[2 * C * K:].detach().double().requires_grad_(True)
    x = enc.double().requires_grad_(True)
    lin = x @ w.t() + b
    strong = torch.sigmoid(lin[..., :C])
    if attention:
        sof = torch.softmax(lin[..., C:], dim=-1).clamp(1e-7, 1.0)
        weak = (strong * sof).sum(1) / sof.sum(1)
    else:
        weak = strong.mean(1)
    bce = torch.nn.functional.binary_cross_entropy
    mse = torch.nn.functional.mse_loss
    loss = bce(strong, kw["y_strong"].double()) + bce(weak, kw["y_weak"].double()) \
        + 0.7 * mse(strong, kw["ema_strong"].double()) + 0.3 * mse(weak, kw["ema_weak"].double())
    loss.backward()
    e_strong = float((saved[0].double() - strong).abs().max())
    e_weak = float((saved[2].double() - weak).abs().max())
    parts = lp.double().sum(0)
    mine = parts[0] / (B * T * C) + parts[1] / (B * C) + 0.7 * parts[2] / (B * T * C) + 0.3 * parts[3] / (B * C)
    e_loss = abs(float(mine) - float(loss)) / abs(float(loss))
    rel = lambda a, r: float((a.double() - r).norm() / r.norm())
    e_dx, e_dw, e_db = rel(dx, x.grad), rel(grad[:2 * C * K].view(2 * C, K), w.grad), rel(grad[2 * C * K:], b.grad)
    print(f"C={C} B={B} T={T} att={attention}: strong {e_strong:.2e} weak {e_weak:.2e} loss {e_loss:.2e} "
          f"dx {e_dx:.2e} dW {e_dw:.2e} db {e_db:.2e}")
    assert e_strong < 4e-6 and e_weak < 4e-6
    assert e_loss < 1e-5
    if T == 1 and attention:
        return                                   # pure cancellation in the attention path: see the module docstring
    assert e_dx < 2e-5 and e_dw < 2e-5 and e_db < 2e-5


@pytest.mark.parametrize("C", [33, 64])
def test_two_passes_give_the_same_bits(C):
    pred, enc, kw = _setup(C, 1, 77, True)
    a, b = _run(pred, enc, kw), _run(pred, enc, kw)
    for u, v in zip(a[0], b[0]):
        assert torch.equal(u, v)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_20_classes_run_what_a_direct_call_runs():
    """Predictor(nclass=20) goes through the same dispatch as any other count: its results equal a direct ops.head_fwd /
    ops.head_bwd call bit for bit (the <20> instances themselves are compared through their code-object metadata)"""
    from bsed_amd import ops
    C, B, T = 20, 1, 77
    pred, enc, kw = _setup(C, B, T, True)
    saved, dx, lp, grad = _run(pred, enc, kw)
    w, b = pred.flat[:2 * C * K], pred.flat[2 * C * K:]
    direct = ops.head_fwd(enc, w, b, B, T, K, C, True)
    for u, v in zip(saved, direct):
        assert torch.equal(u, v)
    dx2, dw_part, db_part, lp2 = ops.head_bwd(enc, w, *direct, B, T, K, C, True, **kw)
    assert torch.equal(dx, dx2) and torch.equal(lp, lp2)
    rows = dw_part.shape[0]
    g2 = torch.zeros_like(grad)
    ops.reduce_partials(dw_part, rows, 1, 2 * C, K, 2 * C, K, g2, 0, K, 1)
    ops.colsum(db_part, rows, 2 * C, 2 * C, g2[2 * C * K:])
    assert torch.equal(grad, g2)
    # the names the roofline table of bench.py reads
    assert ops._head_kernel("fwd", 20) == "head_fwd_kernel<20>" and ops._head_kernel("bwd", 20) == "head_bwd_kernel<20>"
