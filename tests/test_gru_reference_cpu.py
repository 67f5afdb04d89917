"""The float64 GRU restatement of tests/gru_reference.py against torch.nn.GRU in float64, and the conditioning of every
input family tests/test_gru_gpu.py runs: a bar derived from the CPU models means something only where the float64
recurrence agrees with itself."""
import pytest
import torch

import gru_reference as R


def _nn_gru_double(xp, w_hh, b_hh, dout):
    """nn.GRU(768 -> 128, bidirectional) in float64 fed xp through identity input weights: direction d sees columns
    d*384..d*384+383 of xp and adds a zero b_ih, so it consumes exactly the kernels' xp"""
    B, T, _ = xp.shape
    gru = torch.nn.GRU(2 * R.G, R.H, bidirectional=True, batch_first=True).double()
    eye = torch.eye(2 * R.G, dtype=torch.float64)
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")):
            getattr(gru, "weight_ih_l0" + sfx).copy_(eye[d * R.G:(d + 1) * R.G])
            getattr(gru, "weight_hh_l0" + sfx).copy_(w_hh[d])
            getattr(gru, "bias_ih_l0" + sfx).zero_()
            getattr(gru, "bias_hh_l0" + sfx).copy_(b_hh[d])
    x = xp.double().requires_grad_()
    out, _ = gru(x)
    out.backward(dout.double())
    return (out.detach(), x.grad, torch.cat([gru.bias_ih_l0.grad, gru.bias_ih_l0_reverse.grad]),
            torch.cat([gru.bias_hh_l0.grad, gru.bias_hh_l0_reverse.grad]))


@pytest.mark.parametrize("B,T", [(3, 17), (2, 313)])
def test_float64_restatement_equals_nn_gru(B, T):
    xp, w_hh, b_hh, dout = R.make_inputs("init", B, T, seed=11)
    ref = R.reference(xp, w_hh, b_hh, dout)
    out, dx, db_ih, db_hh = _nn_gru_double(xp, w_hh, b_hh, dout)
    errs = {"out": ref["out"] - out, "dxp": ref["dxp"] - dx,
            "db_ih": ref["part_bih"].sum(0) - db_ih, "db_hh": ref["part_bhh"].sum(0) - db_hh}
    for name, e in errs.items():
        e = float(e.abs().max())
        print(f"restatement vs nn.GRU float64 B={B} T={T} {name}: {e:.2e}")
        assert e <= 1e-12, (name, e)
    # the saved gates are what they claim to be: out recomputed from them, step by step
    g = ref["gates"]
    for d in range(2):
        h = ref["out"][..., d * R.H:(d + 1) * R.H]
        hp = torch.zeros_like(h)
        if d == 0:
            hp[:, 1:] = h[:, :-1]
        else:
            hp[:, :-1] = h[:, 1:]
        r, z, n, ghn = g[:, :, d].unbind(2)
        assert float(((1 - z) * n + z * hp - h).abs().max()) <= 1e-15
        xn = xp.double()[..., d * R.G + 2 * R.H:(d + 1) * R.G]
        assert float((torch.tanh(xn + r * ghn) - n).abs().max()) <= 1e-15
        gh_n = hp @ w_hh[d, 2 * R.H:].double().t() + b_hh[d, 2 * R.H:].double()
        assert float((gh_n - ghn).abs().max()) <= 1e-14


@pytest.mark.parametrize("family,B,T", [("init", 3, 17), ("w4", 2, 63), ("x30", 2, 63), ("placed", 2, 17)])
def test_hand_written_bptt_equals_autograd(family, B, T):
    """the error models share _forward / _backward with model("f64"): pinning that to autograd pins their formulas"""
    xp, w_hh, b_hh, dout = R.make_inputs(family, B, T, seed=12)
    ref = R.reference(xp, w_hh, b_hh, dout)
    f64 = R.model("f64", xp, w_hh, b_hh, dout)
    for name in R.TENSORS:
        assert float((f64[name] - ref[name]).abs().max()) <= 1e-12, name
    # dgh differs from dxp in the n gate only, by the factor r
    for d in range(2):
        sl = slice(d * R.G, d * R.G + 2 * R.H)
        assert torch.equal(ref["dxp"][..., sl], ref["dgh"][..., sl])


def test_split_product_is_three_bf16_terms():
    torch.manual_seed(0)
    w = torch.randn(2, R.G, R.H, dtype=torch.float64)
    h = torch.randn(2, 3, R.H, dtype=torch.float64)
    mm = R._Split(w)
    hi, lo = R._bf16_split(h)
    assert torch.equal(hi.float().bfloat16().double(), hi) and torch.equal(lo.float().bfloat16().double(), lo)
    assert float((h.float().double() - hi - lo).abs().max()) <= 2.0 ** -16 * float(h.abs().max())
    want = torch.einsum("dbk,dgk->dbg", hi, mm.hi) + torch.einsum("dbk,dgk->dbg", lo, mm.hi) \
        + torch.einsum("dbk,dgk->dbg", hi, mm.lo)
    assert float((mm.fwd(h) - want).abs().max()) <= 1e-12
    exact = torch.einsum("dbk,dgk->dbg", h, w)
    assert 0.0 < float((mm.fwd(h) - exact).abs().max()) <= 2.0 ** -14 * 128 ** 0.5 * 4.0 * 4.0
    dg = torch.randn(2, 3, R.G, dtype=torch.float64)
    ghi, glo = R._bf16_split(dg)
    want = torch.einsum("dbg,dgk->dbk", ghi, mm.hi) + torch.einsum("dbg,dgk->dbk", glo, mm.hi) \
        + torch.einsum("dbg,dgk->dbk", ghi, mm.lo)
    assert float((mm.bwd(dg) - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("family,B,T", R.CASES)
def test_family_is_well_conditioned(family, B, T):
    """Condition for a GPU case: fp32 floor vs float64 <= 2e-5 absolute on ``out``.  The split model must stay inside
    the 1e-4 the README promises for the logits, which rest on these kernels' outputs.  Everything stays finite."""
    c = R.case(family, B, T)
    for res in (c.ref, c.fp32, c.split):
        for name in R.TENSORS:
            assert bool(torch.isfinite(res[name]).all()), name
    e32, esp = c.model_error("fp32", "out"), c.model_error("split", "out")
    print(f"{family} B={B} T={T}: fp32 floor {e32:.2e} split model {esp:.2e} max|xp| {float(c.xp.abs().max()):.1f}")
    assert e32 <= 2e-5
    assert esp <= 1e-4
    for lab in c.labels():
        assert c.bar(lab, True) >= c.bar(lab, False) > 0.0


def test_saturated_families_saturate():
    c = R.case("x30", 5, 313)
    assert float(c.xp.abs().max()) > 60.0
    r, z = c.ref["gates"][..., 0, :], c.ref["gates"][..., 1, :]
    assert float(((r < 1e-6) | (r > 1 - 1e-6)).double().mean()) > 0.3
    assert float(((z < 1e-6) | (z > 1 - 1e-6)).double().mean()) > 0.3
    c = R.case("placed", 5, 63)
    for t, d, g, k, v in R.placed_index(c.T):
        want = (1.0 if v > 0 else 0.0) if g < 2 else (1.0 if v > 0 else -1.0)
        assert torch.all((c.ref["gates"][:, t, d, g, k] - want).abs() <= 1e-30)
        assert torch.all(c.ref["dxp"][:, t, d * R.G + g * R.H + k].abs() <= 1e-30)
