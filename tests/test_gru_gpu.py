"""GRU recurrences of csrc/gru.hip against the float64 restatement of tests/gru_reference.py: all four kernels
(gru_fwd_kernel<R> / gru_bwd_kernel<R>: "fp32"; gru_fwd_mfma_kernel<SAVE> / gru_bwd_mfma_kernel: "mfma"), element-wise
on out, the four gate planes, dxp, dgh and the bias partials, at the product's sequence lengths and at every edge of the
time loop, the batch tiling and the gate functions.  The backward is always fed the kernel's own forward.

Bars come from the CPU models, never from a kernel: 4 * E_fp32 + tiny for the fp32 register kernels, 4 * (E_fp32 +
E_split) + tiny for the matrix-core kernels (gru_reference.Case.bar).  On the init-weight families ``out`` must also
meet 2e-6 / 2e-5, the bars the README's "logits within 1e-4" rests on.  Every comparison prints a GRUCONF line
(measured error, bar, ratio) before anything is asserted; DESIGN.md section "GRU conformance" keeps the table.

Cases that need their own buffers (one extra batch row of sentinel behind every output, explicit rows_per_wg, NULL
partials) call the C entries through L.lib(); the others go through ops.gru_fwd / ops.gru_bwd.
"""
import pytest
import torch

import gru_reference as R

pytestmark = pytest.mark.gpu

KINDS = ("fp32", "mfma")
CEILING = {"fp32": 2e-6, "mfma": 2e-5}   # out, init-weight families (tests/test_igemm_gpu.py, tests/test_crnn_gpu.py)
SENTINEL = 0x7FC12345                    # a quiet NaN with a payload no kernel produces
ROW = {"out": (256,), "gates": (2, 4, 128), "dxp": (768,), "dgh": (768,)}


def _gpu(c):
    return c.xp.cuda(), c.w_hh.cuda(), c.b_hh.cuda(), c.dout.cuda()


def _report(c, kernel, table):
    bad = []
    for lab, err, bar in table:
        print(f"GRUCONF | {c.family} | {c.B} | {c.T} | {kernel} | {lab} | {err:.2e} | {bar:.2e} | {err / bar:.2f}")
        if not err <= bar:  # NaN fails
            bad.append((lab, err, bar))
    return bad


def _check(c, kind, got, names, tag=""):
    table = c.compare(got, kind == "mfma", names)
    if c.family == "init" and "out" in names:
        err = dict((lab, e) for lab, e, _ in table)["out"]
        table.append(("out (ceiling)", err, CEILING[kind]))
    bad = _report(c, kind + tag, table)
    assert not bad, f"{c.family} B={c.B} T={c.T} {kind}{tag}: (tensor, max |error|, bar) {bad}"


def _run_ops(c, kind):
    """forward + backward through the wrappers -> {name: CPU tensor}, names compared"""
    from bsed_amd import ops
    xp, w_hh, b_hh, dout = _gpu(c)
    mode = "bf16x3" if kind == "mfma" else "fp32"
    out, gates = ops.gru_fwd(xp, w_hh, b_hh, c.B, c.T, save_gates=True, mode=mode)
    dxp, dgh, pih, phh = ops.gru_bwd(dout, out, gates, w_hh, c.B, c.T, mode=mode)
    got = {"out": out, "gates": gates, "dxp": dxp, "dgh": dgh}
    if kind == "mfma":
        assert float(pih[c.B:].abs().max() if pih.shape[0] > c.B else 0.0) == 0.0
        assert float(phh[c.B:].abs().max() if phh.shape[0] > c.B else 0.0) == 0.0
        got.update(part_bih=pih[:c.B], part_bhh=phh[:c.B])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}, tuple(got)


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(t):
    return bool((t.view(torch.int32) == SENTINEL).all())


def _fwd_direct(kind, xp, w_hh, b_hh, B, T, rows=None, save=True):
    """-> (rc, out, gates): buffers of B + 1 batch rows, all sentinel before the call"""
    from bsed_amd import _lib as L
    out = _sentinel(B + 1, T, *ROW["out"])
    gates = _sentinel(B + 1, T, *ROW["gates"]) if save else None
    args = [L.ptr(xp), L.ptr(w_hh), L.ptr(b_hh), L.ptr(out), L.ptr(gates), B, T]
    if kind == "mfma":
        rc = L.lib().bsed_gru_fwd3(*args, L.stream())
    else:
        rc = L.lib().bsed_gru_fwd(*args, rows, L.stream())
    torch.cuda.synchronize()
    return rc, out, gates


def _bwd_direct(kind, dout, out, gates, w_hh, B, T, rows=None, partials=True):
    """-> (rc, dxp, dgh, part_bih, part_bhh): B + 1 batch rows (padded rows + 1 for the partials), all sentinel"""
    from bsed_amd import _lib as L
    dxp, dgh = _sentinel(B + 1, T, 768), _sentinel(B + 1, T, 768)
    pih = phh = None
    args = [L.ptr(dout), L.ptr(out), L.ptr(gates), L.ptr(w_hh), L.ptr(dxp), L.ptr(dgh)]
    if kind == "mfma":
        if partials:
            padded = L.lib().bsed_gru_bwd3_rows(B)
            assert padded == -(-B // 4) * 4
            pih, phh = _sentinel(padded + 1, 768), _sentinel(padded + 1, 768)
        rc = L.lib().bsed_gru_bwd3(*args, L.ptr(pih), L.ptr(phh), B, T, L.stream())
    else:
        rc = L.lib().bsed_gru_bwd(*args, B, T, rows, L.stream())
    torch.cuda.synchronize()
    return rc, dxp, dgh, pih, phh


def _run_direct(c, kind, rows=None):
    """forward + backward on sentinel-backed buffers; asserts nothing was written past batch row B - 1 and that the
    padded rows of the partials are 0.0.  -> ({name: CPU tensor of the B live rows}, names, raw GPU buffers)"""
    xp, w_hh, b_hh, dout = _gpu(c)
    B, T = c.B, c.T
    rc, out, gates = _fwd_direct(kind, xp, w_hh, b_hh, B, T, rows)
    assert rc == 0
    rc, dxp, dgh, pih, phh = _bwd_direct(kind, dout, out[:B], gates[:B], w_hh, B, T, rows)
    assert rc == 0
    raw = {"out": out, "gates": gates, "dxp": dxp, "dgh": dgh}
    for name, t in raw.items():
        assert _untouched(t[B]), f"{name}: batch row {B} (past the end) was written"
    got = {k: v[:B] for k, v in raw.items()}
    if kind == "mfma":
        for name, p in (("part_bih", pih), ("part_bhh", phh)):
            assert _untouched(p[-1]), f"{name}: row {p.shape[0] - 1} (past the padded end) was written"
            if p.shape[0] - 1 > B:
                pad = p[B:-1]
                assert bool((pad == 0.0).all()), f"{name}: padded rows {B}.. are not 0.0"
            got[name] = p[:B]
            raw[name] = p
    return {k: v.cpu() for k, v in got.items()}, tuple(got), raw


# ---------------------------------------------------------------------------------------------------------------------
# accuracy, element-wise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.PRODUCT_T)
@pytest.mark.parametrize("kind", KINDS)
def test_product_length(kind, T):
    """T = 216 (22.05 kHz) and 313 (32 kHz): the lengths every mode of the product runs"""
    c = R.case("init", 5, T)
    got, names = _run_ops(c, kind)
    _check(c, kind, got, names)


@pytest.mark.parametrize("T", R.EDGE_T)
@pytest.mark.parametrize("kind", KINDS)
def test_time_edges(kind, T):
    """T = 1, 2: shorter than the matrix-core kernels' two-step prefetch; odd T: their dummy half-iteration"""
    c = R.case("init", 5, T)
    got, names = _run_ops(c, kind)
    _check(c, kind, got, names)
    if T == 1:
        # h_prev = 0: W_hn h + b_hn is b_hn to the bit, and the gradients have no recurrent term
        ghn = got["gates"][:, 0, :, 3, :]
        assert torch.equal(ghn, c.b_hh[:, 2 * R.H:].expand_as(ghn))
        r, z, n, ghn = (t.double() for t in got["gates"][:, 0].unbind(2))        # (B,2,128) each
        dh = c.dout.double().view(c.B, 2, R.H)
        dn = dh * (1 - z) * (1 - n * n)
        want_x = torch.stack([dn * ghn * r * (1 - r), dh * (0.0 - n) * z * (1 - z), dn], dim=2).view(c.B, 1, 768)
        want_h = torch.stack([dn * ghn * r * (1 - r), dh * (0.0 - n) * z * (1 - z), dn * r], dim=2).view(c.B, 1, 768)
        for name, want in (("dxp", want_x), ("dgh", want_h)):
            err = float((got[name].double() - want).abs().max())
            assert err <= c.bar(name, kind == "mfma"), (name, err)


@pytest.mark.parametrize("B", R.MFMA_B)
def test_batch_remainders_matrix_core(B):
    """every fill of the last 4-row workgroup; idle rows store to the sink, not past row B - 1"""
    c = R.case("init", B, R.REMAINDER_T)
    got, names, _ = _run_direct(c, "mfma")
    _check(c, "mfma", got, names)


def test_rows_per_workgroup_boundary():
    from bsed_amd import ops
    assert ops.gru_rows(128) == 1 and ops.gru_rows(129) == 2


@pytest.mark.parametrize("B", R.FP32_B)
@pytest.mark.parametrize("rows", (1, 2))
def test_batch_remainders_fp32(rows, B):
    """both register-kernel instances at both sides of the ops.gru_rows boundary and with an idle row"""
    c = R.case("init", B, R.REMAINDER_T)
    got, names, _ = _run_direct(c, "fp32", rows)
    _check(c, "fp32", got, names, tag=f"<{rows}>")


def test_null_partials_change_nothing():
    c = R.case("init", 5, R.REMAINDER_T)
    _, _, raw = _run_direct(c, "mfma")
    _, w_hh, _, dout = _gpu(c)
    rc, dxp, dgh, pih, phh = _bwd_direct("mfma", dout, raw["out"][:5], raw["gates"][:5], w_hh, 5, c.T, partials=False)
    assert rc == 0 and pih is None and phh is None
    assert torch.equal(dxp.view(torch.int32), raw["dxp"].view(torch.int32))
    assert torch.equal(dgh.view(torch.int32), raw["dgh"].view(torch.int32))


@pytest.mark.parametrize("T", (63, 313))
@pytest.mark.parametrize("kind", KINDS)
def test_saturated_gates(kind, T):
    """inputs x 30, max |xp| ~ 87: sigmoid_fast = rcp(1 + exp(-x)) passes through exp overflow, tanh_fast cancels"""
    c = R.case("x30", 5, T)
    got, names = _run_ops(c, kind)
    for name in names:
        assert bool(torch.isfinite(got[name]).all()), name
    _check(c, kind, got, names)


@pytest.mark.parametrize("kind", KINDS)
def test_hand_placed_saturation(kind):
    """+-200 in each gate's xp: r / z are 0 or 1, n is +-1 and the gate's own gradient is 0, all to within the bar"""
    c = R.case("placed", 5, 63)
    got, names = _run_ops(c, kind)
    for name in names:
        assert bool(torch.isfinite(got[name]).all()), name
    _check(c, kind, got, names)
    mc = kind == "mfma"
    for t, d, g, k, v in R.placed_index(c.T):
        want = (1.0 if v > 0 else 0.0) if g < 2 else (1.0 if v > 0 else -1.0)
        err = float((got["gates"][:, t, d, g, k].double() - want).abs().max())
        assert err <= c.bar("gates." + R.PLANES[g], mc), (t, d, g, k, err)
        grad = float(got["dxp"][:, t, d * R.G + g * R.H + k].abs().max())
        assert grad <= c.bar("dxp", mc), (t, d, g, k, grad)


@pytest.mark.parametrize("T", (63, 313))
@pytest.mark.parametrize("kind", KINDS)
def test_larger_recurrent_weights(kind, T):
    """w_hh x 4, the largest scale at which the float64 recurrence still agrees with its fp32 restatement"""
    c = R.case("w4", 5, T)
    got, names = _run_ops(c, kind)
    _check(c, kind, got, names)


# ---------------------------------------------------------------------------------------------------------------------
# layout, determinism, contracts: bitwise
# ---------------------------------------------------------------------------------------------------------------------
def _fwd_bwd(kind, xp, w_hh, b_hh, dout, B, T):
    from bsed_amd import ops
    mode = "bf16x3" if kind == "mfma" else "fp32"
    out, gates = ops.gru_fwd(xp, w_hh, b_hh, B, T, save_gates=True, mode=mode)
    dxp, dgh, pih, phh = ops.gru_bwd(dout, out, gates, w_hh, B, T, mode=mode)
    res = [out, gates, dxp, dgh] + ([pih, phh] if kind == "mfma" else [])
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("kind", KINDS)
def test_directions_do_not_mix(kind):
    """an input in one direction's 384 columns only leaves the other direction's half at the zero-input response"""
    c = R.case("init", 5, 63)
    xp, w_hh, b_hh, dout = _gpu(c)
    zero = _fwd_bwd(kind, torch.zeros_like(xp), w_hh, b_hh, dout, c.B, c.T)
    full = _fwd_bwd(kind, xp, w_hh, b_hh, dout, c.B, c.T)
    for d in range(2):
        one = torch.zeros_like(xp)
        one[..., d * R.G:(d + 1) * R.G] = xp[..., d * R.G:(d + 1) * R.G]
        got = _fwd_bwd(kind, one, w_hh, b_hh, dout, c.B, c.T)
        for i, width in enumerate((R.H, None, R.G, R.G)):
            for e, src in ((d, full), (1 - d, zero)):   # own half: as in the full run; other half: zero-input response
                if width is None:
                    assert torch.equal(got[i][:, :, e], src[i][:, :, e])
                else:
                    assert torch.equal(got[i][..., e * width:(e + 1) * width], src[i][..., e * width:(e + 1) * width])
        assert not torch.equal(full[0][..., d * R.H:(d + 1) * R.H], zero[0][..., d * R.H:(d + 1) * R.H])


@pytest.mark.parametrize("T", (63, 64))
@pytest.mark.parametrize("kind", KINDS)
def test_reverse_direction_is_forward_on_reversed_time(kind, T):
    """shared weights, direction 1 fed direction 0's input reversed in time: same kernel, same bits at T-1-t"""
    c = R.case("init", 5, T)
    xp, w_hh, b_hh, dout = _gpu(c)
    xp = torch.cat([xp[..., :R.G], xp[..., :R.G].flip(1)], -1).contiguous()
    dout = torch.cat([dout[..., :R.H], dout[..., :R.H].flip(1)], -1).contiguous()
    w_hh = w_hh[:1].expand(2, -1, -1).contiguous()
    b_hh = b_hh[:1].expand(2, -1).contiguous()
    out, gates, dxp, dgh = _fwd_bwd(kind, xp, w_hh, b_hh, dout, c.B, T)[:4]
    assert torch.equal(out[..., :R.H], out[..., R.H:].flip(1))
    assert torch.equal(gates[:, :, 0], gates[:, :, 1].flip(1))
    assert torch.equal(dxp[..., :R.G], dxp[..., R.G:].flip(1))
    assert torch.equal(dgh[..., :R.G], dgh[..., R.G:].flip(1))
    assert float(out.abs().max()) > 0.1


@pytest.mark.parametrize("family,T", [("init", 313), ("x30", 63)])
@pytest.mark.parametrize("kind", KINDS)
def test_out_does_not_depend_on_saving_gates(kind, family, T):
    from bsed_amd import ops
    c = R.case(family, 5, T)
    xp, w_hh, b_hh, _ = _gpu(c)
    mode = "bf16x3" if kind == "mfma" else "fp32"
    out, gates = ops.gru_fwd(xp, w_hh, b_hh, c.B, T, save_gates=True, mode=mode)
    out_nosave, none = ops.gru_fwd(xp, w_hh, b_hh, c.B, T, save_gates=False, mode=mode)
    assert none is None and gates is not None
    assert torch.equal(out_nosave, out)


@pytest.mark.parametrize("kind", KINDS)
def test_repeatable(kind):
    c = R.case("init", 5, 313)
    xp, w_hh, b_hh, dout = _gpu(c)
    a = _fwd_bwd(kind, xp, w_hh, b_hh, dout, c.B, c.T)
    b = _fwd_bwd(kind, xp, w_hh, b_hh, dout, c.B, c.T)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


ROWS_TRIED = (-1, 0, 1, 2, 3, 4, 5, 8)
ERR_ARG = -1  # BSED_ERR_ARG (csrc/bsed_common.h): refused before any HIP call


@pytest.mark.parametrize("rows", ROWS_TRIED)
@pytest.mark.parametrize("entry", ("bsed_gru_fwd", "bsed_gru_bwd"))
def test_rows_per_wg_contract(entry, rows):
    """Every rows_per_wg the C entry accepts gives reference-correct results on all B rows; every other value returns
    BSED_ERR_ARG, names the entry in bsed_last_error and launches nothing (the outputs keep their sentinel)."""
    from bsed_amd import _lib as L
    c = R.case("init", 8, 5)
    xp, w_hh, b_hh, dout = _gpu(c)
    B, T = c.B, c.T
    # another entry's error first, so that the message read below is this call's
    assert L.lib().bsed_gru_fwd3(None, None, None, None, None, B, T, L.stream()) == ERR_ARG
    if entry == "bsed_gru_fwd":
        rc, out, gates = _fwd_direct("fp32", xp, w_hh, b_hh, B, T, rows)
        outputs = {"out": out, "gates": gates}
    else:
        rc0, out, gates = _fwd_direct("fp32", xp, w_hh, b_hh, B, T, 1)
        assert rc0 == 0
        assert L.lib().bsed_gru_fwd3(None, None, None, None, None, B, T, L.stream()) == ERR_ARG
        rc, dxp, dgh, _, _ = _bwd_direct("fp32", dout, out[:B], gates[:B], w_hh, B, T, rows)
        outputs = {"dxp": dxp, "dgh": dgh}
    if rc != 0:
        assert rc == ERR_ARG
        msg = L.lib().bsed_last_error().decode()
        assert msg.startswith(entry + ":"), msg
        for name, t in outputs.items():
            assert _untouched(t), f"{name} was written by a refused call"
        return
    assert rows > 0
    for name, t in outputs.items():
        assert _untouched(t[B]), f"{name}: batch row {B} (past the end) was written"
    got = {k: v[:B].cpu() for k, v in outputs.items()}
    _check(c, "fp32", got, tuple(got), tag=f"<{rows}>")
