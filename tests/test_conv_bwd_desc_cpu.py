"""bsed_conv_bwd3 / bsed_conv_bwd_plan without a GPU (csrc/conv_bwd.hip): the shapes the one-pass convolution backward
takes and refuses, the LDS check of its two tile buffers, the pointer and G checks of the entry point -- all answered with
BSED_ERR_ARG and a message before any HIP call -- and the plan's rule for which layers it recommends the kernel."""
import ctypes

import pytest

from bsed_amd import _lib as L
from bsed_amd import ops

ERR_ARG = -1
POINTERS = ("in_", "dy", "part", "bn_y", "bn_coef", "bn_mean", "w3s", "d_in")


def _plan(d):
    p = L.STRUCTS["BsedContractPlan"]()
    rc = L.lib().bsed_conv_bwd_plan(ctypes.byref(d), ctypes.byref(p))
    return rc, p, L.lib().bsed_last_error().decode()


def _armed(NB=2, H=9, W=16, CIN=16, N=32):
    """a descriptor the entry point accepts up to the launch: distinct dummy non-null pointers, never dereferenced here"""
    d = ops._conv_bwd_desc(NB, H, W, CIN, N)
    for i, name in enumerate(POINTERS):
        setattr(d, name, 0x1000 * (i + 1))
    d.G = 1
    return d


@pytest.mark.parametrize("shape,label,G,max_G", [
    ((256, 432, 64, 16, 32), "cbwd3_kernel<2, 1, 1, 1>", 256, 256 * 54 * 4),   # the 16 -> 32 layer of the product network: bsed_wgrad3's slab count
    ((256, 216, 32, 32, 64), "cbwd3_kernel<5, 2, 1, 0>", 0, 256 * 27 * 2),     # the 32 -> 64 layer: taken, but its two kernels are faster
    ((3, 5, 16, 16, 32), "cbwd3_kernel<2, 1, 1, 1>", 3, 3),                    # fewer tiles than CUs: one slab per tile
    ((3, 21, 8, 32, 64), "cbwd3_kernel<5, 2, 0, 0>", 0, 6),                    # run-time geometry (8-wide tiles): taken, not recommended
    ((2, 9, 16, 32, 32), "cbwd3_kernel<3, 1, 0, 0>", 0, 4),                    # 32 -> 32: nine items, three per wave at most
    ((2, 9, 16, 8, 64), "cbwd3_kernel<3, 2, 0, 0>", 0, 4),                     # 8 -> 64: tap pairs x two chunks
    ((2, 130, 2, 16, 32), "cbwd3_kernel<3, 1, 0, 0>", 0, 6),                   # 66 x 4 patch: fits with 32 output channels
])
def test_plan_names_the_instance_and_recommends_only_the_measured_layers(shape, label, G, max_G):
    rc, p, msg = _plan(ops._conv_bwd_desc(*shape))
    assert rc == 0, msg
    assert (p.label.decode(), p.G, p.max_G, p.stats_rows) == (label, G, max_G, 0)
    d, plan = ops.conv_bwd_plan(*shape)
    assert plan is not None and plan.label == p.label and d.CINP == 32 and d.NP == shape[4]


@pytest.mark.parametrize("shape,changes,needle", [
    ((2, 9, 16, 16, 32), dict(act_bf16=1), "fp32 activations only"),
    ((2, 9, 16, 16, 128), {}, "N = NP = 32 or 64"),
    ((2, 9, 16, 16, 48), {}, "N = NP = 32 or 64"),
    ((2, 9, 16, 64, 64), {}, "CIN <= 32"),
    ((2, 9, 16, 6, 32), {}, "multiple of 4"),
    ((2, 9, 16, 16, 32), dict(ntaps=3), "nine taps"),
    ((2, 9, 16, 16, 32), dict(dy_pitch=30), "bad pitch"),
    ((2, 9, 16, 16, 32), dict(din_pitch=8), "bad pitch"),
    ((2, 40, 4, 16, 64), {}, "of LDS"),          # 34 x 6 patch, 64 channels: two buffers of 95 KB
    ((2, 130, 2, 16, 64), {}, "of LDS"),         # 66 x 4 patch
])
def test_refused_shapes_and_lds_overflow(shape, changes, needle):
    d = _armed(*shape)
    for k, v in changes.items():
        setattr(d, k, v)
    rc, _, msg = _plan(d)
    assert rc == ERR_ARG and msg.startswith("bsed_conv_bwd3:") and needle in msg, msg
    assert L.lib().bsed_conv_bwd3(ctypes.byref(d), None) == ERR_ARG      # the entry point answers the same, before any HIP call
    assert L.lib().bsed_last_error().decode() == msg
    if not changes:
        assert ops.conv_bwd_plan(*shape)[1] is None                      # the ops query answers None where the plan refuses


def test_taps_must_be_the_row_major_three_by_three():
    d = _armed()
    d.dh[0], d.dh[8] = d.dh[8], d.dh[0]
    d.dw[0], d.dw[8] = d.dw[8], d.dw[0]
    rc, _, msg = _plan(d)
    assert rc == ERR_ARG and "row-major 3 x 3 taps only" in msg


def test_pointer_and_g_checks_come_before_any_hip_call():
    lib = L.lib()
    rc, p, msg = _plan(_armed())
    assert rc == 0, msg
    null = ops._conv_bwd_desc(2, 9, 16, 16, 32)              # the plan ignores pointers and G
    rc0, p0, _ = _plan(null)
    assert rc0 == 0 and (p0.G, p0.max_G, p0.label) == (p.G, p.max_G, p.label)
    for name in POINTERS:
        d = _armed()
        setattr(d, name, None)
        assert lib.bsed_conv_bwd3(ctypes.byref(d), None) == ERR_ARG, name
        assert lib.bsed_last_error().decode() == "bsed_conv_bwd3: null tensor", name
    for name in ("a_scale", "a_shift", "dy_out"):
        d = _armed()
        setattr(d, name, 0x9000)
        assert lib.bsed_conv_bwd3(ctypes.byref(d), None) == ERR_ARG and b"no input affine and no dy_out" in lib.bsed_last_error()
    for name in ("in_", "dy", "bn_y"):
        d = _armed()
        d.d_in = getattr(d, name)
        assert lib.bsed_conv_bwd3(ctypes.byref(d), None) == ERR_ARG and b"must not alias" in lib.bsed_last_error()
    for G in (0, p.max_G + 1):
        d = _armed()
        d.G = G
        assert lib.bsed_conv_bwd3(ctypes.byref(d), None) == ERR_ARG
        assert lib.bsed_last_error().decode() == f"bsed_conv_bwd3: G ({G}) must be in 1..{p.max_G} tiles"
    assert lib.bsed_conv_bwd_plan(None, ctypes.byref(p)) == ERR_ARG and lib.bsed_conv_bwd_plan(ctypes.byref(null), None) == ERR_ARG
    assert lib.bsed_conv_bwd3(None, None) == ERR_ARG


def test_abi_and_the_untouched_weight_gradient_entries():
    assert L.lib().bsed_abi_version() >= 14
    for name in ("bsed_conv_bwd_plan", "bsed_conv_bwd3"):
        assert name in L.FUNCTIONS
    fields = [n for n, _ in L.STRUCTS["BsedWgradDesc"]._fields_]
    assert fields[-3:] == ["w3s", "d_in", "din_pitch"]
    # bsed_wgrad3 ignores the three new fields: the same plan with them set
    d = _armed(2, 37, 32, 32, 64)
    q = L.STRUCTS["BsedContractPlan"]()
    assert L.lib().bsed_wgrad_plan(ctypes.byref(d), L.CONSTANTS["BSED_CONTRACT_WGRAD3"], ctypes.byref(q)) == 0
    assert q.label.decode() == "wgrad3p_kernel<5, 3, 0>"


def test_conv_bn_backward_refuses_a_forced_one_pass_route_it_cannot_run():
    import torch
    w = torch.zeros(128, 64, 3, 3)
    wv = ops.conv3x3_weight(w, 16)
    t = torch.zeros(1)
    with pytest.raises(L.BsedError, match="does not take this layer"):
        ops.conv_bn_backward(t, t, t, t, t, wv, wv, 2, 9, 16, mode="bf16x3", fused=True)
