"""Host side of the Predictor head for any class count (ABI 8): the bound BSED_HEAD_MAX_CLASSES, the dynamic-LDS sizes
that ``bsed_head_lds_bytes`` reports (the launch code takes them from the same function) and the argument checks of
``bsed_head_fwd`` / ``bsed_head_bwd``, which run before any HIP call.  No GPU in this tier."""
import ctypes

import pytest

from bsed_amd import _lib as L

LDS_LIMIT = 160 * 1024          # bytes of LDS one gfx950 workgroup may use


def test_the_class_bound_is_a_header_constant():
    assert L.CONSTANTS["BSED_HEAD_MAX_CLASSES"] == 64
    assert L.lib().bsed_abi_version() >= 8
    assert "bsed_head_lds_bytes" in L.header_symbols()


@pytest.mark.parametrize("backward", [0, 1])
def test_lds_bytes_fit_the_workgroup_for_every_supported_class_count(backward):
    lib = L.lib()
    for C in range(1, L.CONSTANTS["BSED_HEAD_MAX_CLASSES"] + 1):
        n = lib.bsed_head_lds_bytes(C, backward)
        assert 0 < n <= LDS_LIMIT, (C, backward, n)
    assert lib.bsed_head_lds_bytes(0, backward) < 0
    assert lib.bsed_head_lds_bytes(L.CONSTANTS["BSED_HEAD_MAX_CLASSES"] + 1, backward) < 0


def test_lds_bytes_of_the_20_class_launch_are_unchanged():
    lib = L.lib()
    assert lib.bsed_head_lds_bytes(20, 0) == 89536
    assert lib.bsed_head_lds_bytes(20, 1) == 85520


@pytest.mark.parametrize("C", [0, 65, -3])
def test_class_count_out_of_range_is_refused_before_any_hip_call(C):
    lib = L.lib()
    dummy = 0x1000                                         # non-null, never dereferenced on the host
    rc = lib.bsed_head_fwd(dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, 2, 40, 256, C, 1, None)
    msg = lib.bsed_last_error().decode()
    assert rc == -1, (rc, msg)                             # BSED_ERR_ARG
    assert msg.startswith("bsed_head_fwd:") and "<= 64" in msg and f"nclass={C}" in msg, msg
    d = L.STRUCTS["BsedHeadBwdDesc"]()
    for name in ("x", "w", "strong", "sof_raw", "weak", "den", "dx", "dw_part", "db_part", "loss_part"):
        setattr(d, name, dummy)
    d.B, d.T, d.K, d.C, d.attention = 2, 40, 256, C, 1
    rc = lib.bsed_head_bwd(ctypes.byref(d), None)
    msg = lib.bsed_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith("bsed_head_bwd:") and "<= 64" in msg and f"nclass={C}" in msg, msg
