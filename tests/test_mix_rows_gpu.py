"""``bsed_mix_rows`` / ``ops.mix_rows`` on the GPU, bit for bit against ``ict_reference.mix`` (which
test_ict_reference_cpu.py holds against the reference's torch and numpy expressions): both load widths, several jobs in
one launch, a launch larger than its grid, perm entries out of range, and nothing written outside ``out``."""
import ctypes

import numpy as np
import pytest
import torch

import ict_reference as R
from bsed_amd import _lib as L
from bsed_amd import ops

pytestmark = pytest.mark.gpu

# the step's shapes in small: a mel batch, weak targets (C = 20: 16-byte rows), nclass = 3 rows and one odd row (4-byte
# path), strong targets
SHAPES = [(4, 1, 128, 128), (2, 20), (3, 3), (1, 7), (6, 64, 20)]
LAMS = [0.0, 1.0, 0.3137]


def _perm(kind, n):
    if kind == "identity" or n == 1:
        return np.arange(n)
    p = np.roll(np.arange(n), 1)               # one cycle ...
    if n > 2:
        p[[0, 1]] = p[[1, 0]]                  # ... cut so that clip 0 stays in place: [0, n-1, 1, 2, ...]
    assert sorted(p) == list(range(n)) and (kind != "fixed point" or n < 3 or p[0] == 0)
    return p


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(17)
    return [(rng.normal(-40, 20, s)).astype(np.float32) for s in SHAPES]


def _same_bits(got, want):
    return np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.parametrize("kind", ["identity", "fixed point"])
@pytest.mark.parametrize("lam", LAMS)
def test_five_jobs_in_one_launch_match_the_reference_bitwise(inputs, lam, kind):
    lams = [lam, 1.0 - lam if lam in (0.0, 1.0) else 0.3137, lam, 0.5, lam]       # jobs carry their own weights
    perms = [_perm(kind, x.shape[0]) for x in inputs]
    jobs = [(torch.from_numpy(x).cuda(), torch.from_numpy(p.astype(np.int32)).cuda(), l)
            for x, p, l in zip(inputs, perms, lams)]
    outs = ops.mix_rows(jobs)
    again = ops.mix_rows(jobs)
    assert len(outs) == 5
    for x, p, l, o, o2, (xin, _, _) in zip(inputs, perms, lams, outs, again, jobs):
        assert o.shape == x.shape and o.dtype == torch.float32 and o.data_ptr() != xin.data_ptr()
        assert _same_bits(o, R.mix(x, p, l)), (x.shape, l)
        assert torch.equal(o.view(torch.int32), o2.view(torch.int32))              # two launches: identical bits
        assert np.array_equal(xin.cpu().numpy(), x)                                # the input is left alone
        if l == 1.0:
            assert _same_bits(o, x)


@pytest.mark.parametrize("lam", LAMS)
def test_a_base_4_bytes_into_a_buffer_gives_the_bits_of_the_aligned_one(inputs, lam):
    """rows of 20 floats at a 16-byte base take 16-byte loads; the same rows one float further on take 4-byte ones"""
    x = inputs[4].reshape(6, -1)
    p = _perm("fixed point", 6)
    buf = torch.zeros(x.size + 1, device="cuda")
    shifted = buf[1:].view(x.shape)
    shifted.copy_(torch.from_numpy(x))
    aligned = torch.from_numpy(x).cuda()
    assert shifted.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0 and shifted.is_contiguous()
    pd = torch.from_numpy(p.astype(np.int32)).cuda()
    o_shift, o_al = ops.mix_rows([(shifted, pd, lam), (aligned, pd, lam)])
    assert torch.equal(o_shift.view(torch.int32), o_al.view(torch.int32)) and _same_bits(o_al, R.mix(x, p, lam))


def test_a_launch_larger_than_its_grid():
    """(8, 157 * 128 * 8) is 1256 tiles of 256 16-byte chunks; with (24, 157 * 128 * 8) behind it the launch has 5024
    against a grid of 2048 workgroups, which then stride"""
    rng = np.random.default_rng(3)
    xs = [rng.normal(0, 1, (n, 157 * 128 * 8)).astype(np.float32) for n in (8, 24)]
    ps = [rng.permutation(n) for n in (8, 24)]
    outs = ops.mix_rows([(torch.from_numpy(x).cuda(), torch.from_numpy(p.astype(np.int32)).cuda(), 0.3137)
                         for x, p in zip(xs, ps)])
    for x, p, o in zip(xs, ps, outs):
        assert _same_bits(o, R.mix(x, p, 0.3137))


def _raw(x, perm, lam, out):
    """one job through the C entry point, into a caller-owned ``out``"""
    arr = lambda t, v: (t * 1)(v)
    L.call("bsed_mix_rows", arr(ctypes.c_void_p, x.data_ptr()), arr(ctypes.c_void_p, out.data_ptr()),
           arr(ctypes.c_void_p, perm.data_ptr()), arr(ctypes.c_float, lam), arr(ctypes.c_float, 1.0 - lam),
           arr(ctypes.c_int, x.shape[0]), arr(ctypes.c_long, x.numel() // x.shape[0]), 1, L.stream())


@pytest.mark.parametrize("shape,lead", [((2, 20), 4), ((6, 64, 20), 4), ((3, 3), 4), ((1, 7), 4), ((2, 20), 5), ((3, 3), 1)])
def test_the_words_around_out_are_untouched(shape, lead):
    """``out`` sits between canary words (lead of them in front: a multiple of 4 keeps it on a 16-byte boundary)"""
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, shape).astype(np.float32)
    p = _perm("fixed point", shape[0])
    canary = 0x7FC0BEEF                                                            # a NaN pattern no mix produces
    buf = torch.full((lead + x.size + 64,), canary, dtype=torch.int32, device="cuda")
    out = buf[lead:lead + x.size].view(torch.float32).view(shape)
    _raw(torch.from_numpy(x).cuda(), torch.from_numpy(p.astype(np.int32)).cuda(), 0.3137, out)
    assert _same_bits(out, R.mix(x, p, 0.3137))
    assert bool((buf[:lead] == canary).all()) and bool((buf[lead + x.size:] == canary).all())


def test_perm_entries_out_of_range_are_clamped():
    rng = np.random.default_rng(9)
    for shape in ((3, 3), (3, 64)):
        x = rng.normal(0, 1, shape).astype(np.float32)
        bad = np.array([5, -1, 1], dtype=np.int32)
        (o,) = ops.mix_rows([(torch.from_numpy(x).cuda(), torch.from_numpy(bad).cuda(), 0.25)])
        assert _same_bits(o, R.mix(x, [2, 0, 1], 0.25))


def test_wrapper_refuses_what_it_can_see():
    x = torch.zeros(4, 20, device="cuda")
    with pytest.raises(L.BsedError, match="perm entries"):
        ops.mix_rows([(x, torch.zeros(3, dtype=torch.int32, device="cuda"), 0.5)])
    with pytest.raises(L.BsedError, match="dtype"):
        ops.mix_rows([(x, torch.zeros(4, dtype=torch.int64, device="cuda"), 0.5)])
    with pytest.raises(L.BsedError, match="jobs"):
        ops.mix_rows([(x, torch.zeros(4, dtype=torch.int32, device="cuda"), 0.5)] * 9)
