"""Every entry point of csrc/disc.hip against the float64 restatement in tests/disc_reference.py, and every layer of
Clip_Discriminator teacher-forced: layer k is fed the GPU's own record of layer k-1 and compared on its own, so the
conditioning of the deep BatchNorms (which sets the bars of tests/test_disc_gpu.py) never enters.

Bounds.  u = 2^-24 (fp32 unit roundoff), ulp(x) = spacing of fp32 at |x|.
  gathers       identity: bitwise.  With (scale, shift): 2 ulp -- the fmaf rounds once, the 0.2 multiply once.
  scatters      <= 4 taps summed then one multiply: 5 ulp of sum|terms| (elements no tap reaches: exactly 0).
  block sums    a fixed-order fp32 sum of n = 256/(C/4) terms per channel: (n + 2) u sum|terms|, the terms taken at the
                level of the scattered |dcol| (times |y| for the second row), which dominates their own rounding too.
  frame head    dx: 3 ulp (dz is three roundings, times w one more).  dw, db: each thread adds r = ceil(M / 256 G) rows,
                the block adds 256 threads in order, dz carries 3 roundings: (r + 256 + 3) u sum|terms|.
  clip head     4 x the error of the same formulas in torch float32 on the CPU against float64, never below 4 ulp of the
                tensor's largest magnitude (see test_disc_head).
  layers        the bars tests/test_igemm_gpu.py holds the contractions to: 1e-5 (fp32 cores) / 4e-5 (split bf16) of max.
Output buffers are NaN before every launch: an element the kernel does not write fails its comparison."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import disc_reference as R
from oracle import crnn_oracle as co
from oracle import seeded

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
SIZES = [(7, 9), (8, 7), (9, 10), (10, 8), (3, 3)]      # odd/odd, even/odd, odd/even, even/even, the minimum
IM2COL_CAP, S2D_CAP, DROP_CAP = 16384, 32768, 16384     # grid caps of the bsed_im2col_s2 / bsed_s2d_fwd / dropout launches


def _mods():
    from bsed_amd import _lib as L
    from bsed_amd import disc, ops
    return L, disc, ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda", dtype=torch.float32)


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _affine(rng, C):
    return (1 + 0.3 * _f32(rng, C)), 0.2 * _f32(rng, C)


@contextlib.contextmanager
def _nan_outputs():
    """disc.py's wrappers allocate their outputs with torch.empty: make those allocations NaN for the launch"""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(NAN) if t.is_floating_point() else t
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def _within(got, ref, bound, what):
    err = np.abs(got - ref)
    bad = ~(err <= bound)                               # NaN fails
    assert not bad.any(), (what, int(bad.sum()), float(np.nanmax(err / np.maximum(bound, 1e-300))))


# ------------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("Hi,Wi", SIZES)
def test_im2col_s2(Hi, Wi):
    L, disc, ops = _mods()
    rng, N = np.random.default_rng(Hi * 16 + Wi), 2
    for C, CP in ((1, 1), (16, 32), (32, 32)):
        x = _f32(rng, N, Hi, Wi, C)
        x[0, 0, 0, 0], x[1, -1, -1, -1] = 0.0, -0.0
        with _nan_outputs():
            col, Ho, Wo, K = disc._im2col(_dev(x), None, None, N, Hi, Wi, C, CP)
        ref = R.im2col_s2(x, CP=CP)
        assert (Ho, Wo, K) == (R.out_size(Hi), R.out_size(Wi), 16 if C == 1 else 9 * CP) and col.shape == ref.shape
        assert torch.equal(col.cpu(), torch.from_numpy(ref.astype(np.float32))), (C, CP)
        if C == 1:
            assert float(col[:, 9:].abs().max()) == 0.0
            continue
        if CP > C:
            assert float(col.view(-1, 9, CP)[:, :, C:].abs().max()) == 0.0
        sc, sh = _affine(rng, C)
        with _nan_outputs():
            col, *_ = disc._im2col(_dev(x), _dev(sc), _dev(sh), N, Hi, Wi, C, CP)
        ref = R.im2col_s2(x, sc, sh, CP)
        _within(_host(col), ref, 2 * _ulp(ref), ("im2col affine", C, CP))
        if CP > C:
            assert float(col.view(-1, 9, CP)[:, :, C:].abs().max()) == 0.0


@pytest.mark.parametrize("Hi,Wi", SIZES)
def test_s2d_fwd(Hi, Wi):
    L, disc, ops = _mods()
    rng, N = np.random.default_rng(Hi * 16 + Wi + 1000), 2
    for C in (4, 64, 128):
        for Ha, Wa in ((Hi, Wi), (Hi + 1, Wi + 2)):
            y = _f32(rng, N, Ha, Wa, C)
            y[:, Hi:], y[:, :, Wi:] = np.nan, np.nan                # poison outside the valid extent
            with _nan_outputs():
                xp, Hp, Wp = disc._s2d_fwd(_dev(y), None, None, N, Ha, Wa, Hi, Wi, C)
            ref = R.s2d_fwd(y, None, None, Hi, Wi)
            assert xp.shape == ref.shape and (Hp, Wp) == ((Hi + 1) // 2, (Wi + 1) // 2)
            assert torch.equal(xp.cpu(), torch.from_numpy(ref.astype(np.float32))), (C, Ha, Wa)
            sc, sh = _affine(rng, C)
            with _nan_outputs():
                xp, *_ = disc._s2d_fwd(_dev(y), _dev(sc), _dev(sh), N, Ha, Wa, Hi, Wi, C)
            ref = R.s2d_fwd(y, sc, sh, Hi, Wi)
            _within(_host(xp), ref, 2 * _ulp(ref), ("s2d_fwd affine", C, Ha, Wa))


def _gather_taps(x, Ho, Wo):
    """(N,Hi,Wi,C) on the GPU -> (N,Ho,Wo,9,C) in the column order (dw*3 + dh), by strided slicing (exact)"""
    return torch.stack([x[:, dh:dh + 2 * Ho - 1:2, dw:dw + 2 * Wo - 1:2, :] for dw in range(3) for dh in range(3)], 3)


@pytest.mark.parametrize("C,N,Ho,Wo", [(1, 1, 545, 481), (4, 2, 43, 5419)])
def test_im2col_s2_grid_stride(C, N, Ho, Wo):
    """the smallest element count above cap x 256 threads: the grid-stride loop wraps (by 1 and by 2 elements)"""
    L, disc, ops = _mods()
    per_pos = 16 if C == 1 else 9 * C // 4
    total = N * Ho * Wo * per_pos
    assert total - per_pos <= IM2COL_CAP * 256 < total               # one output position fewer would fit the grid
    Hi, Wi = 2 * Ho + 2, 2 * Wo + 1                                  # even rows: the last one is never gathered
    x = torch.randn((N, Hi, Wi, C), device="cuda", generator=torch.Generator(device="cuda").manual_seed(C))
    with _nan_outputs():
        col, ho, wo, K = disc._im2col(x, None, None, N, Hi, Wi, C, C)
    assert (ho, wo) == (Ho, Wo)
    ref = _gather_taps(x, Ho, Wo)
    if C == 1:
        assert torch.equal(col[:, :9], ref.reshape(-1, 9)) and float(col[:, 9:].abs().max()) == 0.0
    else:
        assert torch.equal(col, ref.reshape(-1, 9 * C))


def test_s2d_fwd_grid_stride():
    L, disc, ops = _mods()
    N, C, Hp, Wp = 1, 4, 387, 5419
    assert (N * Hp * Wp - 1) * C <= S2D_CAP * 256 < N * Hp * Wp * C  # one X' position fewer would fit the grid
    Hi, Wi, Ha, Wa = 2 * Hp - 1, 2 * Wp, 2 * Hp, 2 * Wp               # odd valid rows on an even allocated grid
    y = torch.randn((N, Ha, Wa, C), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    y[:, Hi:] = NAN
    with _nan_outputs():
        xp, hp, wp = disc._s2d_fwd(y, None, None, N, Ha, Wa, Hi, Wi, C)
    assert (hp, wp) == (Hp, Wp)
    pad = y.clone()
    pad[:, Hi:] = 0
    ref = pad.view(N, Hp, 2, Wp, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, 4 * C)
    assert torch.equal(xp, ref)


# ------------------------------------------------------------------------------------------------ scatters
def _batch_for(Hi, Wi, C):
    """smallest N >= 2 with at least 3 blocks of 256 float4 groups and a partial last one.  Where Hi*Wi*C/4 is itself
    a multiple of 256 (8 x 7 and 10 x 8 at C = 128) no N leaves a partial block: the other sizes cover it for that C."""
    per = Hi * Wi * (C // 4)
    N = 2
    while N * per < 2 * 256 + 1 or ((N * per) % 256 == 0 and per % 256 != 0):
        N += 1
    return N


def _check_bn_scatter(got_g, got_stats, ref, C, what):
    g = _host(got_g)
    _within(g, ref["g"], 5 * _ulp(ref["abs_g"]), (what, "g"))
    assert np.all(g[ref["abs_g"] == 0] == 0), (what, "unreached elements are exactly 0")
    n = 256 // (C // 4)
    st = _host(got_stats)
    assert st.shape == ref["partials"].shape, (what, st.shape)
    _within(st, ref["partials"], (n + 2) * U * ref["abs_partials"], (what, "block partials"))


@pytest.mark.parametrize("Hi,Wi", SIZES)
def test_col2im_s2(Hi, Wi):
    L, disc, ops = _mods()
    rng = np.random.default_rng(Hi * 16 + Wi + 2000)
    Ho, Wo = R.out_size(Hi), R.out_size(Wi)
    # C = 1: the gradient-reverse scale, and the adjoint identity with the GPU's own gather
    N = 2
    x, d = _f32(rng, N, Hi, Wi, 1), _f32(rng, N * Ho * Wo, 16)
    with _nan_outputs():
        out, st = disc._col2im(_dev(d), None, None, None, N, Hi, Wi, 1, 1, out_scale=-0.37)
        col, *_ = disc._im2col(_dev(x), None, None, N, Hi, Wi, 1, 1)
    ref = R.col2im_s2(d, None, None, None, N, Hi, Wi, 1, 1, out_scale=np.float32(-0.37))
    assert st is None
    _within(_host(out), ref["g"], 5 * _ulp(ref["abs_g"]), "col2im C=1")
    if Hi % 2 == 0:
        assert float(out[:, -1].abs().max()) == 0.0                  # no tap reaches the last row of an even size
    if Wi % 2 == 0:
        assert float(out[:, :, -1].abs().max()) == 0.0
    lhs = float((_host(col)[:, :9] * d[:, :9].astype(np.float64)).sum()) * float(np.float32(-0.37))
    rhs = float((x.astype(np.float64) * _host(out)).sum())
    assert abs(lhs - rhs) <= 5 * 2.0 ** -23 * float((np.abs(x) * ref["abs_g"]).sum())
    for C in (4, 8, 16, 32, 64, 128):                                # every value the argument check admits
        CP = 32 if C == 16 else C
        N = _batch_for(Hi, Wi, C)
        assert -(-N * Hi * Wi * (C // 4) // 256) >= 3
        y, sc_sh = _f32(rng, N, Hi, Wi, C), _affine(rng, C)
        d = _f32(rng, N * Ho * Wo, 9, CP)
        d[:, :, C:] = np.nan                                         # pad channels are never read
        d = d.reshape(N * Ho * Wo, 9 * CP)
        with _nan_outputs():
            g, st = disc._col2im(_dev(d), _dev(y), _dev(sc_sh[0]), _dev(sc_sh[1]), N, Hi, Wi, C, CP)
        ref = R.col2im_s2(d, y, sc_sh[0], sc_sh[1], N, Hi, Wi, C, CP)
        _check_bn_scatter(g, st, ref, C, ("col2im", C))
        if Hi % 2 == 0:
            assert float(g[:, -1].abs().max()) == 0.0
        if Wi % 2 == 0:
            assert float(g[:, :, -1].abs().max()) == 0.0
        # adjoint with the GPU results: mask 1 everywhere (y = scale = shift = 1)
        one = torch.ones(C, device="cuda")
        x = _f32(rng, N, Hi, Wi, C)
        with _nan_outputs():
            back, _ = disc._col2im(_dev(d), torch.ones((N, Hi, Wi, C), device="cuda"), one, one, N, Hi, Wi, C, CP)
            col, *_ = disc._im2col(_dev(x), None, None, N, Hi, Wi, C, CP)
        dz = np.nan_to_num(d.astype(np.float64))
        lhs, rhs = float((_host(col) * dz).sum()), float((x.astype(np.float64) * _host(back)).sum())
        absg = R.scatter_s2(np.abs(dz), N, Hi, Wi, C, CP)
        assert abs(lhs - rhs) <= 5 * 2.0 ** -23 * float((np.abs(x) * absg).sum()), ("adjoint", C)


@pytest.mark.parametrize("Hi,Wi", SIZES)
def test_s2d_bwd(Hi, Wi):
    L, disc, ops = _mods()
    rng = np.random.default_rng(Hi * 16 + Wi + 3000)
    Hp, Wp = (Hi + 1) // 2, (Wi + 1) // 2
    for C in (4, 8, 16, 32, 64, 128):
        for Ha, Wa in ((Hi, Wi), (Hi + 1, Wi + 2)):
            N = _batch_for(Ha, Wa, C)
            y, (sc, sh) = _f32(rng, N, Ha, Wa, C), _affine(rng, C)
            y[:, Hi:], y[:, :, Wi:] = np.nan, np.nan                  # never read outside the valid extent
            d = _f32(rng, N, Hp, Wp, 4 * C)
            with _nan_outputs():
                g, st = disc._s2d_bwd(_dev(d), _dev(y), _dev(sc), _dev(sh), N, Ha, Wa, Hi, Wi, C)
            ref = R.s2d_bwd(d, y, sc, sh, Hi, Wi)
            _check_bn_scatter(g, st, ref, C, ("s2d_bwd", C, Ha, Wa))
            assert float(g[:, Hi:].abs().sum()) == 0.0 and float(g[:, :, Wi:].abs().sum()) == 0.0
            # adjoint with the GPU results, mask 1 everywhere
            x = _f32(rng, N, Ha, Wa, C)
            one = torch.ones(C, device="cuda")
            with _nan_outputs():
                back, _ = disc._s2d_bwd(_dev(d), torch.ones((N, Ha, Wa, C), device="cuda"), one, one, N, Ha, Wa, Hi, Wi, C)
                xp, *_ = disc._s2d_fwd(_dev(x), None, None, N, Ha, Wa, Hi, Wi, C)
            lhs = float((_host(xp) * d.astype(np.float64)).sum())
            rhs = float((x.astype(np.float64) * _host(back)).sum())
            assert abs(lhs - rhs) <= 1e-12 * float((np.abs(_host(xp)) * np.abs(d)).sum()), ("adjoint", C, Ha, Wa)


# ------------------------------------------------------------------------------------------------ clip head
def _head_launch(L, y5, sc, sh, wl, bl, N, Ns, H5, W5, train):
    bufs = dict(d=_nan(N), g5=_nan(N, H5, W5, 8), stats=_nan(N, 2, 8), dwl=_nan(N, 2, 16), dbl=_nan(N, 2, 1),
                loss=_nan(N, 2, 1))
    ins = [_dev(v) for v in (y5, sc, sh, wl, bl)]                    # held until the launch is queued
    L.call("bsed_disc_head", *(L.ptr(t) for t in ins), N, Ns, H5, W5, 8, train,
           *(L.ptr(bufs[k]) for k in ("d", "g5", "stats", "dwl", "dbl", "loss")), L.stream())
    return bufs


@pytest.mark.parametrize("H5,W5", [(1, 7), (5, 7), (2, 2), (3, 3), (4, 8)])
def test_disc_head(H5, W5):
    """Bar per output tensor and case: 4 x max|float32 torch (CPU) - float64| of the same formulas (R.disc_head with
    dtype=float32: the yardstick), never below 4 ulp of the tensor's largest magnitude.

    Measured on MI355X, worst over the 12 cases of each shape, relative to the tensor's largest magnitude, as
    yardstick / kernel error (largest error : bar ratio):
      (H5,W5)  d                    loss                 g5                   stats                dwl                  dbl
      (1,7)    1.5e-7/5.6e-8 (0.12) 4.7e-7/5.0e-8 (0.11) 2.3e-7/5.0e-8 (0.12) 2.0e-7/4.5e-8 (0.11) 2.0e-7/4.3e-8 (0.12) 1.9e-7/5.6e-8 (0.12)
      (5,7)    3.1e-7/3.4e-8 (0.11) 2.6e-7/4.6e-8 (0.12) 3.2e-7/5.6e-8 (0.08) 3.1e-7/5.3e-8 (0.09) 3.7e-7/5.4e-8 (0.08) 3.1e-7/3.7e-8 (0.12)
      (2,2)    8.1e-8/3.0e-8 (0.09) 5.9e-6/4.0e-8 (0.11) 1.8e-7/4.8e-8 (0.10) 2.0e-7/4.7e-8 (0.11) 2.1e-7/4.5e-8 (0.12) 1.7e-7/3.3e-8 (0.08)
      (3,3)    1.2e-7/3.6e-8 (0.11) 2.6e-7/5.6e-8 (0.12) 1.8e-7/4.9e-8 (0.10) 1.9e-7/5.0e-8 (0.12) 3.1e-7/4.7e-8 (0.09) 1.8e-7/3.3e-8 (0.11)
      (4,8)    2.7e-7/4.6e-8 (0.12) 4.5e-7/4.9e-8 (0.11) 2.9e-7/5.0e-8 (0.12) 3.3e-7/4.7e-8 (0.08) 2.8e-7/4.4e-8 (0.11) 2.7e-7/4.6e-8 (0.12)
    The kernel's error is the final rounding to fp32 (<= 0.5 ulp): it computes in double.  The fp32 kernel it replaces
    sat at 0.3 .. 0.9 of the bar for N >= 64 but missed it with one clip, where the yardstick is a single draw of the
    CPU evaluation's rounding: (1,7) N=1 Ns=0 stats 8.36e-8 against 7.02e-8 (4 x the yardstick 1.75e-8); (2,2) N=1 d
    9.19e-9 against the 4 ulp floor 7.45e-9 (z = -3.7 carried 1.6 ulp(z), which is 4.9 ulp of d = 0.02), g5, stats and
    dbl following d (ratios 1.21 .. 1.48)."""
    L, disc, ops = _mods()
    rng = np.random.default_rng(H5 * 16 + W5)
    worst, bad = {}, []
    for N in (1, 64, 65, 130):
        y5, (sc, sh) = _f32(rng, N, H5, W5, 8), _affine(rng, 8)
        wl, bl = _f32(rng, 16), _f32(rng, 1)
        for Ns in sorted({0, N // 2, N}):
            r64 = R.disc_head(y5, sc, sh, wl, bl, Ns)
            r32 = R.disc_head(y5, sc, sh, wl, bl, Ns, dtype=torch.float32)
            b = _head_launch(L, y5, sc, sh, wl, bl, N, Ns, H5, W5, 0)
            for k in ("g5", "stats", "dwl", "dbl", "loss"):
                assert bool(torch.isnan(b[k]).all()), ("train = 0 touched", k)
            b0 = b["d"].clone()
            b = _head_launch(L, y5, sc, sh, wl, bl, N, Ns, H5, W5, 1)
            assert torch.equal(b["d"], b0)
            for k in ("loss", "dbl", "dwl"):
                assert float(b[k][:, 1].abs().max()) == 0.0, ("second row", k)
            got = dict(d=b["d"], loss=b["loss"][:, 0, 0], g5=b["g5"], stats=b["stats"], dwl=b["dwl"][:, 0],
                       dbl=b["dbl"][:, 0, 0])
            for k, t in got.items():
                ref = r64[k].numpy()
                mag = float(np.abs(ref).max())
                yard = float(np.abs(r32[k].double().numpy() - ref).max())
                bar = max(4 * yard, 4 * float(_ulp(np.float64(mag))))
                err = float(np.abs(_host(t) - ref).max())
                w = worst.setdefault(k, [0.0, 0.0, 0.0])
                w[0], w[1], w[2] = max(w[0], yard / mag), max(w[1], err / mag), max(w[2], err / bar)
                if not err <= bar:                                        # NaN fails
                    bad.append((k, N, Ns, f"error {err:.3e}", f"bar {bar:.3e}", f"yardstick {yard:.3e}"))
    print(f"disc_head H5={H5} W5={W5}: " + "; ".join(
        f"{k} yardstick {w[0]:.1e} kernel {w[1]:.1e} (of bar {w[2]:.2f})" for k, w in worst.items()))
    assert not bad, bad


@pytest.mark.parametrize("z0,Ns", [(30.0, 0), (-120.0, 5), (-30.0, 5)])
def test_disc_head_saturated(z0, Ns):
    """|z| > 20 with the wrong label on every sample: the loss is BCE's clamp of the kernel's own d, gradients finite"""
    L, disc, ops = _mods()
    rng = np.random.default_rng(3)
    N, H5, W5 = 5, 2, 7
    y5, (sc, sh) = _f32(rng, N, H5, W5, 8), _affine(rng, 8)
    wl, bl = 0.1 * _f32(rng, 16), np.array([z0], np.float32)
    b = _head_launch(L, y5, sc, sh, wl, bl, N, Ns, H5, W5, 1)
    d = b["d"].cpu()
    lab = (torch.arange(N) < Ns).float()
    want = torch.nn.functional.binary_cross_entropy(d, lab, reduction="none")
    got = b["loss"][:, 0, 0].cpu()
    if abs(z0) > 100 or z0 > 0:
        assert bool(((d == 0) | (d == 1)).all()) and torch.equal(got, want) and bool((got == 100).all())
    else:
        assert float((got - want).abs().max()) <= 2 * float(_ulp(np.float64(want.max())))
    for k in ("g5", "stats", "dwl", "dbl"):
        assert bool(torch.isfinite(b[k]).all()), k


# ------------------------------------------------------------------------------------------------ leaky + dropout
def _leaky_launch(L, a, p, stream, seed, d_out=None):
    n = a.numel()
    out = _nan(n)
    if d_out is None:
        L.call("bsed_leaky_dropout_fwd", L.ptr(a), L.ptr(out), n, 0.2, p, stream, seed, L.stream())
    else:
        L.call("bsed_leaky_dropout_bwd", L.ptr(d_out), L.ptr(a), L.ptr(out), n, 0.2, p, stream, seed, L.stream())
    return out


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _leaky_inputs(n, seed):
    rng = np.random.default_rng(seed)
    a = _f32(rng, n)
    a[:4] = [0.0, -0.0, -1.5, 2.0]
    return a, _f32(rng, n)


@pytest.mark.parametrize("n", [4, 1028, (DROP_CAP * 256 + 1) * 4])
def test_leaky_dropout(n):
    L, disc, ops = _mods()
    a, gup = _leaky_inputs(n, 9)
    s02 = np.float32(0.2)
    lk, dlk = np.where(a > 0, a, s02 * a), np.where(a > 0, np.float32(1), s02)
    ad, gd = _dev(a), _dev(gup)
    # p = 0: exact leaky and its derivative (signed zeros included)
    assert np.array_equal(_bits(_leaky_launch(L, ad, 0.0, 401, 5)), lk.view(np.int32))
    assert np.array_equal(_bits(_leaky_launch(L, ad, 0.0, 401, 5, gd)), (gup * dlk).view(np.int32))
    for p, stream, seed in ((0.3, 401, 77), (0.5, 402, (3 << 32) + 1)) if n < 10 ** 6 else ((0.3, 401, 77),):
        mask = R.keep_mask(n, p, stream, seed)
        mul = np.where(mask, np.float32(1) / (np.float32(1) - np.float32(p)), np.float32(0)).astype(np.float32)
        out = _leaky_launch(L, ad, p, stream, seed)
        assert np.array_equal(_bits(out), (lk * mul).view(np.int32)), ("forward bits", p)
        back = _leaky_launch(L, ad, p, stream, seed, gd)
        assert np.array_equal(_bits(back), ((gup * dlk) * mul).view(np.int32)), ("backward uses the forward's mask", p)
        if n < 10 ** 6:
            r_out, r_da, _ = R.leaky_dropout(a, p, stream, seed, gup)
            _within(_host(out), r_out, 2 * _ulp(r_out), "float64 reference, forward")
            _within(_host(back), r_da, 2 * _ulp(r_da), "float64 reference, backward")
        # the mask of an index does not depend on n
        m = min(n, 1028)
        a0, _ = _leaky_inputs(1028, 9)
        assert np.array_equal(a0[:m], a[:m])
        first = _leaky_launch(L, _dev(a0), p, stream, seed)
        assert np.array_equal(_bits(first)[:m], _bits(out[:m].contiguous()))
        # a positive input: the bits of ops.dropout with the same stream and seed
        pos = (ad.abs() + 0.1)[:min(n, 1 << 20)].contiguous()
        assert torch.equal(_leaky_launch(L, pos, p, stream, seed), ops.dropout(pos, p, stream, seed))


# ------------------------------------------------------------------------------------------------ frame head
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
def test_frame_head(M):
    L, disc, ops = _mods()
    rng = np.random.default_rng(M)
    x, w, b, up = _f32(rng, M, 32), 0.3 * _f32(rng, 32), _f32(rng, 1), _f32(rng, M)
    xd, wd, bd, upd = _dev(x), _dev(w), _dev(b), _dev(up)
    d = _nan(M)
    L.call("bsed_frame_head_fwd", L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(d), M, 32, L.stream())
    ref = R.frame_head_fwd(x, w, b)
    zabs = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)) + abs(float(b[0]))
    _within(_host(d), ref, 0.25 * 33 * U * zabs + 4 * _ulp(ref), "frame_head_fwd")
    dk = d.cpu().numpy()                                            # the backward is fed the kernel's own d
    r = R.frame_head_bwd(x, w, dk, up)
    for G in (1, 3, 8):
        dx, part = _nan(M, 32), _nan(G, 2, 32)
        L.call("bsed_frame_head_bwd", L.ptr(xd), L.ptr(wd), L.ptr(d), L.ptr(upd), L.ptr(dx), L.ptr(part), G, M, 32,
               L.stream())
        _within(_host(dx), r["dx"], 3 * _ulp(r["dx"]), ("dx", G))
        ph = _host(part)
        assert np.all(ph[:, 1, 1:] == 0), "row 1 holds db in column 0 and zeros"
        for blk in range(G):
            if blk * 256 >= M:
                assert np.all(ph[blk] == 0), ("a block without rows", G, blk)
        rows = -(-M // (256 * G))
        _within(ph[:, 0].sum(0), r["dw"], (rows + 256 + 3) * U * r["abs_dw"], ("dw", G))
        _within(ph[:, 1, 0].sum(), r["db"], (rows + 256 + 3) * U * r["abs_db"], ("db", G))


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_scalars_are_rejected_before_any_launch():
    """a bad scalar with valid pointers: BSED_CHECK_ARG returns before the launch, the NaN outputs stay NaN"""
    L, disc, ops = _mods()
    a, o, o2 = torch.ones(4096, device="cuda"), _nan(4096), _nan(4096)
    P, S = L.ptr, L.stream()
    bad = [
        ("bsed_im2col_s2", (P(a), None, None, P(o), 1, 2, 9, 4, 4, S)),             # Hi < 3
        ("bsed_im2col_s2", (P(a), None, None, P(o), 1, 7, 9, 3, 4, S)),             # C not 1 or a multiple of 4
        ("bsed_im2col_s2", (P(a), None, None, P(o), 1, 7, 9, 8, 4, S)),             # CP < C
        ("bsed_im2col_s2", (P(a), P(a), None, P(o), 1, 7, 9, 4, 4, S)),             # scale without shift
        ("bsed_col2im_s2", (P(a), P(a), P(a), P(a), P(o), P(o2), 1, 7, 2, 4, 4, 1.0, S)),      # Wi < 3
        ("bsed_col2im_s2", (P(a), P(a), P(a), P(a), P(o), P(o2), 1, 7, 9, 12, 12, 1.0, S)),    # 256 % (C/4) != 0
        ("bsed_col2im_s2", (P(a), P(a), P(a), P(a), P(o), P(o2), 1, 7, 9, 256, 256, 1.0, S)),  # C > 128
        ("bsed_col2im_s2", (P(a), P(a), P(a), P(a), P(o), P(o2), 1, 7, 9, 8, 4, 1.0, S)),      # CP < C
        ("bsed_s2d_fwd", (P(a), None, None, P(o), 1, 6, 9, 7, 9, 4, S)),            # Ha < Hi
        ("bsed_s2d_fwd", (P(a), None, None, P(o), 1, 7, 9, 7, 9, 6, S)),            # C not a multiple of 4
        ("bsed_s2d_fwd", (P(a), None, None, P(o), 0, 7, 9, 7, 9, 4, S)),            # N = 0
        ("bsed_s2d_bwd", (P(a), P(a), P(a), P(a), P(o), P(o2), 1, 7, 8, 7, 9, 4, S)),          # Wa < Wi
        ("bsed_s2d_bwd", (P(a), P(a), P(a), P(a), P(o), P(o2), 1, 7, 9, 7, 9, 256, S)),        # C > 128
        ("bsed_s2d_bwd", (P(a), P(a), P(a), P(a), P(o), P(o2), 1, 7, 9, 7, 9, 24, S)),         # 256 % (C/4) != 0
        ("bsed_disc_head", (P(a), P(a), P(a), P(a), P(a), 2, 3, 1, 7, 8, 1, P(o), P(o2), P(o2), P(o2), P(o2), P(o2), S)),
        ("bsed_disc_head", (P(a), P(a), P(a), P(a), P(a), 2, 1, 1, 7, 4, 1, P(o), P(o2), P(o2), P(o2), P(o2), P(o2), S)),
        ("bsed_disc_head", (P(a), P(a), P(a), P(a), P(a), 2, 1, 1, 1, 8, 1, P(o), P(o2), P(o2), P(o2), P(o2), P(o2), S)),
        ("bsed_disc_head", (P(a), P(a), P(a), P(a), P(a), 2, 1, 0, 7, 8, 1, P(o), P(o2), P(o2), P(o2), P(o2), P(o2), S)),
        ("bsed_leaky_dropout_fwd", (P(a), P(o), 6, 0.2, 0.0, 1, 0, S)),             # n % 4 != 0
        ("bsed_leaky_dropout_fwd", (P(a), P(o), 8, 0.2, 1.0, 1, 0, S)),             # p = 1
        ("bsed_leaky_dropout_bwd", (P(a), P(a), P(o), 8, 0.2, -0.1, 1, 0, S)),      # p < 0
        ("bsed_leaky_dropout_bwd", (P(a), P(a), P(o), 0, 0.2, 0.0, 1, 0, S)),       # n = 0
        ("bsed_frame_head_fwd", (P(a), P(a), P(a), P(o), 4, 16, S)),                # K != 32
        ("bsed_frame_head_fwd", (P(a), P(a), P(a), P(o), 0, 32, S)),                # M = 0
        ("bsed_frame_head_bwd", (P(a), P(a), P(a), P(a), P(o), P(o2), 0, 4, 32, S)),           # G = 0
        ("bsed_frame_head_bwd", (P(a), P(a), P(a), P(a), P(o), P(o2), 4097, 4, 32, S)),        # G > 4096
        ("bsed_frame_head_bwd", (P(a), P(a), P(a), P(a), P(o), P(o2), 1, 4, 8, S)),            # K != 32
    ]
    for name, args in bad:
        with pytest.raises(L.BsedError):
            L.call(name, *args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(o2).all())


# ------------------------------------------------------------------------------------------------ layers, teacher-forced
@functools.lru_cache(maxsize=None)
def _layer_run(mode, T):
    """one train-mode forward of Clip_Discriminator at N = 3, then per layer: the float64 layer fed the GPU's own record
    of the previous layer, and _conv_backward on a seeded dy.  Shared by the forward and the backward test."""
    L, disc, ops = _mods()
    N, coeff = 3, 0.37
    od = co.Clip_Discriminator()
    seeded.load_seeded(od, 11)
    m = disc.Clip_Discriminator()
    m.load_state_dict(od.state_dict())
    m.conv_mode = mode
    m.train()
    m.zero_grad()
    rng = np.random.default_rng(T)
    feat = _f32(rng, N, T, 256)
    _, ctx = m.run_forward(_dev(feat), n_source=2)
    out = []
    for k in range(1, 6):
        l = ctx["layers"][k - 1]
        p = ctx["layers"][k - 2] if k > 1 else None
        cin, cout = R.CH[k - 1], R.CH[k]
        if p is None:
            y_prev, sc, sh = feat[..., None], None, None
        else:
            y_prev = p["y"][:, :l["Hi"], :l["Wi"]].cpu().numpy()
            sc, sh = p["scale"].cpu().numpy(), p["shift"].cpu().numpy()
        y = l["y"].clone()
        dy = torch.from_numpy(_f32(rng, *y.shape)).cuda()            # on the allocated grid, junk outside (Ho, Wo) included
        w = m.P(f"conv_{k}.weight")
        ref = R.conv_s2_layer(y_prev, sc, sh, w.detach().cpu().numpy(), m.P(f"conv_{k}.bias").detach().cpu().numpy(),
                              dy[:, :l["Ho"], :l["Wo"]].cpu().numpy())
        before = w.grad.clone()
        g_prev, stats = m._conv_backward(k, l, p, dy.clone(), N, coeff)
        out.append(dict(l=l, p=p, y=y, ref=ref, dW=_host(w.grad - before), g_prev=g_prev, stats=stats,
                        mean=l["mean"].clone(), invstd=l["invstd"].clone()))
    torch.cuda.synchronize()
    return out, coeff


MODES_T = [(mode, T) for mode in ("fp32", "bf16x3") for T in (63, 67, 99, 101)]


@pytest.mark.parametrize("mode,T", MODES_T)
def test_layer_forward_teacher_forced(mode, T):
    layers, _ = _layer_run(mode, T)
    tol = 1e-5 if mode == "fp32" else 4e-5
    for k, r in enumerate(layers, 1):
        l, y, ref = r["l"], _host(r["y"]), r["ref"]["out"]
        Ho, Wo = l["Ho"], l["Wo"]
        err = float(np.abs(y[:, :Ho, :Wo] - ref).max() / np.abs(ref).max())
        print(f"layer {k} {mode} T={T}: forward error {err:.2e} of max")
        assert err <= tol, (k, err)                                  # NaN fails
        if l["direct"]:
            assert (l["Ha"], l["Wa"]) == (Ho + 1, Wo + 1)
            assert np.all(y[:, Ho:] == 0) and np.all(y[:, :, Wo:] == 0), (k, "allocated row / column is exactly 0")
        else:
            assert y.shape[1:3] == (Ho, Wo)
        v = y[:, :Ho, :Wo].reshape(-1, y.shape[-1])
        assert v.shape[0] == l["M"]
        mean, var = v.mean(0), v.var(0)
        invstd = 1.0 / np.sqrt(var + 1e-5)
        _within(_host(r["mean"]), mean, 1e-5 * np.abs(mean) + 1e-6, (k, "mean"))
        _within(_host(r["invstd"]), invstd, 1e-5 * invstd, (k, "invstd"))


@pytest.mark.parametrize("mode,T", MODES_T)
def test_layer_backward_teacher_forced(mode, T):
    layers, coeff = _layer_run(mode, T)
    tol = 4e-5        # data- and weight-gradient contractions run on the bf16 cores in both modes
    for k, r in enumerate(layers, 1):
        l, p, ref = r["l"], r["p"], r["ref"]
        e_w = float(np.abs(r["dW"] - ref["dW"]).max() / np.abs(ref["dW"]).max())
        g = _host(r["g_prev"])
        if k == 1:
            want = -float(np.float32(coeff)) * ref["dA"]
            assert r["stats"] is None and g.shape == want.shape
            e_g = float(np.abs(g - want).max() / np.abs(want).max())
        else:
            Hi, Wi = l["Hi"], l["Wi"]
            assert g.shape[1:3] == (p["Ha"], p["Wa"])
            want = ref["g_prev"]
            e_g = float(np.abs(g[:, :Hi, :Wi] - want).max() / np.abs(want).max())
            assert np.all(g[:, Hi:] == 0) and np.all(g[:, :, Wi:] == 0), (k, "outside the valid extent")
            sums = _host(r["stats"]).sum(0)
            _within(sums, ref["sums"], tol * ref["abs_sums"], (k, "sum g, sum g*y"))
        print(f"layer {k} {mode} T={T}: dW error {e_w:.2e}, g_prev error {e_g:.2e} of max")
        assert e_w <= tol and e_g <= tol, (k, e_w, e_g)
