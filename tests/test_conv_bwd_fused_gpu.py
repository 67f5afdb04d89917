"""The one-pass backward of the HBM-bound 3 x 3 convolutions (csrc/conv_bwd.hip, ops.conv_bwd_fused: BatchNorm backward on
load, weight-gradient slabs and data gradient from one d_y image that never leaves the chip) against
  (a) the two kernels it replaces, in the same build: bsed_wgrad3 writing d_y, then the data-gradient contraction;
  (b) the float64 restatement of tests/conv_bwd_reference.py.
Bits.  With 32 output channels the kernel adds a d_in element's products in igemm3s_kernel's order (k half, tap, lo*hi,
hi*lo, hi*hi) -- the data-gradient kernel of the two-kernel route on these maps -- so d_in is BITWISE the two-kernel
route's.  With 64 output channels it keeps igemm3n_kernel's 32 x 32 x 16 order (chunk, tap, k half, ...) and is bitwise
that form's; the route's default there, igemm3n_kernel's 16 x 16 x 32 form, sums a chunk inside one MFMA, which no
32 x 32 x 16 sequence reproduces: against it only the bound holds.  At the plan's slab count a slab holds the tiles
bsed_wgrad3's slab holds, in its order: dW after the reduction is bitwise the two-kernel route's; at a forced G the slab
boundaries differ and the bound holds.
Bounds (taken over, not new): d_in against another split-fp32 kernel of the same contraction 4e-6 of max|ref|
(tests/test_igemm3n_gpu.py); dW after reduction against the two-kernel route 2e-5 of max|ref| (weight gradients whose slab
boundaries differ, tests/test_igemm_gpu.py); against float64 3e-5 of max|ref| for d_in and 4e-5 relative L2 for dW (the
split-fp32 convolution and weight-gradient tests of tests/test_igemm_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

import conv_bwd_reference as R

pytestmark = pytest.mark.gpu

# (B, H, W, CIN, N, G, instance): H is never a multiple of the tile height (8 rows at 16-wide tiles); B = 3: a tile's ring
# crosses the image boundaries on both sides of image 1
CASES = [
    (3, 5, 16, 16, 32, None, "cbwd3_kernel<2, 1, 1, 1>"),   # compile-time 16 -> 32 form; one tile wide, one ragged tile row
    (3, 9, 32, 32, 64, None, "cbwd3_kernel<5, 2, 1, 0>"),   # compile-time 32 -> 64 form; two tiles wide, 12 tiles, 12 slabs
    (3, 9, 32, 16, 32, 5, "cbwd3_kernel<2, 1, 1, 1>"),      # 12 tiles on 5 workgroups: rounds of 3, 3, 2, 2, 2 tiles
    (3, 9, 16, 32, 64, 1, "cbwd3_kernel<5, 2, 1, 0>"),      # G = 1: one workgroup walks all six tiles
    (3, 21, 8, 32, 64, 4, "cbwd3_kernel<5, 2, 0, 0>"),      # run-time geometry: 8-wide tiles, 6 tiles on 4 workgroups
    (3, 9, 16, 32, 32, 3, "cbwd3_kernel<3, 1, 0, 0>"),      # run-time geometry, 32 -> 32: nine single-tap items
    (3, 9, 32, 8, 64, 5, "cbwd3_kernel<3, 2, 0, 0>"),       # run-time geometry, 8 -> 64: tap pairs, idle input-channel quads
]


@functools.lru_cache(maxsize=None)
def _inputs(B, H, W, CIN, N):
    """seeded inputs (NHWC, on the GPU) and the float64 reference, computed once per shape and never modified"""
    rng = np.random.default_rng(1000 * H + 10 * W + CIN + N)
    inp = rng.standard_normal((B, H, W, CIN)).astype(np.float32)
    g = rng.standard_normal((B, H, W, N)).astype(np.float32)
    y = rng.standard_normal((B, H, W, N)).astype(np.float32)
    coef = rng.uniform(0.5, 1.5, (3, N)).astype(np.float32)
    coef[1] *= 0.1
    coef[2] *= 0.01
    mean = (rng.standard_normal(N) * 0.2).astype(np.float32)
    w = (rng.standard_normal((N, CIN, 3, 3)) / np.sqrt(9 * CIN)).astype(np.float32)
    ref = R.conv_bwd(inp, g, y, coef, mean, w)
    return tuple(torch.from_numpy(a).cuda() for a in (inp, g, y, coef, mean, w)), ref


def _fused(t, B, H, W, G):
    from bsed_amd import ops
    inp, g, y, coef, mean, w = t
    wv = ops.conv3x3_weight(w, W)
    d_in, part, G, KP, NP = ops.conv_bwd_fused(inp, g, y, coef, mean, wv, B, H, W, G=G)
    dw = torch.zeros_like(w)
    ops.reduce_partials(part, G, 9, KP, NP, wv.K, wv.N, dw, wv.s_tap, wv.s_k, wv.s_n, defer=False)
    torch.cuda.synchronize()
    return d_in, dw, part


@pytest.mark.parametrize("B,H,W,CIN,N,G,label", CASES)
def test_one_pass_backward_matches_the_two_kernels_and_float64(B, H, W, CIN, N, G, label):
    from bsed_amd import ops
    t, (dW_ref, din_ref, dy_ref) = _inputs(B, H, W, CIN, N)
    inp, g, y, coef, mean, w = t
    assert ops.conv_bwd_plan(B, H, W, CIN, N)[1].label.decode() == label
    d_in, dw, part = _fused(t, B, H, W, G)

    # (a) the two kernels of the same build, as ops.conv_bn_backward(fused=False) chains them
    wv = ops.conv3x3_weight(w, W)
    dw_a = torch.zeros_like(w)
    din_a = ops.conv_bn_backward(inp, g, y, coef, mean, wv, wv.over(dw_a), B, H, W, mode="bf16x3", fused=False)
    # ... and the data gradient once more on igemm3n's 32 x 32 x 16 form, from the d_y the weight gradient wrote
    dy = torch.empty_like(g)
    ops.wgrad(inp, g, B, H, W, CIN, N, taps=ops.TAPS3x3, mode="bf16x3", bn_y=y, bn_coef=coef, bn_mean=mean, dy_out=dy)
    tv = wv.dgrad()
    ops.set_igemm3n_shape(32)
    try:
        w3 = ops.pack_weight3s(tv.source(), 9, tv.N, tv.s_tap, tv.s_k, tv.s_n, K=tv.K)
        din_32 = ops.igemm3(dy, w3, tv.N, B, H, W, tv.K, tv.taps)[0]
    finally:
        ops.set_igemm3n_shape(0)
    torch.cuda.synchronize()
    dmax, wmax = float(np.abs(din_ref).max()), float(np.abs(dW_ref).max())
    e_a = float((d_in - din_a).abs().max())
    e_w = float((dw - dw_a).abs().max())
    e_d64 = float(np.abs(d_in.cpu().double().numpy() - din_ref).max())
    e_w64 = float(np.linalg.norm(dw.cpu().double().numpy() - dW_ref) / np.linalg.norm(dW_ref))
    print(f"{label} B{B} {H}x{W} {CIN}->{N} G={G}: d_in vs two kernels {e_a / dmax:.2e} (4e-6), bitwise vs 32x32x16 "
          f"{torch.equal(d_in, din_32)} vs route {torch.equal(d_in, din_a)}, dW vs two kernels {e_w / wmax:.2e} (2e-5), d_in vs f64 {e_d64 / dmax:.2e} (3e-5), "
          f"dW vs f64 {e_w64:.2e} (4e-5)")
    if N == 32:
        assert torch.equal(d_in, din_a), float((d_in - din_a).abs().max())     # igemm3s_kernel's order: the route's bits
        assert float((d_in - din_32).abs().max()) <= 4e-6 * dmax
    else:
        assert torch.equal(d_in, din_32), float((d_in - din_32).abs().max())
    if G is None:
        assert torch.equal(dw, dw_a), float((dw - dw_a).abs().max())           # the plan's slabs are bsed_wgrad3's
    assert e_a <= 4e-6 * dmax, e_a
    assert e_w <= 2e-5 * wmax, e_w
    # (b) float64
    assert e_d64 < 3e-5 * dmax, e_d64
    assert e_w64 < 4e-5, e_w64

    # two launches on the same inputs: identical bits, slabs included (rows k >= CIN of a slab are padding nobody reads)
    d_in2, dw2, part2 = _fused(t, B, H, W, G)
    assert torch.equal(d_in, d_in2) and torch.equal(part[:, :, :CIN], part2[:, :, :CIN]) and torch.equal(dw, dw2)


@pytest.mark.parametrize("B,H,W,CIN,N,G,label", [CASES[0], CASES[1], CASES[4]])
def test_poisoned_neighbouring_images_do_not_reach_an_image(B, H, W, CIN, N, G, label):
    """the ring of image 1's first and last tile rows is zero padding: with images 0 and 2 all NaN its d_in keeps its bits"""
    t, _ = _inputs(B, H, W, CIN, N)
    clean = _fused(t, B, H, W, G)[0][1].clone()
    inp, g, y, coef, mean, w = t
    poisoned = []
    for a in (inp, g, y):
        a = a.clone()
        a[0] = float("nan")
        a[2] = float("nan")
        poisoned.append(a)
    d_in = _fused((*poisoned, coef, mean, w), B, H, W, G)[0]
    assert torch.equal(d_in[1], clean)
    assert bool(torch.isnan(d_in[0]).all()) and bool(torch.isnan(d_in[2]).all())   # (they really were poisoned)


def test_network_backward_with_the_route_on_and_off(monkeypatch):
    """CRNN.run_backward at B = 2 on a short clip, the one-pass kernel on (where bsed_conv_bwd_plan recommends it: the 16 -> 32
    block; the 32 -> 64 block stays on its two kernels, which are faster) and off: every parameter gradient under the per-tensor bar of tests/test_crnn_gpu.py (L2 error <=
    2e-4 of the tensor's L2 norm + 1e-7).  Dropout on, the deferred-reduction queue as the train step uses it."""
    from bsed_amd import ops
    from test_crnn_gpu import _mine, _oracle
    from oracle import seeded
    seed, B, T = 23, 2, 64
    x = torch.from_numpy(seeded.db_like_input(seed, B, T)).cuda()
    ocrnn, opred = _oracle(0.5, seed)
    grads, routed, launches = [], [], {True: 0, False: 0}
    one_pass = ops.conv_bwd_fused

    def counted(*a, **kw):
        launches[fused] += 1
        return one_pass(*a, **kw)
    monkeypatch.setattr(ops, "conv_bwd_fused", counted)
    for fused in (True, False):
        crnn, _ = _mine(0.5, ocrnn, opred)
        crnn.fused_conv_bwd = fused
        crnn.train(); crnn.set_seed(77)
        enc, ctx = crnn.run_forward(x, save=True)
        routed = [blk for blk in ctx["blocks"][1:] if blk["y"] is not None and
                  (ops.conv_bwd_plan(B, blk["H"], blk["W"], blk["inp"].shape[-1], blk["co"])[1] or ops.ContractPlan()).G > 0]
        d_enc = torch.sin(torch.arange(enc.numel(), device="cuda", dtype=torch.float32)).view_as(enc) * 1e-2
        crnn.zero_grad()
        with ops.deferred_reductions():
            crnn.run_backward(ctx, d_enc)
        torch.cuda.synchronize()
        grads.append({n: crnn.P(n).grad.detach().double().cpu().clone() for n in crnn._poff})
    assert [b["co"] for b in routed] == [32], [(b["H"], b["W"], b["co"]) for b in routed]     # the test is about that block
    bad = []
    for n, ref in grads[1].items():
        err = float((grads[0][n] - ref).norm())
        if err > 2e-4 * float(ref.norm()) + 1e-7:
            bad.append((n, err, float(ref.norm())))
    assert not bad, bad
    assert launches == {True: 1, False: 0}, launches
    # the routed layer keeps the two-kernel route's bits (d_in and, at the plan's slab count, dW), so the whole backward does
    differing = [n for n in grads[1] if not torch.equal(grads[0][n], grads[1][n])]
    assert not differing, differing
