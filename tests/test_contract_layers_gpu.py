"""ops.contract and ops.weight_grad on a WeightView launch the route ops.contract_route names and nothing else, and give
bit for bit what the low-level functions (pack_weight* + igemm*, wgrad + reduce_partials) give when they are handed
the weight's strides, taps and element offset written out as literals.

Forward, data gradient and weight gradient of five layer shapes, each in fp32 and bf16x3, at B = 2, H = 8: the tile is as
tall as the map at W = 16 and taller at every narrower width (every tile partial).  The 16 -> 32 convolution takes the
LDS-resident route both ways, the 128 -> 128 one on a width-1 map is the three-tap centre-column stencil whose gradient
lands at element offset 1, the two linear layers are the GRU's input projection (10 rows) and Frame_Discriminator's
second layer.  Gradients are accumulated into non-zero tensors, the same on both sides.  The weight gradient with
BatchNorm's backward applied on load, and the bf16-activation instance (mode "bf16"), run once, on the 32 -> 64 shape.

The wrappers allocate their outputs themselves, so no output can be poisoned beforehand."""
import functools

import pytest
import torch

from test_graph_step_gpu import _recorded_launches

pytestmark = pytest.mark.gpu

B, H = 2, 8
TAPS3x1 = [(-1, 0), (0, 0), (1, 0)]
TAP1 = [(0, 0)]
# id: (NB, H, W, weight shape, K, N, taps, element offset, s_tap, s_k, s_n, route forward, route dgrad [bf16x3 / bf16])
CASES = {
    "conv16_32_w16": (B, H, 16, (32, 16, 3, 3), 16, 32, None, 0, 1, 9, 16 * 9, "igemm3s", "igemm3s"),
    "conv32_64_w8": (B, H, 8, (64, 32, 3, 3), 32, 64, None, 0, 1, 9, 32 * 9, "igemm3", "igemm3"),
    "conv128_128_w1": (B, H, 1, (128, 128, 3, 3), 128, 128, TAPS3x1, 1, 3, 9, 128 * 9, "igemm3", "igemm3"),
    "linear128_768_m10": (1, 10, 1, (768, 128), 128, 768, TAP1, 0, 0, 1, 128, "igemm3", "igemm3"),
    "linear128_32": (1, 10, 1, (32, 128), 128, 32, TAP1, 0, 0, 1, 128, "igemm3", "igemm3"),
}


def _view(name, w):
    from bsed_amd import ops
    return ops.conv3x3_weight(w, CASES[name][2]) if name.startswith("conv") else ops.linear_weight(w)


def _route_kernels(route, epilogue):
    """the entry points of a route's pack + contraction pair (bsed_igemm with its epilogue)"""
    from bsed_amd import ops
    if route == "igemm3":
        return ({"bsed_pack_weight3s", "bsed_igemm3n"} if ops.igemm3_nsplit() else {"bsed_pack_weight3", "bsed_igemm3"})
    return {"igemm3s": {"bsed_pack_weight3s", "bsed_igemm3s"}, "igemm": {"bsed_pack_weight", f"bsed_igemm:{epilogue}"}}[route]


@functools.lru_cache(maxsize=None)
def _inputs(name, dtype=torch.float32):
    NB, Hh, W, wshape, K, N = CASES[name][:6]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(NB, Hh, W, K, generator=g).to(dtype).cuda()
    dy = torch.randn(NB, Hh, W, N, generator=g).to(dtype).cuda()
    w = (torch.randn(wshape, generator=g) / K ** 0.5).cuda()
    bias = (torch.randn(N, generator=g) * 0.1).cuda()
    dw0 = torch.randn(wshape, generator=g).cuda()
    return x, dy, w, bias, dw0


def _contract_by_hand(route, inp, src, taps, CIN, N, s_tap, s_k, s_n, NB, Hh, W, bias, epilogue):
    from bsed_amd import ops
    if route == "igemm3s":
        wtab = ops.pack_weight3s(src, len(taps), N, s_tap, s_k, s_n, K=CIN)
        return ops.igemm3s(inp, wtab, N, NB, Hh, W, taps, bias=bias, epilogue=epilogue)
    if route == "igemm3":
        w3 = ops.pack_weight3(src, len(taps), CIN, N, s_tap, s_k, s_n)
        return ops.igemm3(inp, w3, N, NB, Hh, W, CIN, taps, bias=bias, epilogue=epilogue)
    assert route == "igemm"
    wpk = ops.pack_weight(src, len(taps), CIN, N, s_tap, s_k, s_n)
    return ops.igemm(inp, wpk, N, NB, Hh, W, CIN, taps=taps, bias=bias, epilogue=epilogue)


def _assert_same(got, want):
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _check_forward_and_dgrad(name, mode, dtype=torch.float32):
    from bsed_amd import ops
    NB, Hh, W, _, K, N, taps, off, s_tap, s_k, s_n, r_fwd, r_dgrad = CASES[name]
    taps = taps or ops.TAPS3x3
    x, dy, w, bias, _ = _inputs(name, dtype)
    wv = _view(name, w)
    src = w.view(-1)[off:] if off else w
    epi = ops.EPI_STATS if name.startswith("conv") else ops.EPI_PLAIN      # a train-mode block; a biased projection
    route = ops.contract_route("forward", K, N, W, len(taps), mode)
    assert route == ("igemm" if mode == "fp32" else r_fwd)
    with _recorded_launches() as names:
        got = ops.contract(x, wv, NB, Hh, W, mode=mode, bias=bias, epilogue=epi)
    assert names == _route_kernels(route, epi), sorted(names)
    with _recorded_launches() as hand_names:
        want = _contract_by_hand(route, x, src, taps, K, N, s_tap, s_k, s_n, NB, Hh, W, bias, epi)
    assert names == hand_names
    assert got[0].shape == (NB, Hh, W, N) and (got[1] is not None) == (epi == ops.EPI_STATS)
    _assert_same(got, want)
    # data gradient: the transposed weight (s_k and s_n swapped) at the mirrored taps, CIN and N swapped
    route = ops.contract_route("dgrad", N, K, W, len(taps), mode)
    assert route == ("igemm" if mode == "fp32" else r_dgrad)
    with _recorded_launches() as names:
        got = ops.contract(dy, wv, NB, Hh, W, mode=mode, direction="dgrad")
    assert names == _route_kernels(route, ops.EPI_PLAIN), sorted(names)
    with _recorded_launches() as hand_names:
        want = _contract_by_hand(route, dy, src, [(-a, -b) for a, b in taps], N, K, s_tap, s_n, s_k, NB, Hh, W, None,
                                 ops.EPI_PLAIN)
    assert names == hand_names
    assert got[0].shape == (NB, Hh, W, K) and got[1] is None
    _assert_same(got, want)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", list(CASES))
def test_contract_runs_its_route_and_equals_it_bitwise(name, mode):
    _check_forward_and_dgrad(name, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", list(CASES))
def test_weight_grad_equals_wgrad_and_reduce_partials_bitwise(name, mode):
    from bsed_amd import ops
    NB, Hh, W, _, K, N, taps, off, s_tap, s_k, s_n = CASES[name][:11]
    taps = taps or ops.TAPS3x3
    x, dy, w, _, dw0 = _inputs(name)
    dw, dw_hand = dw0.clone(), dw0.clone()
    with _recorded_launches() as names:
        assert ops.weight_grad(x, dy, _view(name, w).over(dw), NB, Hh, W, mode=mode) is None
    assert names == {"bsed_wgrad" if mode == "fp32" else "bsed_wgrad3", "bsed_reduce_partials"}, sorted(names)
    with _recorded_launches() as hand_names:
        part, G, KP, NP = ops.wgrad(x, dy, NB, Hh, W, K, N, taps=taps, mode=mode)
        ops.reduce_partials(part, G, len(taps), KP, NP, K, N, dw_hand, s_tap, s_k, s_n, dst_offset=off)
    assert names == hand_names
    assert torch.equal(dw, dw_hand) and not torch.equal(dw, dw0)
    if off:   # the width-1 stencil: only the centre column of the 3x3 weight receives a gradient
        assert torch.equal(dw[..., 0], dw0[..., 0]) and torch.equal(dw[..., 2], dw0[..., 2])
        assert not torch.equal(dw[..., 1], dw0[..., 1])


def _check_bn_on_load(mode, dtype):
    from bsed_amd import ops
    name = "conv32_64_w8"
    NB, Hh, W, _, K, N = CASES[name][:6]
    x, g, w, _, dw0 = _inputs(name, dtype)
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(NB, Hh, W, N, generator=gen).to(dtype).cuda()
    coef = (torch.rand(3, N, generator=gen) + 0.5).cuda()
    mean = (torch.randn(N, generator=gen) * 0.2).cuda()
    dw, dw_hand = dw0.clone(), dw0.clone()
    dy, dy_hand = torch.empty_like(g), torch.empty_like(g)
    with _recorded_launches() as names:
        ops.weight_grad(x, g, ops.conv3x3_weight(w, W).over(dw), NB, Hh, W, mode=mode, bn_y=y, bn_coef=coef, bn_mean=mean,
                        dy_out=dy)
    assert names == {"bsed_wgrad3", "bsed_reduce_partials"}, sorted(names)
    with _recorded_launches() as hand_names:
        part, G, KP, NP = ops.wgrad(x, g, NB, Hh, W, K, N, taps=ops.TAPS3x3, mode=mode, bn_y=y, bn_coef=coef,
                                    bn_mean=mean, dy_out=dy_hand)
        ops.reduce_partials(part, G, 9, KP, NP, K, N, dw_hand, 1, 9, K * 9)
    assert names == hand_names
    assert torch.equal(dw, dw_hand) and not torch.equal(dw, dw0)
    assert dy.dtype == dtype and torch.equal(dy, dy_hand)


def test_weight_grad_with_batchnorm_backward_on_load():
    _check_bn_on_load("bf16x3", torch.float32)


def test_bf16_activation_instance(monkeypatch):
    """mode "bf16": bf16 activation and gradient tensors (fp32 weights and weight gradients) on the N-split kernel"""
    monkeypatch.setenv("BSED_IGEMM3N", "1")
    _check_forward_and_dgrad("conv32_64_w8", "bf16", torch.bfloat16)
    _check_bn_on_load("bf16", torch.bfloat16)


# ---- BsedContractPlan sizes exactly what the kernels write: the C ABI called directly, one guard row / slab beyond the plan ----
GH, GW = 9, 16      # one image, tile 8 x 16: two tile rows, the second partial
PLAN_CASES = [(k, cin, n, abf) for k, cin, ns, abfs in (("igemm", 32, (32, 128), (0,)), ("igemm3", 32, (32, 128), (0,)),
                                                        ("igemm3n", 32, (32, 128), (0, 1)), ("igemm3s", 16, (32,), (0, 1)),
                                                        ("wgrad", 32, (32, 128), (0,)), ("wgrad3", 32, (32, 128), (0, 1)))
              for n in ns for abf in abfs]


@pytest.mark.parametrize("kernel,CIN,N,abf", PLAN_CASES, ids=lambda v: str(v))
def test_plan_sizes_exactly_what_the_kernel_writes(kernel, CIN, N, abf):
    import ctypes

    from bsed_amd import _lib as L, ops
    from test_contract_plan_cpu import _desc, _plan
    dtype = torch.bfloat16 if abf else torch.float32
    g = torch.Generator().manual_seed(CIN + N + abf)
    x = torch.randn(1, GH, GW, CIN, generator=g).to(dtype).cuda()
    d = _desc(kernel, 1, GH, GW, CIN, N, 9, 0 if kernel.startswith("wgrad") else ops.EPI_STATS, abf)
    rc, plan = _plan(kernel, d)
    assert rc == 0, L.lib().bsed_last_error().decode()
    d.G, d.in_ = plan.G, x.data_ptr()
    if kernel.startswith("wgrad"):
        assert plan.stats_rows == 0 and 1 <= plan.G <= plan.max_G == 2
        dy = torch.randn(1, GH, GW, N, generator=g).to(dtype).cuda()
        buf = torch.full((plan.G + 1, 9, CIN, N), float("nan"), device="cuda")
        d.dy, d.part = dy.data_ptr(), buf.data_ptr()
        rows = plan.G
    else:
        # (NWN, MW) of bsed_igemm3n: (1, 4) at N = 32, four partial rows per tile; (4, 1) at N = 128, one
        assert plan.max_G == 2 and plan.stats_rows == (2 * 128 // N if kernel == "igemm3n" else 2)
        w = (torch.randn(9, CIN, N, generator=g) / (9 * CIN) ** 0.5).cuda()
        strides = (CIN * N, N, 1)
        if kernel == "igemm":
            wpk = ops.pack_weight(w, 9, CIN, N, *strides)
        elif kernel == "igemm3":
            wpk = torch.empty((9, CIN // 32, N, 64), device="cuda", dtype=torch.int16)
            L.call("bsed_pack_weight3", w.data_ptr(), wpk.data_ptr(), 9, CIN, N, N, *strides, L.stream())
        else:
            wpk = ops.pack_weight3s(w, 9, N, *strides, K=CIN)
        out = torch.empty((1, GH, GW, N), device="cuda", dtype=dtype)
        buf = torch.full((plan.stats_rows + 1, 2, N), float("nan"), device="cuda")
        d.w, d.out, d.stats = wpk.data_ptr(), out.data_ptr(), buf.data_ptr()
        rows = plan.stats_rows
    L.call("bsed_" + kernel, ctypes.byref(d), L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(buf[:rows]).all(), plan.label
    assert torch.isnan(buf[rows]).all(), plan.label
    if not kernel.startswith("wgrad"):
        assert torch.isfinite(out.float()).all()
