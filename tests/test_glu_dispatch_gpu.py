"""ops.glu_forward / ops.glu_backward launch the route ops.glu_route names and nothing else, and give bit for bit what
that route's own wrapper plus the reductions written out by hand give.

Every route reachable from the two functions is entered, at B = 2, H = 8 (smaller than the tile height of the narrow
maps, so partial tiles): the 16-channel streaming kernels, the bf16-core kernels for C = 32 / 64 and for C = 128, the
fp32-core fused kernel, the unfused three-launch chain and the igemm GLU_POOL forward, on the block shapes of the product
configuration and of the feature-pyramid level (W = 1, pool (2, 1)), plus the one forward shape where the bf16-core
kernel is not built (C = 32, W = 4, pool (2, 2)).

The fused FIRST block is the one GLU route these shapes leave out: block 0 goes through CRNN._block0_forward /
_block0_backward (ops.block0_*), not through glu_forward / glu_backward; tests/test_block0_gpu.py covers it.

The wrappers allocate their outputs themselves, so no output can be poisoned beforehand; dw and db are accumulated into
and start from the same non-zero values on both sides, which also shows that nothing overwrites them."""
import functools

import pytest
import torch

from test_graph_step_gpu import _recorded_launches

pytestmark = pytest.mark.gpu

B, H = 2, 8
DROP, STREAM, SEED = 0.5, 103, 9
SHAPES = [(16, 16, (2, 2)), (32, 16, (2, 2)), (64, 8, (1, 2)), (128, 4, (1, 2)), (128, 1, (2, 1))]
# entry points that tell the routes apart (bsed_igemm with its epilogue), per route
FORWARD_KERNELS = {"glu16": {"bsed_glu16_fwd"}, "glu3": {"bsed_glu_fwd3"}, "igemm": {"bsed_igemm:2"}}
BACKWARD_KERNELS = {"glu16": {"bsed_glu16_bwd"}, "glu3": {"bsed_glu_bwd3"}, "glu3n": {"bsed_glu_bwd3n"},
                    "fused_fp32": {"bsed_glu_bwd_fused"}, "unfused": {"bsed_igemm:3", "bsed_igemm:4"}}
ALL_KERNELS = set().union(*FORWARD_KERNELS.values(), *BACKWARD_KERNELS.values())


@functools.lru_cache(maxsize=None)
def _inputs(C, W, pool):
    g = torch.Generator().manual_seed(1000 * C + 10 * W + pool[0])
    y = torch.randn(B, H, W, C, generator=g).cuda()
    scale = (torch.rand(C, generator=g) + 0.5).cuda()
    shift = (torch.randn(C, generator=g) * 0.3).cuda()
    w = (torch.randn(C, C, generator=g) / C ** 0.5).cuda()
    bias = (torch.randn(C, generator=g) * 0.1).cuda()
    dpool = torch.randn(B, H // pool[0], W // pool[1], C, generator=g).cuda()
    dw0, db0 = torch.randn(C, C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    return y, scale, shift, w, bias, dpool, dw0, db0


def _forward_by_hand(route, y, scale, shift, w, bias, C, W, pool):
    from bsed_amd import ops
    if route == "glu16":
        return ops.glu16_fwd(y, scale, shift, w, bias, B, H, W, pool, DROP, STREAM, SEED)
    if route == "glu3":
        return ops.glu_fwd3(y, scale, shift, w, bias, B, H, W, C, pool, DROP, STREAM, SEED)
    assert route == "igemm"
    wg = ops.pack_weight(w, 1, C, C, 0, 1, C)
    return ops.igemm(y, wg, C, B, H, W, C, bias=bias, epilogue=ops.EPI_GLU_POOL, a_scale=scale, a_shift=shift, e_src=y,
                     e_scale=scale, e_shift=shift, pool=pool, drop_p=DROP, rng_stream=STREAM, seed=SEED)[0]


def _backward_by_hand(route, y, scale, shift, w, bias, dpool, C, W, pool, mode, dw, db):
    from bsed_amd import ops
    args = (B, H, W) + (() if C == 16 else (C,)) + (pool, DROP, STREAM, SEED)
    if route == "glu16":
        g, pdw, pdb, st2, G = ops.glu16_bwd(y, scale, shift, w, bias, dpool, *args)
        ops.reduce_partials(pdw, G, 1, 16, 16, 16, 16, dw, 0, 16, 1)
        ops.stats_to_grad(pdb, C, 0, db)
    elif route == "glu3":
        g, pdw, pdb, st2, G, slabs = ops.glu_bwd3(y, scale, shift, w, bias, dpool, *args)
        ops.reduce_partials(pdw, G * slabs, 1, C, C, C, C, dw, 0, C, 1)
        ops.stats_to_grad(pdb, C, 0, db)
    elif route == "glu3n":
        g, dlin, pdb, st2, G = ops.glu_bwd3n(y, scale, shift, w, bias, dpool, *args)
        ops.stats_to_grad(pdb, C, 0, db)
        part, Gw, KP, NP = ops.wgrad(y, dlin, B, H, W, C, C, a_scale=scale, a_shift=shift, mode=mode)
        ops.reduce_partials(part, Gw, 1, KP, NP, C, C, dw, 0, 1, C)
    elif route == "fused_fp32":
        wfwd = ops.pack_weight(w, 1, C, C, 0, 1, C)
        g, pdw, pdb, st2, G, slabs = ops.glu_bwd_fused(y, scale, shift, wfwd, w, bias, dpool, *args)
        ops.reduce_partials(pdw, G * slabs, 1, C, C, C, C, dw, 0, C, 1)
        ops.stats_to_grad(pdb, C, 0, db)
    else:
        assert route == "unfused"
        wg = ops.pack_weight(w, 1, C, C, 0, 1, C)
        tt = torch.empty_like(y)
        dlin, st = ops.igemm(y, wg, C, B, H, W, C, bias=bias, epilogue=ops.EPI_GLU_BWD, a_scale=scale, a_shift=shift,
                             e_src=y, e_scale=scale, e_shift=shift, e_dpool=dpool, out2=tt, pool=pool, drop_p=DROP,
                             rng_stream=STREAM, seed=SEED)
        ops.stats_to_grad(st, C, 0, db)
        part, G, KP, NP = ops.wgrad(y, dlin, B, H, W, C, C, a_scale=scale, a_shift=shift, mode=mode)
        ops.reduce_partials(part, G, 1, KP, NP, C, C, dw, 0, 1, C)
        wgT = ops.pack_weight(w, 1, C, C, 0, C, 1)
        g, st2 = ops.igemm(dlin, wgT, C, B, H, W, C, epilogue=ops.EPI_ADD_STATS2, out=tt, out2=tt, e_src=y)
    return g, st2


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("C,W,pool", SHAPES + [(32, 4, (2, 2))])
def test_glu_forward_runs_its_route_and_equals_it_bitwise(C, W, pool, mode):
    from bsed_amd import ops
    y, scale, shift, w, bias = _inputs(C, W, pool)[:5]
    route = ops.glu_route("forward", C, W, pool, mode)
    assert route == ("glu16" if C == 16 else "igemm" if mode == "fp32" or W == 4 and pool == (2, 2) else "glu3")
    with _recorded_launches() as names:
        got = ops.glu_forward(y, scale, shift, w, bias, B, H, W, C, pool, DROP, STREAM, SEED, mode=mode)
    assert names & ALL_KERNELS == FORWARD_KERNELS[route], sorted(names)
    with _recorded_launches() as hand_names:
        want = _forward_by_hand(route, y, scale, shift, w, bias, C, W, pool)
    assert names == hand_names
    assert got.shape == (B, H // pool[0], W // pool[1], C) and got.dtype == want.dtype
    assert torch.equal(got, want)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("C,W,pool", SHAPES)
def test_glu_backward_runs_its_route_and_equals_it_bitwise(C, W, pool, mode, fused):
    from bsed_amd import ops
    y, scale, shift, w, bias, dpool, dw0, db0 = _inputs(C, W, pool)
    route = ops.glu_route("backward", C, W, pool, mode, fused)
    assert route == ("glu16" if C == 16 else "unfused" if not fused else "fused_fp32" if mode == "fp32"
                     else "glu3n" if C == 128 else "glu3")
    dw, db, dw_hand, db_hand = dw0.clone(), db0.clone(), dw0.clone(), db0.clone()
    with _recorded_launches() as names:
        g, st2 = ops.glu_backward(y, scale, shift, w, bias, dpool, B, H, W, C, pool, DROP, STREAM, SEED, mode=mode,
                                  fused=fused, dw=dw, db=db)
    assert names & ALL_KERNELS == BACKWARD_KERNELS[route], sorted(names)
    with _recorded_launches() as hand_names:
        g_hand, st2_hand = _backward_by_hand(route, y, scale, shift, w, bias, dpool, C, W, pool, mode, dw_hand, db_hand)
    assert names == hand_names
    for name, a, b in (("g", g, g_hand), ("st2", st2, st2_hand), ("dw", dw, dw_hand), ("db", db, db_hand)):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert g.shape == y.shape and not torch.equal(dw, dw0) and not torch.equal(db, db0)


def test_unknown_mode_is_refused_before_anything_is_launched():
    from bsed_amd import ops
    from bsed_amd._lib import BsedError
    y, scale, shift, w, bias, dpool, dw0, db0 = _inputs(32, 16, (2, 2))
    dw, db = dw0.clone(), db0.clone()
    with _recorded_launches() as names:
        with pytest.raises(BsedError, match="fp16"):
            ops.glu_forward(y, scale, shift, w, bias, B, H, 16, 32, (2, 2), DROP, STREAM, SEED, mode="fp16")
        with pytest.raises(BsedError, match="fp16"):
            ops.glu_backward(y, scale, shift, w, bias, dpool, B, H, 16, 32, (2, 2), DROP, STREAM, SEED, mode="fp16",
                             fused=True, dw=dw, db=db)
    assert names == set()
    assert torch.equal(dw, dw0) and torch.equal(db, db0)
