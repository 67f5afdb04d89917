"""The float64 GLU restatement of tests/glu_reference.py against float64 autograd through the oracle's GLU module, its
companions, and (no GPU) the case tables of tests/test_glu_kernels_gpu.py against bsed_glu_plan: every case is
accepted by the library, and every forced G makes a workgroup walk several work items, with unequal counts."""
import pytest
import torch

import glu_reference as R
import test_glu_kernels_gpu as T
from oracle.crnn_oracle import GLU


def _case(B, H, W, C, pool, p, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, H, W, C, generator=g)
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g) * 0.3
    w = torch.randn(C, C, generator=g) / C ** 0.5
    bias = torch.randn(C, generator=g) * 0.1
    dpool = torch.randn(B, H // pool[0], W // pool[1], C, generator=g)
    mask = (torch.rand(B, H, W, C, generator=g) >= p).float()
    return y, scale, shift, w, bias, pool, mask, p, dpool


def _autograd(y, scale, shift, w, bias, pool, mask, p, dpool):
    """the stage as the model runs it, in float64: BatchNorm apply written as y*scale + shift, the oracle's GLU, a
    multiplication by mask/(1-p), nn.AvgPool2d; xn and lin retained for their gradients"""
    C = y.shape[-1]
    glu = GLU(C).double()
    with torch.no_grad():
        glu.linear.weight.copy_(w)
        glu.linear.bias.copy_(bias)
    kept = {}

    def keep_lin(module, args, out):
        out.retain_grad()
        kept["lin"] = out

    glu.linear.register_forward_hook(keep_lin)
    y = y.double()
    xn = (y * scale.double() + shift.double()).requires_grad_()
    res = glu(xn.permute(0, 3, 1, 2)) * (mask.double() / (1.0 - p)).permute(0, 3, 1, 2)
    pooled = torch.nn.AvgPool2d(pool)(res)
    pooled.backward(dpool.double().permute(0, 3, 1, 2))
    g = xn.grad
    return dict(pooled=pooled.detach().permute(0, 2, 3, 1), g=g, d_lin=kept["lin"].grad, dW=glu.linear.weight.grad,
                db=glu.linear.bias.grad, st=torch.stack([g.sum((0, 1, 2)), (g * y).sum((0, 1, 2))]))


# an odd H with ph = 2 (a remainder row), and the feature-pyramid geometry: pool (2, 1) on W = 1
AUTOGRAD_CASES = [(2, 9, 6, 8, (2, 2), 0.5), (3, 7, 1, 16, (2, 1), 0.25)]


@pytest.mark.parametrize("B,H,W,C,pool,p", AUTOGRAD_CASES)
def test_closed_form_backward_equals_float64_autograd(B, H, W, C, pool, p):
    args = _case(B, H, W, C, pool, p, seed=100 * H + W)
    ref, _, _ = R.glu_reference(*args)
    want = _autograd(*args)
    for name in R.OUTPUTS:
        assert ref[name].shape == want[name].shape, name
        e = float((ref[name] - want[name]).abs().max() / want[name].abs().max())
        print(f"glu_reference vs autograd {B}x{H}x{W}x{C} pool {pool} {name}: {e:.2e}")
        assert e <= 1e-12, (name, e)
    # the remainder rows feed nothing and receive nothing
    Hp = H // pool[0]
    assert float(ref["g"][:, Hp * pool[0]:].abs().max() if H > Hp * pool[0] else 0.0) == 0.0


@pytest.mark.parametrize("B,H,W,C,pool,p", AUTOGRAD_CASES + [(1, 5, 4, 8, (1, 2), 0.0)])
def test_companions_dominate_and_vanish_only_with_every_term(B, H, W, C, pool, p):
    args = _case(B, H, W, C, pool, p, seed=7 * H + W)
    ref, comp, K = R.glu_reference(*args)
    assert set(ref) == set(comp) == set(K) == set(R.OUTPUTS)
    for name in R.OUTPUTS:
        assert bool((ref[name].abs() <= comp[name] * (1.0 + 1e-14)).all()), name
        assert bool((comp[name] >= 0).all()) and K[name] >= 1
        assert bool((ref[name][comp[name] == 0] == 0).all()), name
    Hp = H // pool[0]
    if H > Hp * pool[0]:
        assert float(comp["g"][:, Hp * pool[0]:].max()) == 0.0 and float(comp["d_lin"][:, Hp * pool[0]:].max()) == 0.0
    fwd, fwd_comp, fwd_K = R.glu_reference(*args[:-1])
    assert set(fwd) == {"pooled"} and torch.equal(fwd["pooled"], ref["pooled"]) and fwd_K == {"pooled": C}
    # the bound: zero where the companion is, and a non-zero value there is an infinite miss
    z = torch.zeros(3, dtype=torch.float64)
    assert R.err_over_bound(z, z, z, 4, R.EPS_FP32) == 0.0
    assert R.err_over_bound(z + 1e-30, z, z, 4, R.EPS_FP32) == float("inf")
    assert R.err_over_bound(z + float("nan"), z, z + 1.0, 4, R.EPS_FP32) == float("inf")
    assert R.EPS_FP32 < R.EPS_SPLIT < R.EPS_BF16


def test_bound_sees_one_slightly_wrong_element_that_the_norm_bar_does_not():
    """The hazard glu3.hip records (stale lanes of an accumulator, one wrong position per run) at its mildest: ONE
    element of g off by 2^-12 of its value.  The relative L2 norm over the tensor, the bar of the kernel-vs-kernel
    tests, moves by less than 3e-5; the per-element bound is exceeded several times over."""
    args = _case(2, 9, 16, 32, (2, 2), 0.5, seed=3)
    ref, comp, K = R.glu_reference(*args)
    got = ref["g"].float().double()                       # a kernel that is right to fp32 round-off
    assert R.err_over_bound(got, ref["g"], comp["g"], K["g"], R.EPS_FP32) <= 1.0
    i = int(ref["g"].abs().flatten().argmax())            # the element that moves the norm most
    got.view(-1)[i] *= 1.0 + 2.0 ** -12
    l2 = float((got - ref["g"]).norm() / ref["g"].norm())
    ratio = R.err_over_bound(got, ref["g"], comp["g"], K["g"], R.EPS_FP32)
    print(f"one element off by 2^-12: relative L2 {l2:.2e} (bar 3e-5), err/bound {ratio:.1f}")
    assert l2 < 3e-5 and ratio > 4.0


# tiles of the TILED cases, worked out by hand from B * ceil(H / TH) * (W / TW): what the table's comments claim
TILES = [12, 3, 2, 16, 2, 6, 3, 3, 3, 4, 1]


def _launches():
    """(entry point, case, bf16) of every launch configuration of the GPU test"""
    for case in T.TILED + T.GLU16:
        for entry in T.entries_for(case):
            yield entry, case, False
            if entry in T.HAS_BF16 and T.FIRST_OF_C.get(case[0]) == case:
                yield entry, case, True


def test_every_gpu_case_is_accepted_by_the_plan_and_every_forced_G_is_uneven():
    """No case of the issue's table was refused by bsed_glu_plan, so none was swapped.  Two of its forced G were
    adjusted, both inside forced_Gs: glu_bwd3n counts tile PAIRS, so G = 2 is its natural grid on the two 3-tile cases
    (128, 1x70x4) and (128, 3x9x2) and G = 1 is run there; and where the table's G divides the item count (6 tiles at
    G = 2, every glu16 case at half its natural G) a second, non-dividing G is run besides it."""
    seen = set()
    for entry, case, bf16 in _launches():
        d, plan = T.descriptor(entry, case, bf16)                       # raises if the library refuses the shape
        assert 1 <= plan.G <= plan.max_G
        if case[0] != 16:
            ntiles = TILES[T.TILED.index(case)]
            assert plan.max_G == ((ntiles + 1) // 2 if entry == "bsed_glu_bwd3n" else ntiles), (entry, case)
            assert plan.G == plan.max_G                                 # at these shapes the natural round is one item each
            assert plan.variant == {"bsed_glu_bwd_fused": 8 if case[0] == 128 else 4, "bsed_glu_bwd3n": 0}.get(
                entry, 4 if case[3] >= 16 else -1)
        Gs = T.forced_Gs(case, plan)
        assert len(set(Gs)) == len(Gs) and (Gs or plan.max_G <= 2), (entry, case, Gs)
        if case[0] != 16 and case[5] is not None and entry != "bsed_glu_bwd3n" and plan.max_G >= 2:
            assert Gs[0] == case[5]                                     # the table's G, as the issue gives it
        for G in Gs:
            assert 1 <= G <= plan.max_G and G != plan.G, (entry, case, G)
            assert -(-plan.max_G // G) >= 2, (entry, case, G)           # some workgroup walks at least two items
        if plan.max_G >= 3:                                             # below that no grid can be uneven
            assert any(plan.max_G % G for G in Gs), (entry, case, Gs)   # i % G assignment: unequal counts
        seen.add((entry, bf16))
    assert seen == {(e, False) for e in T.PLAN_ID} | {(e, True) for e in T.HAS_BF16}
    # the compile-time-width and run-time-width builds, every tile width, both pooling heights, the igemm-only forward
    assert {c[3] for c in T.TILED} >= {1, 2, 4, 8, 16, 32} and {c[4] for c in T.TILED} == {(2, 2), (1, 2), (2, 1), (1, 1)}
    assert "bsed_glu_fwd3" not in T.entries_for(T.TILED[2])
    assert all("bsed_glu_fwd3" in T.entries_for(c) for c in T.TILED if c is not T.TILED[2])
    # p = 0.25 reaches every entry point
    assert {e for c in T.QUARTER for e in T.entries_for(c)} == set(T.PLAN_ID)
