"""The float64 first block of tests/block0_reference.py against float64 autograd (conv2d, BatchNorm through explicit
batch statistics, Linear x sigmoid, mask, avg_pool2d), its propagated term against actual perturbations of y, its
bound against deliberately wrong references on every case of the GPU table, and (no GPU) the case tables and grid
rules of tests/test_block0_kernels_gpu.py against bsed_glu_plan."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import block0_reference as R
import test_block0_kernels_gpu as T

C = 16
POS = (0, 1, 2)
TABLE = T.FUSED + T.CONV0_ONLY


def _small(B, H, W, pool, p, seed):
    g = torch.Generator().manual_seed(seed)
    x = (-40.0 + 12.0 * torch.randn(B, H, W, generator=g)).clamp(-80.0, 5.0).double()
    return dict(x=x, cw=torch.randn(C, 9, generator=g).double() * 0.3, cb=torch.randn(C, generator=g).double() * 0.1,
                gamma=torch.rand(C, generator=g).double() + 0.5, beta=torch.randn(C, generator=g).double() * 0.3,
                w=torch.randn(C, C, generator=g).double() * 0.25, bias=torch.randn(C, generator=g).double() * 0.1,
                dpool=torch.randn(B, H // pool[0], W // pool[1], C, generator=g).double() * 1e-2,
                mask=(torch.rand(B, H, W, C, generator=g) >= p).double(), pool=pool, p=p)


def _autograd(t, eps=1e-5):
    """the block as the model states it, in float64, train-mode BatchNorm written out through the batch statistics"""
    cw = t["cw"].clone().requires_grad_()
    w, bias = t["w"].clone().requires_grad_(), t["bias"].clone().requires_grad_()
    y = F.conv2d(t["x"][:, None], cw.view(C, 1, 3, 3), t["cb"], padding=1).permute(0, 2, 3, 1)
    mean, var = y.mean(POS), y.var(POS, unbiased=False)
    invstd = (var + eps).rsqrt()
    xn = (y - mean) * invstd * t["gamma"] + t["beta"]
    xn.retain_grad()
    res = F.linear(xn, w, bias) * torch.sigmoid(xn) * t["mask"] / (1.0 - t["p"])
    pooled = F.avg_pool2d(res.permute(0, 3, 1, 2), t["pool"]).permute(0, 2, 3, 1)      # floor extent
    (pooled * t["dpool"]).sum().backward()
    return dict(y=y.detach(), pooled=pooled.detach(), g=xn.grad, dW=w.grad, db=bias.grad, dW0=cw.grad,
                mean=mean.detach(), invstd=invstd.detach())


AUTOGRAD_CASES = [(2, 5, 6, (2, 2), 0.5), (3, 4, 1, (2, 1), 0.25), (1, 3, 4, (1, 1), 0.0)]


def _reference_of(t, a, **kw):
    """the reference on the inputs t with BatchNorm as scale / shift / coef / mean taken from the statistics of a"""
    scale = t["gamma"] * a["invstd"]
    shift = t["beta"] - a["mean"] * scale
    args = (t["x"], t["cw"], t["cb"], scale, shift, t["w"], t["bias"], t["pool"], t["mask"], t["p"], t["dpool"])
    st = R.block0_reference(*args).ref["st"]
    n = t["x"].numel()
    # d_y = scale (g - mean(g) - xhat mean(g xhat)), xhat = (y - mean) invstd, as A g + B (y - mean) + C
    coef = torch.stack([scale, -scale * a["invstd"] ** 2 * (st[1] - a["mean"] * st[0]) / n, -scale * st[0] / n])
    return R.block0_reference(*args, coef, a["mean"], **kw)


@pytest.mark.parametrize("B,H,W,pool,p", AUTOGRAD_CASES)
def test_reference_equals_float64_autograd(B, H, W, pool, p):
    t = _small(B, H, W, pool, p, seed=100 * H + W)
    a = _autograd(t)
    r = _reference_of(t, a)
    taps = F.unfold(t["x"][:, None], 3, padding=1).view(B, 9, H, W).permute(1, 0, 2, 3)     # an independent halo
    want = dict(a, Gx=torch.einsum("bhwc,tbhw->ct", a["g"], taps),
                st=torch.stack([a["g"].sum(POS), (a["g"] * a["y"]).sum(POS)]),
                sy=torch.stack([a["y"].sum(POS), (a["y"] ** 2).sum(POS)]),
                xr=torch.cat([taps.reshape(9, -1).sum(1), R.pack_upper(taps.reshape(9, -1) @ taps.reshape(9, -1).t())]))
    for name in ("y", "sy", "xr", "pooled", "g", "dW", "db", "st", "Gx", "dW0"):
        assert r.ref[name].shape == want[name].shape, name
        e = float((r.ref[name] - want[name]).abs().max() / want[name].abs().max())
        print(f"block0_reference vs autograd {B}x{H}x{W} pool {pool} {name}: {e:.2e}")
        assert e <= 1e-12, (name, e)
    for name in r.ref:      # companions dominate, and vanish only with the value
        assert bool((r.ref[name].abs() <= r.comp[name] * (1.0 + 1e-14)).all()), name
    assert torch.equal(R.unpack_upper(R.pack_upper(taps.reshape(9, -1) @ taps.reshape(9, -1).t())),
                       taps.reshape(9, -1) @ taps.reshape(9, -1).t())


def _gpu_case(case, p=0.5):
    """reference arguments of a case of the GPU table with a host-made mask (any 0/1 tensor serves here)"""
    t = T._inputs(case)
    B, H, W, pool = case
    mask = (torch.rand(B, H, W, C, generator=torch.Generator().manual_seed(H * W + B)) >= p).float()
    return (t["x"], t["cw"], t["cb"], t["scale"], t["shift"], t["w"], t["bias"], pool, mask, p, t["dpool"], t["coef"],
            t["mean"])


@pytest.mark.parametrize("which", range(len(AUTOGRAD_CASES) + len(T.WIDE)))
def test_propagated_term_bounds_a_perturbation_of_y(which):
    """every output behind y, evaluated at y + s e_y for 20 random sign patterns s, stays within 1.01 x its propagated
    term of its value at y (the 1 % covers the second-order effects, ~1e-6 of the term at this e_y; 2^-40 of the
    value covers the float64 evaluation of the difference itself)"""
    if which < len(AUTOGRAD_CASES):
        B, H, W, pool, p = AUTOGRAD_CASES[which]
        t = _small(B, H, W, pool, p, seed=7 * H + W)
        make = lambda **kw: _reference_of(t, _autograd(t), **kw)      # noqa: E731
    else:
        args = _gpu_case(T.WIDE[which - len(AUTOGRAD_CASES)])
        make = lambda **kw: R.block0_reference(*args, **kw)            # noqa: E731
    r = make()
    g = torch.Generator().manual_seed(which)
    worst = {name: 0.0 for name in R.STAGE}
    for _ in range(20):
        s = (torch.rand(r.y.shape, generator=g) < 0.5).double() * 2.0 - 1.0
        q = make(y_offset=s * r.e_y)
        for name in R.STAGE:
            diff, term = (q.ref[name] - r.ref[name]).abs(), r.prop[name]
            assert bool((diff <= 1.01 * term + 2.0 ** -40 * r.ref[name].abs()).all()), name
            worst[name] = max(worst[name], float((diff / term.clamp_min(1e-300)).max()))
    print("perturbation / propagated term:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v > 0.01 for v in worst.values())      # nor is the term idle: some element moves by 1 % of it


# ---- deliberately wrong references ----
def _clamped(columns):
    def taps(x):
        x = x.detach().cpu().double()
        B, H, W = x.shape
        xp = torch.zeros(B, H + 2, W + 2, dtype=torch.float64)
        xp[:, 1:H + 1, 1:W + 1] = x
        if columns:
            xp[:, 1:H + 1, 0], xp[:, 1:H + 1, W + 1] = x[:, :, 0], x[:, :, W - 1]
        else:
            xp[:, 0, 1:W + 1], xp[:, H + 1, 1:W + 1] = x[:, 0], x[:, H - 1]
        return torch.stack([xp[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)])
    return taps


def _transposed(x):
    return R.conv_taps(x)[[3 * kw + kh for kh in range(3) for kw in range(3)]]


def _dropped(x):
    xt = R.conv_taps(x).clone()
    xt[4] = 0.0           # the centre tap: the one no map is too narrow for
    return xt


WRONG_TAPS = {"halo clamped, columns": _clamped(True), "halo clamped, rows": _clamped(False),
              "taps transposed": _transposed, "one tap dropped": _dropped}


@pytest.mark.parametrize("case", TABLE, ids=T.case_id)
def test_bound_sees_every_wrong_reference(case):
    """worst error / bound >= 10 for pooled, Gx and dW0 under each wrong halo or tap rule, for pooled under a pooling
    that takes the odd last row in (the plan admits no odd last column: W % pw == 0), for dW0 with mean dropped from
    Yx - mean Sx.  A condition on the case inputs (dB-scale x that is not 0 at the borders), not a measurement."""
    args = _gpu_case(case)
    r = R.block0_reference(*args)
    B, H, W, (ph, pw) = case
    seen = {}
    for label, taps in WRONG_TAPS.items():
        q = R.block0_reference(*args, taps=taps)
        for name in ("pooled", "Gx", "dW0"):
            seen[f"{label}: {name}"] = r.err_over_bound(q.ref[name], name, R.EPS_FP32)
    if H % ph:
        Hp, Wp = H // ph, W // pw
        extra = r.res[:, Hp * ph, :Wp * pw].reshape(B, Wp, pw, C).mean(2) / ph
        wrong = r.ref["pooled"].clone()
        wrong[:, Hp - 1] += extra
        seen["odd last row pooled: pooled"] = r.err_over_bound(wrong, "pooled", R.EPS_FP32)
    q = R.block0_reference(*args[:-1], torch.zeros(C))
    seen["mean dropped: dW0"] = r.err_over_bound(q.ref["dW0"], "dW0", R.EPS_FP32)
    for label, ratio in seen.items():
        print(f"{T.case_id(case)} {label}: error / bound {ratio:.3g}")
    assert all(v >= 10.0 for v in seen.values()), {k: v for k, v in seen.items() if not v >= 10.0}
    x = args[0]
    assert float(x[:, 0].abs().min()) > 0 and float(x[:, :, 0].abs().max()) > 0 and float(x[:, :, -1].abs().max()) > 0


@pytest.mark.parametrize("case", TABLE, ids=T.case_id)
def test_reference_outputs_are_not_vacuous(case):
    """at p = 0.5 at least a quarter of the elements of every per-position output are non-zero"""
    r = R.block0_reference(*_gpu_case(case))
    for name in ("y", "pooled", "g", "d_lin"):
        share = float((r.ref[name] != 0).double().mean())
        assert share >= 0.25, (name, share)
    assert float((r.res != 0).double().mean()) >= 0.25
    x = T._inputs(case)["x"]
    assert -80.0 <= float(x.min()) and float(x.max()) <= 5.0 and float(x.mean()) < -10.0     # dB scale
    assert case[1] < 3 or bool((x[-1, -1] == 0).all())       # the 0 dB padding row


# ---- the case tables against the library ----
def test_every_fused_case_is_accepted_by_the_plan_and_the_forced_G_make_the_work_list_carry():
    """No case of the issue's table was refused by bsed_glu_plan (W = 1 included: b0_fetch and B0Win::fetch clamp every
    address into the row and select 0, and no index is formed from W - 2), so none was swapped."""
    for entry in T.PLAN_ID:
        uneven = below = over = 0
        for case in T.FUSED:
            B, H, W, pool = case
            for bf16 in ([False, True] if case in T.WIDE else [False]):
                d, plan = T.descriptor(entry, case, bf16)               # raises if the library refuses the shape
                small = 0 if bf16 and entry == "bsed_block0_fwd" else 16
                assert plan.variant == pool[0] | small, (entry, case, plan.variant)
            chunks, Hp = -(-W // T.CHUNK[entry]), H // pool[0]
            assert plan.max_G == B * Hp * chunks and 1 <= plan.G <= plan.max_G
            Gs = T.forced_Gs(entry, case, plan)
            assert 1 in Gs and plan.G in Gs and all(1 <= G <= plan.max_G for G in Gs), (entry, case, Gs)
            uneven += any(plan.max_G % G for G in Gs)
            below += any(G < chunks * Hp for G in Gs)
            over += any(G > chunks * Hp for G in Gs)
            if plan.max_G >= 3:
                assert any(plan.max_G % G and (chunks == 1 or G % chunks) for G in Gs), (entry, case, Gs)
            if B >= 2 and plan.max_G > Hp * chunks + 1:
                assert any(G > Hp * chunks for G in Gs), (entry, case, Gs)
        assert uneven >= 8 and below >= 8 and over >= 5, (entry, uneven, below, over)
    # every wpr of b0_stats_kernel, both pooling heights and widths, partial and full chunks of both kernels
    assert {(c[2] + 63) // 64 for c in T.FUSED} == {1, 2, 3, 4}
    assert {c[3] for c in T.FUSED} == {(2, 2), (1, 2), (2, 1), (1, 1)}
    assert any(c[1] == c[3][0] == 2 for c in T.FUSED) and any(c[2] == 1 for c in T.FUSED)
    for case in T.FUSED:
        B, H, W, _ = case
        groups = -(-B * H // (4 // ((W + 63) // 64)))
        assert max(T.stats_Gs(case)) > groups and 1 in T.stats_Gs(case)
    for case in TABLE:
        assert max(T.wgrad_Gs(case)) * 256 > T.positions(case) and 1 in T.wgrad_Gs(case)
        assert (case[1] * case[2]) % 256 != 0 or case in T.FUSED
    assert all(c[1] * c[2] % 256 for c in T.CONV0_ONLY)


def test_refused_shapes_are_refused_by_the_plan():
    """what test_refused_arguments_write_nothing passes to the descriptor entry points is refused without a GPU too"""
    for entry, ident in T.PLAN_ID.items():
        for change in (dict(H=1), dict(W=15)):
            d, _ = T.descriptor(entry, T.FUSED[0])
            for k, v in change.items():
                setattr(d, k, v)
            plan = T.L.STRUCTS["BsedGluPlan"]()
            assert T.L.lib().bsed_glu_plan(ctypes.byref(d), T.L.CONSTANTS["BSED_GLU_" + ident], ctypes.byref(plan)) != 0
