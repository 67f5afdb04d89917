"""Every kernel of the first CNN block against the float64 reference of tests/block0_reference.py, element by element:
csrc/block0.hip (b0_stats_kernel + b0_colsum64_kernel, b0_fwd_kernel, b0_bwd_kernel, b0_wgrad_finish_kernel) and the
four-kernel fallback's conv0_fwd_kernel<16|32> / conv0_wgrad_kernel<16|32, BNB> of csrc/cnn_ops.hip.

Every entry point is called through the C ABI (bsed_block0_fwd / _bwd with a BsedGluDesc built here), so the test owns
G and every output: each output is a view into a NaN-filled buffer between two sentinel guard rows (Guarded of
tests/test_glu_kernels_gpu.py); after the launch every element is finite and the guards are intact.  Partial slabs are
reduced here in float64.  Each launch is made twice and must repeat its bits; forced-G and natural-G launches agree
bit for bit on pooled.  The forced G make the B0Idx mixed-radix work list carry across column chunk, pooled row and
image (forced_Gs); bsed_block0_stats is also run with more workgroups than row groups, whose partial rows must be zero.

The dropout mask is never restated: it is read back from b0_fwd itself with ph*pw probe launches (_mask) and must
equal the mask bsed_glu16_fwd applies at the same stream and seed.

Inputs: seeded dB-scale x in [-80, 5] (the recipe of oracle.seeded.db_like_input, restated for any width) with the
last row of the last image at exactly 0 dB, cw ~ 0.3 N(0,1), a BatchNorm taken from the batch statistics of y with
gamma and beta that are not (1, 0), dpool ~ 1e-2 N(0,1).

The chain (test_chain_...) compares conv0's weight gradient, assembled as dW0 = A Gx + B (Yx - mean Sx) + C Sx from fp32
partials, with the direct float64 sum: bound (1) composed from the bounds of Gx, R and Sx, and bar (2), the 1e-5
relative L2 that tests/test_block0_gpu.py holds between the two forms.  Bound (1) divided by |dW0| in L2 -- the cost
of the Yx - mean Sx cancellation on dB-scale input -- is printed per case.  Measured on an MI355X: 1.82e-3
(2x6x128, pool 2x2), 2.14e-3 (2x6x128, pool 1x2), 1.32e-3 (3x7x40), against measured errors of 4.2e-7, 3.5e-7 and
4.5e-7 relative L2 (at most 1e-3 of bound (1) on any element): the fp32 R / Sx partials leave the 1e-5 bar a factor
of 20 of room, and the composed bound overstates the error by three orders of magnitude because the rounding errors
of the partials are independent while the bound adds their absolute values.

tests/test_block0_reference_cpu.py imports the case tables and the G rules from here and checks them against
bsed_glu_plan without a GPU."""
import ctypes
import functools
import math

import pytest
import torch

import block0_reference as R
from bsed_amd import _lib as L
from test_glu_kernels_gpu import SEED, STREAM, Guarded
from test_glu_kernels_gpu import _mask as glu_mask

pytestmark = pytest.mark.gpu

# (B, H, W, pool): the smallest shapes that reach each edge
FUSED = [
    (2, 5, 16, (2, 2)),     # one wave tile; odd H with ph = 2
    (1, 2, 2, (2, 2)),      # H == ph: a single pooled row, both vertical halos zero
    (3, 7, 40, (2, 2)),     # partial wave tiles, idle waves
    (1, 6, 64, (1, 2)),     # b0_stats with wpr = 1; a full backward chunk
    (2, 5, 72, (2, 2)),     # backward chunk tail 64 + 8
    (2, 6, 128, (2, 2)),    # the product width
    (2, 6, 128, (1, 2)),
    (1, 5, 130, (2, 2)),    # forward chunk 128 + 2; wpr = 3
    (2, 4, 192, (2, 1)),    # pw = 1; three backward chunks
    (1, 3, 256, (1, 1)),    # the widest map the plan takes; wpr = 4; no pooling; odd nrows
    (2, 9, 1, (1, 1)),      # W = 1: accepted by the plan, the clamped window addresses stay inside the row
]
# bsed_conv0_fwd / _wgrad also: wider than the fused path takes, and W = 1; H*W no multiple of 256 in either
CONV0_ONLY = [(2, 3, 300, (1, 1)), (1, 7, 1, (1, 1))]
WIDE = [FUSED[5], FUSED[6], FUSED[2]]     # the bf16 instances and the chain: the two 128-wide cases and the 40-wide one
QUARTER = [FUSED[5]]                      # p = 0.25 once per entry point (forward and backward both run here)
CHUNK = {"bsed_block0_fwd": 128, "bsed_block0_bwd": 64}      # columns per work item
PLAN_ID = {"bsed_block0_fwd": "BLOCK0_FWD", "bsed_block0_bwd": "BLOCK0_BWD"}
C = 16



def case_id(case):
    B, H, W, pool = case
    return f"{B}x{H}x{W}-p{pool[0]}{pool[1]}"


def positions(case):
    return case[0] * case[1] * case[2]


def descriptor(entry, case, bf16=False):
    """BsedGluDesc of the entry point on this case, shape fields only, and its plan"""
    B, H, W, pool = case
    d = L.STRUCTS["BsedGluDesc"]()
    d.NB, d.H, d.W, d.C, d.act_bf16 = B, H, W, C, int(bf16)
    d.ph, d.pw = pool
    plan = L.STRUCTS["BsedGluPlan"]()
    L.check(L.lib().bsed_glu_plan(ctypes.byref(d), L.CONSTANTS["BSED_GLU_" + PLAN_ID[entry]], ctypes.byref(plan)), entry)
    return d, plan


def forced_Gs(entry, case, plan):
    """The grid sizes of a launch with plan.max_G = B * Hp * chunks work items (item i goes to workgroup i % G and the
    kernel walks i, i + G, ... as a mixed-radix number (image, pooled row, chunk)): 1, the plan's, then
      * the smallest G >= 2 that does not divide max_G and, where the map has several chunks, is no multiple of
        chunks: the chunk digit carries into the pooled row;
      * the smallest G > Hp * chunks that does not divide max_G (any such G where none exists), where max_G allows
        one: the stride's image digit is non-zero and both lower digits carry."""
    B, H, W, pool = case
    chunks, Hp = -(-W // CHUNK[entry]), H // pool[0]
    assert plan.max_G == B * Hp * chunks
    Gs = [1, plan.G]
    uneven = [G for G in range(2, plan.max_G) if plan.max_G % G and (chunks == 1 or G % chunks)]
    Gs += uneven[:1]
    over = [G for G in range(Hp * chunks + 1, plan.max_G + 1)]
    Gs += ([G for G in over if plan.max_G % G] or over)[:1]
    return sorted(set(Gs))


def stats_Gs(case):
    """bsed_block0_stats: 1, the G ops.block0_stats picks, and one more than the row groups ceil(NB*H / rpw)"""
    B, H, W, _ = case
    rpw = 4 // ((W + 63) // 64)
    return sorted({1, min(2048, max(1, positions(case) // 256)), -(-B * H // rpw) + 1})


def wgrad_Gs(case):
    """bsed_conv0_wgrad: 1, the G ops.conv0_wgrad picks, and one with G * 256 > positions (idle threads and workgroups)"""
    n = positions(case)
    return sorted({1, min(1024, max(1, n // 256)), n // 256 + 2})


# ---- inputs, masks and references: made once per case, never modified ----
@functools.lru_cache(maxsize=None)
def _inputs(case):
    """CPU float32 tensors of the case"""
    B, H, W, pool = case
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B + pool[0])
    base = -40.0 + 12.0 * torch.randn(B, H, W, generator=g)
    centre = torch.rand(B, H, 1, generator=g) * max(W - 1, 1)
    ridge = 25.0 * torch.exp(-0.5 * ((torch.arange(W)[None, None, :] - centre) / 4.0) ** 2)
    x = (base + ridge).clamp(-80.0, 5.0)
    if H >= 3:
        x[-1, H - 1] = 0.0                                  # the product pads short clips with 0 dB
    t = dict(x=x, cw=torch.randn(C, 9, generator=g) * 0.3, cb=torch.randn(C, generator=g) * 0.1,
             cw32=torch.randn(32, 9, generator=g) * 0.3, cb32=torch.randn(32, generator=g) * 0.1,
             w=torch.randn(C, C, generator=g) * 0.25, bias=torch.randn(C, generator=g) * 0.1,
             dpool=torch.randn(B, H // pool[0], W // pool[1], C, generator=g) * 1e-2,
             dy32=torch.randn(B, H, W, 32, generator=g) * 1e-2)
    # BatchNorm of the batch statistics of y (float64), gamma / beta not the identity; coefficients of a BatchNorm
    # backward of the right magnitudes (the chain test takes the kernels' own instead)
    for co, sfx in ((C, ""), (32, "32")):
        y = R.block0_reference(x, t["cw" + sfx], t["cb" + sfx]).ref["y"]
        mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False)
        scale = torch.linspace(0.5, 1.5, co, dtype=torch.float64) / (var + 1e-5).sqrt()
        t["mean" + sfx] = mean.float()
        t["coef" + sfx] = torch.stack([scale, 1e-3 * scale * torch.randn(co, generator=g).double(),
                                       1e-3 * torch.randn(co, generator=g).double()]).float()
        if co == C:
            t["scale"] = scale.float()
            t["shift"] = (torch.linspace(-0.3, 0.3, co, dtype=torch.float64) - mean * scale).float()
    return t


@functools.lru_cache(maxsize=None)
def _device_inputs(case):
    return {k: v.cuda() for k, v in _inputs(case).items()}


def launch(entry, case, p, G=None, bf16=False, inputs=None):
    """One BsedGluDesc entry point at grid size G (None: the plan's) into guarded outputs, made twice: the two launches
    must agree bit for bit.  Returns the outputs on the CPU in float64, partial slabs reduced in float64: pooled | dW,
    db, st, Gx ((16,9) = [c][t]); the backward also "db_row1" = the largest |value| in the second rows of part_db."""
    B, H, W, pool = case
    t = dict(_device_inputs(case), **(inputs or {}))
    d, plan = descriptor(entry, case, bf16)
    d.drop_p, d.rng_stream, d.seed = p, STREAM, SEED
    d.G = plan.G if G is None else G
    act = torch.bfloat16 if bf16 else torch.float32
    for name in ("x", "cw", "cb", "scale", "shift", "w", "bias"):
        setattr(d, name, L.ptr(t[name]))
    what = f"{entry}{'[bf16]' if bf16 else ''} {case_id(case)} p={p} G={d.G}"
    raw = []
    for _ in range(2):
        if entry == "bsed_block0_fwd":
            out = {"pooled": Guarded((B, H // pool[0], W // pool[1], C), act)}
            d.pooled = L.ptr(out["pooled"].view, act)
        else:
            dpool = t["dpool"].to(act)
            d.dpool = L.ptr(dpool, act)
            out = {"part_dw": Guarded((d.G, C, C)), "part_db": Guarded((d.G, 2, C)), "part_st": Guarded((d.G, 2, C)),
                   "part_gx": Guarded((d.G, 9, C))}
            for name, o in out.items():
                setattr(d, name, L.ptr(o.view))
        L.call(entry, ctypes.byref(d), L.stream())
        torch.cuda.synchronize()
        for name, o in out.items():
            o.check(f"{what} {name}")
            assert bool(torch.isfinite(o.view.float()).all()), f"{what} {name}: not finite"
        raw.append(out)
    for name in raw[0]:
        a, b = raw[0][name].view, raw[1][name].view
        bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(a.view(bits), b.view(bits)), f"{what} {name}: two launches differ"
    out = raw[0]
    if entry == "bsed_block0_fwd":
        return {"pooled": out["pooled"].view.double().cpu()}
    db = out["part_db"].view.double().sum(0).cpu()
    return {"dW": out["part_dw"].view.double().sum(0).cpu(), "db": db[0], "st": out["part_st"].view.double().sum(0).cpu(),
            "Gx": out["part_gx"].view.double().sum(0).t().contiguous().cpu(),
            "db_row1": out["part_db"].view[:, 1].abs().max().double().cpu()}


@functools.lru_cache(maxsize=None)
def _mask(case, p):
    """The keep-mask (B,H,W,16) of 0/1 that b0_fwd applies at drop probability p, stream STREAM, seed SEED, read back
    from b0_fwd itself.  With cw = the centre tap alone (= 1) and cb = 0 every channel of y is x; with W_lin = 0,
    bias = 1, scale = 1, shift = 0 and x = +30 at ONE slot of every pooling window, -30 elsewhere, res is
    sig*keep/(1-p) = keep/(1-p) at the slot and < 1e-12 elsewhere, so pooled*ph*pw*(1-p) is the slot's keep bit.
    Positions outside the pooled extent feed nothing in either direction; their bits stay 1."""
    B, H, W, pool = case
    if p == 0.0:
        return torch.ones(B, H, W, C)
    ph, pw = pool
    Hp, Wp = H // ph, W // pw
    mask = torch.ones(B, H, W, C)
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    centre = torch.zeros(C, 9, device="cuda")
    centre[:, 4] = 1.0
    for dh in range(ph):
        for dw in range(pw):
            x = torch.full((B, H, W), -30.0)
            x[:, dh:Hp * ph:ph, dw:Wp * pw:pw] = 30.0
            probe = dict(x=x.cuda(), cw=centre, cb=zero, scale=one, shift=zero, w=torch.zeros(C, C, device="cuda"), bias=one)
            bit = launch("bsed_block0_fwd", case, p, inputs=probe)["pooled"] * (ph * pw * (1.0 - p))
            assert bool(((bit.abs() <= 1e-3) | ((bit - 1.0).abs() <= 1e-3)).all()), "probe values are not keep bits"
            mask[:, dh:Hp * ph:ph, dw:Wp * pw:pw] = (bit > 0.5).float()
    # the four-kernel form applies the same bits: glu16's mask, read back the same way from bsed_glu16_fwd
    assert torch.equal(mask, glu_mask((C, B, H, W, pool), p)), f"{case_id(case)} p={p}: not the mask of bsed_glu16_fwd"
    return mask


def _rounded(t, bf16):
    return R.bf16(t) if bf16 else t


@functools.lru_cache(maxsize=None)
def _reference(case, p, bf16=False):
    t = _inputs(case)
    return R.block0_reference(_rounded(t["x"], bf16), _rounded(t["cw"], bf16), t["cb"], t["scale"], t["shift"], t["w"],
                              t["bias"], case[3], _mask(case, p), p, _rounded(t["dpool"], bf16))


def judge(label, got, ref, eps, failures, names=None):
    """the bound on every element of every output of `got`; prints max err / bound before it judges"""
    for name in names or got:
        ratio = ref.err_over_bound(got[name], name, eps)
        print(f"{label} {name}: max err/bound {ratio:.3f}")
        if not ratio <= 1.0:
            failures.append(f"{label} {name}: err/bound {ratio:.3f}")


def run_entry(entry, case, p, failures, bf16=False):
    """every grid size against the reference; the forced ones against the plan's: bit for bit on pooled"""
    eps = R.EPS_BF16 if bf16 else R.EPS_FP32
    ref = _reference(case, p, bf16)
    _, plan = descriptor(entry, case, bf16)
    nat = launch(entry, case, p, bf16=bf16)
    for G in forced_Gs(entry, case, plan):
        got = nat if G == plan.G else launch(entry, case, p, G=G, bf16=bf16)
        label = f"{entry}{'[bf16]' if bf16 else ''} {case_id(case)} p={p} G={G}"
        judge(label, got, ref, eps, failures, [n for n in got if n != "db_row1"])
        if "pooled" in got and not torch.equal(got["pooled"], nat["pooled"]):
            n = int((got["pooled"] != nat["pooled"]).sum())
            failures.append(f"{label} pooled: {n} elements differ from the natural-G launch")
        if "db_row1" in got and float(got["db_row1"]) != 0.0:
            failures.append(f"{label}: the second row of part_db is not exactly 0")


FUSED_RUNS = [(c, p) for c in FUSED for p in (0.0, 0.5)] + [(c, 0.25) for c in QUARTER]


def _ids(v):
    return case_id(v) if isinstance(v, tuple) else (f"drop{v}" if isinstance(v, float) else f"co{v}")


@pytest.mark.parametrize("case,p", FUSED_RUNS, ids=_ids)
def test_fused_forward_and_backward_equal_the_float64_reference(case, p):
    failures = []
    for entry in ("bsed_block0_fwd", "bsed_block0_bwd"):
        run_entry(entry, case, p, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", WIDE, ids=_ids)
def test_bf16_instances_equal_the_float64_reference_of_the_rounded_inputs(case):
    """b0_fwd / b0_bwd<.., ABF = 1>: bf16 pooled out, bf16 dpool in, p = 0.5, every grid size; the reference takes x, cw
    and dpool rounded to bf16, the bound is that of EPS_BF16"""
    failures = []
    for entry in ("bsed_block0_fwd", "bsed_block0_bwd"):
        run_entry(entry, case, 0.5, failures, bf16=True)
    assert not failures, "\n".join(failures)


def test_the_probed_mask_is_a_mask_with_the_keep_rate_of_p():
    for case, p in ((FUSED[5], 0.5), (FUSED[5], 0.25), (FUSED[9], 0.5)):
        _, H, W, (ph, pw) = case
        m = _mask(case, p)[:, :H // ph * ph, :W // pw * pw]
        n = m.numel()
        assert bool(((m == 0) | (m == 1)).all())
        assert abs(float(m.mean()) - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / n) + 1.0 / n


# ---- the four-kernel fallback's conv kernels ----
def _conv_inputs(case, CO):
    t, sfx = _device_inputs(case), "" if CO == C else "32"
    return t["x"], t["cw" + sfx], t["cb" + sfx], t["coef" + sfx], t["mean" + sfx], t["dy32"][..., :CO].contiguous()


@functools.lru_cache(maxsize=None)
def _conv_reference(case, CO):
    t, sfx = _inputs(case), "" if CO == C else "32"
    return R.block0_reference(t["x"], t["cw" + sfx], t["cb" + sfx])


@pytest.mark.parametrize("CO", [16, 32], ids=_ids)
@pytest.mark.parametrize("case", FUSED + CONV0_ONLY, ids=_ids)
def test_conv0_fwd_equals_the_float64_reference(case, CO):
    """y per element within e_y; the per-tile statistics, reduced here, against sum y and sum y^2"""
    B, H, W, _ = case
    x, cw, cb = _conv_inputs(case, CO)[:3]
    ref = _conv_reference(case, CO)
    nt = L.lib().bsed_conv0_num_tiles(B, H, W)
    assert nt == B * -(-H * W // 256)
    failures, raw = [], []
    for _ in range(2):
        y, st = Guarded((B, H, W, CO)), Guarded((nt, 2, CO))
        L.call("bsed_conv0_fwd", L.ptr(x), L.ptr(cw), L.ptr(cb), L.ptr(y.view), L.ptr(st.view), B, H, W, CO, L.stream())
        torch.cuda.synchronize()
        y.check("conv0_fwd y"), st.check("conv0_fwd stats")
        raw.append((y, st))
    assert torch.equal(raw[0][0].view, raw[1][0].view) and torch.equal(raw[0][1].view, raw[1][1].view)
    got = {"y": raw[0][0].view.double().cpu(), "sy": raw[0][1].view.double().sum(0).cpu()}
    judge(f"bsed_conv0_fwd<{CO}> {case_id(case)}", got, ref, R.EPS_FP32, failures)
    # without the statistics: the same y
    y = Guarded((B, H, W, CO))
    L.call("bsed_conv0_fwd", L.ptr(x), L.ptr(cw), L.ptr(cb), L.ptr(y.view), None, B, H, W, CO, L.stream())
    torch.cuda.synchronize()
    y.check("conv0_fwd y (no stats)")
    assert torch.equal(y.view, raw[0][0].view)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("CO", [16, 32], ids=_ids)
@pytest.mark.parametrize("case", FUSED + CONV0_ONLY, ids=_ids)
def test_conv0_wgrad_equals_the_float64_reference(case, CO):
    """sum d_y x_t with d_y given, and with BatchNorm's backward applied on load to (g, the stored y)"""
    B, H, W, _ = case
    x, _, _, coef, mean, dy = _conv_inputs(case, CO)
    y = _conv_reference(case, CO).ref["y"].float()           # the stored y: an input of this kernel, exact as given
    yd = y.cuda()
    failures = []
    for bnb in (False, True):
        ref, comp, K = R.conv0_wgrad_reference(x, dy, *((y, coef, mean) if bnb else ()))
        assert K == positions(case)
        for G in wgrad_Gs(case):
            part = Guarded((G, 9, CO))
            L.call("bsed_conv0_wgrad", L.ptr(x), L.ptr(dy), L.ptr(yd) if bnb else None, L.ptr(coef) if bnb else None,
                   L.ptr(mean) if bnb else None, L.ptr(part.view), G, B, H, W, CO, L.stream())
            torch.cuda.synchronize()
            part.check(f"conv0_wgrad G={G}")
            got = part.view.double().sum(0).t().cpu()
            ratio = R.G.err_over_bound(got, ref, comp, K, R.EPS_FP32)
            print(f"bsed_conv0_wgrad<{CO}, {bnb}> {case_id(case)} G={G} dW0: max err/bound {ratio:.3f}")
            if not ratio <= 1.0:
                failures.append(f"bsed_conv0_wgrad<{CO}, {bnb}> G={G}: err/bound {ratio:.3f}")
            idle = part.view[-(-positions(case) // 256):]
            if idle.numel() and float(idle.abs().max()) != 0.0:
                failures.append(f"bsed_conv0_wgrad<{CO}, {bnb}> G={G}: partial rows of idle workgroups are not zero")
    assert not failures, "\n".join(failures)


# ---- statistics ----
def launch_stats(case, G, inputs=None):
    """bsed_block0_stats at grid size G into guarded outputs: (stats (G,2,16), xr_part (G,54), xr64 (54))"""
    B, H, W, _ = case
    t = inputs or _device_inputs(case)
    cwt = t["cw"].t().contiguous()
    out = Guarded((G, 2, C)), Guarded((G, R.NXR)), Guarded((R.NXR,), torch.float64)
    L.call("bsed_block0_stats", L.ptr(t["x"]), L.ptr(cwt), L.ptr(t["cb"]), L.ptr(out[0].view), L.ptr(out[1].view),
           L.ptr(out[2].view, torch.float64), G, B, H, W, C, L.stream())
    torch.cuda.synchronize()
    for o, name in zip(out, ("stats", "xr_part", "xr64")):
        o.check(f"bsed_block0_stats {case_id(case)} G={G} {name}")
    return out


@pytest.mark.parametrize("case", FUSED, ids=_ids)
def test_block0_stats_equal_the_float64_reference(case):
    """sum y, sum y^2 and all 54 entries of xr64; xr64 is the float64 sum of xr_part; idle workgroups write zeros"""
    B, H, W, _ = case
    ref = _conv_reference(case, C)
    rpw = 4 // ((W + 63) // 64)
    failures = []
    for G in stats_Gs(case):
        a, b = launch_stats(case, G), launch_stats(case, G)
        for u, v in zip(a, b):
            assert torch.equal(u.view, v.view), "two launches differ"
        stats, xr_part, xr64 = (o.view for o in a)
        got = {"sy": stats.double().sum(0).cpu(), "xr": xr64.cpu()}
        judge(f"bsed_block0_stats {case_id(case)} G={G}", got, ref, R.EPS_FP32, failures)
        part = xr_part.double().sum(0).cpu()
        if not bool(((part - got["xr"]).abs() <= 2.0 ** -50 * xr_part.double().abs().sum(0).cpu()).all()):
            failures.append(f"G={G}: xr64 is not the float64 sum of xr_part")
        used = -(-B * H // rpw)
        if G > used and (float(stats[used:].abs().max()) != 0.0 or float(xr_part[used:].abs().max()) != 0.0):
            failures.append(f"G={G}: partial rows of idle workgroups are not zero")
    assert not failures, "\n".join(failures)


# ---- the finishing formula on its own ----
def _ulp32(v):
    """spacing of float32 at |v| (float64 tensor in, float64 out)"""
    f = v.float().abs()
    return (torch.nextafter(f, torch.full_like(f, math.inf)) - f).double()


@pytest.mark.parametrize("G", [1, 63, 64, 65, 130])
def test_wgrad_finish_is_the_float64_formula(G):
    """dW0 = A Gx + B (Yx - mean Sx) + C Sx from synthetic Gx partial rows, xr64 computed in float64 on the host from
    dB-scale x, random float32 coef and mean: within 1 ulp of the fp32 result (plus 1 ulp of the destination when
    accumulating: the sum is rounded once more)"""
    t = _inputs(FUSED[5])
    g = torch.Generator().manual_seed(G)
    part = torch.randn(G, 9, C, generator=g)
    xr = R.block0_reference(t["x"], t["cw"], t["cb"]).ref["xr"]
    coef = torch.randn(3, C, generator=g) * torch.tensor([[0.05], [1e-3], [1e-3]])
    mean = torch.randn(C, generator=g) * 20.0 - 10.0
    cw, cb = t["cw"].double(), t["cb"].double()
    A, Bc, Cc = (v[:, None] for v in coef.double())
    sx, r = xr[:9][None], R.unpack_upper(xr[9:])
    want = A * part.double().sum(0).t() + Bc * (cw @ r + cb[:, None] * sx - mean.double()[:, None] * sx) + Cc * sx
    dev = [v.cuda() for v in (part, coef, mean, t["cw"], t["cb"])]
    for accumulate in (0, 1):
        dst = Guarded((C, 9))
        base = torch.randn(C, 9, generator=g) * float(want.abs().mean())
        if accumulate:
            dst.view.copy_(base)
        L.call("bsed_block0_wgrad_finish", L.ptr(dev[0]), G, L.ptr(xr.cuda(), torch.float64), L.ptr(dev[1]), L.ptr(dev[2]),
               L.ptr(dev[3]), L.ptr(dev[4]), L.ptr(dst.view), accumulate, C, L.stream())
        torch.cuda.synchronize()
        dst.check(f"wgrad_finish G={G} accumulate={accumulate}")
        got = dst.view.double().cpu()
        if accumulate:
            tol = _ulp32(want) + _ulp32(base.double() + want)
            err = (got - (base.double() + want.float().double())).abs().minimum((got - (base.double() + want)).abs())
        else:
            tol, err = _ulp32(want), (got - want).abs()
        print(f"bsed_block0_wgrad_finish G={G} accumulate={accumulate}: max err/ulp {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), (G, accumulate, float((err / tol).max()))


# ---- the chain ----
@pytest.mark.parametrize("case", WIDE, ids=_ids)
def test_chain_assembles_conv0_weight_gradient_of_the_float64_reference(case):
    """block0_stats -> ops.bn_finalize -> block0_bwd -> ops.bn_bwd -> block0_wgrad_finish against the reference's
    dW0 (the direct sum of d_y x_t), evaluated with the kernels' own float32 scale / shift / coef / mean as given
    inputs (tests/test_stats_kernels_gpu.py pins those)"""
    from bsed_amd import ops
    B, H, W, pool = case
    n, p = positions(case), 0.5
    t = _device_inputs(case)
    stats, _, xr64 = (o.view for o in launch_stats(case, min(2048, max(1, n // 256))))
    gamma, beta = torch.linspace(0.5, 1.5, C, device="cuda"), torch.linspace(-0.3, 0.3, C, device="cuda")
    rmean, rvar = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    nbt = torch.zeros((), device="cuda", dtype=torch.int64)
    mean, invstd, scale, shift = ops.bn_finalize(stats.contiguous(), C, float(n), 1e-5, 0.1, gamma, beta, rmean, rvar, nbt)
    d, plan = descriptor("bsed_block0_bwd", case)
    d.drop_p, d.rng_stream, d.seed, d.G = p, STREAM, SEED, plan.G
    own = dict(t, scale=scale, shift=shift)
    for name in ("x", "cw", "cb", "scale", "shift", "w", "bias", "dpool"):
        setattr(d, name, L.ptr(own[name]))
    part = {"part_dw": Guarded((d.G, C, C)), "part_db": Guarded((d.G, 2, C)), "part_st": Guarded((d.G, 2, C)),
            "part_gx": Guarded((d.G, 9, C))}
    for name, o in part.items():
        setattr(d, name, L.ptr(o.view))
    L.call("bsed_block0_bwd", ctypes.byref(d), L.stream())
    dgamma, dbeta = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    coef = ops.bn_bwd(part["part_st"].view.contiguous(), C, float(n), gamma, mean, invstd, dgamma, dbeta, None, t["x"],
                      apply=False)
    dst = Guarded((C, 9))
    L.call("bsed_block0_wgrad_finish", L.ptr(part["part_gx"].view), d.G, L.ptr(xr64, torch.float64), L.ptr(coef),
           L.ptr(mean), L.ptr(t["cw"]), L.ptr(t["cb"]), L.ptr(dst.view), 0, C, L.stream())
    torch.cuda.synchronize()
    for name, o in list(part.items()) + [("dst", dst)]:
        o.check(f"chain {case_id(case)} {name}")
    i = _inputs(case)
    ref = R.block0_reference(i["x"], i["cw"], i["cb"], scale.cpu(), shift.cpu(), i["w"], i["bias"], pool, _mask(case, p), p,
                             i["dpool"], coef.cpu(), mean.cpu())
    got = dst.view.double().cpu()
    b1 = R.composed_dw0_bound(ref, i["cw"], i["cb"], coef.cpu(), mean.cpu(), R.EPS_FP32)
    err = (got - ref.ref["dW0"]).abs()
    ratio, l2 = float((err / b1).max()), float(err.norm() / ref.ref["dW0"].norm())
    print(f"chain {case_id(case)} dW0: max err/bound(1) {ratio:.3f}; relative L2 {l2:.2e} (bar 1e-5); "
          f"bound(1) / |dW0| in L2 {float(b1.norm() / ref.ref['dW0'].norm()):.2e}")
    assert ratio <= 1.0, ratio
    assert l2 <= 1e-5, l2


# ---- argument checks ----
def test_refused_arguments_write_nothing():
    """a refused call returns an error before any launch: every output stays NaN between intact guards"""
    case = FUSED[0]
    B, H, W, pool = case
    t = _device_inputs(case)
    cwt = t["cw"].t().contiguous()

    def untouched(outs, what):
        torch.cuda.synchronize()
        for o in outs:
            assert bool(torch.isnan(o.view).all()), f"{what}: an output was written"
            o.view.zero_()
            o.check(what)                      # the guards (check wants the view written)

    lib = L.lib()
    for label, W_, CO_ in (("W = 257", 257, C), ("CO = 8", W, 8)):
        outs = Guarded((4, 2, C)), Guarded((4, R.NXR)), Guarded((R.NXR,), torch.float64)
        big = torch.zeros(B, H, 257, device="cuda")
        rc = lib.bsed_block0_stats(L.ptr(big), L.ptr(cwt), L.ptr(t["cb"]), L.ptr(outs[0].view), L.ptr(outs[1].view),
                                   L.ptr(outs[2].view, torch.float64), 4, B, H, W_, CO_, L.stream())
        assert rc != 0, label
        untouched(outs, f"bsed_block0_stats {label}")
    bad = {"H < ph": dict(H=1), "W % pw != 0": dict(W=15), "G = 0": dict(G=0), "G = max_G + 1": dict(G=None)}
    for entry in ("bsed_block0_fwd", "bsed_block0_bwd"):
        for label, change in bad.items():
            d, plan = descriptor(entry, case)
            d.drop_p, d.rng_stream, d.seed, d.G = 0.5, STREAM, SEED, plan.G
            for name in ("x", "cw", "cb", "scale", "shift", "w", "bias"):
                setattr(d, name, L.ptr(t[name]))
            for k, v in change.items():
                setattr(d, k, plan.max_G + 1 if v is None else v)
            rows = plan.max_G + 1
            if entry == "bsed_block0_fwd":
                outs = [Guarded((B, H // pool[0], W // pool[1], C))]
                d.pooled = L.ptr(outs[0].view)
            else:
                d.dpool = L.ptr(t["dpool"])
                outs = [Guarded((rows, C, C)), Guarded((rows, 2, C)), Guarded((rows, 2, C)), Guarded((rows, 9, C))]
                d.part_dw, d.part_db, d.part_st, d.part_gx = (L.ptr(o.view) for o in outs)
            rc = getattr(lib, entry)(ctypes.byref(d), L.stream())
            assert rc != 0, (entry, label)
            untouched(outs, f"{entry} {label}")
    part = torch.zeros(4, 9, C, device="cuda")
    xr64 = torch.zeros(R.NXR, device="cuda", dtype=torch.float64)
    for label, G, mean in (("G = 0", 0, t["mean"]), ("null pointer", 4, None)):
        dst = Guarded((C, 9))
        rc = lib.bsed_block0_wgrad_finish(L.ptr(part), G, L.ptr(xr64, torch.float64), L.ptr(t["coef"]), L.ptr(mean),
                                          L.ptr(t["cw"]), L.ptr(t["cb"]), L.ptr(dst.view), 0, C, L.stream())
        assert rc != 0, label
        untouched([dst], f"bsed_block0_wgrad_finish {label}")
