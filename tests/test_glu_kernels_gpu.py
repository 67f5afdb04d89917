"""Every GLU kernel against the float64 reference of tests/glu_reference.py, element by element, with dropout on and
off, at the smallest shapes that reach each edge of the tile loops, and with the persistent rounds forced uneven.

The tiled and streaming entry points (bsed_glu16_fwd / _bwd, bsed_glu_fwd3, bsed_glu_bwd3, bsed_glu_bwd3n,
bsed_glu_bwd_fused) are called through the C ABI with a BsedGluDesc built here, so that the test owns the output
tensors and d.G: every output is a view into a NaN-filled buffer between two sentinel guard rows, and BsedGluDesc.G
(accepted for 1..max_G) makes a workgroup walk several tiles at a few hundred positions.  The two routes through
csrc/igemm.hip (the GLU_POOL forward, the unfused GLU_BWD -> wgrad -> ADD_STATS2 chain) are called through ops.
Partial slabs are reduced here in float64, so a reducer cannot mask or fake a kernel error.

Dropout masks are never restated: the tiled kernels and the igemm epilogues key the mask on the element index
pos*C + n like the stand-alone dropout kernel, whose output on a tensor of ones IS the mask; glu16's two-per-hash
mask is read back from glu16_fwd itself with ph*pw probe launches (see _mask).

Per output: (1) the derived per-element bound of glu_reference, (2) the precision bars the kernel-vs-kernel tests
hold, now against float64, (3) forced-G and natural-G runs agree bit for bit on the per-position outputs.  The test
prints max err / bound per entry point and output before it asserts.

tests/test_glu_reference_cpu.py imports the case tables and forced_Gs from here and checks them against bsed_glu_plan
without a GPU."""
import ctypes
import functools
import math

import pytest
import torch

import glu_reference as R
from bsed_amd import _lib as L

pytestmark = pytest.mark.gpu

STREAM, SEED = 103, 9
GUARD_FLOATS = 256
SENTINEL = 12345.0

# (C, B, H, W, pool, forced G): the tile is TW = min(W, 16), TH = 128 / TW
TILED = [
    (32, 2, 19, 32, (2, 2), 5),    # compile-time TW = 16, ragged tile rows (19 = 2*8 + 3), odd H with ph = 2, 12 tiles
    (32, 1, 37, 8, (2, 2), 2),     # run-time-width build (TW = 8, TH = 16), 3 tiles
    (32, 2, 9, 4, (2, 2), 1),      # TW = 4 with ph = 2: no glu_fwd3 (igemm forward); glu_bwd3 / glu_bwd_fused
    (64, 2, 27, 32, (1, 2), 3),    # 16 tiles, ragged rows
    (64, 1, 17, 8, (2, 2), 1),     # TW = 8, odd H, 2 tiles
    (128, 2, 21, 16, (1, 2), 2),   # 6 tiles; glu_bwd3n pairs
    (128, 1, 21, 16, (1, 2), 1),   # odd tile count: the last glu_bwd3n pair has one tile
    (128, 1, 70, 4, (1, 2), 2),    # TW = 4, TH = 32, ragged
    (128, 3, 9, 2, (1, 2), 2),     # TW = 2, one partial tile per image
    (128, 2, 131, 1, (2, 1), 1),   # feature-pyramid level: W = 1, odd H
    (128, 1, 12, 8, (1, 1), None),  # no pooling
]
# glu16: chunk tails (72 = 64 + 8), the product width 128, two 128-column chunks, odd H; forced G = half the natural
GLU16 = [(16, 2, 9, 16, (2, 2)), (16, 1, 5, 72, (2, 2)), (16, 2, 6, 128, (2, 2)), (16, 1, 4, 192, (2, 2)),
         (16, 2, 9, 16, (1, 2))]
# p = 0 and p = 0.5 on every case; p = 0.25 once per entry point: these three cases reach all of them
QUARTER = [TILED[0], TILED[5], GLU16[0]]
FIRST_OF_C = {32: TILED[0], 64: TILED[3], 128: TILED[5]}      # the unfused chain and the bf16 instances run here

PLAN_ID = {"bsed_glu16_fwd": "16_FWD", "bsed_glu16_bwd": "16_BWD", "bsed_glu_bwd_fused": "BWD_FUSED",
           "bsed_glu_fwd3": "FWD3", "bsed_glu_bwd3": "BWD3", "bsed_glu_bwd3n": "BWD3N"}
EPS = {"bsed_glu16_fwd": R.EPS_FP32, "bsed_glu16_bwd": R.EPS_FP32, "bsed_glu_bwd_fused": R.EPS_FP32,
       "bsed_glu_fwd3": R.EPS_SPLIT, "bsed_glu_bwd3": R.EPS_SPLIT, "bsed_glu_bwd3n": R.EPS_SPLIT,
       "igemm": R.EPS_FP32, "unfused": R.EPS_FP32}
FORWARD = ("bsed_glu16_fwd", "bsed_glu_fwd3", "igemm")
HAS_BF16 = ("bsed_glu_fwd3", "bsed_glu_bwd3", "bsed_glu_bwd3n")


def case_id(case):
    C, B, H, W, pool = case[:5]
    return f"C{C}-{B}x{H}x{W}-p{pool[0]}{pool[1]}"


def entries_for(case):
    """the C-ABI entry points that take this case"""
    from bsed_amd import ops
    C, _, _, W, pool = case[:5]
    if C == 16:
        return ["bsed_glu16_fwd", "bsed_glu16_bwd"]
    return ((["bsed_glu_fwd3"] if ops.glu_fwd3_supported(W, C, pool) else []) + ["bsed_glu_bwd_fused"] +
            (["bsed_glu_bwd3n"] if C == 128 else ["bsed_glu_bwd3"]))


def descriptor(entry, case, bf16=False):
    """BsedGluDesc of the entry point on this case, shape fields only, and its plan"""
    from bsed_amd import ops
    C, B, H, W, pool = case[:5]
    d = L.STRUCTS["BsedGluDesc"]()
    d.NB, d.H, d.W, d.C, d.act_bf16 = B, H, W, C, int(bf16)
    d.ph, d.pw = pool
    if C != 16:
        d.TH, d.TW = ops.tile_for(W)
    plan = L.STRUCTS["BsedGluPlan"]()
    L.check(L.lib().bsed_glu_plan(ctypes.byref(d), L.CONSTANTS["BSED_GLU_" + PLAN_ID[entry]], ctypes.byref(plan)), entry)
    return d, plan


def forced_Gs(case, plan):
    """The grid sizes other than the plan's that a launch with plan.max_G work items (tiles; tile pairs for glu_bwd3n;
    rows or row chunks for glu16) is run at: the table's G (half the natural G for glu16), clamped to max_G - 1 where
    the entry point has fewer items than the table's tile count supposes (glu_bwd3n's pairs).  Work item i goes to
    workgroup i % G, so the counts differ iff G does not divide max_G; where the table's G divides it, the smallest
    G >= 2 that does not is run as well."""
    if plan.max_G < 2:
        return []
    table_G = max(1, plan.G // 2) if case[0] == 16 else case[5]
    Gs = [] if table_G is None else [max(1, min(table_G, plan.max_G - 1))]
    if not any(plan.max_G % G for G in Gs):
        Gs += [G for G in range(2, plan.max_G) if plan.max_G % G and G != plan.G][:1]
    return Gs


# ---- inputs, masks and references: made once per case, never modified ----
@functools.lru_cache(maxsize=None)
def _inputs(case):
    C, B, H, W, pool = case[:5]
    g = torch.Generator().manual_seed(100000 * C + 1000 * H + 10 * W + B + pool[0])
    y = torch.randn(B, H, W, C, generator=g)
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g) * 0.3
    w = torch.randn(C, C, generator=g) / C ** 0.5
    bias = torch.randn(C, generator=g) * 0.1
    dpool = torch.randn(B, H // pool[0], W // pool[1], C, generator=g)
    return dict(y=y, scale=scale, shift=shift, w=w, bias=bias, dpool=dpool)


@functools.lru_cache(maxsize=None)
def _device_inputs(case, bf16=False):
    t = {k: v.cuda() for k, v in _inputs(case).items()}
    if bf16:
        t["y"], t["dpool"] = t["y"].bfloat16(), t["dpool"].bfloat16()
    return t


class Guarded:
    """an output tensor as a view into a NaN-filled buffer, one sentinel guard row below and one above it"""

    def __init__(self, shape, dtype=torch.float32):
        n = math.prod(shape)
        self.guard = GUARD_FLOATS * 4 // torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((n + 2 * self.guard,), math.nan, dtype=dtype, device="cuda")
        self.buf[:self.guard] = SENTINEL
        self.buf[self.guard + n:] = SENTINEL
        self.view = self.buf[self.guard:self.guard + n].view(shape)

    def check(self, what):
        assert not bool(torch.isnan(self.view).any()), f"{what}: elements of the output were not written"
        bits = torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32
        want = torch.full((self.guard,), SENTINEL, dtype=self.buf.dtype, device="cuda").view(bits)
        assert torch.equal(self.buf[:self.guard].view(bits), want), f"{what}: the guard row below was written"
        assert torch.equal(self.buf[-self.guard:].view(bits), want), f"{what}: the guard row above was written"


def launch(entry, case, p, G=None, bf16=False, inputs=None):
    """One launch of a BsedGluDesc entry point at grid size G (None: the plan's) into guarded outputs.  Returns the
    outputs on the CPU in float64, partial slabs reduced in float64: pooled | g, d_lin (glu_bwd3n), dW, db, st."""
    from bsed_amd import ops
    C, B, H, W, pool = case[:5]
    t = inputs or _device_inputs(case, bf16)
    d, plan = descriptor(entry, case, bf16)
    d.drop_p, d.rng_stream, d.seed = p, STREAM, SEED
    d.G = plan.G if G is None else G
    act = torch.bfloat16 if bf16 else torch.float32
    for name in ("scale", "shift", "w", "bias"):
        setattr(d, name, L.ptr(t[name]))
    d.y = L.ptr(t["y"], act)
    out, keep = {}, []
    if entry in FORWARD:
        out["pooled"] = Guarded((B, H // pool[0], W // pool[1], C), act)
        d.pooled = L.ptr(out["pooled"].view, act)
    else:
        d.dpool = L.ptr(t["dpool"], act)
        out["g"] = Guarded((B, H, W, C), act)
        d.g = L.ptr(out["g"].view, act)
        slabs = plan.dw_rows // plan.G
        if entry == "bsed_glu_bwd3n":
            out["d_lin"] = Guarded((B, H, W, C), act)
            d.dlin = L.ptr(out["d_lin"].view, act)
            keep.append(torch.empty(plan.table_bytes, device="cuda", dtype=torch.uint8))
            d.frag_table = keep[0].data_ptr()
        else:
            # plan.dw_rows * C * C elements at the natural G, G * slabs * C * C at a forced one
            out["part_dw"] = Guarded((plan.dw_rows if G is None else G * slabs, C, C))
            d.part_dw = L.ptr(out["part_dw"].view)
        if entry == "bsed_glu_bwd_fused":
            keep.append(ops.pack_weight(t["w"], 1, C, C, 0, 1, C))
            d.wfwd = L.ptr(keep[-1])
        out["part_db"], out["part_st"] = Guarded((d.G, 2, C)), Guarded((d.G, 2, C))
        d.part_db, d.part_st = L.ptr(out["part_db"].view), L.ptr(out["part_st"].view)
    L.call(entry, ctypes.byref(d), L.stream())
    torch.cuda.synchronize()
    for name, o in out.items():
        o.check(f"{entry} {case_id(case)} p={p} G={d.G} {name}")
    res = {name: out[name].view.double().cpu() for name in ("pooled", "g", "d_lin") if name in out}
    if entry == "bsed_glu_bwd3n":        # dW as the product takes it: a 1-tap weight gradient of the kernel's own d_lin
        part, _, _, _ = ops.wgrad(t["y"], out["d_lin"].view, B, H, W, C, C, a_scale=t["scale"], a_shift=t["shift"],
                                  mode="bf16x3")
        res["dW"] = part.double().sum(0)[0, :C, :C].t().cpu()          # slabs are [k = c][n]
    elif "part_dw" in out:
        res["dW"] = out["part_dw"].view.double().sum(0).cpu()          # slabs are [n][c]
    if "part_db" in out:
        res["db"] = out["part_db"].view.double().sum(0)[0].cpu()
        res["st"] = out["part_st"].view.double().sum(0).cpu()
    return res


@functools.lru_cache(maxsize=None)
def _mask(case, p):
    """the keep-mask (B,H,W,C) of 0/1 that the kernels of this case apply at drop probability p, stream STREAM, seed
    SEED, read back from the project's own kernels"""
    from bsed_amd import ops
    C, B, H, W, pool = case[:5]
    if p == 0.0:
        return torch.ones(B, H, W, C)
    if C != 16:      # drop_mul on the element index pos*C + n == the stand-alone dropout kernel on index i
        return (ops.dropout(torch.ones(B, H, W, C, device="cuda"), p, STREAM, SEED) != 0).float().cpu()
    # glu16: the 16-bit two-per-hash mask has no stand-alone kernel.  With W_lin = 0, bias = 1, scale = 1, shift = 0
    # and y = +30 at ONE slot of every pooling window, -30 elsewhere, res is sig*keep/(1-p) = keep/(1-p) at the slot
    # and < 1e-12 elsewhere, so pooled*ph*pw*(1-p) is the slot's keep bit.  Positions outside the pooled extent feed
    # nothing in either direction; their bits stay 1.
    ph, pw = pool
    Hp, Wp = H // ph, W // pw
    mask = torch.ones(B, H, W, C)
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    for dh in range(ph):
        for dw in range(pw):
            y = torch.full((B, H, W, C), -30.0)
            y[:, dh:Hp * ph:ph, dw:Wp * pw:pw] = 30.0
            probe = dict(y=y.cuda(), scale=one, shift=zero, w=torch.zeros(C, C, device="cuda"), bias=one)
            bit = launch("bsed_glu16_fwd", case, p, inputs=probe)["pooled"] * (ph * pw * (1.0 - p))
            assert bool(((bit.abs() <= 1e-3) | ((bit - 1.0).abs() <= 1e-3)).all()), "probe values are not keep bits"
            mask[:, dh:Hp * ph:ph, dw:Wp * pw:pw] = (bit > 0.5).float()
    return mask


@functools.lru_cache(maxsize=None)
def _reference(case, p, bf16=False):
    t = _inputs(case)
    y, dpool = (t["y"].bfloat16(), t["dpool"].bfloat16()) if bf16 else (t["y"], t["dpool"])
    return R.glu_reference(y, t["scale"], t["shift"], t["w"], t["bias"], case[4], _mask(case, p), p, dpool)


def compare(label, got, case, p, eps, failures, bf16=False):
    """bound (1) on every element of every output of `got`, then the precision bars (2); prints before it judges"""
    ref, comp, K = _reference(case, p, bf16)
    for name, val in got.items():
        assert val.shape == ref[name].shape, (label, name, val.shape)
        ratio = R.err_over_bound(val, ref[name], comp[name], K[name], eps)
        print(f"{label} {case_id(case)} p={p} {name}: max err/bound {ratio:.3f}")
        if not ratio <= 1.0:
            failures.append(f"{label} {name}: err/bound {ratio:.3f}")
        if bf16:
            continue
        err = val - ref[name]
        if name == "pooled":      # the bar of test_glu_forward_split_fp32_matches_torch
            e, bar = float(err.abs().max()), (2e-5 if p == 0.0 else 4e-5) * max(1.0, float(ref[name].abs().max()))
        else:                     # the bar of the kernel-vs-kernel backward tests
            e, bar = float(err.norm() / ref[name].norm()), 3e-5
        if not e <= bar:
            failures.append(f"{label} {name}: {e:.3e} above the bar {bar:.1e}")


def run_entry(entry, case, p, failures, bf16=False):
    """natural-G launch against the reference; every forced G against the reference and against the natural launch:
    bit for bit on the per-position outputs, within the bound on the reduced sums"""
    eps = R.EPS_BF16 if bf16 else EPS[entry]
    label = entry + ("[bf16]" if bf16 else "")
    nat = launch(entry, case, p, bf16=bf16)
    compare(label, nat, case, p, eps, failures, bf16)
    _, plan = descriptor(entry, case, bf16)
    ref, comp, K = _reference(case, p, bf16)
    for G in forced_Gs(case, plan):
        forced = launch(entry, case, p, G=G, bf16=bf16)
        compare(f"{label} G={G}", forced, case, p, eps, failures, bf16)
        for name, val in forced.items():
            if name in ("pooled", "g", "d_lin"):
                if not torch.equal(val, nat[name]):
                    n = int((val != nat[name]).sum())
                    failures.append(f"{label} G={G} {name}: {n} elements differ from the natural-G launch")
            elif not bool(((val - nat[name]).abs() <= R.bound(comp[name], K[name], eps)).all()):
                failures.append(f"{label} G={G} {name}: differs from the natural-G launch by more than the bound")


def run_igemm_routes(case, p, failures, unfused):
    """the fp32-mode forward (EPI_GLU_POOL) and, once per C, the unfused backward chain, through ops"""
    from bsed_amd import ops
    C, B, H, W, pool = case[:5]
    t = _device_inputs(case)
    args = (t["y"], t["scale"], t["shift"], t["w"], t["bias"])
    assert ops.glu_route("forward", C, W, pool, "fp32") == "igemm"
    pooled = ops.glu_forward(*args, B, H, W, C, pool, p, STREAM, SEED, mode="fp32")
    compare("igemm", {"pooled": pooled.double().cpu()}, case, p, EPS["igemm"], failures)
    if unfused:
        assert ops.glu_route("backward", C, W, pool, "fp32", fused=False) == "unfused"
        dw, db = torch.zeros(C, C, device="cuda"), torch.zeros(C, device="cuda")
        g, st = ops.glu_backward(*args, t["dpool"], B, H, W, C, pool, p, STREAM, SEED, mode="fp32", fused=False,
                                 dw=dw, db=db)
        got = {"g": g, "dW": dw, "db": db, "st": st.double().sum(0)}
        compare("unfused", {k: v.double().cpu() for k, v in got.items()}, case, p, EPS["unfused"], failures)


TILED_RUNS = [(c, p) for c in TILED for p in (0.0, 0.5)] + [(c, 0.25) for c in QUARTER if c[0] != 16]
GLU16_RUNS = [(c, p) for c in GLU16 for p in (0.0, 0.5)] + [(c, 0.25) for c in QUARTER if c[0] == 16]


@pytest.mark.parametrize("case,p", TILED_RUNS, ids=lambda v: case_id(v) if isinstance(v, tuple) else f"drop{v}")
def test_tiled_kernels_equal_the_float64_reference(case, p):
    failures = []
    for entry in entries_for(case):
        run_entry(entry, case, p, failures)
    run_igemm_routes(case, p, failures, unfused=FIRST_OF_C[case[0]] == case)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case,p", GLU16_RUNS, ids=lambda v: case_id(v) if isinstance(v, tuple) else f"drop{v}")
def test_glu16_kernels_equal_the_float64_reference(case, p):
    failures = []
    for entry in entries_for(case):
        run_entry(entry, case, p, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("C", [32, 64, 128])
def test_bf16_activation_instances_equal_the_float64_reference_of_the_rounded_inputs(C):
    """bf16 y / dpool in, bf16 pooled / g / d_lin out, p = 0.5, natural and forced G; bound (1) at EPS_BF16 and the
    bitwise agreement of the two grids (their precision bars stay at model level, tests/test_bf16_mode_gpu.py)"""
    case, failures = FIRST_OF_C[C], []
    for entry in entries_for(case):
        if entry in HAS_BF16:
            run_entry(entry, case, 0.5, failures, bf16=True)
    assert not failures, "\n".join(failures)


def test_dropout_masks_read_back_from_the_kernels_are_masks():
    """the probes of glu16 and the stand-alone kernel give 0/1 tensors with the keep rate of p, and the glu16 mask is
    not the tiled kernels' mask (two bits per hash against one): reading it back was necessary"""
    for case, p in ((GLU16[0], 0.5), (GLU16[2], 0.25), (TILED[0], 0.5), (TILED[5], 0.25)):
        _, _, H, W, (ph, pw) = case[:5]
        m = _mask(case, p)[:, :H // ph * ph, :W // pw * pw]       # the pooled extent: glu16's bits outside it are unread
        n = m.numel()
        assert bool(((m == 0) | (m == 1)).all())
        assert abs(float(m.mean()) - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / n) + 1.0 / n
    C, B, H, W, pool = GLU16[2]
    assert pool == (2, 2) and H % 2 == 0
    from bsed_amd import ops
    tiled_rule = (ops.dropout(torch.ones(B, H, W, C, device="cuda"), 0.5, STREAM, SEED) != 0).float().cpu()
    assert not torch.equal(tiled_rule, _mask(GLU16[2], 0.5))
