"""BsedGluDesc / bsed_glu_plan (no GPU): the grid sizes, slab counts and template choices of the eight GLU and first-block
entry points against a table written out from the measured values, their argument checks (all before the first HIP
call), and the KernelTimer labels ops builds from the plan's variant -- bench.py joins its roofline table on them."""
import ctypes

import pytest

from bsed_amd import _lib as L
from test_glu_route_cpu import FILTERS, FPN_LEVEL, POOLING, WIDTHS

K = {n[len("BSED_GLU_"):]: v for n, v in L.CONSTANTS.items() if n.startswith("BSED_GLU_")}
ENTRY = {"16_FWD": "bsed_glu16_fwd", "16_BWD": "bsed_glu16_bwd", "BLOCK0_FWD": "bsed_block0_fwd",
         "BLOCK0_BWD": "bsed_block0_bwd", "BWD_FUSED": "bsed_glu_bwd_fused", "FWD3": "bsed_glu_fwd3",
         "BWD3": "bsed_glu_bwd3", "BWD3N": "bsed_glu_bwd3n"}
STREAMING = ("16_FWD", "16_BWD", "BLOCK0_FWD", "BLOCK0_BWD")
HEIGHTS = [628, 314, 157, 157, 157, 157, 157]     # a 10 s clip through the pooling of the product configuration
TABLE_BYTES = 131072


def _tile(W):
    tw = min(W, 16)
    return 128 // tw, tw


def _desc(kernel, B, H, W, C, pool, abf=0):
    d = L.STRUCTS["BsedGluDesc"]()
    d.NB, d.H, d.W, d.C, d.act_bf16 = B, H, W, C, abf
    d.ph, d.pw = pool
    if kernel not in STREAMING:
        d.TH, d.TW = _tile(W)
    return d


def _plan(kernel, *shape, **kw):
    p = L.STRUCTS["BsedGluPlan"]()
    rc = L.lib().bsed_glu_plan(ctypes.byref(_desc(kernel, *shape, **kw)), K[kernel], ctypes.byref(p))
    assert rc == 0, (kernel, shape, L.lib().bsed_last_error().decode())
    return p.G, p.dw_rows, p.table_bytes, p.variant


def test_one_plan_id_per_entry_point_and_the_retired_queries_are_gone():
    assert sorted(K.values()) == list(range(8)) and set(K) == set(ENTRY)
    assert set(ENTRY.values()) <= set(L.FUNCTIONS) and L.lib().bsed_abi_version() >= 11
    for name in ("bsed_glu_fwd3_auto_g", "bsed_glu_bwd3_auto_g", "bsed_glu_bwd_slabs", "bsed_glu_bwd3_slabs",
                 "bsed_glu_bwd3n_table_bytes"):
        assert name not in L.FUNCTIONS
    for entry in ENTRY.values():
        assert L.FUNCTIONS[entry] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])


# (kernel, B, H, W, C, pool, act_bf16) -> (G, dw_rows, table_bytes, variant), worked out by hand from
# ntiles = B * ceil(H / TH) * (W / TW) and the grid table of the kernels
LITERAL = {
    # first block, (628, 128) map, pool (2, 2): 314 pooled rows per clip
    ("16_FWD", 256, 628, 128, 16, (2, 2), 0): (8192, 0, 0, 0),
    ("16_FWD", 24, 628, 128, 16, (2, 2), 0): (7536, 0, 0, 0),
    ("16_BWD", 256, 628, 128, 16, (2, 2), 0): (2048, 2048, 0, 0),
    ("16_BWD", 24, 628, 128, 16, (2, 2), 0): (2048, 2048, 0, 0),
    ("BLOCK0_FWD", 256, 628, 128, 16, (2, 2), 0): (8192, 0, 0, 2 | 16),
    ("BLOCK0_FWD", 256, 628, 128, 16, (2, 2), 1): (8192, 0, 0, 2),          # the bf16 forward is built without SMALL
    ("BLOCK0_FWD", 24, 628, 128, 16, (2, 2), 0): (7536, 0, 0, 2 | 16),
    ("BLOCK0_BWD", 256, 628, 128, 16, (2, 2), 0): (8192, 8192, 0, 2 | 16),
    ("BLOCK0_BWD", 256, 628, 128, 16, (2, 2), 1): (8192, 8192, 0, 2 | 16),
    ("BLOCK0_BWD", 24, 628, 128, 16, (2, 2), 0): (7536, 7536, 0, 2 | 16),
    # block 1: C = 32, (314, 64), tile 8 x 16: 40 * 4 tiles per clip
    ("FWD3", 256, 314, 64, 32, (2, 2), 0): (1536, 0, 0, 4),
    ("BWD3", 256, 314, 64, 32, (2, 2), 0): (768, 3072, 0, 4),
    ("BWD_FUSED", 256, 314, 64, 32, (2, 2), 0): (768, 3072, 0, 4),
    ("FWD3", 24, 314, 64, 32, (2, 2), 1): (1536, 0, 0, 4),
    # block 2: C = 64, (157, 32): 20 * 2 tiles per clip
    ("FWD3", 256, 157, 32, 64, (1, 2), 0): (1536, 0, 0, 4),
    ("BWD3", 256, 157, 32, 64, (1, 2), 1): (512, 2048, 0, 4),
    ("BWD_FUSED", 256, 157, 32, 64, (1, 2), 0): (512, 1024, 0, 4),
    ("BWD3", 24, 157, 32, 64, (1, 2), 0): (512, 2048, 0, 4),               # 960 tiles
    # block 3: C = 128, (157, 16): 20 tiles per clip
    ("FWD3", 256, 157, 16, 128, (1, 2), 0): (512, 0, 0, 4),
    ("BWD3N", 256, 157, 16, 128, (1, 2), 0): (256, 0, TABLE_BYTES, 0),
    ("BWD_FUSED", 256, 157, 16, 128, (1, 2), 0): (256, 256, 0, 8),
    ("BWD3N", 24, 157, 16, 128, (1, 2), 0): (240, 0, TABLE_BYTES, 0),      # 480 tiles, two at a time
    # block 6: C = 128, (157, 2), tile 64 x 2: 3 tiles per clip
    ("FWD3", 256, 157, 2, 128, (1, 2), 0): (512, 0, 0, -1),
    ("BWD3N", 256, 157, 2, 128, (1, 2), 1): (256, 0, TABLE_BYTES, 0),
    ("FWD3", 24, 157, 2, 128, (1, 2), 0): (72, 0, 0, -1),
    ("BWD3N", 24, 157, 2, 128, (1, 2), 0): (36, 0, TABLE_BYTES, 0),
    ("BWD_FUSED", 24, 157, 2, 128, (1, 2), 0): (72, 72, 0, 8),
    # feature-pyramid level: W = 1, tile 128 x 1: 2 tiles per clip
    ("FWD3", 24, 157, 1, 128, (2, 1), 0): (48, 0, 0, -1),
    ("BWD3N", 24, 157, 1, 128, (2, 1), 0): (24, 0, TABLE_BYTES, 0),
    # edges: H = 1; H no multiple of TH (130 = 2 * 64 + 2) with an odd tile count for glu3n
    ("FWD3", 2, 1, 16, 32, (1, 2), 0): (2, 0, 0, 4),
    ("BWD3", 2, 1, 16, 32, (1, 2), 0): (2, 8, 0, 4),
    ("BWD_FUSED", 2, 1, 16, 64, (1, 2), 0): (2, 4, 0, 4),
    ("16_FWD", 2, 1, 16, 16, (1, 2), 0): (2, 0, 0, 0),
    ("16_BWD", 2, 1, 16, 16, (1, 2), 0): (2, 2, 0, 0),
    ("BLOCK0_BWD", 2, 1, 16, 16, (1, 2), 0): (2, 2, 0, 1 | 16),
    ("BWD3N", 1, 130, 2, 128, (1, 2), 0): (2, 0, TABLE_BYTES, 0),           # 3 tiles -> 2 workgroups
    ("BWD3N", 3, 130, 2, 128, (1, 2), 0): (5, 0, TABLE_BYTES, 0),           # 9 tiles -> 5
    ("FWD3", 1, 130, 2, 128, (1, 2), 0): (3, 0, 0, -1),
    ("BWD_FUSED", 1, 130, 2, 128, (1, 2), 0): (3, 3, 0, 8),
    # block0's SMALL on both sides of 2^28 positions (2048 * 1024 * 128 = 2^28)
    ("BLOCK0_FWD", 2048, 1023, 128, 16, (1, 2), 0): (8192, 0, 0, 1 | 16),
    ("BLOCK0_FWD", 2048, 1024, 128, 16, (1, 2), 0): (8192, 0, 0, 1),
    ("BLOCK0_BWD", 2048, 1023, 128, 16, (2, 2), 1): (8192, 8192, 0, 2 | 16),
    ("BLOCK0_BWD", 2048, 1024, 128, 16, (2, 2), 1): (8192, 8192, 0, 2),
    # block0_fwd takes 128 columns per work item: two chunks per pooled row at W = 192
    ("BLOCK0_FWD", 2, 18, 192, 16, (2, 2), 0): (36, 0, 0, 2 | 16),
    ("BLOCK0_BWD", 2, 18, 192, 16, (2, 2), 0): (18, 18, 0, 2 | 16),
}


@pytest.mark.parametrize("case", list(LITERAL), ids=lambda c: "-".join(map(str, c[:5])) + f"-p{c[5][0]}{c[5][1]}-ab{c[6]}")
def test_plan_equals_the_literal_table(case):
    kernel, *shape, abf = case
    assert _plan(kernel, *shape, abf=abf) == LITERAL[case]


def _formula(kernel, B, H, W, C, pool):
    """(G, dw_rows, table_bytes) from the grid table of the kernels, restated"""
    ph = pool[0]
    TH, TW = _tile(W)
    ntiles = B * ((H + TH - 1) // TH) * (W // TW)
    if kernel == "16_FWD":
        return min(B * (H // ph), 8192), 0, 0
    if kernel == "16_BWD":
        return min(2048, B * H), min(2048, B * H), 0
    if kernel == "BLOCK0_FWD":
        return min(B * (H // ph) * ((W + 127) // 128), 8192), 0, 0
    if kernel == "BLOCK0_BWD":
        return min(8192, B * (H // ph)), min(8192, B * (H // ph)), 0
    if kernel == "BWD_FUSED":
        G = min(ntiles, {128: 256, 64: 512, 32: 768}[C])
        return G, G * {128: 1, 64: 2, 32: 4}[C], 0
    if kernel == "FWD3":
        return min(ntiles, 512 if C == 128 else 1536), 0, 0
    if kernel == "BWD3":
        G = min(ntiles, 768 if C == 32 else 512)
        return G, 4 * G, 0
    return min((ntiles + 1) // 2, 256), 0, TABLE_BYTES


def _kernels_for(C):
    return STREAMING if C == 16 else ("BWD_FUSED", "FWD3") + (("BWD3N",) if C == 128 else ("BWD3",))


@pytest.mark.parametrize("B", [256, 24])
def test_plan_of_every_product_shape(B):
    shapes = list(zip(FILTERS, HEIGHTS, WIDTHS, POOLING)) + [(FPN_LEVEL[0], 157, FPN_LEVEL[1], FPN_LEVEL[2])]
    for C, H, W, pool in shapes:
        for kernel in _kernels_for(C):
            got = _plan(kernel, B, H, W, C, pool)
            assert got[:3] == _formula(kernel, B, H, W, C, pool), (kernel, C, H, W)
            if kernel in ("FWD3", "BWD3"):
                assert got[3] == (4 if W >= 16 else -1)


@pytest.mark.parametrize("W", [2, 4, 8, 16, 32, 64])
def test_plan_of_every_tile_width(W):
    for C in (32, 64, 128):
        for kernel in _kernels_for(C):
            for H in (1, 10, 130):
                got = _plan(kernel, 2, H, W, C, (1, 2))
                assert got[:3] == _formula(kernel, 2, H, W, C, (1, 2)), (kernel, C, H, W)
                assert got[3] == {"BWD_FUSED": 8 if C == 128 else 4, "BWD3N": 0}.get(kernel, 4 if W >= 16 else -1)


# ---- argument checks of the eight entry points: every one runs before the first HIP call ----
READS = {"16_FWD": "y scale shift w bias pooled", "16_BWD": "y scale shift w bias dpool g part_dw part_db part_st",
         "BLOCK0_FWD": "x cw cb scale shift w bias pooled",
         "BLOCK0_BWD": "x cw cb scale shift w bias dpool part_dw part_db part_st part_gx",
         "BWD_FUSED": "y scale shift w wfwd bias dpool g part_dw part_db part_st",
         "FWD3": "y scale shift w bias pooled", "BWD3": "y scale shift w bias dpool g part_dw part_db part_st",
         "BWD3N": "y scale shift w bias dpool g dlin part_db part_st frag_table"}
POINTERS = "x y cw cb scale shift w wfwd bias dpool pooled g dlin part_dw part_db part_st part_gx frag_table".split()
DEFECTS = ("null tensor", "unused tensor", "C", "TH*TW", "TW does not divide W", "pool 3", "G = 0", "G too large")


def _valid(kernel):
    """a descriptor the entry point accepts, with dummy non-null pointers (never dereferenced on the host)"""
    C = 16 if kernel in STREAMING else 128 if kernel == "BWD3N" else 64
    d = _desc(kernel, 2, 16, 32, C, (1, 2))
    for name in READS[kernel].split():
        setattr(d, name, 0x1000)
    d.G = 1
    return d


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("kernel", list(ENTRY))
def test_ill_formed_descriptor_is_rejected_before_any_hip_call(kernel, defect):
    lib = L.lib()
    d = _valid(kernel)
    p = L.STRUCTS["BsedGluPlan"]()
    assert lib.bsed_glu_plan(ctypes.byref(d), K[kernel], ctypes.byref(p)) == 0      # the base descriptor is well formed
    assert 1 <= p.G <= p.max_G
    want = ""
    if defect == "null tensor":
        name = READS[kernel].split()[-1]
        setattr(d, name, None)
        want = "null tensor " + name
    elif defect == "unused tensor":
        name = next(n for n in POINTERS if n not in READS[kernel].split())
        setattr(d, name, 0x1000)
        want = "does not read " + name
    elif defect == "C":
        d.C = 48
        want = "built for"
    elif defect == "TH*TW":
        d.TH, d.TW = 4, 16
        want = "TH = TW = 0" if kernel in STREAMING else "TH*TW must be 128"
    elif defect == "TW does not divide W":
        d.TH, d.TW, d.W = 8, 16, 24
        want = "TH = TW = 0" if kernel in STREAMING else "TW must divide W"
    elif defect == "pool 3":
        d.pw = 3
        want = "pooling windows"
    elif defect == "G = 0":
        d.G = 0
        want = "G must be in 1.."
    else:
        d.G = p.max_G + 1
        want = f"G must be in 1..{p.max_G}"
    rc = getattr(lib, ENTRY[kernel])(ctypes.byref(d), None)
    msg = lib.bsed_last_error().decode()
    assert rc == -1, (kernel, defect, rc, msg)                      # BSED_ERR_ARG: no HIP call was reached
    assert msg.startswith(ENTRY[kernel] + ":") and want in msg, (kernel, defect, msg)


def test_null_descriptor_and_unknown_kernel():
    lib = L.lib()
    for entry in ENTRY.values():
        assert getattr(lib, entry)(None, None) == -1 and lib.bsed_last_error().decode().startswith(entry + ":")
    p = L.STRUCTS["BsedGluPlan"]()
    assert lib.bsed_glu_plan(ctypes.byref(_valid("FWD3")), 8, ctypes.byref(p)) == -1
    assert lib.bsed_glu_plan(None, 0, ctypes.byref(p)) == -1


# ---- the labels of ops.KernelTimer, as the expressions of the positional-argument wrappers gave them ----
LABELS = {
    "fp32": ["glu16_fwd_kernel", "glu16_bwd_kernel", "b0_fwd_kernel<2, true, 0>", "b0_bwd_kernel<2, true, 0>",
             "glu_bwd_fused_kernel<32, 4>", "glu_fwd3_kernel<32, 4, 0>", "glu_bwd3_kernel<32, 4, 0>",
             "glu_bwd_fused_kernel<64, 4>", "glu_fwd3_kernel<64, 4, 0>", "glu_bwd3_kernel<64, 4, 0>",
             "glu_bwd_fused_kernel<128, 8>", "glu_fwd3_kernel<128, 4, 0>", "glu_bwd3n_kernel<0>"] +
            ["glu_bwd_fused_kernel<128, 8>", "glu_fwd3_kernel<128, -1, 0>", "glu_bwd3n_kernel<0>"] * 3,
    "bf16": ["b0_fwd_kernel<2, false, 1>", "b0_bwd_kernel<2, true, 1>",
             "glu_fwd3_kernel<32, 4, 1>", "glu_bwd3_kernel<32, 4, 1>", "glu_fwd3_kernel<64, 4, 1>",
             "glu_bwd3_kernel<64, 4, 1>", "glu_fwd3_kernel<128, 4, 1>", "glu_bwd3n_kernel<1>"] +
            ["glu_fwd3_kernel<128, -1, 1>", "glu_bwd3n_kernel<1>"] * 3,
}


@pytest.mark.parametrize("B", [256, 24])
def test_kernel_timer_labels_of_the_product_shapes(B):
    from bsed_amd import ops

    def label(kernel, C, H, W, pool, abf):
        d = _desc(kernel, B, H, W, C, pool, abf)
        return ops._glu_label(ENTRY[kernel], d, ops._glu_plan(ENTRY[kernel], d))

    shapes = list(zip(FILTERS, HEIGHTS, WIDTHS, POOLING))
    got = {"fp32": [], "bf16": []}
    for C, H, W, pool in shapes:
        for kernel in _kernels_for(C):
            got["fp32"].append(label(kernel, C, H, W, pool, 0))
            if kernel not in ("16_FWD", "16_BWD", "BWD_FUSED"):
                got["bf16"].append(label(kernel, C, H, W, pool, 1))
    assert got == LABELS
