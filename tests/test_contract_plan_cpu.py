"""BsedContractPlan / bsed_igemm_plan / bsed_wgrad_plan (no GPU): the grid size, the rows of statistics and the
KernelTimer label -- bench.py joins its roofline table on it -- of the six contraction entry points.

Origin of the literal table: it was recorded from the commit BEFORE the plan queries existed, on a CPU box (every query
involved is host only): G and the statistics rows from the queries this change retired (bsed_igemm_num_tiles,
bsed_igemm3s_auto_g2, bsed_igemm3n_stats_rows, bsed_wgrad_auto_g, bsed_wgrad3_auto_g), the labels from the expressions
ops.py then restated (kc / bn / pv / nv) and from its decoders of bsed_igemm3n_variant, bsed_wgrad_variant and
bsed_wgrad3_variant.  The knob table was recorded the same way."""
import ctypes
import os

import pytest

from bsed_amd import _lib as L
from test_capi_cpu import _CONV_ENTRIES, _GEOMETRY_DEFECTS, _conv_desc
from test_contract_route_cpu import FILTERS, OTHERS, WIDTHS
from test_glu_desc_cpu import HEIGHTS

K = {n[len("BSED_CONTRACT_"):].lower(): v for n, v in L.CONSTANTS.items() if n.startswith("BSED_CONTRACT_")}
TAPS = {9: [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)], 3: [(-1, 0), (0, 0), (1, 0)], 1: [(0, 0)],
        4: [(0, 0), (0, 1), (1, 0), (1, 1)]}      # 3 x 3, the width-1 centre column, a plain GEMM, space-to-depth
T = 157                                            # frames of a 10 s clip behind the CNN
RETIRED = ("bsed_igemm_num_tiles", "bsed_igemm3s_auto_g", "bsed_igemm3s_auto_g2", "bsed_igemm3n_stats_rows",
           "bsed_igemm3n_variant", "bsed_wgrad_auto_g", "bsed_wgrad_variant", "bsed_wgrad3_auto_g", "bsed_wgrad3_variant")


def _tile(W):
    tw = min(W, 16)
    return 128 // tw, tw


def _desc(kernel, NB, H, W, CIN, N, ntaps, flag, abf):
    """descriptor with all pointers null; flag = the epilogue (igemm*: 0 PLAIN, 1 STATS) or bn_y set (wgrad*)"""
    wg = kernel.startswith("wgrad")
    d = L.STRUCTS["BsedWgradDesc" if wg else "BsedIgemmDesc"]()
    d.NB, d.H, d.W, d.CIN, d.N, d.NP = NB, H, W, CIN, N, (N + 31) // 32 * 32
    d.TH, d.TW = _tile(W)
    taps = TAPS[ntaps]
    d.ntaps = ntaps
    for i, (a, b) in enumerate(taps):
        d.dh[i], d.dw[i] = a, b
    d.hh, d.hw = max(abs(a) for a, _ in taps), max(abs(b) for _, b in taps)
    d.in_pitch, d.act_bf16 = CIN, abf
    if wg:
        d.dy_pitch, d.CINP = N, (CIN + 31) // 32 * 32
        if flag:
            d.bn_y = d.bn_coef = d.bn_mean = 0x1000
    else:
        d.out_pitch = d.e_pitch = N
        d.ph = d.pw = 1
        d.Hp, d.Wp = H, W
        d.epilogue = flag
    return d


def _plan(kernel, d):
    p = L.STRUCTS["BsedContractPlan"]()
    query = L.lib().bsed_wgrad_plan if kernel.startswith("wgrad") else L.lib().bsed_igemm_plan
    rc = query(ctypes.byref(d), K[kernel], ctypes.byref(p))
    return rc, p


def _cases():
    """(kernel, H, W, CIN, N, ntaps, flag, abf) of the product configuration; H = 0: a linear layer over B * T rows
    (NB = 1, W = 1), otherwise NB = B"""
    out = []

    def family(H, W, cin, n, ntaps, bn=True):
        for k, m, epi in ((cin, n, 1 if bn else 0), (n, cin, 0)):      # forward (STATS under a BatchNorm), data gradient
            out.append(("igemm", H, W, k, m, ntaps, epi, 0))
            if ntaps == 9 and k in (16, 32) and m <= 32:
                out.extend(("igemm3s", H, W, k, m, ntaps, epi, ab) for ab in (0, 1))
            if k % 32 == 0:
                out.append(("igemm3", H, W, k, m, ntaps, epi, 0))
                out.extend(("igemm3n", H, W, k, m, ntaps, epi, ab) for ab in (0, 1))
        out.append(("wgrad", H, W, cin, n, ntaps, 0, 0))
        for f in ((0, 1) if bn else (0,)):
            out.extend(("wgrad3", H, W, cin, n, ntaps, f, ab) for ab in (0, 1))

    for i in range(1, 7):
        family(HEIGHTS[i], WIDTHS[i], FILTERS[i - 1], FILTERS[i], 9)
        c = FILTERS[i]                                                  # the GLU's Linear weight gradient: 1 tap, C -> C
        out.append(("wgrad", HEIGHTS[i], WIDTHS[i], c, c, 1, 0, 0))
        out.extend(("wgrad3", HEIGHTS[i], WIDTHS[i], c, c, 1, 0, ab) for ab in (0, 1))
    for cin, n, W, ntaps in OTHERS:
        if ntaps == 1:
            family(0, 1, cin, n, 1, bn=False)      # GRU projections, the FPN fuse, dense_softmax, the frame discriminator
        elif ntaps == 3:
            family(T, W, cin, n, 3)                # the width-1 feature-pyramid level
        else:
            family(W, W, cin, n, 4)                # the clip discriminator's space-to-depth layers
    return out


# key of _cases() -> (label, (G, stats_rows) at B = 24, (G, stats_rows) at B = 256)
LITERAL = {
    ("igemm", 314, 64, 16, 32, 9, 1, 0): ("igemm_kernel<16, 32, 1>", (3840, 3840), (40960, 40960)),
    ("igemm3s", 314, 64, 16, 32, 9, 1, 0): ("igemm3s_kernel<1, 9, 1, 32, 0>", (1024, 1024), (1024, 1024)),
    ("igemm3s", 314, 64, 16, 32, 9, 1, 1): ("igemm3s_kernel<1, 9, 1, 32, 1>", (1024, 1024), (1024, 1024)),
    ("igemm", 314, 64, 32, 16, 9, 0, 0): ("igemm_kernel<32, 32, 0>", (3840, 3840), (40960, 40960)),
    ("igemm3s", 314, 64, 32, 16, 9, 0, 0): ("igemm3s_kernel<0, 9, 2, 16, 0>", (768, 768), (768, 768)),
    ("igemm3s", 314, 64, 32, 16, 9, 0, 1): ("igemm3s_kernel<0, 9, 2, 16, 1>", (768, 768), (768, 768)),
    ("igemm3", 314, 64, 32, 16, 9, 0, 0): ("igemm3_kernel<32, 0, 1, 6>", (3840, 3840), (40960, 40960)),
    ("igemm3n", 314, 64, 32, 16, 9, 0, 0): ("igemm3n_kernel<1, 4, 0, 6, 1, 3, 0, 1>", (3840, 15360), (40960, 163840)),
    ("igemm3n", 314, 64, 32, 16, 9, 0, 1): ("igemm3n_kernel<1, 4, 0, 3, 1, 3, 1, 0>", (3840, 15360), (40960, 163840)),
    ("wgrad", 314, 64, 16, 32, 9, 0, 0): ("wgrad_kernel<2, 4>", (512, 0), (512, 0)),
    ("wgrad3", 314, 64, 16, 32, 9, 0, 0): ("wgrad3p_kernel<3, 6, 0>", (256, 0), (256, 0)),
    ("wgrad3", 314, 64, 16, 32, 9, 0, 1): ("wgrad3p_kernel<3, 6, 1>", (256, 0), (256, 0)),
    ("wgrad3", 314, 64, 16, 32, 9, 1, 0): ("wgrad3p_kernel<3, 6, 0>", (256, 0), (256, 0)),
    ("wgrad3", 314, 64, 16, 32, 9, 1, 1): ("wgrad3p_kernel<3, 6, 1>", (256, 0), (256, 0)),
    ("wgrad", 314, 64, 32, 32, 1, 0, 0): ("wgrad_kernel<1, 4>", (512, 0), (512, 0)),
    ("wgrad3", 314, 64, 32, 32, 1, 0, 0): ("wgrad3_kernel<1, 4, true, 0>", (1024, 0), (1024, 0)),
    ("wgrad3", 314, 64, 32, 32, 1, 0, 1): ("wgrad3_kernel<1, 4, true, 1>", (1024, 0), (1024, 0)),
    ("igemm", 157, 32, 32, 64, 9, 1, 0): ("igemm_kernel<32, 64, 1>", (960, 960), (10240, 10240)),
    ("igemm3", 157, 32, 32, 64, 9, 1, 0): ("igemm3_kernel<64, 1, 1, 6>", (960, 960), (10240, 10240)),
    ("igemm3n", 157, 32, 32, 64, 9, 1, 0): ("igemm3n_kernel<2, 2, 1, 6, 1, 3, 0, 1>", (960, 1920), (10240, 20480)),
    ("igemm3n", 157, 32, 32, 64, 9, 1, 1): ("igemm3n_kernel<2, 2, 1, 3, 1, 3, 1, 0>", (960, 1920), (10240, 20480)),
    ("igemm", 157, 32, 64, 32, 9, 0, 0): ("igemm_kernel<32, 32, 0>", (960, 960), (10240, 10240)),
    ("igemm3", 157, 32, 64, 32, 9, 0, 0): ("igemm3_kernel<32, 0, 1, 6>", (960, 960), (10240, 10240)),
    ("igemm3n", 157, 32, 64, 32, 9, 0, 0): ("igemm3n_kernel<1, 4, 0, 6, 1, 3, 0, 1>", (960, 3840), (10240, 40960)),
    ("igemm3n", 157, 32, 64, 32, 9, 0, 1): ("igemm3n_kernel<1, 4, 0, 3, 1, 3, 1, 0>", (960, 3840), (10240, 40960)),
    ("wgrad", 157, 32, 32, 64, 9, 0, 0): ("wgrad_kernel<5, 4>", (512, 0), (512, 0)),
    ("wgrad3", 157, 32, 32, 64, 9, 0, 0): ("wgrad3p_kernel<5, 3, 0>", (256, 0), (256, 0)),
    ("wgrad3", 157, 32, 32, 64, 9, 0, 1): ("wgrad3p_kernel<5, 3, 1>", (256, 0), (256, 0)),
    ("wgrad3", 157, 32, 32, 64, 9, 1, 0): ("wgrad3p_kernel<5, 3, 0>", (256, 0), (256, 0)),
    ("wgrad3", 157, 32, 32, 64, 9, 1, 1): ("wgrad3p_kernel<5, 3, 1>", (256, 0), (256, 0)),
    ("wgrad", 157, 32, 64, 64, 1, 0, 0): ("wgrad_kernel<1, 4>", (512, 0), (512, 0)),
    ("wgrad3", 157, 32, 64, 64, 1, 0, 0): ("wgrad3_kernel<1, 4, true, 0>", (512, 0), (512, 0)),
    ("wgrad3", 157, 32, 64, 64, 1, 0, 1): ("wgrad3_kernel<1, 4, true, 1>", (512, 0), (512, 0)),
    ("igemm", 157, 16, 64, 128, 9, 1, 0): ("igemm_kernel<32, 128, 1>", (480, 480), (5120, 5120)),
    ("igemm3", 157, 16, 64, 128, 9, 1, 0): ("igemm3_kernel<128, 1, 1, 6>", (480, 480), (5120, 5120)),
    ("igemm3n", 157, 16, 64, 128, 9, 1, 0): ("igemm3n_kernel<4, 1, 1, 6, 1, 2, 0, 1>", (480, 480), (5120, 5120)),
    ("igemm3n", 157, 16, 64, 128, 9, 1, 1): ("igemm3n_kernel<4, 1, 1, 3, 1, 3, 1, 0>", (480, 480), (5120, 5120)),
    ("igemm", 157, 16, 128, 64, 9, 0, 0): ("igemm_kernel<32, 64, 0>", (480, 480), (5120, 5120)),
    ("igemm3", 157, 16, 128, 64, 9, 0, 0): ("igemm3_kernel<64, 0, 1, 6>", (480, 480), (5120, 5120)),
    ("igemm3n", 157, 16, 128, 64, 9, 0, 0): ("igemm3n_kernel<2, 2, 0, 6, 1, 3, 0, 1>", (480, 960), (5120, 10240)),
    ("igemm3n", 157, 16, 128, 64, 9, 0, 1): ("igemm3n_kernel<2, 2, 0, 3, 1, 3, 1, 0>", (480, 960), (5120, 10240)),
    ("wgrad", 157, 16, 64, 128, 9, 0, 0): ("wgrad_kernel<9, 4>", (256, 0), (256, 0)),
    ("wgrad3", 157, 16, 64, 128, 9, 0, 0): ("wgrad3p_kernel<9, 1, 0>", (128, 0), (128, 0)),
    ("wgrad3", 157, 16, 64, 128, 9, 0, 1): ("wgrad3p_kernel<9, 1, 1>", (128, 0), (128, 0)),
    ("wgrad3", 157, 16, 64, 128, 9, 1, 0): ("wgrad3p_kernel<9, 1, 0>", (128, 0), (128, 0)),
    ("wgrad3", 157, 16, 64, 128, 9, 1, 1): ("wgrad3p_kernel<9, 1, 1>", (128, 0), (128, 0)),
    ("wgrad", 157, 16, 128, 128, 1, 0, 0): ("wgrad_kernel<2, 8>", (256, 0), (256, 0)),
    ("wgrad3", 157, 16, 128, 128, 1, 0, 0): ("wgrad1_kernel<false, 0>", (256, 0), (256, 0)),
    ("wgrad3", 157, 16, 128, 128, 1, 0, 1): ("wgrad1_kernel<false, 1>", (256, 0), (256, 0)),
    ("igemm", 157, 8, 128, 128, 9, 1, 0): ("igemm_kernel<32, 128, 1>", (240, 240), (2560, 2560)),
    ("igemm3", 157, 8, 128, 128, 9, 1, 0): ("igemm3_kernel<128, 1, 1, 6>", (240, 240), (2560, 2560)),
    ("igemm3n", 157, 8, 128, 128, 9, 1, 0): ("igemm3n_kernel<4, 1, 1, 6, 1, 2, 0, 1>", (240, 240), (2560, 2560)),
    ("igemm3n", 157, 8, 128, 128, 9, 1, 1): ("igemm3n_kernel<4, 1, 1, 3, 1, 3, 1, 0>", (240, 240), (2560, 2560)),
    ("igemm", 157, 8, 128, 128, 9, 0, 0): ("igemm_kernel<32, 128, 0>", (240, 240), (2560, 2560)),
    ("igemm3", 157, 8, 128, 128, 9, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (240, 240), (2560, 2560)),
    ("igemm3n", 157, 8, 128, 128, 9, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 1, 2, 0, 1>", (240, 240), (2560, 2560)),
    ("igemm3n", 157, 8, 128, 128, 9, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 1, 3, 1, 0>", (240, 240), (2560, 2560)),
    ("wgrad", 157, 8, 128, 128, 9, 0, 0): ("wgrad_kernel<9, 4>", (128, 0), (128, 0)),
    ("wgrad3", 157, 8, 128, 128, 9, 0, 0): ("wgrad3p_kernel<9, 2, 0>", (64, 0), (64, 0)),
    ("wgrad3", 157, 8, 128, 128, 9, 0, 1): ("wgrad3p_kernel<9, 2, 1>", (64, 0), (64, 0)),
    ("wgrad3", 157, 8, 128, 128, 9, 1, 0): ("wgrad3p_kernel<9, 2, 0>", (64, 0), (64, 0)),
    ("wgrad3", 157, 8, 128, 128, 9, 1, 1): ("wgrad3p_kernel<9, 2, 1>", (64, 0), (64, 0)),
    ("wgrad", 157, 8, 128, 128, 1, 0, 0): ("wgrad_kernel<2, 8>", (240, 0), (256, 0)),
    ("wgrad3", 157, 8, 128, 128, 1, 0, 0): ("wgrad1_kernel<false, 0>", (240, 0), (256, 0)),
    ("wgrad3", 157, 8, 128, 128, 1, 0, 1): ("wgrad1_kernel<false, 1>", (240, 0), (256, 0)),
    ("igemm", 157, 4, 128, 128, 9, 1, 0): ("igemm_kernel<32, 128, 1>", (120, 120), (1280, 1280)),
    ("igemm3", 157, 4, 128, 128, 9, 1, 0): ("igemm3_kernel<128, 1, 1, 9>", (120, 120), (1280, 1280)),
    ("igemm3n", 157, 4, 128, 128, 9, 1, 0): ("igemm3n_kernel<4, 1, 1, 9, 1, 2, 0, 1>", (120, 120), (1280, 1280)),
    ("igemm3n", 157, 4, 128, 128, 9, 1, 1): ("igemm3n_kernel<4, 1, 1, 5, 1, 3, 1, 0>", (120, 120), (1280, 1280)),
    ("igemm", 157, 4, 128, 128, 9, 0, 0): ("igemm_kernel<32, 128, 0>", (120, 120), (1280, 1280)),
    ("igemm3", 157, 4, 128, 128, 9, 0, 0): ("igemm3_kernel<128, 0, 1, 9>", (120, 120), (1280, 1280)),
    ("igemm3n", 157, 4, 128, 128, 9, 0, 0): ("igemm3n_kernel<4, 1, 0, 9, 1, 2, 0, 1>", (120, 120), (1280, 1280)),
    ("igemm3n", 157, 4, 128, 128, 9, 0, 1): ("igemm3n_kernel<4, 1, 0, 5, 1, 3, 1, 0>", (120, 120), (1280, 1280)),
    ("wgrad", 157, 4, 128, 128, 9, 0, 0): ("wgrad_kernel<5, 4>", (64, 0), (64, 0)),
    ("wgrad3", 157, 4, 128, 128, 9, 0, 0): ("wgrad3p_kernel<5, 4, 0>", (32, 0), (32, 0)),
    ("wgrad3", 157, 4, 128, 128, 9, 0, 1): ("wgrad3p_kernel<5, 4, 1>", (32, 0), (32, 0)),
    ("wgrad3", 157, 4, 128, 128, 9, 1, 0): ("wgrad3p_kernel<5, 4, 0>", (32, 0), (32, 0)),
    ("wgrad3", 157, 4, 128, 128, 9, 1, 1): ("wgrad3p_kernel<5, 4, 1>", (32, 0), (32, 0)),
    ("wgrad", 157, 4, 128, 128, 1, 0, 0): ("wgrad_kernel<2, 8>", (120, 0), (256, 0)),
    ("wgrad3", 157, 4, 128, 128, 1, 0, 0): ("wgrad1_kernel<false, 0>", (120, 0), (256, 0)),
    ("wgrad3", 157, 4, 128, 128, 1, 0, 1): ("wgrad1_kernel<false, 1>", (120, 0), (256, 0)),
    ("igemm", 157, 2, 128, 128, 9, 1, 0): ("igemm_kernel<32, 128, 1>", (72, 72), (768, 768)),
    ("igemm3", 157, 2, 128, 128, 9, 1, 0): ("igemm3_kernel<128, 1, 1, 9>", (72, 72), (768, 768)),
    ("igemm3n", 157, 2, 128, 128, 9, 1, 0): ("igemm3n_kernel<4, 1, 1, 9, 1, 2, 0, 1>", (72, 72), (768, 768)),
    ("igemm3n", 157, 2, 128, 128, 9, 1, 1): ("igemm3n_kernel<4, 1, 1, 5, 1, 3, 1, 0>", (72, 72), (768, 768)),
    ("igemm", 157, 2, 128, 128, 9, 0, 0): ("igemm_kernel<32, 128, 0>", (72, 72), (768, 768)),
    ("igemm3", 157, 2, 128, 128, 9, 0, 0): ("igemm3_kernel<128, 0, 1, 9>", (72, 72), (768, 768)),
    ("igemm3n", 157, 2, 128, 128, 9, 0, 0): ("igemm3n_kernel<4, 1, 0, 9, 1, 2, 0, 1>", (72, 72), (768, 768)),
    ("igemm3n", 157, 2, 128, 128, 9, 0, 1): ("igemm3n_kernel<4, 1, 0, 5, 1, 3, 1, 0>", (72, 72), (768, 768)),
    ("wgrad", 157, 2, 128, 128, 9, 0, 0): ("wgrad_kernel<5, 4>", (32, 0), (32, 0)),
    ("wgrad3", 157, 2, 128, 128, 9, 0, 0): ("wgrad3p_kernel<5, 5, 0>", (32, 0), (32, 0)),
    ("wgrad3", 157, 2, 128, 128, 9, 0, 1): ("wgrad3p_kernel<5, 5, 1>", (32, 0), (32, 0)),
    ("wgrad3", 157, 2, 128, 128, 9, 1, 0): ("wgrad3p_kernel<5, 5, 0>", (32, 0), (32, 0)),
    ("wgrad3", 157, 2, 128, 128, 9, 1, 1): ("wgrad3p_kernel<5, 5, 1>", (32, 0), (32, 0)),
    ("wgrad", 157, 2, 128, 128, 1, 0, 0): ("wgrad_kernel<2, 8>", (72, 0), (256, 0)),
    ("wgrad3", 157, 2, 128, 128, 1, 0, 0): ("wgrad1_kernel<false, 0>", (72, 0), (256, 0)),
    ("wgrad3", 157, 2, 128, 128, 1, 0, 1): ("wgrad1_kernel<false, 1>", (72, 0), (256, 0)),
    ("igemm", 157, 1, 128, 128, 3, 1, 0): ("igemm_kernel<32, 128, 1>", (48, 48), (512, 512)),
    ("igemm3", 157, 1, 128, 128, 3, 1, 0): ("igemm3_kernel<128, 1, 1, 6>", (48, 48), (512, 512)),
    ("igemm3n", 157, 1, 128, 128, 3, 1, 0): ("igemm3n_kernel<4, 1, 1, 6, 0, 2, 0, 1>", (48, 48), (512, 512)),
    ("igemm3n", 157, 1, 128, 128, 3, 1, 1): ("igemm3n_kernel<4, 1, 1, 3, 0, 3, 1, 0>", (48, 48), (512, 512)),
    ("igemm", 157, 1, 128, 128, 3, 0, 0): ("igemm_kernel<32, 128, 0>", (48, 48), (512, 512)),
    ("igemm3", 157, 1, 128, 128, 3, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (48, 48), (512, 512)),
    ("igemm3n", 157, 1, 128, 128, 3, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (48, 48), (512, 512)),
    ("igemm3n", 157, 1, 128, 128, 3, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (48, 48), (512, 512)),
    ("wgrad", 157, 1, 128, 128, 3, 0, 0): ("wgrad_kernel<3, 4>", (48, 0), (128, 0)),
    ("wgrad3", 157, 1, 128, 128, 3, 0, 0): ("wgrad3p_kernel<3, 0, 0>", (48, 0), (64, 0)),
    ("wgrad3", 157, 1, 128, 128, 3, 0, 1): ("wgrad3p_kernel<3, 0, 1>", (48, 0), (64, 0)),
    ("wgrad3", 157, 1, 128, 128, 3, 1, 0): ("wgrad3p_kernel<3, 0, 0>", (48, 0), (64, 0)),
    ("wgrad3", 157, 1, 128, 128, 3, 1, 1): ("wgrad3p_kernel<3, 0, 1>", (48, 0), (64, 0)),
    ("igemm", 0, 1, 128, 768, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 128, 768, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 128, 768, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 128, 768, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("igemm", 0, 1, 768, 128, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 768, 128, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 768, 128, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 768, 128, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("wgrad", 0, 1, 128, 768, 1, 0, 0): ("wgrad_kernel<2, 8>", (30, 0), (42, 0)),
    ("wgrad3", 0, 1, 128, 768, 1, 0, 0): ("wgrad1_kernel<false, 0>", (30, 0), (40, 0)),
    ("wgrad3", 0, 1, 128, 768, 1, 0, 1): ("wgrad1_kernel<false, 1>", (30, 0), (40, 0)),
    ("igemm", 0, 1, 256, 768, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 256, 768, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 256, 768, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 256, 768, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("igemm", 0, 1, 768, 256, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 768, 256, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 768, 256, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 768, 256, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("wgrad", 0, 1, 256, 768, 1, 0, 0): ("wgrad_kernel<2, 8>", (21, 0), (21, 0)),
    ("wgrad3", 0, 1, 256, 768, 1, 0, 0): ("wgrad1_kernel<false, 0>", (21, 0), (21, 0)),
    ("wgrad3", 0, 1, 256, 768, 1, 0, 1): ("wgrad1_kernel<false, 1>", (21, 0), (21, 0)),
    ("igemm", 0, 1, 512, 256, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 512, 256, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 512, 256, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 512, 256, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("igemm", 0, 1, 256, 512, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 256, 512, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 256, 512, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 256, 512, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("wgrad", 0, 1, 512, 256, 1, 0, 0): ("wgrad_kernel<2, 8>", (30, 0), (32, 0)),
    ("wgrad3", 0, 1, 512, 256, 1, 0, 0): ("wgrad1_kernel<false, 0>", (30, 0), (32, 0)),
    ("wgrad3", 0, 1, 512, 256, 1, 0, 1): ("wgrad1_kernel<false, 1>", (30, 0), (32, 0)),
    ("igemm", 0, 1, 128, 128, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 128, 128, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 128, 128, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 128, 128, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("wgrad", 0, 1, 128, 128, 1, 0, 0): ("wgrad_kernel<2, 8>", (30, 0), (256, 0)),
    ("wgrad3", 0, 1, 128, 128, 1, 0, 0): ("wgrad1_kernel<false, 0>", (30, 0), (256, 0)),
    ("wgrad3", 0, 1, 128, 128, 1, 0, 1): ("wgrad1_kernel<false, 1>", (30, 0), (256, 0)),
    ("igemm", 0, 1, 256, 128, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 256, 128, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 256, 128, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 256, 128, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("igemm", 0, 1, 128, 256, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 128, 256, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 128, 256, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 128, 256, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("wgrad", 0, 1, 256, 128, 1, 0, 0): ("wgrad_kernel<2, 8>", (30, 0), (128, 0)),
    ("wgrad3", 0, 1, 256, 128, 1, 0, 0): ("wgrad1_kernel<false, 0>", (30, 0), (128, 0)),
    ("wgrad3", 0, 1, 256, 128, 1, 0, 1): ("wgrad1_kernel<false, 1>", (30, 0), (128, 0)),
    ("igemm", 0, 1, 128, 32, 1, 0, 0): ("igemm_kernel<32, 32, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 128, 32, 1, 0, 0): ("igemm3_kernel<32, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 128, 32, 1, 0, 0): ("igemm3n_kernel<1, 4, 0, 6, 0, 3, 0, 0>", (30, 120), (314, 1256)),
    ("igemm3n", 0, 1, 128, 32, 1, 0, 1): ("igemm3n_kernel<1, 4, 0, 3, 0, 3, 1, 0>", (30, 120), (314, 1256)),
    ("igemm", 0, 1, 32, 128, 1, 0, 0): ("igemm_kernel<32, 128, 0>", (30, 30), (314, 314)),
    ("igemm3", 0, 1, 32, 128, 1, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 32, 128, 1, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (30, 30), (314, 314)),
    ("igemm3n", 0, 1, 32, 128, 1, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (30, 30), (314, 314)),
    ("wgrad", 0, 1, 128, 32, 1, 0, 0): ("wgrad_kernel<1, 4>", (30, 0), (256, 0)),
    ("wgrad3", 0, 1, 128, 32, 1, 0, 0): ("wgrad3_kernel<1, 4, true, 0>", (30, 0), (314, 0)),
    ("wgrad3", 0, 1, 128, 32, 1, 0, 1): ("wgrad3_kernel<1, 4, true, 1>", (30, 0), (314, 0)),
    ("igemm", 64, 64, 512, 64, 4, 1, 0): ("igemm_kernel<32, 64, 1>", (768, 768), (8192, 8192)),
    ("igemm3", 64, 64, 512, 64, 4, 1, 0): ("igemm3_kernel<64, 1, 1, 6>", (768, 768), (8192, 8192)),
    ("igemm3n", 64, 64, 512, 64, 4, 1, 0): ("igemm3n_kernel<2, 2, 1, 6, 0, 3, 0, 0>", (768, 1536), (8192, 16384)),
    ("igemm3n", 64, 64, 512, 64, 4, 1, 1): ("igemm3n_kernel<2, 2, 1, 3, 0, 3, 1, 0>", (768, 1536), (8192, 16384)),
    ("igemm", 64, 64, 64, 512, 4, 0, 0): ("igemm_kernel<32, 128, 0>", (768, 768), (8192, 8192)),
    ("igemm3", 64, 64, 64, 512, 4, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (768, 768), (8192, 8192)),
    ("igemm3n", 64, 64, 64, 512, 4, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (768, 768), (8192, 8192)),
    ("igemm3n", 64, 64, 64, 512, 4, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (768, 768), (8192, 8192)),
    ("wgrad", 64, 64, 512, 64, 4, 0, 0): ("wgrad_kernel<5, 4>", (64, 0), (64, 0)),
    ("wgrad3", 64, 64, 512, 64, 4, 0, 0): ("wgrad3p_kernel<5, 0, 0>", (32, 0), (32, 0)),
    ("wgrad3", 64, 64, 512, 64, 4, 0, 1): ("wgrad3p_kernel<5, 0, 1>", (32, 0), (32, 0)),
    ("wgrad3", 64, 64, 512, 64, 4, 1, 0): ("wgrad3p_kernel<5, 0, 0>", (32, 0), (32, 0)),
    ("wgrad3", 64, 64, 512, 64, 4, 1, 1): ("wgrad3p_kernel<5, 0, 1>", (32, 0), (32, 0)),
    ("igemm", 32, 32, 256, 32, 4, 1, 0): ("igemm_kernel<32, 32, 1>", (192, 192), (2048, 2048)),
    ("igemm3", 32, 32, 256, 32, 4, 1, 0): ("igemm3_kernel<32, 1, 1, 6>", (192, 192), (2048, 2048)),
    ("igemm3n", 32, 32, 256, 32, 4, 1, 0): ("igemm3n_kernel<1, 4, 1, 6, 0, 3, 0, 0>", (192, 768), (2048, 8192)),
    ("igemm3n", 32, 32, 256, 32, 4, 1, 1): ("igemm3n_kernel<1, 4, 1, 3, 0, 3, 1, 0>", (192, 768), (2048, 8192)),
    ("igemm", 32, 32, 32, 256, 4, 0, 0): ("igemm_kernel<32, 128, 0>", (192, 192), (2048, 2048)),
    ("igemm3", 32, 32, 32, 256, 4, 0, 0): ("igemm3_kernel<128, 0, 1, 6>", (192, 192), (2048, 2048)),
    ("igemm3n", 32, 32, 32, 256, 4, 0, 0): ("igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", (192, 192), (2048, 2048)),
    ("igemm3n", 32, 32, 32, 256, 4, 0, 1): ("igemm3n_kernel<4, 1, 0, 3, 0, 3, 1, 0>", (192, 192), (2048, 2048)),
    ("wgrad", 32, 32, 256, 32, 4, 0, 0): ("wgrad_kernel<2, 4>", (128, 0), (128, 0)),
    ("wgrad3", 32, 32, 256, 32, 4, 0, 0): ("wgrad3p_kernel<3, 0, 0>", (64, 0), (64, 0)),
    ("wgrad3", 32, 32, 256, 32, 4, 0, 1): ("wgrad3p_kernel<3, 0, 1>", (64, 0), (64, 0)),
    ("wgrad3", 32, 32, 256, 32, 4, 1, 0): ("wgrad3p_kernel<3, 0, 0>", (64, 0), (64, 0)),
    ("wgrad3", 32, 32, 256, 32, 4, 1, 1): ("wgrad3p_kernel<3, 0, 1>", (64, 0), (64, 0)),
}


def test_the_literal_table_covers_the_product_configuration():
    assert set(_cases()) == set(LITERAL)
    assert {k[0] for k in LITERAL} == set(K) and sorted(K.values()) == list(range(6))


@pytest.mark.parametrize("kernel", list(K))
def test_plan_equals_the_literal_table(kernel):
    bad = []
    for key, (label, at24, at256) in LITERAL.items():
        if key[0] != kernel:
            continue
        _, H, W, CIN, N, ntaps, flag, abf = key
        for B, want in ((24, at24), (256, at256)):
            NB, rows = (B, H) if H else (1, B * T)
            rc, p = _plan(kernel, _desc(kernel, NB, rows, W, CIN, N, ntaps, flag, abf))
            got = (rc, p.label.decode(), (p.G, p.stats_rows))
            if got != (0, label, want) or not 1 <= p.G <= p.max_G:
                bad.append((key, B, got, L.lib().bsed_last_error().decode()))
    assert not bad, bad


# the labels of six igemm3n shapes and (G, label) of four wgrad3 shapes under the test hooks
KNOB_SHAPES = [(24, 157, 16, 64, 128, 9, 1, 0), (24, 157, 16, 64, 128, 9, 1, 1), (24, 157, 4, 128, 128, 9, 1, 0),
               (24, 157, 32, 32, 64, 9, 1, 0), (1, 24 * T, 1, 128, 768, 1, 0, 0), (1, 24 * T, 1, 768, 128, 1, 0, 0)]
KNOBS = {
    "default": ["igemm3n_kernel<4, 1, 1, 6, 1, 2, 0, 1>", "igemm3n_kernel<4, 1, 1, 3, 1, 3, 1, 0>",
                "igemm3n_kernel<4, 1, 1, 9, 1, 2, 0, 1>", "igemm3n_kernel<2, 2, 1, 6, 1, 3, 0, 1>",
                "igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", "igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>"],
    "shape32": ["igemm3n_kernel<4, 1, 1, 6, 1, 3, 0, 0>", "igemm3n_kernel<4, 1, 1, 3, 1, 3, 1, 0>",
                "igemm3n_kernel<4, 1, 1, 9, 1, 2, 0, 0>", "igemm3n_kernel<2, 2, 1, 6, 1, 3, 0, 0>",
                "igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 0>", "igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 0>"],
    "wpe2": ["igemm3n_kernel<4, 1, 1, 6, 1, 2, 0, 1>", "igemm3n_kernel<4, 1, 1, 3, 1, 3, 1, 0>",
             "igemm3n_kernel<4, 1, 1, 9, 1, 2, 0, 1>", "igemm3n_kernel<2, 2, 1, 6, 1, 3, 0, 1>",
             "igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", "igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>"],
    "wpe3": ["igemm3n_kernel<4, 1, 1, 6, 1, 3, 0, 1>", "igemm3n_kernel<4, 1, 1, 3, 1, 3, 1, 0>",
             "igemm3n_kernel<4, 1, 1, 9, 1, 3, 0, 1>", "igemm3n_kernel<2, 2, 1, 6, 1, 3, 0, 1>",
             "igemm3n_kernel<4, 1, 0, 6, 0, 3, 0, 0>", "igemm3n_kernel<4, 1, 0, 6, 0, 3, 0, 0>"],
    "wpe8": ["igemm3n_kernel<4, 1, 1, 6, 1, 2, 0, 1>", "igemm3n_kernel<4, 1, 1, 3, 1, 3, 1, 0>",
             "igemm3n_kernel<4, 1, 1, 9, 1, 2, 0, 1>", "igemm3n_kernel<2, 2, 1, 6, 1, 3, 0, 1>",
             "igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>", "igemm3n_kernel<4, 1, 0, 6, 0, 2, 0, 1>"],
}
NOPIPE_SHAPES = [(24, 314, 64, 16, 32, 9, 1, 0), (24, 157, 16, 64, 128, 9, 0, 1), (24, 157, 2, 128, 128, 9, 1, 0),
                 (24, 157, 16, 128, 128, 1, 0, 0)]
NOPIPE = {
    None: [(256, "wgrad3p_kernel<3, 6, 0>"), (128, "wgrad3p_kernel<9, 1, 1>"), (32, "wgrad3p_kernel<5, 5, 0>"),
           (256, "wgrad1_kernel<false, 0>")],
    "1": [(1024, "wgrad3_kernel<2, 4, true, 0>"), (256, "wgrad3_kernel<9, 4, true, 1>"), (64, "wgrad3_kernel<5, 4, true, 0>"),
          (256, "wgrad1_kernel<false, 0>")],
}


def test_the_igemm3n_hooks_change_the_label_as_they_changed_the_variant():
    lib = L.lib()
    hooks = {"default": lambda: None, "shape32": lambda: lib.bsed_igemm3n_set_shape(32),
             "wpe2": lambda: lib.bsed_igemm3n_set_wpe(2), "wpe3": lambda: lib.bsed_igemm3n_set_wpe(3),
             "wpe8": lambda: lib.bsed_igemm3n_set_wpe(8)}
    try:
        for name, want in KNOBS.items():
            lib.bsed_igemm3n_set_shape(0)
            lib.bsed_igemm3n_set_wpe(0)
            hooks[name]()
            got = [_plan("igemm3n", _desc("igemm3n", *s))[1].label.decode() for s in KNOB_SHAPES]
            assert got == want, name
    finally:
        lib.bsed_igemm3n_set_shape(0)
        lib.bsed_igemm3n_set_wpe(0)


def test_wgrad3_nopipe_changes_the_plan_as_it_changed_auto_g_and_the_variant():
    before = os.environ.get("BSED_WGRAD3_NOPIPE")
    try:
        for env, want in NOPIPE.items():
            os.environ.pop("BSED_WGRAD3_NOPIPE", None)
            if env:
                os.environ["BSED_WGRAD3_NOPIPE"] = env
            plans = [_plan("wgrad3", _desc("wgrad3", *s))[1] for s in NOPIPE_SHAPES]
            assert [(p.G, p.label.decode()) for p in plans] == want, env
    finally:
        os.environ.pop("BSED_WGRAD3_NOPIPE", None)
        if before is not None:
            os.environ["BSED_WGRAD3_NOPIPE"] = before


def _kernel_of(entry):
    return entry[len("bsed_"):]


@pytest.mark.parametrize("defect", list(_GEOMETRY_DEFECTS))
@pytest.mark.parametrize("entry", _CONV_ENTRIES)
def test_ill_formed_tile_geometry_is_refused_by_the_plan_as_by_the_entry_point(entry, defect):
    rc, _ = _plan(_kernel_of(entry), _conv_desc(entry, **_GEOMETRY_DEFECTS[defect]))
    msg = L.lib().bsed_last_error().decode()
    assert rc == -1, (entry, defect, rc, msg)
    # wgrad_prepare serves both weight-gradient entries and reports as bsed_wgrad
    assert msg.startswith("bsed_wgrad:" if entry == "bsed_wgrad3" else entry + ":"), (entry, defect, msg)


@pytest.mark.parametrize("entry", _CONV_ENTRIES)
def test_a_descriptor_without_pointers_is_planned_and_the_entry_point_still_wants_them(entry):
    lib = L.lib()
    d = _conv_desc(entry)
    d.G = 1
    rc, with_pointers = _plan(_kernel_of(entry), d)
    assert rc == 0, lib.bsed_last_error().decode()
    for name in ("in_", "w", "out", "dy", "part"):
        if hasattr(d, name):
            setattr(d, name, None)
    rc, p = _plan(_kernel_of(entry), d)
    assert rc == 0, lib.bsed_last_error().decode()
    assert (p.G, p.max_G, p.stats_rows, p.label) == (with_pointers.G, with_pointers.max_G, with_pointers.stats_rows,
                                                     with_pointers.label) and p.label.startswith(_kernel_of(entry)[:5].encode())
    assert getattr(lib, entry)(ctypes.byref(d), None) == -1                       # BSED_ERR_ARG: no HIP call was reached
    assert lib.bsed_last_error().decode() == entry + ": null tensor"


def test_unknown_kernel_null_arguments_and_the_igemm3s_grid_check():
    lib = L.lib()
    p = L.STRUCTS["BsedContractPlan"]()
    d, w = _conv_desc("bsed_igemm"), _conv_desc("bsed_wgrad")
    for k in (-1, 4, 5, 6):
        assert lib.bsed_igemm_plan(ctypes.byref(d), k, ctypes.byref(p)) == -1
    for k in (-1, 0, 3, 6):
        assert lib.bsed_wgrad_plan(ctypes.byref(w), k, ctypes.byref(p)) == -1
    assert lib.bsed_igemm_plan(None, 0, ctypes.byref(p)) == -1 and lib.bsed_igemm_plan(ctypes.byref(d), 0, None) == -1
    assert lib.bsed_wgrad_plan(None, 4, ctypes.byref(p)) == -1 and lib.bsed_wgrad_plan(ctypes.byref(w), 4, None) == -1
    # bsed_igemm3s reads its grid size from the descriptor: 1..max_G
    s = _conv_desc("bsed_igemm3s")
    rc, plan = _plan("igemm3s", s)
    assert rc == 0 and plan.max_G == 4 and plan.G == 4 and plan.stats_rows == 4     # 2 images x 2 tile rows x 1 tile column
    for G in (0, plan.max_G + 1):
        s.G = G
        assert lib.bsed_igemm3s(ctypes.byref(s), None) == -1
        assert lib.bsed_last_error().decode() == f"bsed_igemm3s: G must be in 1..{plan.max_G} tiles"


def test_igemm3s_supported_answers_from_the_plan_what_the_python_formula_answered():
    from bsed_amd import ops

    def formula(W, CIN, ntaps):                                  # the retired copy of the P.PP <= 256 / 192 check
        TH, TW = _tile(W)
        halo = 1 if ntaps > 1 else 0
        return CIN in (16, 32) and (TH + 2 * halo) * (TW + 2 * halo) <= (256 if CIN == 16 else 192)

    for W in (1, 2, 4, 8, 16, 32, 64, 128):
        for ntaps in (1, 9):
            for CIN in (16, 32):
                assert ops.igemm3s_supported(W, CIN, ntaps) is formula(W, CIN, ntaps), (W, CIN, ntaps)
            assert ops.igemm3s_supported(W, 64, ntaps) is False
        assert ops.igemm3s_supported(W, 16) is formula(W, 16, 9)


def test_the_retired_queries_are_gone_and_the_six_entry_points_take_a_descriptor_and_a_stream():
    for name in RETIRED:
        assert name not in L.FUNCTIONS
    for entry in _CONV_ENTRIES:
        assert L.FUNCTIONS[entry] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    for query in ("bsed_igemm_plan", "bsed_wgrad_plan"):
        assert L.FUNCTIONS[query] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
    assert L.lib().bsed_abi_version() >= 12
    plan = L.STRUCTS["BsedContractPlan"]
    assert [n for n, _ in plan._fields_] == ["G", "max_G", "stats_rows", "label"] and ctypes.sizeof(plan) == 108
