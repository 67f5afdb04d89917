"""Plain CPU restatements of the bidirectional GRU recurrence of csrc/gru.hip, and the error models its tests' bars
come from.  Not a test module: tests/test_gru_reference_cpu.py checks it, tests/test_gru_gpu.py compares the kernels
with it.

Everything takes what the kernels take: ``xp (B,T,768)`` = x @ W_ih^T + b_ih as fp32 values ([dir*384 + gate*128 + k]),
``w_hh (2,384,128)``, ``b_hh (2,384)``, h0 = 0, gate order r, z, n, b_hn inside the r-gated term.  Results come in the
kernels' layouts: ``out (B,T,256)``, ``gates (B,T,2,4,128)`` = r, z, n, W_hn h + b_hn, ``dxp`` / ``dgh (B,T,768)`` for
L = sum(out * dout), and ``part_bih`` / ``part_bhh (B,768)``: their sums over time per batch row.

Three models:
  reference()      float64, a Python loop over time, gradients by autograd through the loop (dgh through a zero leaf
                   added to the hidden-side pre-activation W_hh h + b_hh);
  model("fp32")    the fp32 floor: the same loop and its hand-written BPTT in float32;
  model("split")   the matrix-core kernels' arithmetic model: float64, but h @ W_hh^T (and dg @ W_hh in the backward) is
                   h_hi W_hi + h_lo W_hi + h_hi W_lo with hi = bf16(x) round-to-nearest-even, lo = bf16(x - hi), the
                   left operand first rounded to fp32, products and sums in float64.
model("f64") is the hand-written BPTT in float64; the CPU test pins it to the autograd result, which is what makes the
two error models restatements of the same recurrence.
"""
import functools
import math

import numpy as np
import torch

H, G = 128, 384


def _steps(x, n):
    """(B,T,2*n) in time order -> (2,B,T,n) in step order: direction 1 walks the sequence backwards"""
    return torch.stack([x[..., :n], x[..., n:].flip(1)])


def _unsteps(y):
    """(2,B,T,...) in step order -> (B,T,2,...) in time order"""
    return torch.stack([y[0], y[1].flip(1)], dim=2)


def _bf16_split(x):
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.double(), lo.double()


class _Plain:
    def __init__(self, w):
        self.w, self.wt = w, w.transpose(1, 2)

    def fwd(self, h):   # (2,B,128) -> (2,B,384)
        return torch.bmm(h, self.wt)

    def bwd(self, dg):  # (2,B,384) -> (2,B,128)
        return torch.bmm(dg, self.w)


class _Split:
    def __init__(self, w):
        self.hi, self.lo = _bf16_split(w)

    def _mm(self, a, transpose):
        ahi, alo = _bf16_split(a)
        whi, wlo = (self.hi.transpose(1, 2), self.lo.transpose(1, 2)) if transpose else (self.hi, self.lo)
        return torch.bmm(ahi, whi) + torch.bmm(alo, whi) + torch.bmm(ahi, wlo)

    def fwd(self, h):
        return self._mm(h, True)

    def bwd(self, dg):
        return self._mm(dg, False)


def _forward(xs, mm, b_hh, eps=None):
    """xs (2,B,T,384) in step order -> h (2,B,T,128), gates (2,B,T,4,128)"""
    _, B, T, _ = xs.shape
    h = torch.zeros(2, B, H, dtype=xs.dtype)
    hs, gs = [], []
    for s in range(T):
        gh = mm.fwd(h) + b_hh[:, None, :]
        if eps is not None:
            gh = gh + eps[:, :, s]
        x = xs[:, :, s]
        r = torch.sigmoid(x[..., :H] + gh[..., :H])
        z = torch.sigmoid(x[..., H:2 * H] + gh[..., H:2 * H])
        ghn = gh[..., 2 * H:]
        n = torch.tanh(x[..., 2 * H:] + r * ghn)
        h = (1.0 - z) * n + z * h
        hs.append(h)
        gs.append(torch.stack([r, z, n, ghn], dim=2))
    return torch.stack(hs, dim=2), torch.stack(gs, dim=2)


def _backward(hs, gs, ds, mm):
    """hand-written BPTT in step order, the kernels' formulas: -> dxp, dgh (2,B,T,384)"""
    _, B, T, _ = hs.shape
    dhrec = torch.zeros(2, B, H, dtype=hs.dtype)
    dx, dg = [None] * T, [None] * T
    for s in range(T - 1, -1, -1):
        r, z, n, ghn = gs[:, :, s].unbind(2)
        hp = hs[:, :, s - 1] if s > 0 else torch.zeros_like(dhrec)
        dh = ds[:, :, s] + dhrec
        dn_pre = dh * (1.0 - z) * (1.0 - n * n)
        dz_pre = dh * (hp - n) * z * (1.0 - z)
        dr_pre = dn_pre * ghn * r * (1.0 - r)
        dghn = dn_pre * r
        dx[s] = torch.cat([dr_pre, dz_pre, dn_pre], -1)
        dg[s] = torch.cat([dr_pre, dz_pre, dghn], -1)
        dhrec = dh * z + mm.bwd(dg[s])
    return torch.stack(dx, dim=2), torch.stack(dg, dim=2)


def _pack(hs, gs, dx=None, dg=None):
    B, T = hs.shape[1:3]
    res = {"out": _unsteps(hs).reshape(B, T, 2 * H), "gates": _unsteps(gs)}
    if dx is not None:
        res["dxp"] = _unsteps(dx).reshape(B, T, 2 * G)
        res["dgh"] = _unsteps(dg).reshape(B, T, 2 * G)
        res["part_bih"] = res["dxp"].sum(1)
        res["part_bhh"] = res["dgh"].sum(1)
    return {k: v.detach() for k, v in res.items()}


def reference(xp, w_hh, b_hh, dout=None):
    """float64 restatement; gradients by autograd through the loop"""
    xp64 = xp.double().clone().requires_grad_(dout is not None)
    eps = torch.zeros_like(xp64, requires_grad=dout is not None)
    hs, gs = _forward(_steps(xp64, G), _Plain(w_hh.double()), b_hh.double(), _steps(eps, G))
    res = _pack(hs, gs)
    if dout is not None:
        out = _unsteps(hs).reshape(res["out"].shape)
        (out * dout.double()).sum().backward()
        res.update(dxp=xp64.grad, dgh=eps.grad, part_bih=xp64.grad.sum(1), part_bhh=eps.grad.sum(1))
    return res


def model(kind, xp, w_hh, b_hh, dout=None):
    """kind: "f64" | "fp32" | "split" (module docstring); forward and hand-written BPTT fed its own forward"""
    dt = torch.float32 if kind == "fp32" else torch.float64
    mm = _Split(w_hh.double()) if kind == "split" else _Plain(w_hh.to(dt))
    with torch.no_grad():
        hs, gs = _forward(_steps(xp.to(dt), G), mm, b_hh.to(dt))
        if dout is None:
            return _pack(hs, gs)
        dx, dg = _backward(hs, gs, _steps(dout.to(dt), H), mm)
        return _pack(hs, gs, dx, dg)


# ---------------------------------------------------------------------------------------------------------------------
# Input families.  Weights are nn.GRU's default draw U(-1/sqrt(128), 1/sqrt(128)) = |w| <= 0.088; xp is the projection
# of randn inputs, rounded to fp32 once: every model and every kernel consumes those same fp32 values.
#   init     default weights, randn inputs
#   w4       w_hh scaled by 4 (a trained GRU is not at init scale; x 8 is chaotic and not used)
#   x30      inputs scaled by 30: max |xp| ~ 85-90, most gates saturated
#   placed   init, with +-200 placed in each gate's xp at PLACED positions
# ---------------------------------------------------------------------------------------------------------------------
PLACED = [  # (t as a fraction of T-1, dir, gate, unit, value): every gate, both signs, both directions
    (0.0, 0, 0, 5, 200.0), (0.0, 1, 0, 6, -200.0), (0.5, 0, 1, 17, 200.0), (0.5, 1, 1, 18, -200.0),
    (1.0, 0, 2, 127, 200.0), (1.0, 1, 2, 0, -200.0), (0.5, 1, 0, 64, 200.0), (0.5, 0, 2, 33, -200.0),
]


def placed_index(T):
    return [(int(round(f * (T - 1))), d, g, k, v) for f, d, g, k, v in PLACED]


def make_inputs(family, B, T, seed):
    assert family in ("init", "w4", "x30", "placed"), family
    gen = torch.Generator().manual_seed(seed)
    a = 1.0 / math.sqrt(H)

    def uni(*shape):
        return (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * a

    w_ih, w_hh, b_ih, b_hh = uni(2 * G, H), uni(2, G, H), uni(2 * G), uni(2, G)
    x = torch.randn(B, T, H, generator=gen, dtype=torch.float64)
    dout = torch.randn(B, T, 2 * H, generator=gen, dtype=torch.float64).float()
    if family == "x30":
        x = x * 30.0
    if family == "w4":
        w_hh = w_hh * 4.0
    xp = (x @ w_ih.t() + b_ih).float()
    if family == "placed":
        for t, d, g, k, v in placed_index(T):
            xp[:, t, d * G + g * H + k] = v
    return xp, w_hh.float(), b_hh.float(), dout


# every (family, B, T) the GPU tests run; tests/test_gru_reference_cpu.py checks each one's conditioning
SEED = 3
PRODUCT_T = (216, 313)
EDGE_T = (1, 2, 3, 4, 63, 64)
MFMA_B = (1, 2, 3, 4, 5, 7, 8, 9)
FP32_B = (1, 2, 3, 128, 129)
REMAINDER_T = 7
CASES = sorted(set(
    [("init", 5, T) for T in PRODUCT_T + EDGE_T]
    + [("init", B, REMAINDER_T) for B in MFMA_B + FP32_B]
    + [("init", 8, 5)]                                      # the rows_per_wg contract
    + [("x30", 5, 63), ("x30", 5, 313), ("placed", 5, 63)]
    + [("w4", 5, 63), ("w4", 5, 313)]))
TENSORS = ("out", "gates", "dxp", "dgh", "part_bih", "part_bhh")
PLANES = ("r", "z", "n", "ghn")


class Case:
    """inputs, float64 reference and error models of one (family, B, T); models are computed on first use"""

    def __init__(self, family, B, T):
        assert (family, B, T) in CASES, (family, B, T)
        self.family, self.B, self.T = family, B, T
        self.xp, self.w_hh, self.b_hh, self.dout = make_inputs(family, B, T, SEED)
        self.ref = reference(self.xp, self.w_hh, self.b_hh, self.dout)

    @functools.cached_property
    def fp32(self):
        return model("fp32", self.xp, self.w_hh, self.b_hh, self.dout)

    @functools.cached_property
    def split(self):
        return model("split", self.xp, self.w_hh, self.b_hh, self.dout)

    def _views(self, res, name):
        """(label, tensor) pairs a bar is computed for: gates go plane by plane"""
        if name == "gates":
            return [(f"gates.{p}", res["gates"][..., i, :]) for i, p in enumerate(PLANES)]
        return [(name, res[name])]

    def model_error(self, kind, label):
        name = label.partition(".")[0]
        got = dict(self._views(getattr(self, kind), name))[label]
        want = dict(self._views(self.ref, name))[label]
        return float((got.double() - want).abs().max())

    def bar(self, label, matrix_core):
        """4 * E_fp32 (+ E_split for the matrix-core kernels) + 4 ulp of the tensor's max magnitude in fp32"""
        name = label.partition(".")[0]
        want = dict(self._views(self.ref, name))[label]
        tiny = 4.0 * float(np.spacing(np.float32(want.abs().max())))
        e = self.model_error("fp32", label) + (self.model_error("split", label) if matrix_core else 0.0)
        return 4.0 * e + tiny

    def labels(self, names=TENSORS):
        return [lab for n in names for lab, _ in self._views(self.ref, n)]

    def compare(self, got, matrix_core, names=TENSORS):
        """got: {tensor name: CPU tensor}.  -> [(label, measured max |error|, bar)], element-wise against float64"""
        table = []
        for n in names:
            for (lab, g), (_, w) in zip(self._views(got, n), self._views(self.ref, n)):
                assert g.shape == w.shape, (lab, g.shape, w.shape)
                err = float((g.double() - w).abs().max())  # NaN propagates: an unwritten or non-finite element fails
                table.append((lab, err, self.bar(lab, matrix_core)))
        return table


@functools.lru_cache(maxsize=None)
def case(family, B, T):
    return Case(family, B, T)
