"""Thin typed wrappers over the kernel-level C ABI (include/bsed.h).  No math happens here: every
function fills a descriptor with device pointers / shapes and launches HIP kernels on the current
stream.  Activations are NHWC fp32 tensors."""
import ctypes
import functools
import os
from typing import NamedTuple

import torch

from . import _lib as L

# epilogue ids and job limits of include/bsed.h; the descriptor and job structs come from the same parse (_lib.py)
EPI_PLAIN, EPI_STATS, EPI_GLU_POOL, EPI_GLU_BWD, EPI_ADD_STATS2 = (
    L.CONSTANTS["BSED_EPI_" + n] for n in ("PLAIN", "STATS", "GLU_POOL", "GLU_BWD", "ADD_STATS2"))
PACK_MAX_JOBS = L.CONSTANTS["BSED_PACK_MAX_JOBS"]
REDUCE_MAX_JOBS = L.CONSTANTS["BSED_REDUCE_MAX_JOBS"]
BN_EVAL_MAX_JOBS = L.CONSTANTS["BSED_BN_EVAL_MAX_JOBS"]
MIX_MAX_JOBS = L.CONSTANTS["BSED_MIX_MAX_JOBS"]
IgemmDesc, WgradDesc, HeadBwdDesc, PackJob, ReduceJob, BnEvalJob, GluDesc, GluPlan, ContractPlan = (
    L.STRUCTS["Bsed" + n] for n in ("IgemmDesc", "WgradDesc", "HeadBwdDesc", "PackJob", "ReduceJob", "BnEvalJob", "GluDesc",
                                    "GluPlan", "ContractPlan"))

TAPS3x3 = [(kh - 1, kw - 1) for kh in range(3) for kw in range(3)]
TAP1 = ((0, 0),)   # a plain GEMM: (positions, CIN) x (CIN, N)


class WeightView(NamedTuple):
    """A weight as a contraction reads it: w[tap][k][n] = tensor.view(-1)[offset + tap * s_tap + k * s_k + n * s_n] for
    the `taps` (dh, dw) input offsets, k < K input and n < N output channels.  conv3x3_weight and linear_weight build the
    views of torch's layouts; contract and weight_grad take nothing else for a weight or its gradient."""
    tensor: torch.Tensor
    offset: int
    taps: tuple
    K: int
    N: int
    s_tap: int
    s_k: int
    s_n: int

    def dgrad(self):
        """the view the data gradient contracts with: the transposed weight at the mirrored taps"""
        return self._replace(taps=tuple((-a, -b) for a, b in self.taps), K=self.N, N=self.K, s_k=self.s_n, s_n=self.s_k)

    def over(self, tensor):
        """the same geometry over another tensor of the same layout (the weight's gradient)"""
        return self._replace(tensor=tensor)

    def source(self):
        """the tensor from `offset` on: what the pack kernels read"""
        return self.tensor.view(-1)[self.offset:] if self.offset else self.tensor


def conv3x3_weight(w, W):
    """View of a (co, cin, 3, 3) weight for the 3x3 / pad 1 convolution of a width-W map.  On a width-1 map (the FPN
    levels) the six taps with dw != 0 only ever see zero padding: the convolution is exactly its centre column, a 3x1
    stencil over weight[co][ci][kh][1] (element offset 1, tap stride 3)."""
    co, cin = w.shape[:2]
    if W > 1:
        return WeightView(w, 0, tuple(TAPS3x3), cin, co, 1, 9, cin * 9)
    return WeightView(w, 1, ((-1, 0), (0, 0), (1, 0)), cin, co, 3, 9, cin * 9)


def linear_weight(w, N=None, K=None):
    """View of an (N, K) matrix of y = x W^T, or -- with N and K given -- of a flat slice holding one (the GRU's (768, nin)
    double-direction slices of the arena, a (N, K, 1, 1) convolution weight)"""
    if N is None:
        N, K = w.shape
    return WeightView(w, 0, TAP1, K, N, 0, 1, K)


class KernelTimer:
    """Per-launch HIP-event timing of EVERY entry-point call of a step (bench.py's roofline leg).  Events are recorded
    on the stream the kernels are launched on (torch's current stream).  key = (kernel label, shape tag): the label is
    the kernel's name as rocprofv3 prints it (template instance included) so that bench.py's table and the committed
    rocprof summary can be joined by name."""

    def __init__(self, main_stream=()):
        self.records = {}  # key -> [flops_per_launch, [(start, end), ...], algorithmic_bytes_per_launch]
        self._last, self._chain = {}, False
        # the step's own stream = the stream that is current when the timer is made (the null stream reads as None).
        # (Taking the stream of the first LAUNCH instead made the mean-teacher step's table name the teacher's stream
        # "main": its forward is the first thing a step enqueues.)
        # main_stream: the raw handle (``torch.cuda.Stream.cuda_stream``) of the stream the step runs on when that is not
        # the caller's (SEDTrainer runs the mean-teacher step on a high-priority stream of its own).
        if main_stream != ():
            self._main = main_stream or None
        else:
            try:
                self._main = L.stream().value
            except Exception:
                self._main = ()    # no GPU yet: fall back to the stream of the first launch
        self.side = {}     # key -> [flops, [(start, end), ...], bytes] of launches on any other stream: they run
        #                    beside main-stream kernels, so their event pairs time contention (and queueing) as well

    @staticmethod
    def prime(n=4096):
        """Create, record and retire n timing events once: the runtime grows its signal pool in steps that stall the
        stream for tens of milliseconds the first time a process holds a few hundred events (measured ~45 ms on a
        fresh MI355X box); doing it here keeps that out of whatever is timed later."""
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
        for e in evs:
            e.record()
        torch.cuda.synchronize()
        del evs

    def launch(self, key, flops, fn, nbytes):
        """One event per launch: on an in-order stream that the host keeps fed, the event recorded after launch i is also
        the start of launch i+1 (half the events of a start/end pair per launch: each event costs the GPU ~1.5 us).  A
        launch that follows anything other than a timed launch (the first of a step: host-side work in between) gets
        its own start event."""
        sid = L.stream().value
        if self._main == ():
            self._main = sid
        if sid != self._main:
            # a side-stream launch (GRU weight gradients beside the next recurrence, the next batch's mel transform
            # beside the GRU forward) shares the chip with main-stream kernels: its own event pair, kept apart from
            # the main-stream table (summary(side=True))
            s = torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.side.setdefault(key, [flops, [], nbytes])[1].append((s, e))
            return
        s = self._last.get(sid) if self._chain else None
        if s is None:
            s = torch.cuda.Event(enable_timing=True)
            s.record()
        fn()
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self._last[sid], self._chain = e, True
        rec = self.records.setdefault(key, [flops, [], nbytes])
        rec[1].append((s, e))

    def break_chain(self):
        """call between steps (or around host-side work): the next launch records its own start event"""
        self._chain = False

    def summary(self, side=False):
        """{key: (launches, total_ms, avg_ms, flops_per_launch, bytes_per_launch)} -- call after a device sync"""
        out = {}
        for key, (flops, evs, nbytes) in (self.side if side else self.records).items():
            ms = [s.elapsed_time(e) for s, e in evs]
            out[key] = (len(ms), float(sum(ms)), float(sum(ms) / len(ms)), flops, nbytes)
        return out


def set_timer(t):
    L.timer = t


def _launch(key, flops, fn, nbytes=None):
    """Announce the algorithmic work of the entry-point call ``fn`` makes.  key = (kernel, taps, CIN, N, H, W) for the
    contraction kernels or (kernel, tag) for the others.  nbytes = ALGORITHMIC HBM bytes of the launch (each activation
    tensor the op must read or write, once; weights and partial slabs not counted); default: a (positions, CIN) input
    and a (positions, N) output in fp32, positions recovered from the FLOP count."""
    if L.timer is not None:
        if nbytes is None:
            _, taps, cin, n, _, _ = key
            nbytes = 4.0 * (flops / (2.0 * taps * cin * n)) * (cin + n)
        if len(key) == 6:
            key = (key[0], "t%d CIN%d N%d %dx%d" % tuple(key[1:]))
        L.pending = (key, float(flops), float(nbytes))
    fn()


def _note(kernel, tag, flops, nbytes):
    """announce the next L.call (for wrappers whose call is written inline)"""
    if L.timer is not None:
        L.pending = ((kernel, tag), float(flops), float(nbytes))


def round_up(v, m):
    return (v + m - 1) // m * m


def tile_for(W):
    tw = min(W, 16)
    return 128 // tw, tw


def _p(t):
    return L.ptr(t).value if t is not None else None


def _pa(t):
    """pointer of an ACTIVATION tensor: fp32, or bf16 in the "bf16" throughput mode (the C ABI keeps float* types)"""
    return L.ptr(t, t.dtype if t is not None and t.dtype == torch.bfloat16 else None)


def _abf(*ts):
    """1 if the activation tensors are bf16 (all of them), 0 if fp32"""
    ts = [t for t in ts if t is not None]
    bf = [t.dtype == torch.bfloat16 for t in ts]
    if any(bf) and not all(bf):
        raise L.BsedError("mixed fp32 / bf16 activation tensors: " + ", ".join(str(t.dtype) for t in ts))
    return 1 if bf and bf[0] else 0


def _esz(t):
    return 2.0 if t.dtype == torch.bfloat16 else 4.0


def _dp(t, offset=0):
    """device pointer (int) of tensor storage + element offset; tensor need not be contiguous as a whole"""
    return None if t is None else t.data_ptr() + t.element_size() * offset


def pack_weight(src, ntaps, K, N, s_tap, s_k, s_n, src_offset=0):
    NP = round_up(N, 32)
    dst = torch.empty((ntaps, K, NP), device=src.device, dtype=torch.float32)
    _note("pack_weight_kernel", "", 0.0, 4.0 * dst.numel())
    L.call("bsed_pack_weight", _dp(src, src_offset), L.ptr(dst), ntaps, K, N, NP, s_tap, s_k, s_n, L.stream())
    return dst


def _tile_taps(d, H, W, taps):
    """Tile, taps and halo of an IgemmDesc / WgradDesc"""
    d.TH, d.TW = tile_for(W)
    hh = hw = 0
    for i, (a, b) in enumerate(taps):
        d.dh[i], d.dw[i] = a, b
        hh, hw = max(hh, abs(a)), max(hw, abs(b))
    d.hh, d.hw, d.ntaps = hh, hw, len(taps)


def _contract_plan(entry, d):
    """BsedContractPlan of the contraction entry point's launch for the shape fields of d: the grid size G (stored into
    d.G), the rows of statistics the launch writes and, as plan.label, the instance it runs (the KernelTimer label)"""
    plan = ContractPlan()
    query = L.lib().bsed_wgrad_plan if isinstance(d, WgradDesc) else L.lib().bsed_igemm_plan
    L.check(query(ctypes.byref(d), L.CONSTANTS["BSED_CONTRACT_" + entry[len("bsed_"):].upper()], ctypes.byref(plan)), entry)
    d.G = plan.G
    return plan


def _igemm_desc(NB, H, W, CIN, N, NP, taps, epilogue, valid=None):
    """IgemmDesc of a contraction without pooling, with dense rows (pitch = channel count); the pointers, and whatever
    else differs, are the caller's."""
    d = IgemmDesc()
    _tile_taps(d, H, W, taps)
    d.NB, d.H, d.W, d.CIN, d.N, d.NP = NB, H, W, CIN, N, NP
    d.in_pitch, d.out_pitch, d.e_pitch = CIN, N, N
    d.ph = d.pw = 1
    d.Hp, d.Wp = H, W
    d.epilogue = epilogue
    if valid:
        d.valid_h, d.valid_w = valid
    return d


def igemm(inp, wpk, N, NB, H, W, CIN, taps=((0, 0),), bias=None, out=None, epilogue=EPI_PLAIN, in_pitch=None,
          out_pitch=None, a_scale=None, a_shift=None, e_src=None, e_scale=None, e_shift=None, e_dpool=None,
          out2=None, pool=(1, 1), drop_p=0.0, rng_stream=0, seed=0, in_offset=0, want_stats=False, valid=None):
    """Launch the implicit GEMM.  Returns (out, stats or None).  valid = (h, w): only output positions inside that
    extent are stored / enter the STATS sums (the rest of a freshly allocated ``out`` is zero)."""
    NP = wpk.shape[2]
    d = _igemm_desc(NB, H, W, CIN, N, NP, taps, epilogue, valid)
    ph, pw = pool
    Hp, Wp = H // ph, W // pw
    dev = inp.device
    if out is None:
        shape = (NB, Hp, Wp, N) if epilogue == EPI_GLU_POOL else (NB, H, W, N)
        out = (torch.zeros if valid else torch.empty)(shape, device=dev, dtype=torch.float32)
    d.in_ = _dp(inp, in_offset); d.w = _p(wpk); d.bias = _p(bias); d.out = _p(out); d.out2 = _p(out2)
    d.a_scale = _p(a_scale); d.a_shift = _p(a_shift); d.e_src = _p(e_src)
    d.e_scale = _p(e_scale); d.e_shift = _p(e_shift); d.e_dpool = _p(e_dpool)
    if in_pitch is not None:
        d.in_pitch = in_pitch
    if out_pitch is not None:
        d.out_pitch = out_pitch
    d.ph, d.pw, d.Hp, d.Wp = ph, pw, Hp, Wp
    d.drop_p, d.rng_stream, d.seed = drop_p, rng_stream, seed
    plan = _contract_plan("bsed_igemm", d)
    stats = None
    if epilogue in (EPI_STATS, EPI_GLU_BWD, EPI_ADD_STATS2):
        stats = torch.empty((plan.stats_rows, 2, N), device=dev, dtype=torch.float32)
        d.stats = _p(stats)
    _launch((plan.label.decode(), len(taps), CIN, N, H, W), 2.0 * NB * H * W * len(taps) * CIN * N,
            lambda: L.call("bsed_igemm", ctypes.byref(d), L.stream()))
    return out, stats


_pack_memo = None   # {(kind, data_ptr, args): packed tensor} while an ops.pack_cache() block is open
_pack_plan = None   # the PackPlan of the open outermost block, if it was given one


class PackPlan:
    """Which packed weight copies a recurring ``pack_cache`` block asked for last time.  The next block given the same
    plan makes ALL of them in one launch on entry (``bsed_pack_weights_batch``) instead of one 5-7 us launch per weight
    on the forward's and backward's critical path (fourteen per CRNN train step).  Entries a block did not use are
    dropped when it closes; new requests are packed on the spot and join the plan.  Same kernels' element code: same
    bits as the unplanned path (tests/test_pack_plan_gpu.py)."""

    def __init__(self):
        self.entries = {}     # key -> (kind, src, ntaps, K, N, s_tap, s_k, s_n)
        self.used = set()

    @staticmethod
    def _numel(kind, ntaps, K, N):
        NP = round_up(N, 32)
        return ntaps * (K // 32) * NP * 64 if kind == 0 else (NP // 32) * ntaps * (K // 16) * 2 * 64 * 8

    def replay(self, memo):
        stream = L.stream()
        todo = [(k, v) for k, v in self.entries.items() if k[2] == stream.value]
        self.used = set()
        if not todo:
            return
        dev = todo[0][1][1].device
        sizes = [self._numel(v[0], v[2], v[3], v[4]) for _, v in todo]
        buf = torch.empty(sum(sizes), device=dev, dtype=torch.int16)
        _note("pack_weights_batch_kernel", "", 0.0, 4.0 * buf.numel())
        off = 0
        jobs = []
        for (key, (kind, src, ntaps, K, N, s_tap, s_k, s_n)), n in zip(todo, sizes):
            NP = round_up(N, 32)
            shape = (ntaps, K // 32, NP, 64) if kind == 0 else (NP // 32, ntaps, K // 16, 2, 64, 8)
            dst = buf[off:off + n].view(shape)
            off += n
            memo[key] = (dst, src)
            jobs.append((src.data_ptr(), dst.data_ptr(), kind, ntaps, K, N, NP, s_tap, s_k, s_n))
        for j0 in range(0, len(jobs), PACK_MAX_JOBS):
            part = jobs[j0:j0 + PACK_MAX_JOBS]
            arr = (PackJob * len(part))()
            for a, (sp, dp, kind, ntaps, K, N, NP, s_tap, s_k, s_n) in zip(arr, part):
                a.src = sp; a.dst = dp
                a.kind, a.ntaps, a.K, a.N, a.NP = kind, ntaps, K, N, NP
                a.s_tap, a.s_k, a.s_n = s_tap, s_k, s_n
            L.call("bsed_pack_weights_batch", arr, len(part), stream)

    def close(self):
        stream = L.stream().value
        for k in [k for k in self.entries if k[2] == stream and k not in self.used]:
            del self.entries[k]


class pack_cache:
    """Inside this block the caller guarantees that no weight tensor changes (a train step before its optimizer
    update): a packed / split copy of a weight (pack_weight3, pack_weight3s) is made once per (tensor, layout) and
    reused by every forward / backward pass in the block -- two half-batch passes of a mean-teacher or adversarial step
    pack each weight once instead of twice.  With a ``PackPlan`` (a block that recurs, e.g. the train step) the copies
    the previous block used are all made in one launch on entry."""

    def __init__(self, plan=None):
        self._plan = plan

    def __enter__(self):
        global _pack_memo, _pack_plan
        self._outer = _pack_memo
        self._outer_plan = _pack_plan
        if _pack_memo is None:
            _pack_memo = {}
            _pack_plan = self._plan
            if _pack_plan is not None:
                _pack_plan.replay(_pack_memo)
        return self

    def __exit__(self, *exc):
        global _pack_memo, _pack_plan
        if self._outer is None and _pack_plan is not None:
            _pack_plan.close()
        _pack_memo = self._outer
        _pack_plan = self._outer_plan
        return False


def _pack_lookup(key):
    if _pack_memo is not None and key in _pack_memo:
        if _pack_plan is not None:
            _pack_plan.used.add(key)
        return _pack_memo[key][0]
    return None


def _pack_store(key, dst, src, kind, ntaps, K, N, s_tap, s_k, s_n):
    if _pack_memo is not None:
        _pack_memo[key] = (dst, src)   # src kept alive: its address is the key
        if _pack_plan is not None:
            _pack_plan.entries[key] = (kind, src, ntaps, K, N, s_tap, s_k, s_n)
            _pack_plan.used.add(key)


def igemm3_nsplit():
    """True: ops.igemm3 runs the round-3 kernel (csrc/igemm3n.hip: a wave owns 32 output channels, weight fragments
    straight from global memory, one barrier per 32-channel chunk) and pack_weight3 emits its fragment-order table;
    BSED_IGEMM3N=0 = the slab kernel of rounds 1-2 (csrc/igemm3.hip)."""
    return os.environ.get("BSED_IGEMM3N", "1") != "0"


def pack_weight3(src, ntaps, K, N, s_tap, s_k, s_n):
    """bf16 hi/lo split weights for igemm3: uint16 (ntaps, K/32, NP, 64), or -- for the N-split kernel -- the
    fragment-order table of pack_weight3s, int16 (NP/32, ntaps, K/16, 2, 64, 8)"""
    if igemm3_nsplit():
        return pack_weight3s(src, ntaps, N, s_tap, s_k, s_n, K=K)
    key = ("w3", src.data_ptr(), L.stream().value, ntaps, K, N, s_tap, s_k, s_n)
    hit = _pack_lookup(key)
    if hit is not None:
        return hit
    NP = round_up(N, 32)
    dst = torch.empty((ntaps, K // 32, NP, 64), device=src.device, dtype=torch.int16)
    _note("pack_weight3_kernel", "", 0.0, 4.0 * dst.numel())
    L.call("bsed_pack_weight3", _dp(src), dst.data_ptr(), ntaps, K, N, NP, s_tap, s_k, s_n, L.stream())
    _pack_store(key, dst, src, 0, ntaps, K, N, s_tap, s_k, s_n)
    return dst


def pack_weight3s(src, ntaps, N, s_tap, s_k, s_n, K=16):
    """pre-split weights of a CIN = 16 / 32 convolution in fragment order: int16 (NP/32, ntaps, K/16, 2, 64, 8)"""
    key = ("w3s", src.data_ptr(), L.stream().value, ntaps, N, s_tap, s_k, s_n, K)
    hit = _pack_lookup(key)
    if hit is not None:
        return hit
    NP = round_up(N, 32)
    dst = torch.empty((NP // 32, ntaps, K // 16, 2, 64, 8), device=src.device, dtype=torch.int16)
    _note("pack_weight3s_kernel", "", 0.0, 4.0 * dst.numel())
    L.call("bsed_pack_weight3s", _dp(src), dst.data_ptr(), ntaps, K, N, NP, s_tap, s_k, s_n, L.stream())
    _pack_store(key, dst, src, 1, ntaps, K, N, s_tap, s_k, s_n)
    return dst


@functools.lru_cache(maxsize=None)
def igemm3s_supported(W, CIN, ntaps=9):
    """True iff bsed_igemm3s takes CIN input channels over ntaps (9 or 1) taps on a width-W map: its plan's answer for a
    one-row map of that width (the checks do not depend on the other sizes)"""
    d = _igemm_desc(1, 1, W, CIN, 32, 32, TAPS3x3[:ntaps] if ntaps > 1 else TAP1, EPI_PLAIN)
    return L.lib().bsed_igemm_plan(ctypes.byref(d), L.CONSTANTS["BSED_CONTRACT_IGEMM3S"], ctypes.byref(ContractPlan())) == 0


def _igemm3_launch(entry, inp, w, N, NP, NB, H, W, CIN, taps, bias, epilogue, valid=None):
    """One split-fp32 forward contraction (bsed_igemm3 / bsed_igemm3s / bsed_igemm3n) with packed weights w of NP output
    channels: buffers sized by the entry point's plan.  Returns (out, stats (plan.stats_rows, 2, N) or None)."""
    d = _igemm_desc(NB, H, W, CIN, N, NP, taps, epilogue, valid)
    d.act_bf16 = _abf(inp)
    plan = _contract_plan(entry, d)
    out = (torch.zeros if valid else torch.empty)((NB, H, W, N), device=inp.device, dtype=inp.dtype)
    stats = torch.empty((plan.stats_rows, 2, N), device=inp.device, dtype=torch.float32) if epilogue == EPI_STATS else None
    d.in_ = _dp(inp); d.w = w.data_ptr(); d.bias = _p(bias); d.out = out.data_ptr(); d.stats = _p(stats)
    _launch((plan.label.decode(), len(taps), CIN, N, H, W), 2.0 * NB * H * W * len(taps) * CIN * N,
            lambda: L.call(entry, ctypes.byref(d), L.stream()), _esz(inp) * NB * H * W * (CIN + N))
    return out, stats


def igemm3s(inp, wtab, N, NB, H, W, taps, bias=None, epilogue=EPI_PLAIN):
    """CIN = 16 / 32 convolution on the bf16 cores (split-fp32), all taps' weights resident in LDS.
    Returns (out, stats (G,2,N) or None)."""
    return _igemm3_launch("bsed_igemm3s", inp, wtab, N, wtab.shape[0] * 32, NB, H, W, 16 * wtab.shape[2], taps, bias, epilogue)


def igemm3(inp, w3, N, NB, H, W, CIN, taps, bias=None, epilogue=EPI_PLAIN, valid=None):
    """3x3 conv forward / dgrad on the bf16 matrix cores with split-fp32 operands.  Returns (out, stats or None).
    valid: see igemm.  w3: the fragment-order table of pack_weight3s for the layer (K = CIN; bsed_igemm3n) or the slab
    layout of bsed_pack_weight3 (bsed_igemm3)."""
    if w3.dim() == 6:
        if w3.shape[2] * 16 != CIN or w3.shape[1] != len(taps):
            raise L.BsedError(f"igemm3: weight table packed for K={w3.shape[2] * 16}, {w3.shape[1]} taps; "
                              f"called with CIN={CIN}, {len(taps)} taps")
        return _igemm3_launch("bsed_igemm3n", inp, w3, N, w3.shape[0] * 32, NB, H, W, CIN, taps, bias, epilogue, valid)
    if inp.dtype != torch.float32:
        raise L.BsedError("bf16 activations need the N-split route of igemm3 (igemm3_nsplit()), not the slab kernel")
    return _igemm3_launch("bsed_igemm3", inp, w3, N, w3.shape[2], NB, H, W, CIN, taps, bias, epilogue, valid)


def set_igemm3n_shape(shape):
    """A/B knob: MFMA shape of the nine-tap N-split instances: 16 (16 x 16 x 32), 32 (32 x 32 x 16), 0 / None = default"""
    L.lib().bsed_igemm3n_set_shape(shape or 0)


def set_igemm3n_wpe(wpe):
    """A/B knob of the BN = 128 build: 2 / 3 = built for that many waves per SIMD whatever the shape; + 8 = no raised
    wave priority outside the MFMA loop; 0 / None = default"""
    L.lib().bsed_igemm3n_set_wpe(wpe or 0)


def contract_route(direction, CIN, N, W, ntaps, mode):
    """Name of the kernel that runs the PLAIN / STATS contraction of CIN input with N output channels over ntaps taps on a
    width-W map, in the contraction's own terms (a data gradient has the layer's CIN and N swapped).  The only place that
    compares them with mode (the caller's conv_mode); contract switches on the name, and a new contraction kernel is
    wired in here."""
    if mode not in ("fp32", "bf16x3", "bf16"):
        raise L.BsedError(f"contract_route: unknown mode {mode!r}")
    if direction not in ("forward", "dgrad"):
        raise L.BsedError(f"contract_route: unknown direction {direction!r}")
    if mode == "fp32":
        return "igemm"        # the fp32-core kernel (csrc/igemm.hip)
    if ntaps == 9 and (CIN == 16 and igemm3s_supported(W, 16) if direction == "forward" else
                       CIN == 32 and N <= 32 and igemm3s_supported(W, 32)):
        return "igemm3s"      # the bf16 cores, all taps' weights resident in LDS (csrc/igemm3.hip)
    if CIN % 32 == 0:
        return "igemm3"       # the bf16 cores: slab or N-split kernel, as igemm3_nsplit() says
    return "igemm"            # channel counts neither bf16-core kernel is built for


def contract(inp, wv, NB, H, W, *, mode, direction="forward", bias=None, epilogue=EPI_PLAIN, valid=None):
    """Pack the weights of the WeightView wv and run the PLAIN / STATS contraction with them on the kernel contract_route
    names.  direction="dgrad": wv is the layer's forward view and inp the gradient of its output; the contraction runs
    over wv.dgrad().  Returns (out, stats or None).  mode: the caller's conv_mode."""
    if direction == "dgrad":
        wv = wv.dgrad()
    src, taps, CIN, N, strides = wv.source(), wv.taps, wv.K, wv.N, wv[5:]
    route = contract_route(direction, CIN, N, W, len(taps), mode)
    if route == "igemm3s":
        wtab = pack_weight3s(src, len(taps), N, *strides, K=CIN)
        return igemm3s(inp, wtab, N, NB, H, W, taps, bias=bias, epilogue=epilogue)
    if route == "igemm3":
        w3 = pack_weight3(src, len(taps), CIN, N, *strides)
        return igemm3(inp, w3, N, NB, H, W, CIN, taps, bias=bias, epilogue=epilogue, valid=valid)
    wpk = pack_weight(src, len(taps), CIN, N, *strides)
    return igemm(inp, wpk, N, NB, H, W, CIN, taps=taps, bias=bias, epilogue=epilogue, valid=valid)


def wgrad(inp, dy, NB, H, W, CIN, N, taps=((0, 0),), in_pitch=None, dy_pitch=None, a_scale=None, a_shift=None,
          in_offset=0, dy_offset=0, *, mode, bn_y=None, bn_coef=None, bn_mean=None, dy_out=None, G=None):
    """Partial slabs of dW; returns (part, G, CINP, NP).  mode: the caller's conv_mode -- "fp32" = the fp32-core
    kernels, "bf16x3" / "bf16" = split-fp32 operands on the bf16 cores.  G: number of partial slabs (None or 0: the
    plan's); the library takes 1..number of tiles and refuses anything else.
    bn_y / bn_coef / bn_mean: `dy` is dL/d(BatchNorm output) and BatchNorm's backward is applied on load (bf16x3 only);
    dy_out then receives d_y for the data-gradient convolution."""
    if mode not in ("fp32", "bf16x3", "bf16"):
        raise L.BsedError(f"wgrad: unknown mode {mode!r}")
    sfx = "3" if mode in ("bf16x3", "bf16") else ""
    d = WgradDesc()
    _tile_taps(d, H, W, taps)
    CINP, NP = round_up(CIN, 32), round_up(N, 32)
    d.in_ = _dp(inp, in_offset); d.dy = _dp(dy, dy_offset)
    d.a_scale = _p(a_scale); d.a_shift = _p(a_shift)
    d.act_bf16 = _abf(inp, dy, bn_y, dy_out)
    if d.act_bf16 and sfx != "3":
        raise L.BsedError("bf16 activations need the split-fp32 / bf16 weight-gradient kernels (mode bf16x3 or bf16)")
    d.bn_y, d.bn_coef, d.bn_mean, d.dy_out = _dp(bn_y), _p(bn_coef), _p(bn_mean), _dp(dy_out)
    d.in_pitch = CIN if in_pitch is None else in_pitch
    d.dy_pitch = N if dy_pitch is None else dy_pitch
    d.NB, d.H, d.W, d.CIN, d.CINP, d.N, d.NP = NB, H, W, CIN, CINP, N, NP
    plan = _contract_plan(f"bsed_wgrad{sfx}", d)
    G = d.G = G or plan.G
    part = torch.empty((G, len(taps), CINP, NP), device=inp.device, dtype=torch.float32)
    d.part = _p(part)
    # algorithmic bytes: the input and dy once; with the fused BatchNorm backward also y (read) and d_y (written)
    nbytes = _esz(inp) * NB * H * W * (CIN + N * (1 + (1 if bn_y is not None else 0) + (1 if dy_out is not None else 0)))
    # the label = the template instance as rocprofv3 prints it (bench.py joins the two by name)
    _launch((plan.label.decode(), len(taps), CIN, N, H, W),
            2.0 * NB * H * W * len(taps) * CIN * N, lambda: L.call(f"bsed_wgrad{sfx}", ctypes.byref(d), L.stream()), nbytes)
    return part, G, CINP, NP


_rq = None   # the active queue of deferred reductions: dict(stream=..., jobs=[(ReduceJob fields..., keepalive)])


class deferred_reductions:
    """Inside this block the partial-slab reductions whose results nothing in the block reads (weight and bias
    gradients: only the optimizer / the gradient all-reduce need them) are queued instead of launched, and go out
    together -- one bsed_reduce_partials_batch launch per flush instead of ~30 launches of 10 us each.  flush() in the
    middle publishes everything queued so far (the data-parallel trainer does that before its early all-reduce).
    Reductions issued on another stream than the one the block was opened on run immediately."""

    def __enter__(self):
        global _rq
        self._outer = _rq
        _rq = {"stream": L.stream().value, "jobs": []}
        return self

    def __exit__(self, *exc):
        global _rq
        try:
            if exc[0] is None:
                flush_reductions()
        finally:
            _rq = self._outer
        return False


def flush_reductions():
    """launch what the active queue holds (jobs writing the same destination go to successive launches, in order)"""
    if _rq is None or not _rq["jobs"]:
        return
    pending, _rq["jobs"] = _rq["jobs"], []
    while pending:
        batch, rest, seen = [], [], set()
        for job in pending:
            key = job[1]
            if key in seen or len(batch) == REDUCE_MAX_JOBS or rest:
                rest.append(job)          # keep the order of everything behind the first job that has to wait
            else:
                seen.add(key)
                batch.append(job)
        arr = (ReduceJob * len(batch))()
        nel = 0
        for i, (part, dst_ptr, G, ntaps, KP, NP, K, N, s_tap, s_k, s_n, acc) in enumerate(batch):
            arr[i].part, arr[i].dst = part.data_ptr(), dst_ptr
            arr[i].G, arr[i].ntaps, arr[i].KP, arr[i].NP, arr[i].K, arr[i].N = G, ntaps, KP, NP, K, N
            arr[i].accumulate, arr[i].s_tap, arr[i].s_k, arr[i].s_n = acc, s_tap, s_k, s_n
            nel += part.numel()
        _note("reduce_partials_batch_kernel", f"jobs{len(batch)}", float(nel), 4.0 * nel)
        L.call("bsed_reduce_partials_batch", arr, len(batch), L.stream())
        pending = rest


def reduce_partials(part, G, ntaps, KP, NP, K, N, dst, s_tap, s_k, s_n, accumulate=True, dst_offset=0, defer=True):
    """defer=False: run now even inside ops.deferred_reductions() (the caller reads dst right away)"""
    if defer and _rq is not None and _rq["stream"] == L.stream().value:
        _rq["jobs"].append((part, _dp(dst, dst_offset), G, ntaps, KP, NP, K, N, s_tap, s_k, s_n, 1 if accumulate else 0))
        return
    _note("reduce_partials_kernel", f"G{G}", float(part.numel()), 4.0 * part.numel())
    L.call("bsed_reduce_partials", L.ptr(part), G, ntaps, KP, NP, K, N, _dp(dst, dst_offset), s_tap, s_k, s_n,
           1 if accumulate else 0, L.stream())


def weight_grad(inp, dy, gv, NB, H, W, *, mode, accumulate=True, defer=True, **kw):
    """dW of the contraction whose forward weight view has gv's geometry, from its input and the gradient dy of its
    output, reduced into gv (a view .over() the gradient tensor).  **kw: wgrad's pitches, offsets, a_scale / a_shift and
    bn_* / dy_out fusion arguments."""
    part, G, KP, NP = wgrad(inp, dy, NB, H, W, gv.K, gv.N, taps=gv.taps, mode=mode, **kw)
    reduce_partials(part, G, len(gv.taps), KP, NP, gv.K, gv.N, gv.tensor, gv.s_tap, gv.s_k, gv.s_n, accumulate=accumulate,
                    dst_offset=gv.offset, defer=defer)


def _conv_bwd_desc(NB, H, W, CIN, N, act_bf16=0):
    """the shape fields of bsed_conv_bwd3's descriptor: a 3x3 / pad 1 convolution of CIN -> N channels with dense rows"""
    d = WgradDesc()
    _tile_taps(d, H, W, TAPS3x3)
    d.NB, d.H, d.W, d.CIN, d.CINP, d.N, d.NP = NB, H, W, CIN, round_up(CIN, 32), N, round_up(N, 32)
    d.in_pitch, d.dy_pitch, d.din_pitch, d.act_bf16 = CIN, N, CIN, act_bf16
    return d


def conv_bwd_plan(NB, H, W, CIN, N, act_bf16=0):
    """(descriptor, BsedContractPlan) of the one-pass backward kernel (bsed_conv_bwd3) for a 3x3 convolution under a
    BatchNorm, or (descriptor, None) where the kernel does not take the shape (L.last_error() says why).  plan.G = 0:
    the kernel takes it, but the library keeps the layer on its two kernels (bsed_conv_bwd_plan's rule)."""
    d = _conv_bwd_desc(NB, H, W, CIN, N, act_bf16)
    plan = ContractPlan()
    if L.lib().bsed_conv_bwd_plan(ctypes.byref(d), ctypes.byref(plan)) != 0:
        return d, None
    return d, plan


def conv_bwd_fused(inp, g, y, coef, mean, wv, NB, H, W, G=None, planned=None):
    """One pass over inp, g and y (csrc/conv_bwd.hip): BatchNorm backward on load, the partial slabs of the weight gradient
    AND the data gradient, d_y never written.  wv: the layer's forward WeightView.  G: number of partial slabs (default:
    the plan's; the kernel takes any 1..max_G).  planned: conv_bwd_plan's (descriptor, plan) of this shape where the
    caller has asked already.  Returns (d_in, part, G, CINP, NP); raises where the kernel does not take the shape."""
    CIN, N = wv.K, wv.N
    d, plan = planned or conv_bwd_plan(NB, H, W, CIN, N, _abf(inp, g, y))
    if plan is None or wv.taps != tuple(TAPS3x3):
        raise L.BsedError("conv_bwd_fused: " + (L.lib().bsed_last_error().decode() if plan is None else "3x3 taps only"))
    G = G or plan.G or min(256, plan.max_G)
    tv = wv.dgrad()
    wtab = pack_weight3s(tv.source(), 9, tv.N, tv.s_tap, tv.s_k, tv.s_n, K=tv.K)
    d_in = torch.empty((NB, H, W, CIN), device=inp.device, dtype=torch.float32)
    part = torch.empty((G, 9, d.CINP, d.NP), device=inp.device, dtype=torch.float32)
    d.in_ = _dp(inp); d.dy = _dp(g); d.part = _p(part); d.G = G
    d.bn_y, d.bn_coef, d.bn_mean = _dp(y), _p(coef), _p(mean)
    d.w3s, d.d_in = wtab.data_ptr(), _p(d_in)
    # algorithmic work: both contractions; inp, g and y read once, d_in written once
    _launch((plan.label.decode(), 9, CIN, N, H, W), 2 * 2.0 * NB * H * W * 9 * CIN * N,
            lambda: L.call("bsed_conv_bwd3", ctypes.byref(d), L.stream()), 4.0 * NB * H * W * (2 * CIN + 2 * N))
    return d_in, part, G, d.CINP, d.NP


def conv_bn_backward(inp, g, y, coef, mean, wv, gv, NB, H, W, *, mode, need_dgrad=True, fused=None):
    """Backward of a 3x3 convolution whose output feeds a train-mode BatchNorm, in the split-fp32 modes: g = dL/d(BatchNorm
    output), y = the convolution's output, coef / mean from bn_bwd(apply=False).  dW is reduced into gv; returns dL/d(inp)
    (None without need_dgrad).  fused: None = bsed_conv_bwd_plan decides between the one-pass kernel and the two kernels
    it replaces (weight gradient writing d_y, data gradient reading it back); False = the two kernels; True = the one-pass
    kernel or an error."""
    use, planned = False, None
    if fused is not False and need_dgrad and mode == "bf16x3":
        planned = conv_bwd_plan(NB, H, W, wv.K, wv.N, _abf(inp, g, y))
        plan = planned[1]
        use = plan is not None and wv.taps == tuple(TAPS3x3) and (fused is True or plan.G > 0)
    if fused is True and not use:
        raise L.BsedError("conv_bn_backward: the one-pass kernel does not take this layer: " +
                          L.lib().bsed_last_error().decode())
    if use:
        d_in, part, G, KP, NP = conv_bwd_fused(inp, g, y, coef, mean, wv, NB, H, W, planned=planned)
        reduce_partials(part, G, 9, KP, NP, gv.K, gv.N, gv.tensor, gv.s_tap, gv.s_k, gv.s_n, dst_offset=gv.offset)
        return d_in
    dy = torch.empty_like(g) if need_dgrad else None
    weight_grad(inp, g, gv, NB, H, W, mode=mode, bn_y=y, bn_coef=coef, bn_mean=mean, dy_out=dy)
    if not need_dgrad:
        return None
    return contract(dy, wv, NB, H, W, mode=mode, direction="dgrad")[0]


_scratch = {}


def stats_scratch(C, device):
    key = (C, str(device), L.stream().value)   # one scratch per stream: launches of different streams may overlap
    s = _scratch.get(key)
    if s is None:
        s = _scratch[key] = torch.empty((L.lib().bsed_stats_scratch_bytes(C) + 7) // 8, device=device,
                                        dtype=torch.float64)
    return s


def conv0_fwd(x, w, bias, NB, H, W, CO, want_stats):
    y = torch.empty((NB, H, W, CO), device=x.device, dtype=torch.float32)
    stats = None
    nt = L.lib().bsed_conv0_num_tiles(NB, H, W)
    if want_stats:
        stats = torch.empty((nt, 2, CO), device=x.device, dtype=torch.float32)
    _note(f"conv0_fwd_kernel<{CO}>", f"{H}x{W}", 2.0 * 9 * CO * NB * H * W, 4.0 * NB * H * W * (1 + CO))
    L.call("bsed_conv0_fwd", L.ptr(x), _dp(w), _dp(bias), L.ptr(y), _p(stats), NB, H, W, CO, L.stream())
    return y, stats


def conv0_wgrad(x, dy, NB, H, W, CO, y=None, coef=None, mean=None):
    """y/coef/mean given: dy is dL/d(BatchNorm output) and BatchNorm's backward is applied on load"""
    G = min(1024, max(1, (NB * H * W) // 256))
    part = torch.empty((G, 9, CO), device=x.device, dtype=torch.float32)
    # x, dy (= g) and, with the fused BatchNorm backward, y: each read once
    _note(f"conv0_wgrad_kernel<{CO}, {'true' if y is not None else 'false'}>", f"{H}x{W}",
          2.0 * 9 * CO * NB * H * W, 4.0 * NB * H * W * (1 + CO * (2 if y is not None else 1)))
    L.call("bsed_conv0_wgrad", L.ptr(x), L.ptr(dy), _p(y), _p(coef), _p(mean), L.ptr(part), G, NB, H, W, CO,
           L.stream())
    return part, G


# The eight GLU / first-block entry points: one descriptor (BsedGluDesc), one plan query.  entry point -> its
# BSED_GLU_* id, whether it cuts the map into tiles, and the KernelTimer label of the instance it launches, a format
# over C, the plan's variant (v), the PH / SMALL halves of block0's variant and act_bf16 (ab)
_GLU_KERNELS = {
    "bsed_glu16_fwd": (L.CONSTANTS["BSED_GLU_16_FWD"], False, "glu16_fwd_kernel"),
    "bsed_glu16_bwd": (L.CONSTANTS["BSED_GLU_16_BWD"], False, "glu16_bwd_kernel"),
    "bsed_block0_fwd": (L.CONSTANTS["BSED_GLU_BLOCK0_FWD"], False, "b0_fwd_kernel<{ph}, {small}, {ab}>"),
    "bsed_block0_bwd": (L.CONSTANTS["BSED_GLU_BLOCK0_BWD"], False, "b0_bwd_kernel<{ph}, {small}, {ab}>"),
    "bsed_glu_bwd_fused": (L.CONSTANTS["BSED_GLU_BWD_FUSED"], True, "glu_bwd_fused_kernel<{C}, {v}>"),
    "bsed_glu_fwd3": (L.CONSTANTS["BSED_GLU_FWD3"], True, "glu_fwd3_kernel<{C}, {v}, {ab}>"),
    "bsed_glu_bwd3": (L.CONSTANTS["BSED_GLU_BWD3"], True, "glu_bwd3_kernel<{C}, {v}, {ab}>"),
    "bsed_glu_bwd3n": (L.CONSTANTS["BSED_GLU_BWD3N"], True, "glu_bwd3n_kernel<{ab}>"),
}
_GLU_ACTIVATIONS = ("y", "dpool", "pooled", "g", "dlin")   # fp32, or all bf16 in the "bf16" mode (_pa, _abf)
_GLU_PARAMETERS = ("cw", "cb", "w", "bias")                # may be views into a flat parameter buffer (_dp)


def _glu_plan(entry, d):
    """BsedGluPlan of the entry point's launch for the shape fields of d; sets d.G to the plan's"""
    plan = GluPlan()
    L.check(L.lib().bsed_glu_plan(ctypes.byref(d), _GLU_KERNELS[entry][0], ctypes.byref(plan)), entry)
    d.G = plan.G
    return plan


def _glu_label(entry, d, plan):
    v = plan.variant
    return _GLU_KERNELS[entry][2].format(C=d.C, v=v, ph=v & 15, small="true" if v >> 4 else "false", ab=d.act_bf16)


def _glu_desc(entry, NB, H, W, C, pool, drop_p, rng_stream, seed, **tensors):
    """(BsedGluDesc, its plan) of the entry point's launch on these tensors"""
    d = GluDesc(NB=NB, H=H, W=W, C=C, ph=pool[0], pw=pool[1], drop_p=drop_p, rng_stream=rng_stream, seed=seed,
                act_bf16=_abf(*(tensors.get(n) for n in _GLU_ACTIVATIONS)))
    if _GLU_KERNELS[entry][1]:
        d.TH, d.TW = tile_for(W)
    for name, t in tensors.items():
        setattr(d, name, _pa(t) if name in _GLU_ACTIVATIONS else _dp(t) if name in _GLU_PARAMETERS else L.ptr(t))
    return d, _glu_plan(entry, d)


def _glu_launch(entry, d, plan, flops, nbytes):
    """launch the entry point; the KernelTimer hears of it under the label of the instance the plan names"""
    if L.timer is not None:
        label = _glu_label(entry, d, plan)
        if _GLU_KERNELS[entry][1]:
            return _launch((label, 1, d.C, d.C, d.H, d.W), flops, lambda: L.call(entry, ctypes.byref(d), L.stream()), nbytes)
        _note(label, f"{d.H}x{d.W}", flops, nbytes)
    L.call(entry, ctypes.byref(d), L.stream())


def _glu_partials(plan, C, dev):
    """partial sums of a GLU backward as its plan sizes them: (part_dw (dw_rows,C,C), part_db (G,2,C), part_st (G,2,C))"""
    return (torch.empty((plan.dw_rows, C, C), device=dev, dtype=torch.float32),
            torch.empty((plan.G, 2, C), device=dev, dtype=torch.float32),
            torch.empty((plan.G, 2, C), device=dev, dtype=torch.float32))


def glu16_fwd(y, scale, shift, wg, bg, B, H, W, pool, drop_p, rng_stream, seed):
    ph, pw = pool
    out = torch.empty((B, H // ph, W // pw, 16), device=y.device, dtype=torch.float32)
    d, plan = _glu_desc("bsed_glu16_fwd", B, H, W, 16, pool, drop_p, rng_stream, seed, y=y, scale=scale,
                        shift=shift, w=wg, bias=bg, pooled=out)
    _glu_launch("bsed_glu16_fwd", d, plan, 2.0 * B * H * W * 256, 4.0 * B * H * W * 16 * (1.0 + 1.0 / (ph * pw)))
    return out


def glu16_bwd(y, scale, shift, wg, bg, dpool, B, H, W, pool, drop_p, rng_stream, seed):
    """returns (g, part_dw (G,16,16), part_db (G,2,16), part_st (G,2,16), G)"""
    ph, pw = pool
    g = torch.empty_like(y)
    d, plan = _glu_desc("bsed_glu16_bwd", B, H, W, 16, pool, drop_p, rng_stream, seed, y=y, scale=scale,
                        shift=shift, w=wg, bias=bg, dpool=dpool, g=g)
    part_dw, part_db, part_st = _glu_partials(plan, 16, y.device)
    d.part_dw, d.part_db, d.part_st = L.ptr(part_dw), L.ptr(part_db), L.ptr(part_st)
    _glu_launch("bsed_glu16_bwd", d, plan, 3 * 2.0 * B * H * W * 256,
                4.0 * B * H * W * 16 * (2.0 + 1.0 / (ph * pw)))
    return g, part_dw, part_db, part_st, plan.G


def block0_stats(x, cw, cb, NB, H, W):
    """train-mode statistics of the first block from x alone: returns (stats (G,2,16) for bn_finalize, xr64 (54,) fp64)"""
    G = int(min(2048, max(1, (NB * H * W) // 256)))
    dev = x.device
    stats = torch.empty((G, 2, 16), device=dev, dtype=torch.float32)
    xr_part = torch.empty((G, 54), device=dev, dtype=torch.float32)
    xr64 = torch.empty(54, device=dev, dtype=torch.float64)
    _note("b0_stats_kernel", f"{H}x{W}", 2.0 * NB * H * W * (9 * 16 + 16 + 54), 4.0 * NB * H * W)
    cwt = cw.detach().reshape(16, 9).t().contiguous()   # [tap][channel]: channel pairs become packed scalar operands
    L.call("bsed_block0_stats", L.ptr(x), L.ptr(cwt), _dp(cb), L.ptr(stats), L.ptr(xr_part),
           L.ptr(xr64, torch.float64), G, NB, H, W, 16, L.stream())
    return stats, xr64


def block0_fwd(x, cw, cb, scale, shift, wg, bg, B, H, W, pool, drop_p, rng_stream, seed, out_dtype=torch.float32):
    ph, pw = pool
    out = torch.empty((B, H // ph, W // pw, 16), device=x.device, dtype=out_dtype)
    d, plan = _glu_desc("bsed_block0_fwd", B, H, W, 16, pool, drop_p, rng_stream, seed, x=x, cw=cw, cb=cb,
                        scale=scale, shift=shift, w=wg, bias=bg, pooled=out)
    _glu_launch("bsed_block0_fwd", d, plan, 2.0 * B * H * W * (9 * 16 + 256),
                B * H * W * (4.0 + _esz(out) * 16.0 / (ph * pw)))
    return out


def block0_bwd(x, cw, cb, scale, shift, wg, bg, dpool, B, H, W, pool, drop_p, rng_stream, seed):
    """returns (part_dw (G,16,16), part_db (G,2,16), part_st (G,2,16), part_gx (G,9,16), G)"""
    ph, pw = pool
    d, plan = _glu_desc("bsed_block0_bwd", B, H, W, 16, pool, drop_p, rng_stream, seed, x=x, cw=cw, cb=cb,
                        scale=scale, shift=shift, w=wg, bias=bg, dpool=dpool)
    part_dw, part_db, part_st = _glu_partials(plan, 16, x.device)
    part_gx = torch.empty((plan.G, 9, 16), device=x.device, dtype=torch.float32)
    d.part_dw, d.part_db, d.part_st, d.part_gx = L.ptr(part_dw), L.ptr(part_db), L.ptr(part_st), L.ptr(part_gx)
    _glu_launch("bsed_block0_bwd", d, plan, 2.0 * B * H * W * (2 * 9 * 16 + 3 * 256),
                B * H * W * (4.0 + _esz(dpool) * 16.0 / (ph * pw)))
    return part_dw, part_db, part_st, part_gx, plan.G


def block0_wgrad_finish(part_gx, G, xr64, coef, mean, cw, cb, dst, accumulate=True):
    _note("b0_wgrad_finish_kernel", f"G{G}", float(part_gx.numel()), 4.0 * part_gx.numel())
    L.call("bsed_block0_wgrad_finish", L.ptr(part_gx), G, L.ptr(xr64, torch.float64), L.ptr(coef), L.ptr(mean),
           _dp(cw), _dp(cb), _dp(dst), 1 if accumulate else 0, 16, L.stream())


def _glu_bwd_tiled(entry, esz, y, dpool, B, H, W, C, pool, drop_p, rng_stream, seed, **weights):
    """a tiled fused GLU backward with its weight-gradient slabs; returns (g, part_dw (G*slabs,C,C), part_db (G,2,C),
    part_st (G,2,C), G, slabs)"""
    g = torch.empty_like(y)
    d, plan = _glu_desc(entry, B, H, W, C, pool, drop_p, rng_stream, seed, y=y, dpool=dpool, g=g, **weights)
    part_dw, part_db, part_st = _glu_partials(plan, C, y.device)
    d.part_dw, d.part_db, d.part_st = L.ptr(part_dw), L.ptr(part_db), L.ptr(part_st)
    _glu_launch(entry, d, plan, 3 * 2.0 * B * H * W * C * C,
                esz * B * H * W * C * (2.0 + 1.0 / (pool[0] * pool[1])))  # y, g, d_pooled
    return g, part_dw, part_db, part_st, plan.G, plan.dw_rows // plan.G


def glu_bwd_fused(y, scale, shift, wfwd, w, bias, dpool, B, H, W, C, pool, drop_p, rng_stream, seed):
    """fp32-core fused GLU backward (C in {32,64,128}); returns (g, part_dw, part_db, part_st, G, slabs)"""
    return _glu_bwd_tiled("bsed_glu_bwd_fused", 4.0, y, dpool, B, H, W, C, pool, drop_p, rng_stream, seed,
                          scale=scale, shift=shift, wfwd=wfwd, w=w, bias=bias)


def glu_fwd3_supported(W, C, pool):
    TH, TW = tile_for(W)
    return (C in (32, 64, 128) and (pool[1] == 1 or TW >= 2) and
            (pool[0] == 1 or ((TW in (2, 8, 16) or (TW == 1 and pool[1] == 1)) and TH % 2 == 0)))


def glu_fwd3(y, scale, shift, w, bias, B, H, W, C, pool, drop_p, rng_stream, seed):
    """split-fp32 GLU forward: BN-apply -> Linear -> gate -> dropout -> avg-pool in one pass over y"""
    ph, pw = pool
    out = torch.empty((B, H // ph, W // pw, C), device=y.device, dtype=y.dtype)
    d, plan = _glu_desc("bsed_glu_fwd3", B, H, W, C, pool, drop_p, rng_stream, seed, y=y, scale=scale, shift=shift,
                        w=w, bias=bias, pooled=out)
    _glu_launch("bsed_glu_fwd3", d, plan, 2.0 * B * H * W * C * C,
                _esz(y) * B * H * W * C * (1.0 + 1.0 / (ph * pw)))  # y, pooled
    return out


def glu_bwd3(y, scale, shift, w, bias, dpool, B, H, W, C, pool, drop_p, rng_stream, seed):
    """split-fp32 fused GLU backward (C in {32,64}); returns like glu_bwd_fused"""
    return _glu_bwd_tiled("bsed_glu_bwd3", _esz(y), y, dpool, B, H, W, C, pool, drop_p, rng_stream, seed,
                          scale=scale, shift=shift, w=w, bias=bias)


_frag_tables = {}


def glu_bwd3n(y, scale, shift, w, bias, dpool, B, H, W, C, pool, drop_p, rng_stream, seed):
    """split-fp32 GLU backward for C = 128 without the weight gradient: returns (g, d_lin, part_db, part_st, G)"""
    dev = y.device
    g = torch.empty_like(y)
    dlin = torch.empty_like(y)
    d, plan = _glu_desc("bsed_glu_bwd3n", B, H, W, C, pool, drop_p, rng_stream, seed, y=y, scale=scale,
                        shift=shift, w=w, bias=bias, dpool=dpool, g=g, dlin=dlin)
    tb = _frag_tables.get(str(dev))
    if tb is None:
        tb = _frag_tables[str(dev)] = torch.empty(plan.table_bytes, device=dev, dtype=torch.uint8)
    part_db = torch.empty((plan.G, 2, C), device=dev, dtype=torch.float32)
    part_st = torch.empty((plan.G, 2, C), device=dev, dtype=torch.float32)
    d.part_db, d.part_st, d.frag_table = L.ptr(part_db), L.ptr(part_st), tb.data_ptr()
    _glu_launch("bsed_glu_bwd3n", d, plan, 2 * 2.0 * B * H * W * C * C,
                _esz(y) * B * H * W * C * (3.0 + 1.0 / (pool[0] * pool[1])))  # y, g, d_lin, d_pooled
    return g, dlin, part_db, part_st, plan.G


def glu_route(direction, C, W, pool, mode, fused=True):
    """Name of the kernel route that runs the GLU half of a CNN block (BN-apply -> Linear -> gate -> dropout -> avg-pool)
    with C channels on a width-W map.  The only place that compares C, W, pool, mode (the caller's conv_mode) and fused
    (False: the unfused backward chain, a cross-check); glu_forward / glu_backward switch on the name, and a new GLU
    kernel is wired in here.  The fused first block (block0_*) is a whole block, not a route of this table."""
    if mode not in ("fp32", "bf16x3", "bf16"):
        raise L.BsedError(f"glu_route: unknown mode {mode!r}")
    if direction not in ("forward", "backward"):
        raise L.BsedError(f"glu_route: unknown direction {direction!r}")
    if C == 16:
        return "glu16"        # 4 FLOP/B: one HBM-bound streaming pass instead of MFMA tiles (csrc/glu_small.hip)
    if direction == "forward":
        if mode != "fp32" and glu_fwd3_supported(W, C, pool):
            return "glu3"     # the bf16 cores, operands fetched in MFMA register layout (csrc/glu3.hip)
        return "igemm"        # the fp32-core contraction with the GLU_POOL epilogue (csrc/igemm.hip)
    if C in (32, 64) and fused and mode != "fp32":
        return "glu3"         # all three contractions on the bf16 cores (csrc/glu3.hip)
    if C == 128 and fused and mode != "fp32":
        return "glu3n"        # lin recompute + g on the bf16 cores; d_lin goes through HBM to a 1-tap weight gradient
    if C in (32, 64, 128) and fused:
        return "fused_fp32"   # three chained MFMA contractions per tile, y read once, g written once (csrc/glu_bwd.hip)
    return "unfused"          # igemm GLU_BWD (d_lin, gate term) -> 1-tap weight gradient -> igemm ADD_STATS2 (g)


def glu_forward(y, scale, shift, w, bias, B, H, W, C, pool, drop_p, rng_stream, seed, *, mode):
    """GLU half of a block on the conv output y (B,H,W,C) with BatchNorm's scale / shift; returns the pooled output"""
    route = glu_route("forward", C, W, pool, mode)
    if route == "glu16":
        return glu16_fwd(y, scale, shift, w, bias, B, H, W, pool, drop_p, rng_stream, seed)
    if route == "glu3":
        return glu_fwd3(y, scale, shift, w, bias, B, H, W, C, pool, drop_p, rng_stream, seed)
    wg = pack_weight(w, 1, C, C, 0, 1, C)
    return igemm(y, wg, C, B, H, W, C, bias=bias, epilogue=EPI_GLU_POOL, a_scale=scale, a_shift=shift, e_src=y,
                 e_scale=scale, e_shift=shift, pool=pool, drop_p=drop_p, rng_stream=rng_stream, seed=seed)[0]


def glu_backward(y, scale, shift, w, bias, dpool, B, H, W, C, pool, drop_p, rng_stream, seed, *, mode, fused, dw, db):
    """Backward of glu_forward: accumulates the GLU linear's gradients into dw / db; returns (g, st2) = dL/d(BatchNorm
    output) and the BatchNorm-backward partial sums"""
    route = glu_route("backward", C, W, pool, mode, fused)
    dpool = dpool.contiguous()
    tail = (pool, drop_p, rng_stream, seed)
    if route in ("glu3n", "unfused"):   # d_lin goes through HBM: dW_glu = d_lin^T @ bn(y) is a 1-tap weight gradient
        if route == "glu3n":
            g, dlin, pdb, st2, _ = glu_bwd3n(y, scale, shift, w, bias, dpool, B, H, W, C, *tail)
        else:                           # (1) recompute lin, form d_lin and the gate-branch term (into tt)
            tt = torch.empty_like(y)
            dlin, pdb = igemm(y, pack_weight(w, 1, C, C, 0, 1, C), C, B, H, W, C, bias=bias, epilogue=EPI_GLU_BWD,
                              a_scale=scale, a_shift=shift, e_src=y, e_scale=scale, e_shift=shift, e_dpool=dpool,
                              out2=tt, pool=pool, drop_p=drop_p, rng_stream=rng_stream, seed=seed)
        stats_to_grad(pdb, C, 0, db)
        weight_grad(y, dlin, linear_weight(dw), B, H, W, a_scale=scale, a_shift=shift, mode=mode)
        if route == "unfused":          # (3) g = d_lin @ W_glu + gate term, with the BatchNorm-backward sums
            g, st2 = igemm(dlin, pack_weight(w, 1, C, C, 0, C, 1), C, B, H, W, C, epilogue=EPI_ADD_STATS2, out=tt,
                           out2=tt, e_src=y)
        return g, st2
    if route == "glu16":
        g, pdw, pdb, st2, G = glu16_bwd(y, scale, shift, w, bias, dpool, B, H, W, *tail)
        slabs = 1
    elif route == "glu3":
        g, pdw, pdb, st2, G, slabs = glu_bwd3(y, scale, shift, w, bias, dpool, B, H, W, C, *tail)
    else:
        wfwd = pack_weight(w, 1, C, C, 0, 1, C)
        g, pdw, pdb, st2, G, slabs = glu_bwd_fused(y, scale, shift, wfwd, w, bias, dpool, B, H, W, C, *tail)
    reduce_partials(pdw, G * slabs, 1, C, C, C, C, dw, 0, C, 1)
    stats_to_grad(pdb, C, 0, db)
    return g, st2


def bn_finalize(stats, C, count, eps, momentum, gamma, beta, rmean, rvar, nbt):
    dev = stats.device
    mean, invstd, scale, shift = (torch.empty(C, device=dev, dtype=torch.float32) for _ in range(4))
    _note("stats_chunk_kernel+stats_finish_kernel", f"C{C}", 0.0, 4.0 * stats.numel())
    L.call("bsed_bn_finalize", L.ptr(stats), stats.shape[0], C, count, eps, momentum, _dp(gamma), _dp(beta), _dp(rmean),
           _dp(rvar), _dp(nbt), L.ptr(mean), L.ptr(invstd), L.ptr(scale),
           L.ptr(shift), L.ptr(stats_scratch(C, dev), torch.float64), L.stream())
    return mean, invstd, scale, shift


def bn_eval(C, eps, gamma, beta, rmean, rvar):
    dev = gamma.device
    scale, shift = (torch.empty(C, device=dev, dtype=torch.float32) for _ in range(2))
    L.call("bsed_bn_eval", C, eps, _dp(gamma), _dp(beta), _dp(rmean), _dp(rvar), L.ptr(scale), L.ptr(shift),
           L.stream())
    return scale, shift


def bn_eval_batch(layers, eps):
    """[(C, gamma, beta, running_mean, running_var), ...] -> [(scale, shift), ...] in one launch (eval-mode forward)"""
    dev = layers[0][1].device
    out = torch.empty(2 * sum(l[0] for l in layers), device=dev, dtype=torch.float32)
    arr = (BnEvalJob * len(layers))()
    res, off = [], 0
    for a, (C, gamma, beta, rmean, rvar) in zip(arr, layers):
        scale, shift = out[off:off + C], out[off + C:off + 2 * C]
        off += 2 * C
        a.gamma, a.beta, a.running_mean, a.running_var = _dp(gamma), _dp(beta), _dp(rmean), _dp(rvar)
        a.scale, a.shift, a.C = scale.data_ptr(), shift.data_ptr(), C
        res.append((scale, shift))
    _note("bn_eval_batch_kernel", "", 0.0, 4.0 * 3 * out.numel())
    L.call("bsed_bn_eval_batch", arr, len(layers), eps, L.stream())
    return res


def bn_bwd(stats, C, count, gamma, mean, invstd, dgamma, dbeta, g_inout, y, apply=True):
    """apply=False: only dgamma/dbeta and the (3,C) coefficients [A|B|C] of d_y = A g + B (y-mean) + C (returned);
    the consumer applies the map on load (conv0_wgrad)."""
    dev = stats.device
    coef = torch.empty((3, C), device=dev, dtype=torch.float32)
    _note("bn_bwd_apply_kernel" if apply else "stats_chunk_kernel+stats_finish_kernel", f"C{C}", 3.0 * y.numel() if apply else 0.0,
          12.0 * y.numel() if apply else 4.0 * stats.numel())
    L.call("bsed_bn_bwd", L.ptr(stats), stats.shape[0], C, count, _dp(gamma), L.ptr(mean), L.ptr(invstd), _dp(dgamma),
           _dp(dbeta), 1,
           L.ptr(g_inout) if apply else None, L.ptr(y) if apply else None,
           y.numel() if apply else C, L.ptr(coef), L.ptr(stats_scratch(C, dev), torch.float64),
           L.stream())
    return coef


def stats_to_grad(stats, C, which, dst):
    if _rq is not None and _rq["stream"] == L.stream().value and which == 0 and stats.dim() == 3 and stats.shape[1] == 2:
        # row 0 of every (2, C) partial: a queued slab reduction with K = 1 of KP = 2 rows (fp32 sums, fixed order)
        _rq["jobs"].append((stats, _dp(dst), stats.shape[0], 1, 2, C, 1, C, 0, 0, 1, 1))
        return
    _note("stats_chunk_kernel+stats_finish_kernel", f"C{C}", 0.0, 4.0 * stats.numel())
    L.call("bsed_stats_to_grad", L.ptr(stats), stats.shape[0], C, which, _dp(dst), 1,
           L.ptr(stats_scratch(C, stats.device), torch.float64), L.stream())


def colsum(inp, M, C, pitch, dst, accumulate=True, in_offset=0):
    G = int(min(512, M))
    part = torch.empty((G, 2, C), device=inp.device, dtype=torch.float32)
    _note("colsum_kernel", f"C{C}", float(M) * C, 4.0 * M * C)
    if _rq is not None and _rq["stream"] == L.stream().value:
        L.call("bsed_colsum_part", _dp(inp, in_offset), M, C, pitch, L.ptr(part), G,
               L.stream())
        _rq["jobs"].append((part, _dp(dst), G, 1, 2, C, 1, C, 0, 0, 1, 1 if accumulate else 0))
        return
    L.call("bsed_colsum", _dp(inp, in_offset), M, C, pitch, L.ptr(part), G,
           _dp(dst), 1 if accumulate else 0, L.ptr(stats_scratch(C, inp.device), torch.float64), L.stream())


def dropout(x, p, rng_stream, seed):
    out = torch.empty_like(x)
    _note("dropout_kernel", "", float(x.numel()), 8.0 * x.numel())
    L.call("bsed_dropout", L.ptr(x), L.ptr(out), x.numel(), p, rng_stream, seed, L.stream())
    return out


def gru_rows(B):
    """rows per workgroup of the fp32 register kernels so that (B/R) x 2 directions fills the 256 CUs"""
    return 1 if B * 2 <= 256 else 2


def gru_fwd(xp, w_hh, b_hh, B, T, save_gates, mode="fp32"):
    out = torch.empty((B, T, 256), device=xp.device, dtype=torch.float32)
    gates = torch.empty((B, T, 2, 4, 128), device=xp.device, dtype=torch.float32) if save_gates else None
    _note("gru_fwd_mfma_kernel<true>" if mode == "bf16x3" else "gru_fwd_kernel", f"T{T}", 2.0 * B * T * 2 * 128 * 384,
          4.0 * B * T * (768 + 256 + (1024 if save_gates else 0)))
    if mode == "bf16x3":  # matrix-core recurrence, split-fp32 operands
        L.call("bsed_gru_fwd3", L.ptr(xp), _dp(w_hh), _dp(b_hh), L.ptr(out), _p(gates), B, T,
               L.stream())
    else:
        L.call("bsed_gru_fwd", L.ptr(xp), _dp(w_hh), _dp(b_hh), L.ptr(out), _p(gates), B, T, gru_rows(B),
               L.stream())
    return out, gates


def gru_bwd(dout, out, gates, w_hh, B, T, mode="fp32"):
    dxp = torch.empty((B, T, 768), device=dout.device, dtype=torch.float32)
    dgh = torch.empty((B, T, 768), device=dout.device, dtype=torch.float32)
    _note("gru_bwd_mfma_kernel" if mode == "bf16x3" else "gru_bwd_kernel", f"T{T}", 2.0 * B * T * 2 * 128 * 384,
          4.0 * B * T * (256 + 256 + 1024 + 768 + 768))
    if mode == "bf16x3":
        rows = L.lib().bsed_gru_bwd3_rows(B)
        pih = torch.empty((rows, 768), device=dout.device, dtype=torch.float32)
        phh = torch.empty((rows, 768), device=dout.device, dtype=torch.float32)
        L.call("bsed_gru_bwd3", L.ptr(dout), L.ptr(out), L.ptr(gates), _dp(w_hh), L.ptr(dxp), L.ptr(dgh),
               L.ptr(pih), L.ptr(phh), B, T, L.stream())
        return dxp, dgh, pih, phh
    else:
        L.call("bsed_gru_bwd", L.ptr(dout), L.ptr(out), L.ptr(gates), _dp(w_hh), L.ptr(dxp), L.ptr(dgh), B, T,
               gru_rows(B), L.stream())
    return dxp, dgh, None, None


def max_over_time(y):
    """(B,T,C) -> (B,C) maximum over time (weak targets of the train loop: ``target.max(-2)[0]``)"""
    y = y.contiguous().float()
    B, T, C = y.shape
    out = torch.empty((B, C), device=y.device, dtype=torch.float32)
    _note("max_over_time_kernel", f"T{T}", 0.0, 4.0 * (y.numel() + out.numel()))
    L.call("bsed_max_over_time", L.ptr(y), L.ptr(out), B, T, C, L.stream())
    return out


def _head_kernel(direction, C):
    """the instance bsed_head_fwd / bsed_head_bwd launch for C classes (csrc/head.hip): the 20-class build, or NT tiles
    of 32 columns over the 2C logits with the weights in LDS (C <= 32) or read from L2 (33..64)"""
    if C == 20:
        return f"head_{direction}_kernel<20>"
    return f"head_{direction}_n_kernel<{(2 * C + 31) // 32},{'lds' if C <= 32 else 'l2'}>"


def head_fwd(x, w, b, B, T, K, C, attention):
    dev = x.device
    strong = torch.empty((B, T, C), device=dev, dtype=torch.float32)
    sof = torch.empty((B, T, C), device=dev, dtype=torch.float32)
    weak = torch.empty((B, C), device=dev, dtype=torch.float32)
    den = torch.empty((B, C), device=dev, dtype=torch.float32)
    S = L.lib().bsed_head_splits(B, T)
    part = torch.empty((B, S, 2, C), device=dev, dtype=torch.float32) if S > 1 else None
    _note(_head_kernel("fwd", C), f"T{T}", 2.0 * B * T * K * 2 * C, 4.0 * B * T * (K + 2 * C))
    L.call("bsed_head_fwd", L.ptr(x), _dp(w), _dp(b), L.ptr(strong), L.ptr(sof), L.ptr(weak), L.ptr(den), L.ptr(part),
           B, T, K, C, 1 if attention else 0, L.stream())
    return strong, sof, weak, den


def head_bwd(x, w, strong, sof, weak, den, B, T, K, C, attention, y_strong=None, y_weak=None, ema_strong=None,
             ema_weak=None, g_strong=None, g_weak=None, w_strong=1.0, w_weak=1.0, w_cons_s=0.0, w_cons_w=0.0,
             ema_strong2=None, w_cons_s2=0.0, n_strong=None, n_weak=None):
    """n_strong / n_weak: element counts the 'mean' reductions divide by (default B*T*C and B*C; pass the FULL batch
    counts when the call covers only a slice of the batch)"""
    dev = x.device
    d = HeadBwdDesc()
    dx = torch.empty((B, T, K), device=dev, dtype=torch.float32)
    S = L.lib().bsed_head_splits(B, T)                               # rows per clip in the partial outputs
    dw_part = torch.empty((B * S, 2 * C, K), device=dev, dtype=torch.float32)
    db_part = torch.empty((B * S, 2 * C), device=dev, dtype=torch.float32)
    loss_part = torch.empty((B * S, 6), device=dev, dtype=torch.float32)
    d.x = _p(x); d.w = _dp(w); d.strong = _p(strong); d.sof_raw = _p(sof); d.weak = _p(weak); d.den = _p(den)
    d.y_strong = _p(y_strong); d.y_weak = _p(y_weak); d.ema_strong = _p(ema_strong); d.ema_weak = _p(ema_weak)
    d.g_strong_ext = _p(g_strong); d.g_weak_ext = _p(g_weak); d.ema_strong2 = _p(ema_strong2)
    d.w_strong, d.w_weak, d.w_cons_s, d.w_cons_w, d.w_cons_s2 = w_strong, w_weak, w_cons_s, w_cons_w, w_cons_s2
    d.inv_n_strong = 1.0 / (n_strong if n_strong else B * T * C)
    d.inv_n_weak = 1.0 / (n_weak if n_weak else B * C)
    d.dx = _p(dx); d.dw_part = _p(dw_part); d.db_part = _p(db_part); d.loss_part = _p(loss_part)
    d.B, d.T, d.K, d.C, d.attention = B, T, K, C, 1 if attention else 0
    _note(_head_kernel("bwd", C), f"T{T}", 3 * 2.0 * B * T * K * 2 * C, 4.0 * B * T * (2 * K + 4 * C))
    L.call("bsed_head_bwd", ctypes.byref(d), L.stream())
    return dx, dw_part, db_part, loss_part


def tag_head_fwd(x, logits):
    """CNN-only tagging head (csrc/tag.hip): x, logits (B,T,128) -> (strong (B,T,128), weak (B,128))"""
    B, T, C = x.shape
    S = L.lib().bsed_tag_splits(B, T)
    strong = torch.empty_like(x)
    weak = torch.empty((B, C), device=x.device, dtype=torch.float32)
    part = torch.empty((B, S, 2, C), device=x.device, dtype=torch.float32)
    _note("tag_pool_kernel", f"T{T}", 12.0 * B * T * C, 12.0 * B * T * C)
    L.call("bsed_tag_head_fwd", L.ptr(x), L.ptr(logits), L.ptr(strong), L.ptr(weak), L.ptr(part), B, T, C, L.stream())
    return strong, weak


def adam_step(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    _note("adam_kernel", "", 12.0 * p.numel(), 28.0 * p.numel())
    L.call("bsed_adam_step", L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, betas[0], betas[1], eps,
           weight_decay, step, grad_scale, L.stream())


def sgd_step(p, g, buf, lr, momentum, weight_decay, first_step, nesterov=True, grad_scale=1.0):
    _note("sgd_kernel", "", 6.0 * p.numel(), 20.0 * p.numel())
    L.call("bsed_sgd_step", L.ptr(p), L.ptr(g), L.ptr(buf), p.numel(), lr, momentum, weight_decay,
           1 if first_step else 0, 1 if nesterov else 0, grad_scale, L.stream())


def roll(x, B, H, W, sh=None, sw=None):
    """per-sample torch.roll of a contiguous (B,H,W[,..]) tensor viewed as (B,H,W); sh/sw: int32 device tensors (B)"""
    out = torch.empty_like(x)
    _note("roll_kernel", "", 0.0, 8.0 * x.numel())
    L.call("bsed_roll", L.ptr(x), L.ptr(out), B, H, W, L.ptr(sh, torch.int32), L.ptr(sw, torch.int32), L.stream())
    return out


def mix_rows(jobs):
    """jobs: [(x, perm, lam), ...] (at most MIX_MAX_JOBS) -> [lam * x + (1 - lam) * x[perm], ...] over the rows of every
    x, in ONE launch (the inputs, labels or teacher targets of the mixup passes; rounding rule: include/bsed.h).  x: a
    contiguous fp32 tensor, viewed as (x.shape[0], -1); perm: an int32 device tensor of x.shape[0] entries."""
    n = len(jobs)
    ins, outs, perms = ((ctypes.c_void_p * n)() for _ in range(3))
    lam, oml = (ctypes.c_float * n)(), (ctypes.c_float * n)()
    rows, row_len = (ctypes.c_int * n)(), (ctypes.c_long * n)()
    res, total = [], 0
    for i, (x, perm, l) in enumerate(jobs):
        if x.dim() < 1 or x.shape[0] < 1 or x.numel() < 1:
            raise L.BsedError(f"mix_rows: job {i} has no rows or empty rows (shape {tuple(x.shape)})")
        if perm.numel() != x.shape[0]:
            raise L.BsedError(f"mix_rows: job {i} has {x.shape[0]} rows but {perm.numel()} perm entries")
        out = torch.empty_like(x)
        ins[i], outs[i], perms[i] = L.ptr(x).value, L.ptr(out).value, L.ptr(perm, torch.int32).value
        lam[i], oml[i] = l, 1.0 - l          # rounded to float32 here; the subtraction is done in double
        rows[i], row_len[i] = x.shape[0], x.numel() // x.shape[0]
        total += x.numel()
        res.append(out)
    _note("mix_rows_kernel", f"{n} jobs", 3.0 * total, 12.0 * total)
    L.call("bsed_mix_rows", ins, outs, perms, lam, oml, rows, row_len, n, L.stream())
    return res


def axpy(y, x, a=1.0):
    """y += a * x in place (contiguous fp32 tensors of equal size)"""
    _note("axpy_kernel", "", 2.0 * y.numel(), 12.0 * y.numel())
    L.call("bsed_axpy", L.ptr(y), L.ptr(x.contiguous()), y.numel(), a, L.stream())
    return y


def ema_update(ema, p, alpha):
    _note("ema_kernel", "", 3.0 * p.numel(), 12.0 * p.numel())
    L.call("bsed_ema_update", L.ptr(ema), L.ptr(p), p.numel(), alpha, L.stream())


def ema_update_i64(ema, p, alpha):
    L.call("bsed_ema_update_i64", L.ptr(ema, torch.int64), L.ptr(p, torch.int64), p.numel(), alpha,
           L.stream())


def upsample_time(inp, T_out, out=None, out_offset=0):
    """(B,T_in,C) -> (B,T_out,C) linear interpolation along time (align_corners=True); ``out`` may be a wider
    (B,T_out,P) buffer whose columns out_offset..out_offset+C receive the result (concatenation without a copy)"""
    B, T_in, C = inp.shape
    if out is None:
        out = torch.empty((B, T_out, C), device=inp.device, dtype=torch.float32)
    L.call("bsed_upsample_time_fwd", L.ptr(inp), _dp(out, out_offset), B, T_in, T_out, C, inp.shape[2], out.shape[2],
           L.stream())
    return out


def upsample_time_bwd(dout, T_in, C, in_offset=0):
    """adjoint of upsample_time: dout (B,T_out,P) columns in_offset..in_offset+C -> (B,T_in,C)"""
    B, T_out, P = dout.shape
    din = torch.empty((B, T_in, C), device=dout.device, dtype=torch.float32)
    L.call("bsed_upsample_time_bwd", _dp(dout, in_offset), L.ptr(din), B, T_in, T_out, C, P, C, L.stream())
    return din


def synth_mix(bank, bg_off, bg_len, bg_phase, bg_gain, n_ev, src, on, length, g, inv_fade, B, n, K, coverage=0.0, out=None):
    """``bsed_synth_mix``: B clips of n samples mixed from the flat fp32 ``bank`` (include/bsed.h states the arithmetic).
    The tables are device tensors: bg_off / bg_len / bg_phase (B) and src / on / length (B, K) int64, bg_gain (B) and
    g / inv_fade (B, K) float32, n_ev (B) int32.  coverage: the mean number of events over an output sample (for the
    work announcement alone) -> (B, n) float32."""
    if out is None:
        out = torch.empty((B, n), device=bank.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, n):
        raise L.BsedError(f"synth_mix: out must be ({B}, {n}), got {tuple(out.shape)}")
    i64 = torch.int64
    # bytes: the output, the background and `coverage` snippet samples per output sample; flops: a multiply for the
    # background, two multiplies for the fade, the fade product and the multiply-add per covered sample
    _note("synth_mix_kernel", f"n{n} K{K}", B * n * (1.0 + 5.0 * coverage), 4.0 * B * n * (2.0 + coverage))
    L.call("bsed_synth_mix", L.ptr(bank), bank.numel(), L.ptr(bg_off, i64), L.ptr(bg_len, i64), L.ptr(bg_phase, i64),
           L.ptr(bg_gain), L.ptr(n_ev, torch.int32), L.ptr(src, i64), L.ptr(on, i64), L.ptr(length, i64), L.ptr(g),
           L.ptr(inv_fade), B, n, K, L.ptr(out), L.stream())
    return out


def synth_targets(n_ev, cls, on_f, off_f, B, K, T, C):
    """``bsed_synth_targets``: int32 device tables n_ev (B) and cls / on_f / off_f (B, K) -> (strong (B, T, C),
    weak (B, C)) float32, every element written by the one launch."""
    strong = torch.empty((B, T, C), device=n_ev.device, dtype=torch.float32)
    weak = torch.empty((B, C), device=n_ev.device, dtype=torch.float32)
    i32 = torch.int32
    _note("synth_targets_kernel", f"T{T} C{C}", 0.0, 4.0 * B * C * (T + 1))
    L.call("bsed_synth_targets", L.ptr(n_ev, i32), L.ptr(cls, i32), L.ptr(on_f, i32), L.ptr(off_f, i32), B, K, T, C,
           L.ptr(strong), L.ptr(weak), L.stream())
    return strong, weak


def loudness(x, seg_off, seg_len, sr, max_len, counts=False, samples=None):
    """``bsed_loudness``: the BS.1770-4 integrated loudness (LUFS) of S segments of the flat fp32 device buffer ``x``
    (include/bsed.h states the rules).  seg_off / seg_len: (S,) int64 device tensors; max_len: a host bound on the
    lengths (a longer segment is measured over its first max_len samples).  samples: the effective samples of all
    segments, for the work announcement alone (default S * max_len).  -> loud (S,) float64, or (loud, counts (S, 3)
    int32: blocks, blocks above the absolute gate, blocks above both) with ``counts=True``.  Two launches, no host sync."""
    S, sr, max_len = int(seg_off.numel()), int(sr), int(max_len)
    if int(seg_len.numel()) != S:
        raise L.BsedError(f"loudness: {S} offsets but {int(seg_len.numel())} lengths")
    nbytes = L.lib().bsed_loudness_ws_bytes(S, max_len, sr)
    if nbytes < 0:
        raise L.BsedError("loudness: " + L.lib().bsed_last_error().decode())
    ws = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)
    loud = torch.empty(S, device=x.device, dtype=torch.float64)
    cnt = torch.empty((S, 3), device=x.device, dtype=torch.int32) if counts else None
    n_samples = float(S * max_len if samples is None else samples)
    _note("loudness_hops_kernel", f"S{S} sr{sr}", 40.0 * n_samples, 4.0 * n_samples)    # two passes of 9 fma, 2 fma for y^2
    L.call("bsed_loudness", L.ptr(x), x.numel(), L.ptr(seg_off, torch.int64), L.ptr(seg_len, torch.int64), S, max_len, sr,
           L.ptr(ws, torch.float64), nbytes, L.ptr(loud, torch.float64), L.ptr(cnt, torch.int32), L.stream())
    return (loud, cnt) if counts else loud
