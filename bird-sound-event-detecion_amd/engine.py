"""Train step / EMA / schedules: the host-side mirror of one iteration of the reference's ``train_mt``.

  train_step            <- reference src/main_baseline.py:197-598 (one loop iteration, no ISP):
                           student forward on the synthetic and the real batch, optional EMA-teacher
                           forward on the noisy real batch, BCE strong/weak + MSE consistency, backward,
                           optimizer step, EMA update.
  update_ema_variables  <- src/main_baseline.py:91-105
  adjust_learning_rate  <- src/main_baseline.py:53-88
  ramps                 <- src/utilities/ramps.py:4-30

Everything between the waveform batch and the updated parameters runs in HIP kernels on the current
stream; the host only sequences launches (no ``.item()`` / device syncs inside the step, unlike the
reference's >= 6 syncs per iteration).  Data parallelism: one process per GPU; the gradients of CRNN, Predictor
and discriminator live in ONE flat arena (``parallel.GradArena``) whose all-reduce (RCCL through
``torch.distributed``, backend "nccl") is started from inside the last backward pass, as soon as every gradient
but the first two CNN blocks' has been enqueued, and overlaps the rest of it; the 1/world factor is folded into
the optimizer kernel.
"""
import contextlib
from typing import Any, NamedTuple

import numpy as np

import torch

from . import _lib as L
from . import ops
from . import parallel


# ----------------------------------------------------------------------------- schedules
def exp_rampup(current, rampup_length):
    if rampup_length == 0:
        return 1.0
    current = np.clip(current, 0.0, rampup_length)
    phase = 1.0 - current / rampup_length
    return float(np.exp(-5.0 * phase * phase))


def sigmoid_rampdown(current, rampup_length):
    if rampup_length == 0:
        return 1.0
    current = np.clip(current, 0.0, rampup_length)
    phase = 1.0 - current / rampup_length
    return float(np.exp(-12.5 * phase * phase))


def adjust_learning_rate(optimizer, rampup_value, rampdown_value=1, optimizer_d=None, optimizer_crnn=None,
                         c_epoch=None, rampup_value_adv=None, max_learning_rate=0.0005):
    """Same schedule and argument order as the reference; ``optimizer`` objects need ``param_groups``
    (torch optimizers) or an ``lr`` attribute (FlatAdam / FlatSGD below)."""
    lr = rampup_value * rampdown_value * max_learning_rate
    if c_epoch is not None and c_epoch > 100:
        lr = lr * (0.5 ** (1 + ((c_epoch - 100) // 20)))

    def _set(opt, value):
        if hasattr(opt, "param_groups"):
            for g in opt.param_groups:
                g["lr"] = value
        else:
            opt.lr = value
    _set(optimizer, lr)
    if optimizer_d is not None:
        _set(optimizer_d, lr * 0.1)
    if optimizer_crnn is not None:
        _set(optimizer_crnn, lr * 0.1)
    return lr


def _state_arenas(module):
    """A module's whole state as flat arenas: ([parameters, float buffers (BatchNorm running statistics) if it has any],
    the int64 num_batches_tracked counters or None)."""
    floats = [module.flat] + ([module.flat_buf] if getattr(module, "flat_buf", None) is not None else [])
    return floats, getattr(module, "nbt", None)


@torch.no_grad()
def update_ema_variables(model, ema_model, alpha, global_step):
    """ema = ema*alpha' + model*(1-alpha'), alpha' = min(1 - 1/(step+1), alpha), over EVERY state entry
    (parameters, BatchNorm running statistics and the int64 num_batches_tracked counters), one kernel per
    flat arena.  (The reference implementation raises for a plain CRNN because of its "cnn." key quirk --
    DESIGN.md D8 -- this is the update it intends.)"""
    alpha = min(1 - 1 / (global_step + 1), alpha)
    (floats, nbt), (ema_floats, ema_nbt) = _state_arenas(model), _state_arenas(ema_model)
    for dst, src in zip(ema_floats, floats):
        ops.ema_update(dst, src, alpha)
    if nbt is not None:
        ops.ema_update_i64(ema_nbt, nbt, alpha)


# ----------------------------------------------------------------------------- optimizers on flat arenas
def _ref_params(modules):
    """[(module index, offset, numel, shape)] in the reference optimizer's parameter order
    (``list(crnn.parameters()) + list(predictor.parameters())``, src/main_baseline.py:865)"""
    out = []
    for k, m in enumerate(modules):
        names = m.reference_param_names() if hasattr(m, "reference_param_names") else [n for n, _ in m.named_parameters()]
        for n in names:
            p = m.P(n)
            out.append((k, m._poff[n], p.numel(), tuple(p.shape)))
    return out


class _FlatOptimizer:
    """What FlatAdam and FlatSGD share: the modules, and the table that maps the reference's per-parameter optimizer
    state onto per-module arenas."""

    def __init__(self, modules):
        self.modules = list(modules)
        self._params = _ref_params(self.modules)
        self.step_count = 0

    def zero_grad(self, set_to_none=False):
        for m in self.modules:
            m.flat_grad.zero_()

    def _slices(self, *arenas):
        """per parameter, in reference order: (shape, its slice of each of ``arenas``, lists of one tensor per module)"""
        return [(shape, [a[k][off:off + n] for a in arenas]) for k, off, n, shape in self._params]


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam(lr, betas, eps, weight_decay) over the flat arenas of several modules.  ``state_dict`` /
    ``load_state_dict`` speak torch.optim.Adam's format (per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` in
    the reference's parameter order, CPU tensors), so the ``optimizer`` entry of a checkpoint loads on either side."""

    def __init__(self, modules, lr=0.001, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(modules)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.m = [torch.zeros_like(m.flat) for m in self.modules]
        self.v = [torch.zeros_like(m.flat) for m in self.modules]

    def step(self, grad_scale=1.0):
        self.step_count += 1
        for mod, m, v in zip(self.modules, self.m, self.v):
            ops.adam_step(mod.flat, mod.flat_grad, m, v, self.lr, self.step_count, self.betas, self.eps,
                          self.weight_decay, grad_scale)

    def state_dict(self):
        state = {}
        if self.step_count > 0:
            for i, (shape, (m, v)) in enumerate(self._slices(self.m, self.v)):
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": m.view(shape).detach().cpu().clone(),
                            "exp_avg_sq": v.view(shape).detach().cpu().clone()}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "params": list(range(len(self._params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        if "param_groups" not in sd:          # round-1 files: {"step", "lr", "m", "v"}
            self.step_count, self.lr = sd["step"], sd["lr"]
            for dst, src in zip(self.m + self.v, sd["m"] + sd["v"]):
                dst.copy_(src)
            return
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps = g["lr"], tuple(g["betas"]), g["eps"]
        self.weight_decay = g.get("weight_decay", 0.0)
        if len(g["params"]) != len(self._params):
            raise L.BsedError(f"optimizer state has {len(g['params'])} parameters, the modules have {len(self._params)}")
        steps = set()
        for idx, (_, (m, v)) in zip(g["params"], self._slices(self.m, self.v)):
            st = sd["state"].get(idx)
            if st is None:
                m.zero_(); v.zero_()
                continue
            m.copy_(torch.as_tensor(st["exp_avg"]).reshape(-1))
            v.copy_(torch.as_tensor(st["exp_avg_sq"]).reshape(-1))
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise L.BsedError(f"per-parameter step counts differ ({sorted(steps)}): one flat Adam step cannot hold them")
        self.step_count = steps.pop() if steps else 0


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, nesterov=True, weight_decay) (reference main_scmt_ada_weak.py:854-866);
    state_dict in torch.optim.SGD's format (``momentum_buffer`` per parameter)."""

    def __init__(self, modules, lr=0.001, momentum=0.9, weight_decay=1e-4, nesterov=True):
        super().__init__(modules)
        self.lr, self.momentum, self.weight_decay, self.nesterov = lr, momentum, weight_decay, nesterov
        self.buf = [torch.zeros_like(m.flat) for m in self.modules]

    def step(self, grad_scale=1.0):
        for mod, buf in zip(self.modules, self.buf):
            ops.sgd_step(mod.flat, mod.flat_grad, buf, self.lr, self.momentum, self.weight_decay,
                         self.step_count == 0, self.nesterov, grad_scale)
        self.step_count += 1

    def state_dict(self):
        state = {}
        for i, (shape, (buf,)) in enumerate(self._slices(self.buf)):
            state[i] = {"momentum_buffer": buf.view(shape).detach().cpu().clone() if self.step_count > 0 else None}
        group = {"lr": self.lr, "momentum": self.momentum, "dampening": 0, "weight_decay": self.weight_decay,
                 "nesterov": self.nesterov, "maximize": False, "foreach": None, "differentiable": False, "fused": None,
                 "params": list(range(len(self._params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        self.lr, self.momentum, self.weight_decay = g["lr"], g["momentum"], g.get("weight_decay", 0.0)
        self.nesterov = g.get("nesterov", True)
        seen = False
        for idx, (_, (buf,)) in zip(g["params"], self._slices(self.buf)):
            mb = (sd["state"].get(idx) or {}).get("momentum_buffer")
            if mb is None:
                buf.zero_()
            else:
                buf.copy_(torch.as_tensor(mb).reshape(-1)); seen = True
        self.step_count = 1 if seen else 0      # only "first step or not" matters to the kernel


# ----------------------------------------------------------------------------- waveform inputs, one step ahead
class _Prefetched(NamedTuple):
    """features of ``wav`` made on the feature stream for step ``step``; ``event`` follows the transform"""
    wav: torch.Tensor
    noisy: bool
    step: int
    feats: Any
    event: torch.cuda.Event


class _Uploaded(NamedTuple):
    """the host batch ``wav`` copied into the device tensor ``slot`` for step ``step``; ``event`` follows the copy"""
    wav: torch.Tensor
    slot: torch.Tensor
    event: torch.cuda.Event
    step: int


class _WaveInputs:
    """The ahead-of-time staging of ``from_wave`` inputs: a feature stream on which the NEXT step's waveform -> dB-mel
    transforms run, a copy stream on which its host waveforms are uploaded into two alternating device slots, and the
    two tables (keyed by ``id`` of the caller's tensor) that hand the results to the step they were made for.  The
    caller passes the step number; ``step`` always names the step that trains on the input."""

    def __init__(self, frontend, device, seed, rank):
        self.frontend, self.device, self.seed, self.rank = frontend, device, seed, rank
        self.prefetched, self.feat_stream = {}, None
        self.uploaded, self.copy_stream, self.slots = {}, None, {}

    def device_wave(self, wav):
        """A waveform batch as a device tensor.  Device tensors pass through.  A HOST tensor (pinned memory, if the
        upload is to overlap anything) that ``upload_ahead`` was given was uploaded on the copy stream one step ago: the
        current stream waits for that copy's event.  An unannounced host tensor is uploaded
        here, on the current stream, in front of its consumer (blocking upload: the PCIe time is then inside the step)."""
        if wav.is_cuda:
            return wav
        up = self.uploaded.pop(id(wav), None)
        if up is not None and up.wav is wav:
            cur = torch.cuda.current_stream()
            cur.wait_event(up.event)
            up.slot.record_stream(cur)
            return up.slot
        return wav.to(self.device, non_blocking=True)

    def upload_ahead(self, waves, step):
        """Start the host -> device copies of step ``step``'s waveforms, the NEXT step's, on the copy stream (the copy
        engine works beside this step's kernels: 226 MB per 256 clips = ~4 ms of PCIe at 57 GB/s).
        Device tensors and ``None`` are skipped.  Two device slots per
        shape alternate: the slot refilled now held the batch of two steps ago, whose transform was enqueued on the feature
        stream during the step before last."""
        host = [w for w in waves if w is not None and not w.is_cuda]
        if not host:
            return
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream()
        self.copy_stream.wait_stream(torch.cuda.current_stream())
        if self.feat_stream is not None:
            self.copy_stream.wait_stream(self.feat_stream)
        with torch.cuda.stream(self.copy_stream):
            for k, w in enumerate(host):
                slots = self.slots.setdefault((k, tuple(w.shape), w.dtype), [None, None])
                i = step % 2
                if slots[i] is None:
                    slots[i] = torch.empty(w.shape, dtype=w.dtype, device=self.device)
                slots[i].copy_(w, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self.uploaded[id(w)] = _Uploaded(w, slots[i], ev, step)

    def _transform(self, wav, step, noisy, views=None):
        dwav = self.device_wave(wav)
        T = self.frontend.num_frames(dwav.shape[1])
        return self.frontend.transform(dwav, max_frames=T, noisy=noisy, views=views,
                                       seed=parallel.rank_seed(self.seed, step, self.rank))

    def features(self, wav, step, noisy=False, views=None):
        """The dB-mel input of step ``step`` (with ``noisy``: the pair of it and its noisy twin).
        views: (shift_frames, shift_bins) of the ISP step -- every input comes back as the triple (x, x time-rolled,
        x frequency-rolled); such inputs are never prefetched"""
        pre = self.prefetched.pop(id(wav), None) if views is None else None
        if pre is not None and pre.wav is wav and (pre.noisy, pre.step) == (noisy, step):
            # computed on the feature stream during the previous step (prefetch): same kernels, same seed, same values
            cur = torch.cuda.current_stream()
            cur.wait_event(pre.event)
            for t in (pre.feats if isinstance(pre.feats, tuple) else (pre.feats,)):
                t.record_stream(cur)
            return pre.feats
        return self._transform(wav, step, noisy, views)

    def prefetch(self, waves, step):
        """Enqueue the waveform -> dB-mel transforms of step ``step``, the NEXT one, on the feature stream.  Called from
        the CRNN's recurrence hook: the two GRU layers are latency-bound and occupy half the chip (one workgroup per 4 batch
        rows), the mel kernels run beside them.  waves: [(wav, noisy), ...]; the caller must leave the waveform tensors
        untouched until that step has consumed them.  Host waveforms were put on the copy stream at the start
        of this step (upload_ahead); the feature stream waits for their events."""
        if self.feat_stream is None:
            self.feat_stream = torch.cuda.Stream()
        self.feat_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.feat_stream):
            for wav, noisy in waves:
                feats = self._transform(wav, step, noisy)
                ev = torch.cuda.Event()
                ev.record()
                self.prefetched[id(wav)] = _Prefetched(wav, noisy, step, feats, ev)

    def drop_stale(self, step):
        """Entries announced for step ``step`` or an earlier one that nobody consumed (the caller passed other tensors:
        last batch of an epoch, a skipped batch, an exception between steps) would otherwise pin a waveform batch, its
        feature tensors and an event forever."""
        for table in (self.prefetched, self.uploaded):
            for k in [k for k, v in table.items() if v.step <= step]:
                del table[k]


# ----------------------------------------------------------------------------- the captured step
class _CapturedStep:
    """Everything a held HIP graph of the plain step owns: the graph, its static inputs, the device-resident step state
    its nodes read, and the dict of loss tensors they write.  Dropping the object returns all of it."""
    SEED, STEP = 0, 1       # elements of ``state``: the addend of every dropout seed (uint64), of Adam's step count (int32)

    def __init__(self, x, y, from_wave, device, lr, seed_inc):
        """zero addends: the scalars the capture bakes are those of the captured step itself"""
        self.graph = torch.cuda.CUDAGraph()
        self.x, self.y, self.from_wave, self.seed_inc = x, y, from_wave, seed_inc
        self.state = torch.zeros(4, device=device, dtype=torch.int64)
        self.lr_host = float(lr)
        self.lr = torch.full((1,), self.lr_host, device=device, dtype=torch.float32)
        self.out = None

    def _addends(self):
        return self.state[self.SEED:self.SEED + 1].data_ptr(), self.state[self.STEP:self.STEP + 1].data_ptr()

    @contextlib.contextmanager
    def bound(self):
        """the library reads this step state inside the block (the capture, on the capturing thread), and nowhere else"""
        L.check(L.lib().bsed_set_step_state(*self._addends(), self.lr.data_ptr()), "bsed_set_step_state")
        try:
            yield
        finally:
            L.check(L.lib().bsed_set_step_state(None, None, None), "bsed_set_step_state")

    def advance(self):
        """one step further, in stream order: the last node of the graph, and what an eager step between replays enqueues"""
        L.check(L.lib().bsed_step_state_advance(*self._addends(), self.seed_inc, 1, L.stream()), "bsed_step_state_advance")

    def check_inputs(self, x, y):
        for name, t, g in (("syn_x", x, self.x), ("syn_y", y, self.y)):
            if not isinstance(t, torch.Tensor) or t.shape != g.shape or t.dtype != g.dtype or \
                    (t.device != g.device and t.device.type != "cpu"):
                got = (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__
                raise L.BsedError(f"replay_step: {name} must be {tuple(g.shape)} {g.dtype} on {g.device} as captured, "
                                  f"got {got}")

    def replay(self, x, y, lr):
        """copy the inputs into the static tensors, refresh the device learning rate if it changed, replay"""
        if lr != self.lr_host:
            self.lr.fill_(lr)
            self.lr_host = lr
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        self.graph.replay()
        return self.out


# ----------------------------------------------------------------------------- the train step
# ----------------------------------------------------------------------------- interpolation consistency (mixup)
class IctPlan:
    """The draws of one ISP iteration's interpolation consistency (mixup) passes, on the host: a mixing weight and a
    permutation of the clips for each of the three mixed batches (reference src/main.py:387,427,460) --
      lam_weak,   perm_weak    the weakly labelled half of the real batch, ``real[:half]``
      lam_strong, perm_strong  the synthetic (strongly labelled) batch
      lam_unl,    perm_unl     the unlabelled half of the real batch, ``real[half:]``
    Checked here, without a GPU: every perm is a permutation of ``range(len(perm))`` and every lam lies in [0, 1]
    (``BsedError`` otherwise).  ``check_sizes`` holds the perms against the batch a step is given."""

    def __init__(self, lam_weak, perm_weak, lam_strong, perm_strong, lam_unl, perm_unl):
        for name, lam, perm in (("weak", lam_weak, perm_weak), ("strong", lam_strong, perm_strong), ("unl", lam_unl, perm_unl)):
            try:
                lam, perm = float(lam), tuple(int(v) for v in perm)
            except (TypeError, ValueError):
                raise L.BsedError(f"IctPlan: lam_{name} must be a number and perm_{name} a sequence of integers") from None
            if not 0.0 <= lam <= 1.0:          # false for NaN too
                raise L.BsedError(f"IctPlan: lam_{name} = {lam} lies outside [0, 1]")
            if not perm or sorted(perm) != list(range(len(perm))):
                raise L.BsedError(f"IctPlan: perm_{name} = {list(perm)} is not a permutation of range({len(perm)})")
            setattr(self, "lam_" + name, lam)
            setattr(self, "perm_" + name, perm)

    def check_sizes(self, n_weak, n_strong, n_unl):
        for name, n in (("weak", n_weak), ("strong", n_strong), ("unl", n_unl)):
            if len(getattr(self, "perm_" + name)) != n:
                raise L.BsedError(f"IctPlan: perm_{name} permutes {len(getattr(self, 'perm_' + name))} clips, the batch "
                                  f"has {n}")
        return self

    @property
    def lams(self):
        return self.lam_weak, self.lam_strong, self.lam_unl


def draw_ict(rng, n_weak, n_strong, n_unl, sup_alpha=1.0, usup_alpha=2.0):
    """An ``IctPlan`` drawn on the host from ``rng``, a ``numpy.random.Generator``, in the order of the reference's
    calls (src/main.py:387,427,460): the weak half, the synthetic batch, then the unlabelled half, and for each
    ``beta(alpha, alpha)`` then ``permutation(n)`` (mixup_data_sup / mixup_data, src/main.py:127-156; alpha =
    mixup_sup_alpha 1.0 for the two labelled batches and mixup_usup_alpha 2.0 for the unlabelled one, :368-369).
    ``alpha <= 0`` draws no beta and gives lam = 1, as mixup_data_sup does.  The draws are this project's own stream: the
    reference draws from ``np.random``'s global state, and parity with that state is not claimed."""
    draws = []
    for n, alpha in ((n_weak, sup_alpha), (n_strong, sup_alpha), (n_unl, usup_alpha)):
        if n < 1:
            raise L.BsedError(f"draw_ict: every mixed batch needs at least one clip (got {n_weak}, {n_strong}, {n_unl})")
        draws.append(float(rng.beta(alpha, alpha)) if alpha > 0.0 else 1.0)
        draws.append(rng.permutation(n))
    return IctPlan(*draws)


class SEDTrainer:
    """One object = the state of a training run on ONE GPU (rank).  ``train_step`` is one iteration of the
    reference's ``train_mt`` loop body.  The dataset scaler needs no argument here: every ``from_wave`` input (prefetched
    ones and captured steps included) comes from ``frontend.transform``, so a ``MelFrontEnd`` with a ``Scaler`` attached
    feeds normalised features, as the reference's ``Normalize(scaler)`` transform does."""

    def __init__(self, crnn, predictor, ema_crnn=None, ema_predictor=None, optimizer=None, frontend=None,
                 max_consistency_cost=1.0, ema_alpha=0.999, process_group=None, seed=2023, domain_loss=None,
                 optimizer_d=None):
        """domain_loss: a ``disc.ConditionalDomainAdversarialLoss`` (adversarial variant, reference
        src/main_scmt_ada_weak.py:312-339,527-528,568-574); optimizer_d steps its discriminator."""
        self.domain_loss, self.optimizer_d = domain_loss, optimizer_d
        if domain_loss is not None and optimizer_d is None:
            self.optimizer_d = FlatSGD([domain_loss.domain_discriminator], lr=0.0005 * 0.1)
        self.crnn, self.predictor = crnn, predictor
        self.ema_crnn, self.ema_predictor = ema_crnn, ema_predictor
        self.optimizer = optimizer or FlatAdam([crnn, predictor], lr=0.0005)
        self.frontend = frontend
        self.max_consistency_cost, self.ema_alpha = max_consistency_cost, ema_alpha
        self.global_step = 0
        self.seed = seed
        self.pg = process_group
        # mean teacher: the EMA pair's forward on its own stream beside the student's passes (False: inline)
        self.teacher_overlap = True
        self._teacher_stream = None
        self._step_stream = None
        # the packed weight copies a step needs, made in ONE launch at its start from the second step on
        # (ops.PackPlan; None: one launch per weight at first use, the pre-plan behaviour)
        self._pack_plans = {}
        self._graph = None          # a _CapturedStep: capture_step / replay_step / release_graph
        self.world = 1
        self.rank = 0
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
            self.rank = torch.distributed.get_rank(process_group)
        # from_wave inputs: features and host uploads one step ahead (train_step(..., next_waves=...)); the staging keeps
        # the front end, seed and rank it is given here and is told the step number per call: it never reads the trainer
        self._inputs = _WaveInputs(frontend, crnn.flat.device, seed, self.rank)
        # one gradient arena for everything this rank differentiates: [CRNN (first blocks lead) | Predictor | D]
        self.arena = parallel.GradArena([crnn, predictor, self._disc], tail_floats=crnn.tail_grad_floats(),
                                        group=process_group)

    @property
    def _disc(self):
        return self.domain_loss.domain_discriminator if self.domain_loss is not None else None

    def _plan(self, which):
        if self._pack_plans is None:
            return None
        return self._pack_plans.setdefault(which, ops.PackPlan())

    def broadcast_parameters(self, src=0):
        """identical initial weights / statistics on every rank"""
        if self.world == 1:
            return
        for m in (self.crnn, self.predictor, self.ema_crnn, self.ema_predictor, self._disc):
            if m is None:
                continue
            floats, nbt = _state_arenas(m)
            parallel.broadcast_flat(floats, src, self.pg)
            if nbt is not None:
                parallel.broadcast_flat([nbt], src, self.pg)

    # ------------------------------------------------------------------ the frame every step shares
    def _wave_features(self, syn_x, real_x, real_x_ema, views=None):
        """The dB-mel inputs ``(syn, real, real_ema)`` of this step from its waveforms (prefetched ones are picked up),
        then the staging entries nobody consumed are dropped.  With the EMA teacher and no ``real_x_ema`` the noisy twin
        of the real batch is drawn with the step's rank seed; a given ``real_x_ema`` passes through.  views: the ISP
        step's (shift_frames, shift_bins) -- every transformed input is then the triple (x, time-rolled, frequency-rolled)."""
        features, step = self._inputs.features, self.global_step
        syn_x = features(syn_x, step, views=views)
        if real_x is not None and self.ema_crnn is not None and real_x_ema is None:
            real_x, real_x_ema = features(real_x, step, noisy=True, views=views)
        elif real_x is not None:
            real_x = features(real_x, step, views=views)
        self._inputs.drop_stale(step)
        return syn_x, real_x, real_x_ema

    def _begin_step(self, adv):
        """every module the step uses in train mode (host flags only), the gradient arena zeroed; returns the step seed"""
        for m in (self.crnn, self.predictor, self.ema_crnn, self.ema_predictor, self._disc if adv else None):
            if m is not None:
                m.train()
        self.arena.zero_()
        return parallel.rank_seed(self.seed, self.global_step, self.rank)

    def _teacher_forward(self, x, seed):
        self.ema_crnn.set_seed(seed)
        enc_e, _ = self.ema_crnn.run_forward(x, save=False)
        strong_e, _, weak_e, _ = self.ema_predictor.run_forward(enc_e)
        return strong_e, weak_e

    def _domain_grads(self, enc_s, enc_r, out):
        """the domain loss on the encodings of the synthetic and the real batch; returns its feature gradients
        (d enc_s, d enc_r), which arrive through the gradient-reverse layer"""
        out["domain"] = self.domain_loss(None, enc_s, None, enc_r)
        return self.domain_loss.backward_features()

    def _finish_step(self, adv, ema):
        """data-parallel gradient exchange (wait for the early segment's all-reduce, started inside the last backward
        pass, and exchange the tail), the optimizer steps, the EMA update"""
        self.arena.finish()
        self.optimizer.step(grad_scale=1.0 / self.world)
        if adv:
            self.optimizer_d.step(grad_scale=1.0 / self.world)
        self.global_step += 1
        if ema:
            update_ema_variables(self.crnn, self.ema_crnn, self.ema_alpha, self.global_step)
            update_ema_variables(self.predictor, self.ema_predictor, self.ema_alpha, self.global_step)

    def train_step(self, syn_x, syn_y, real_x=None, real_y_weak=None, real_x_ema=None, consistency_cost=None,
                   from_wave=False, next_waves=None):
        """One iteration (see ``_train_step`` for the arguments).  With the EMA teacher on its own stream the step itself
        runs on a HIGH-PRIORITY stream of the trainer: the teacher's forward (normal priority) then fills the CUs the
        student's passes leave idle instead of taking turns with them -- 17.23 -> 16.96 ms per mean-teacher step at
        B = 128 + 128 (against the caller's stream), same kernels in the same per-stream order: same bits.  The caller's
        stream waits for the step (torch offers no priority BELOW the default one, so the side streams cannot be
        lowered instead).  Without a teacher stream the step stays on the caller's stream
        (measured: no gain for the plain step, 13.48-13.50 vs 13.52-13.53 ms)."""
        mt = self.ema_crnn is not None and real_x is not None
        if not (mt and self.teacher_overlap):
            out = self._train_step(syn_x, syn_y, real_x, real_y_weak, real_x_ema, consistency_cost, from_wave, next_waves)
            if self._graph is not None:
                # an eager step of a trainer that holds a graph is one step of ITS sequence: the advance the graph ends
                # with is enqueued behind it, so the next replay continues one step later (no EMA teacher here: a
                # trainer that has one cannot capture)
                self._graph.advance()
            return out
        caller = torch.cuda.current_stream()
        if self._step_stream is None:
            self._step_stream = torch.cuda.Stream(priority=-1)
        self._step_stream.wait_stream(caller)
        with torch.cuda.stream(self._step_stream):
            out = self._train_step(syn_x, syn_y, real_x, real_y_weak, real_x_ema, consistency_cost, from_wave, next_waves)
        caller.wait_stream(self._step_stream)
        for v in out.values():
            if isinstance(v, torch.Tensor):
                v.record_stream(caller)
        return out

    def _train_step(self, syn_x, syn_y, real_x=None, real_y_weak=None, real_x_ema=None, consistency_cost=None,
                    from_wave=False, next_waves=None):
        """syn_x/real_x: (B,1,T,F) dB-mel batches, or (B,n) waveforms with ``from_wave=True`` (the mel stage then
        runs on the GPU inside the step).  syn_y: (B,T',C) strong targets; real_y_weak: (B,C).
        Mean teacher is active iff EMA models were given AND a real batch is passed.
        next_waves (with from_wave): ``(next_syn_wav, next_real_wav or None)`` -- the waveforms the NEXT call will be
        given.  Their mel transforms are enqueued on a second stream while this step's recurrences run (a two-deep
        input pipeline: every step still transforms one batch, one step ahead); the next call must pass the same
        tensor objects, unmodified.  Results are bit-identical to the unpipelined step.  The waveforms may be HOST
        tensors (pinned): the next step's are then uploaded on a copy stream at the start of this step, beside its
        kernels, into two alternating device slots (an unannounced host batch is uploaded in front of its transform).
        Returns a dict of DEVICE tensors with the per-term loss sums (no host sync)."""
        crnn, pred = self.crnn, self.predictor
        mt = self.ema_crnn is not None and real_x is not None
        if next_waves is not None and not from_wave:
            raise L.BsedError("train_step(next_waves=...) prefetches waveform features: it needs from_wave=True")
        if from_wave:
            if self.frontend is None:
                raise L.BsedError("train_step(from_wave=True) needs a MelFrontEnd")
            if next_waves is not None:
                nxt = [(next_waves[0], False)]
                if len(next_waves) > 1 and next_waves[1] is not None:
                    nxt.append((next_waves[1], mt and real_x_ema is None))
                # one-shot: fires at the first recurrence
                crnn.rnn_hook = lambda: self._inputs.prefetch(nxt, self.global_step + 1)
            syn_x, real_x, real_x_ema = self._wave_features(syn_x, real_x, real_x_ema)
            if next_waves is not None:
                self._inputs.upload_ahead(next_waves, self.global_step + 1)
        adv = self.domain_loss is not None and real_x is not None
        step_seed = self._begin_step(adv)
        out = {}
        B, Tp, C = syn_y.shape
        # (weights are constant until the optimizer step: packed / split copies of a weight tensor are made once and
        #  shared by the forward and backward passes of the step's batches -- ops.pack_cache)
        x_ema = real_x_ema if real_x_ema is not None else real_x      # the teacher's input
        teacher = None
        if mt and self.teacher_overlap:
            # The EMA teacher's forward depends on nothing the student computes in this step: it is enqueued on its own
            # stream NOW and fills the chip beside the student's latency-bound kernels (recurrences, small launches);
            # the consistency loss of the real batch waits for its event.  Same kernels, same inputs: same bits.
            if self._teacher_stream is None:
                self._teacher_stream = torch.cuda.Stream()
            main = torch.cuda.current_stream()
            self._teacher_stream.wait_stream(main)       # features and last step's EMA update are ordered before it
            with torch.cuda.stream(self._teacher_stream), torch.no_grad(), ops.pack_cache(self._plan("teacher")):
                strong_e, weak_e = self._teacher_forward(x_ema, step_seed * 4 + 2)
                ev = torch.cuda.Event()
                ev.record()
            teacher = (strong_e, weak_e, ev)
        with ops.pack_cache(self._plan("step")):
            # ---- student on the synthetic batch: strong + weak BCE
            crnn.set_seed(step_seed * 4 + 0)
            enc_s, ctx_s = crnn.run_forward(syn_x, save=True)
            saved_s = pred.run_forward(enc_s)
            y_weak_syn = ops.max_over_time(syn_y)
            dx, lp = pred.run_backward(enc_s, saved_s, y_strong=syn_y.contiguous(), y_weak=y_weak_syn)
            out["syn"] = lp
            dft = None
            if adv:
                # domain loss on the SAME encodings (the reference runs a second, numerically identical forward when
                # dropout is 0 -- SURVEY.md 8d); its feature gradients arrive through the gradient-reverse layer
                crnn.set_seed(step_seed * 4 + 1)
                enc_r, ctx_r = crnn.run_forward(real_x, save=True)
                dfs, dft = self._domain_grads(enc_s, enc_r, out)
                ops.axpy(dx, dfs)
            # the gradient exchange starts inside the LAST backward pass of the step
            last_is_syn = real_x is None or not (mt or dft is not None)
            crnn.run_backward(ctx_s, dx, on_early_grads=self.arena.begin_early if last_is_syn else None)
            del ctx_s
            # ---- student on the real batch (+ EMA teacher on its noisy twin)
            if real_x is not None:
                if not adv:
                    crnn.set_seed(step_seed * 4 + 1)
                    enc_r, ctx_r = crnn.run_forward(real_x, save=mt)
                saved_r = pred.run_forward(enc_r)
                if mt:
                    w = self.max_consistency_cost if consistency_cost is None else consistency_cost
                    if teacher is not None:
                        strong_e, weak_e, ev = teacher
                        torch.cuda.current_stream().wait_event(ev)
                        strong_e.record_stream(torch.cuda.current_stream())
                        weak_e.record_stream(torch.cuda.current_stream())
                    else:
                        with torch.no_grad():
                            strong_e, weak_e = self._teacher_forward(x_ema, step_seed * 4 + 2)
                    dx, lp = pred.run_backward(enc_r, saved_r, y_weak=real_y_weak.contiguous(), ema_strong=strong_e,
                                               ema_weak=weak_e, w_cons_s=w, w_cons_w=w)
                    if dft is not None:
                        ops.axpy(dx, dft)
                    crnn.run_backward(ctx_r, dx, on_early_grads=self.arena.begin_early)
                    out["real"] = lp
                    del ctx_r
                elif dft is not None:
                    crnn.run_backward(ctx_r, dft.contiguous(), on_early_grads=self.arena.begin_early)
                    del ctx_r
        self._finish_step(adv, ema=mt)
        out["shape"] = (B, Tp, C)
        return out

    # ------------------------------------------------------------------ HIP-graph replay of the plain step
    def capture_step(self, syn_x, syn_y, from_wave=False, warmup=3):
        """Capture the plain train step (synthetic batch only: BASELINE configs[2], the reference's ``train_mt`` without
        ``-mt``) of THIS shape in a HIP graph.  At the reference's batch of 24 (src/data/config.py:70) a step is ~95
        launches of 10-40 us each and the host needs 2.6 ms to enqueue what the GPU runs in < 2 ms: replaying a graph
        removes the host from the loop.  ``warmup`` eager steps run first (allocator, weight-pack plan, lazy tables).
        Returns after the capture; then call ``replay_step(syn_x, syn_y)``.

        What changes from step to step lives in DEVICE memory: an addend of every dropout seed and of Adam's step count,
        both advanced by the last node of the graph, and the learning rate, which ``replay_step`` refreshes from
        ``optimizer.lr``; inputs are copied into the graph's static tensors.  The library is pointed at that memory
        (``bsed_set_step_state``) only while the step is being captured, on the capturing thread: the graph's nodes carry
        the pointers they were captured with, the trainer keeps the memory for exactly as long as it keeps the graph (one
        ``_CapturedStep`` owns both, and ``release_graph`` drops it), and after
        ``capture_step`` has returned or raised the library holds no pointer.  Any number of trainers of a process may
        hold a graph.  The contract,
        for every ``conv_mode`` and A/B switch of the model (tests/test_graph_step_gpu.py): a sequence of steps gives the
        same bits whether its steps are replayed or eager, including
          - ``train_step`` calls of this trainer between replays (any batch size: the last batch of an epoch) -- they
            run on the host's scalars and advance the device state by one step;
          - ``adjust_learning_rate`` / any assignment to ``optimizer.lr`` between steps;
          - steps of OTHER trainers in the process, eager or replayed, and direct calls of ``ops.dropout``, the GLU
            wrappers or ``ops.adam_step``, which never see this trainer's state.
        Refused with ``BsedError``: EMA teacher, discriminator, a data-parallel group (their per-step host decisions
        are not graph nodes) and an optimizer other than ``FlatAdam`` (its per-step scalars are not device-resident)."""
        if self.ema_crnn is not None or self.domain_loss is not None or self.world != 1:
            raise L.BsedError("capture_step covers the plain single-rank step (no EMA teacher, no discriminator, no "
                              "data-parallel group: their per-step host decisions are not graph nodes yet)")
        if not isinstance(self.optimizer, FlatAdam):
            raise L.BsedError("capture_step needs a FlatAdam optimizer: only its step count and learning rate are read "
                              "from device memory by a replayed step")
        self.release_graph()
        x, y = syn_x.clone(), syn_y.clone()
        for _ in range(warmup):
            self._train_step(x, y, from_wave=from_wave)
        seed_inc = (parallel.rank_seed(self.seed, 1, self.rank) - parallel.rank_seed(self.seed, 0, self.rank)) * 4
        step = _CapturedStep(x, y, from_wave, self.crnn.flat.device, self.optimizer.lr, seed_inc)
        base_step, base_count = self.global_step, self.optimizer.step_count
        torch.cuda.synchronize()
        try:
            with step.bound(), torch.cuda.graph(step.graph):
                step.out = self._train_step(x, y, from_wave=from_wave)
                step.advance()
        finally:
            # the capture ran no kernel: undo its host-side bookkeeping (the first replay IS that step)
            self.global_step, self.optimizer.step_count = base_step, base_count
        self._graph = step
        return self

    def replay_step(self, syn_x, syn_y):
        """One captured step on new inputs: tensors of exactly the captured shapes and dtypes, on the captured device (or
        in host memory: the copy into the static tensor uploads them); anything else raises ``BsedError`` before
        anything is copied or launched.  The step uses the optimizer's current ``lr``.  Returns the same dict of device
        tensors as ``train_step`` (overwritten by the next replay)."""
        if self._graph is None:
            raise L.BsedError("replay_step: this trainer holds no captured graph (capture_step makes one, release_graph "
                              "drops it)")
        self._graph.check_inputs(syn_x, syn_y)
        out = self._graph.replay(syn_x, syn_y, float(self.optimizer.lr))
        self.global_step += 1
        self.optimizer.step_count += 1
        return out

    def release_graph(self):
        """back to eager steps only: the graph is dropped, and its static input tensors, its device-resident step state
        and its output tensors go with it (a dict ``replay_step`` returned keeps its own tensors alive)"""
        self._graph = None

    # ------------------------------------------------------------------ ISP (shift-consistency) iteration
    # (no step-state advance as in train_step: ISP needs the EMA teacher, and a trainer that has one cannot hold a graph)
    def train_step_isp(self, syn_x, syn_y, real_x, real_y_weak, real_x_ema=None, shift_frames=None, shift_bins=None,
                       consistency_cost=None, pooling_time_ratio=4, from_wave=False, ict=None):
        """One iteration of ``train_mt`` with ``-mt -ISP`` (reference src/main_baseline.py:229-277,337-420,431-529):
        on top of the mean-teacher step, time-rolled and frequency-rolled views of the synthetic and the real batch go
        through the student (4 extra forward/backward passes) and of the noisy real batch through the teacher (2 extra
        forwards).  shift_frames[k] (a multiple of pooling_time_ratio) / shift_bins[k] are the per-sample rolls the
        reference draws with random.randint(-64,64)*4 / random.randint(-4,4); the first half of the real batch is the
        weakly labelled half (its weak targets enter the frequency-shift class loss).

        Inputs: dB-mel tensors (B,1,T,F) -- the rolled views are then ``bsed_roll`` copies -- or, with ``from_wave=True``,
        (B,n) waveforms (device or host, as ``train_step``): the mel stage runs inside the step and writes every input
        together with its two views (``MelFrontEnd.transform(views=...)``, one kernel per batch, no roll pass over a
        full-size input).  real_x_ema=None (waveforms only) draws the noisy twin of the real batch with the step's
        rank seed, as ``train_step`` does; a given real_x_ema is a dB-mel tensor in both forms.

        With a ``domain_loss`` (src/main_scmt_ada_weak.py:318-339,527-528,568-574: the script's full mode) the domain
        loss is evaluated once, on the encodings of the two base passes, its feature gradients join the base passes'
        backward through the gradient-reverse layer, and ``optimizer_d`` steps the discriminator -- the convention of
        ``train_step``: one forward pair serves the class losses and the domain loss.

        ict: an ``IctPlan`` (``draw_ict``) adds the interpolation consistency (mixup) passes of src/main.py:366-372,
        385-392,425-432,451-470,483 -- three more student passes and one more teacher pass.  The reference's
        ``[weak | unlabel | strong]`` masks (main.py:367,373) map onto this step's batches: the synthetic batch is the
        strongly labelled one, ``real[:half]`` the weakly labelled and ``real[half:]`` the unlabelled half.
          ict_weak    student on the mix of ``real_x[:half]``: weak BCE against the mix of ``real_y_weak[:half]``
          ict_strong  student on the mix of ``syn_x``: strong BCE against the mix of ``syn_y``
          ict_unl     student on the mix of ``real_x[half:]``: cc * MSE(strong) + cc * MSE(weak) against the mix of the
                      teacher's predictions on the CLEAN ``real_x[half:]`` (main.py:453-457), each mean over that pass
        BCE is linear in its target, so BCE against the mixed target is the reference's ``mixup_criterion``.  The mixes
        are ``ops.mix_rows`` launches: one at the start of the step (three inputs, two label tensors), one after the
        teacher passes (its two targets); with ``from_wave`` they read the dB-mel tensors the mel stage wrote.
        Dropout seed slots (``step_seed * 16 + slot``): student passes 0-5 as before, 6 ict_weak, 7 ict_strong,
        11 ict_unl; teacher passes 8-10 as before, 12 the ICT teacher pass.  ``ict=None``: the step without them, launch
        for launch.  Both halves of the real batch must then hold a clip and the perms fit the batches (``BsedError``
        before anything is launched).  ``out`` gains "ict_weak", "ict_strong", "ict_unl" and "ict" = the three lams."""
        if self.ema_crnn is None:
            raise L.BsedError("ISP needs the EMA teacher (the reference's consistency_cost only exists with -mt)")
        if shift_frames is None or shift_bins is None:
            raise L.BsedError("train_step_isp needs the per-sample shift_frames and shift_bins")
        if from_wave and self.frontend is None:
            raise L.BsedError("train_step_isp(from_wave=True) needs a MelFrontEnd")
        if real_x_ema is None and not from_wave:
            raise L.BsedError("train_step_isp on dB-mel tensors needs real_x_ema (the noisy twin of the real batch); "
                              "from_wave=True draws it from the waveforms")
        crnn, pred = self.crnn, self.predictor
        cc = self.max_consistency_cost if consistency_cost is None else consistency_cost
        dev = crnn.flat.device
        B, Tp, C = syn_y.shape
        half = real_y_weak.shape[0] // 2
        if ict is not None:
            if half < 1 or B - half < 1:
                raise L.BsedError(f"train_step_isp(ict=...) mixes the weakly labelled and the unlabelled half of the "
                                  f"real batch: both need a clip (got {half} and {B - half})")
            ict.check_sizes(half, B, B - half)
        sh = torch.as_tensor(list(shift_frames), dtype=torch.int32, device=dev)
        sf = torch.as_tensor(list(shift_bins), dtype=torch.int32, device=dev)
        sp = torch.as_tensor([int(v / pooling_time_ratio) for v in shift_frames], dtype=torch.int32, device=dev)
        # the three inputs and their rolled views: written by the mel stage (waveforms), or rolled where they are used
        views = {}
        if from_wave:
            views["syn"], views["real"], ema = self._wave_features(syn_x, real_x, real_x_ema, views=(sh, sf))
            syn_x, real_x = views["syn"][0], views["real"][0]
            if real_x_ema is None:
                views["ema"], real_x_ema = ema, ema[0]
        adv = self.domain_loss is not None
        step_seed = self._begin_step(adv)
        syn_x, real_x, real_x_ema = syn_x.contiguous(), real_x.contiguous(), real_x_ema.contiguous()
        T, F = syn_x.shape[2], syn_x.shape[3]
        base = {"syn": syn_x, "real": real_x, "ema": real_x_ema}

        def view(which, axis):
            if which in views:
                return views[which][1 if axis == "t" else 2]
            return ops.roll(base[which], B, T, F, sh=sh) if axis == "t" else ops.roll(base[which], B, T, F, sw=sf)

        syn_y = syn_y.contiguous()
        y_weak_syn = ops.max_over_time(syn_y)
        n_s, n_w = B * Tp * C, B * C
        out = {"shape": (B, Tp, C)}
        if ict is not None:
            # the three mixed inputs and the two mixed label tensors, in one launch
            perms = torch.as_tensor(ict.perm_weak + ict.perm_strong + ict.perm_unl, dtype=torch.int32, device=dev)
            p_weak, p_strong, p_unl = perms[:half], perms[half:half + B], perms[half + B:]
            real_unl = real_x[half:]
            mix_x_weak, mix_x_syn, mix_x_unl, mix_y_weak, mix_y_syn = ops.mix_rows([
                (real_x[:half], p_weak, ict.lam_weak), (syn_x, p_strong, ict.lam_strong), (real_unl, p_unl, ict.lam_unl),
                (real_y_weak[:half].contiguous(), p_weak, ict.lam_weak), (syn_y, p_strong, ict.lam_strong)])

        def fwd(x, slot):
            crnn.set_seed(step_seed * 16 + slot)
            enc, ctx = crnn.run_forward(x, save=True)
            return enc, pred.run_forward(enc), ctx

        with ops.pack_cache(self._plan("isp")):   # six student and three teacher passes on unchanged weights: one pack per weight
            # base passes (identical to the mean-teacher step)
            enc_s, sv_s, ctx_s = fwd(syn_x, 0)
            enc_r, sv_r, ctx_r = fwd(real_x, 1)
            with torch.no_grad():
                strong_e, weak_e = self._teacher_forward(real_x_ema, step_seed * 16 + 8)
                strong_e_sh, _ = self._teacher_forward(view("ema", "t"), step_seed * 16 + 9)
                strong_e_fs, _ = self._teacher_forward(view("ema", "f"), step_seed * 16 + 10)
                if ict is not None:
                    # the teacher on the CLEAN unlabelled half (the student's input, not the noisy twin); its two
                    # outputs mixed like the input: the targets of the ict_unl pass
                    mix_e_strong, mix_e_weak = ops.mix_rows([(t, p_unl, ict.lam_unl) for t in
                                                             self._teacher_forward(real_unl, step_seed * 16 + 12)])
            strong_r_roll = ops.roll(sv_r[0], B, Tp, C, sh=sp)      # detached by construction
            strong_s_roll = ops.roll(sv_s[0], B, Tp, C, sh=sp)
            y_s_roll = ops.roll(syn_y, B, Tp, C, sh=sp)
            dfs = dft = None
            if adv:
                # domain loss on the base passes' encodings; its feature gradients arrive through the gradient-reverse
                # layer and join the class-loss gradients of those two passes
                dfs, dft = self._domain_grads(enc_s, enc_r, out)
            dx, out["syn"] = pred.run_backward(enc_s, sv_s, y_strong=syn_y, y_weak=y_weak_syn)
            if dfs is not None:
                ops.axpy(dx, dfs)
            crnn.run_backward(ctx_s, dx)
            dx, out["real"] = pred.run_backward(enc_r, sv_r, y_weak=real_y_weak.contiguous(), ema_strong=strong_e,
                                                ema_weak=weak_e, w_cons_s=cc, w_cons_w=cc)
            if dft is not None:
                ops.axpy(dx, dft)
            crnn.run_backward(ctx_r, dx)
            del ctx_s, ctx_r
            # real, time shift: 1/2 cc MSE vs teacher(shifted) + cc/2 MSE vs the rolled (detached) base prediction
            enc, sv, ctx = fwd(view("real", "t"), 2)
            dx, out["real_shift"] = pred.run_backward(enc, sv, ema_strong=strong_e_sh, w_cons_s=0.5 * cc,
                                                      ema_strong2=strong_r_roll, w_cons_s2=0.5 * cc)
            crnn.run_backward(ctx, dx)
            # real, frequency shift: 1/2 cc MSE vs teacher(freq-shifted); weak BCE on the weakly labelled half only
            enc, sv, ctx = fwd(view("real", "f"), 3)
            parts, lps = [], []
            for lo, hi, yw in ((0, half, real_y_weak[:half].contiguous()), (half, B, None)):
                if hi <= lo:
                    continue
                d, lp = pred.run_backward(enc[lo:hi], tuple(t[lo:hi] for t in sv), y_weak=yw, ema_strong=strong_e_fs[lo:hi],
                                          w_cons_s=0.5 * cc, n_strong=n_s, n_weak=max(half, 1) * C)
                parts.append(d); lps.append(lp)
            out["real_fshift_weak_half"], out["real_fshift_rest"] = lps[0], lps[-1]
            crnn.run_backward(ctx, torch.cat(parts, 0))
            # synthetic, time shift: strong BCE vs the rolled target + cc/2 MSE vs the rolled (detached) base prediction
            enc, sv, ctx = fwd(view("syn", "t"), 4)
            dx, out["syn_shift"] = pred.run_backward(enc, sv, y_strong=y_s_roll, ema_strong=strong_s_roll, w_cons_s=0.5 * cc)
            crnn.run_backward(ctx, dx)
            if ict is not None:
                # interpolation consistency: the mixed weak half (weak BCE), the mixed synthetic batch (strong BCE), the
                # mixed unlabelled half (MSE vs the mixed teacher predictions); means over each pass's own elements
                enc, sv, ctx = fwd(mix_x_weak, 6)
                dx, out["ict_weak"] = pred.run_backward(enc, sv, y_weak=mix_y_weak)
                crnn.run_backward(ctx, dx)
                enc, sv, ctx = fwd(mix_x_syn, 7)
                dx, out["ict_strong"] = pred.run_backward(enc, sv, y_strong=mix_y_syn)
                crnn.run_backward(ctx, dx)
                enc, sv, ctx = fwd(mix_x_unl, 11)
                dx, out["ict_unl"] = pred.run_backward(enc, sv, ema_strong=mix_e_strong, ema_weak=mix_e_weak,
                                                       w_cons_s=cc, w_cons_w=cc)
                crnn.run_backward(ctx, dx)
                out["ict"] = ict.lams
            # synthetic, frequency shift: strong + weak BCE vs the unshifted targets
            enc, sv, ctx = fwd(view("syn", "f"), 5)
            dx, out["syn_fshift"] = pred.run_backward(enc, sv, y_strong=syn_y, y_weak=y_weak_syn)
            crnn.run_backward(ctx, dx, on_early_grads=self.arena.begin_early)
        del ctx
        self._finish_step(adv, ema=True)
        out["isp"] = (cc, half)
        return out

    @staticmethod
    def isp_loss_value(out):
        """scalar the reference would log for an ISP iteration (host sync)"""
        B, Tp, C = out["shape"]
        cc, half = out["isp"]
        n_s, n_w = B * Tp * C, B * C
        g = {k: v.double().sum(0).cpu() for k, v in out.items() if isinstance(v, torch.Tensor)}
        loss = g["syn"][0] / n_s + g["syn"][1] / n_w                                   # strong + weak class (syn)
        loss += g["real"][1] / n_w + cc * (g["real"][2] / n_s + g["real"][3] / n_w)     # weak class (real) + consistency
        loss += g["syn_fshift"][1] / n_w + g["real_fshift_weak_half"][1] / (max(half, 1) * C)  # weak freq-shift class
        loss += g["syn_shift"][0] / n_s                                                 # strong shift class
        loss += g["syn_fshift"][0] / n_s                                                # strong freq-shift class
        loss += 0.5 * cc * (g["syn_shift"][2] / n_s + g["real_shift"][4] / n_s)        # consistency_loss_shift
        fs = g["real_fshift_weak_half"][2] + (g["real_fshift_rest"][2] if half < B else 0.0)
        loss += 0.5 * cc * (g["real_shift"][2] / n_s + fs / n_s)                         # 1/2 (strong shift + freq shift vs EMA)
        if "ict" in out:                                  # the four mixup terms of src/main.py:483
            t = SEDTrainer.ict_loss_terms(out)
            loss += t["mixup_weak_class_loss"] + t["mixup_strong_class_loss"]
            loss += cc * (t["mixup_cons_weak_loss"] + t["mixup_cons_strong_loss"])
        if "domain" in out:
            loss += float(out["domain"])
        return float(loss)

    @staticmethod
    def ict_loss_terms(out):
        """the four interpolation consistency terms of an ISP iteration run with an ``IctPlan``, under the names the
        reference logs them by (src/main.py:392,432,464-470; host sync).  The two consistency terms are the plain means,
        BEFORE the multiplication by the consistency cost, as the reference logs them."""
        B, Tp, C = out["shape"]
        _, half = out["isp"]
        w, s, u = (out[k].double().sum(0).cpu() for k in ("ict_weak", "ict_strong", "ict_unl"))
        return {"mixup_weak_class_loss": float(w[1] / (half * C)),
                "mixup_strong_class_loss": float(s[0] / (B * Tp * C)),
                "mixup_cons_weak_loss": float(u[3] / ((B - half) * C)),
                "mixup_cons_strong_loss": float(u[2] / ((B - half) * Tp * C))}

    @staticmethod
    def loss_value(out, consistency_cost=1.0):
        """Host-side assembly of the scalar the reference logs (syncs: call it outside the timed loop)."""
        B, Tp, C = out["shape"]
        s = out["syn"].double().sum(0).cpu()
        loss = float(s[0] / (B * Tp * C) + s[1] / (B * C))
        if "real" in out:
            r = out["real"].double().sum(0).cpu()
            loss += float(r[1] / (B * C) + consistency_cost * (r[2] / (B * Tp * C) + r[3] / (B * C)))
        if "domain" in out:
            loss += float(out["domain"])
        return loss
