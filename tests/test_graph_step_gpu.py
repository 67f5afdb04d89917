"""HIP-graph replay of the plain train step (engine.SEDTrainer.capture_step / replay_step): the reference's batch of 24
(its src/data/config.py:70: batch_size = 12 -> 24 clips per step, src/main_baseline.py:737-740) is host-bound
in eager mode.  A replayed step must equal the eager step BIT FOR BIT: the per-step scalars a capture bakes (dropout seed,
Adam step count, learning rate) are also read from device memory, which the library is pointed at (bsed_set_step_state)
only while the step is being captured; the first two are advanced by a node of the graph, the third is refreshed by
replay_step.  A graph carries the pointers it was captured with: nothing outside a capture reads them.

The reference of every test here is the EAGER path of the same build: a fresh trainer with the same seeds and inputs that
takes the same sequence of steps through ``train_step`` only and never captures a graph (the eager path itself is pinned
against the oracle in tests/test_crnn_gpu.py, test_block0_gpu.py, ...).  The bar is equality: ``torch.equal`` on the
parameters, the BatchNorm running statistics and Adam's moments, ``==`` on the host loss values and the step counters,
after EVERY compared step.  No tolerance anywhere.  Dropout is 0.5 throughout so that every mask matters.

What the cases cover (each one states the failure it would catch):
  a. every kernel route that carries a dropout seed (exact-fp32 mode, both A/B switches, the waveform front end);
  b. the masks really advance from replay to replay (guards a. against a seed frozen on BOTH sides);
  c. eager steps of the same trainer between replays (the smaller last batch of an epoch), release, re-capture;
     release_graph frees the static inputs and the step state with the graph;
  d. a learning-rate schedule (engine.adjust_learning_rate before every step);
  e. what a held graph must not touch (the step state is bound for the capture only): a second trainer's eager steps,
     its own capture and replays interleaved with the first's, direct calls of ops.dropout / ops.adam_step, and
     whatever runs after a trainer was dropped without release_graph;
  f. replay_step / capture_step refuse what they cannot do, before touching anything."""
import contextlib
import gc

import pytest
import torch

from oracle import crnn_oracle as co
from oracle import seeded
from test_crnn_gpu import _mine, _oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,T,mode", [(4, 128, "bf16x3"), (24, 865, "bf16x3"), (6, 128, "bf16")])
def test_replayed_steps_equal_eager_steps_bitwise(B, T, mode):
    from bsed_amd.engine import FlatAdam, SEDTrainer
    xs = [torch.from_numpy(seeded.db_like_input(70 + k, B, T)).cuda() for k in range(4)]
    ys = [torch.from_numpy(seeded.strong_targets(80 + k, B, T // 4)).cuda() for k in range(4)]
    ocrnn, opred = _oracle(0.5, 9)
    res = {}
    for how in ("eager", "graph"):
        crnn, pred = _mine(0.5, ocrnn, opred, mode)
        tr = SEDTrainer(crnn, pred, optimizer=FlatAdam([crnn, pred], lr=1e-3), seed=11)
        losses = []
        if how == "eager":
            for _ in range(3):
                tr.train_step(xs[0], ys[0])
            for k in (1, 2, 3):
                losses.append(SEDTrainer.loss_value(tr.train_step(xs[k], ys[k])))
        else:
            tr.capture_step(xs[0], ys[0], warmup=3)
            try:
                for k in (1, 2, 3):
                    losses.append(SEDTrainer.loss_value(tr.replay_step(xs[k], ys[k])))
            finally:
                tr.release_graph()
        torch.cuda.synchronize()
        res[how] = (losses, crnn.flat.clone(), pred.flat.clone(), crnn.flat_buf.clone(), tr.global_step,
                    tr.optimizer.step_count)
    assert res["eager"][0] == res["graph"][0], (res["eager"][0], res["graph"][0])
    for i in (1, 2, 3):
        assert torch.equal(res["eager"][i], res["graph"][i]), i
    assert res["eager"][4:] == res["graph"][4:] == (6, 6)


# ------------------------------------------------------------------------------------------------------------------
# helpers of the cases a-f
# ------------------------------------------------------------------------------------------------------------------
B0, T0 = 4, 128


def _batches(n, B=B0, T=T0, base=70):
    xs = [torch.from_numpy(seeded.db_like_input(base + k, B, T)).cuda() for k in range(n)]
    ys = [torch.from_numpy(seeded.strong_targets(base + 10 + k, B, T // 4)).cuda() for k in range(n)]
    return list(zip(xs, ys))


def _trainer(mode="bf16x3", switches=(), lr=1e-3, frontend=None, weights=9, seed=11):
    """a fresh trainer: seeded weights, dropout 0.5, the A/B switches set on the model before its first step"""
    from bsed_amd.engine import FlatAdam, SEDTrainer
    ocrnn, opred = _oracle(0.5, weights)
    crnn, pred = _mine(0.5, ocrnn, opred, mode)
    for name, value in switches:
        assert hasattr(crnn, name), name
        setattr(crnn, name, value)
    return SEDTrainer(crnn, pred, optimizer=FlatAdam([crnn, pred], lr=lr), frontend=frontend, seed=seed)


def _snap(tr, loss=None):
    """everything a step leaves behind, copied"""
    torch.cuda.synchronize()
    return {"loss": loss, "crnn.flat": tr.crnn.flat.clone(), "pred.flat": tr.predictor.flat.clone(),
            "crnn.flat_buf": tr.crnn.flat_buf.clone(), "crnn.nbt": tr.crnn.nbt.clone(),
            "adam.m": [t.clone() for t in tr.optimizer.m], "adam.v": [t.clone() for t in tr.optimizer.v],
            "global_step": tr.global_step, "step_count": tr.optimizer.step_count}


def _assert_same(got, want, where):
    assert got.keys() == want.keys()
    for k, w in want.items():
        g = got[k]
        if isinstance(w, torch.Tensor):
            assert torch.equal(g, w), f"{where}: {k} differs in {int((g != w).sum())} of {w.numel()} entries"
        elif isinstance(w, list):
            for i, (gi, wi) in enumerate(zip(g, w)):
                assert torch.equal(gi, wi), f"{where}: {k}[{i}] differs in {int((gi != wi).sum())} of {wi.numel()} entries"
        else:
            assert g == w, f"{where}: {k} is {g!r}, the eager trainer has {w!r}"


def _run(tr, script, graph, from_wave=False):
    """Take ``tr`` through ``script`` and return one snapshot per step.  Entries:
         ("capture", x, y, warmup)  graph side: capture_step; eager side: ``warmup`` train_steps on (x, y)
         ("replay", x, y)           graph side: replay_step;  eager side: train_step
         ("eager", x, y)            train_step on both sides
         ("release",)               graph side: release_graph
         ("lr", ramp)               engine.adjust_learning_rate(optimizer, rampup_value=ramp) on both sides"""
    try:
        snaps = [_apply(tr, entry, graph, from_wave) for entry in script]
    finally:
        tr.release_graph()
    return [s for s in snaps if s is not None]


def _apply(tr, entry, graph, from_wave=False):
    """one entry of a ``_run`` script; the snapshot after it if it is a step, else None"""
    from bsed_amd.engine import SEDTrainer, adjust_learning_rate
    kw = {"from_wave": True} if from_wave else {}
    op, *a = entry
    if op == "capture":
        if graph:
            tr.capture_step(a[0], a[1], warmup=a[2], **kw)
        else:
            for _ in range(a[2]):
                tr.train_step(a[0], a[1], **kw)
    elif op == "replay":
        out = tr.replay_step(a[0], a[1]) if graph else tr.train_step(a[0], a[1], **kw)
        return _snap(tr, SEDTrainer.loss_value(out))
    elif op == "eager":
        return _snap(tr, SEDTrainer.loss_value(tr.train_step(a[0], a[1], **kw)))
    elif op == "release":
        if graph:
            tr.release_graph()
    elif op == "lr":
        adjust_learning_rate(tr.optimizer, rampup_value=a[0])
    else:
        raise AssertionError(op)
    return None


def _compare(make_trainer, script, from_wave=False, what=""):
    """the same script on two fresh trainers, one replaying and one all-eager: equal after every step"""
    eager = _run(make_trainer(), script, graph=False, from_wave=from_wave)
    graph = _run(make_trainer(), script, graph=True, from_wave=from_wave)
    assert len(eager) == len(graph) and len(eager) >= 3
    for i, (g, e) in enumerate(zip(graph, eager)):
        _assert_same(g, e, f"{what} step {i + 1} of {len(eager)}")
    return eager, graph


@contextlib.contextmanager
def _recorded_launches():
    """names of the library entry points called inside the block; bsed_igemm with its epilogue ("bsed_igemm:2")"""
    from bsed_amd import _lib
    names, real = set(), _lib.call

    def call(name, *args):
        names.add(f"{name}:{args[0]._obj.epilogue}" if name == "bsed_igemm" else name)
        return real(name, *args)
    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = real


def _standard_script(data, warmup=3):
    return [("capture", *data[0], warmup)] + [("replay", *d) for d in data[1:]]


# ------------------------------------------------------------------------------------------------------------------
# a. every kernel route that carries a dropout seed
# ------------------------------------------------------------------------------------------------------------------
ROUTES = {
    # id: (conv_mode, switches, entry points the step must go through, entry points it must NOT go through)
    "fp32": ("fp32", (), {"bsed_igemm:2", "bsed_glu_bwd_fused", "bsed_block0_fwd", "bsed_dropout"},
             {"bsed_glu_fwd3", "bsed_glu_bwd3", "bsed_glu_bwd3n", "bsed_igemm:3"}),
    "fp32-unfused-glu-bwd": ("fp32", (("fused_glu_bwd", False),), {"bsed_igemm:2", "bsed_igemm:3"},
                             {"bsed_glu_fwd3", "bsed_glu_bwd3", "bsed_glu_bwd3n", "bsed_glu_bwd_fused"}),
    "bf16x3-block0-unfused": ("bf16x3", (("block0_fused", False),), {"bsed_glu16_fwd", "bsed_glu16_bwd", "bsed_glu_fwd3"},
                              {"bsed_block0_fwd", "bsed_block0_bwd"}),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_replayed_steps_equal_eager_steps_on_every_dropout_route(route):
    """The GLU epilogues of csrc/igemm.hip (GLU_POOL forward, GLU_BWD backward), csrc/glu_bwd.hip and both kernels of
    csrc/glu_small.hip take a dropout seed like block0.hip / glu3.hip do.  One that used the seed baked at capture would
    replay the capture step's masks in its blocks for ever while the other blocks advance: losses and parameters leave
    the eager trainer's at the first replay.  The test also pins that the switches really route the step through the
    kernels it is named for (otherwise it would pass by testing the default route three times)."""
    from bsed_amd import ops
    assert (ops.EPI_GLU_POOL, ops.EPI_GLU_BWD) == (2, 3)
    mode, switches, must, must_not = ROUTES[route]
    data = _batches(4)
    with _recorded_launches() as names:
        tr = _trainer(mode, switches)
        tr.train_step(*data[0])
        torch.cuda.synchronize()
    assert must <= names and not (must_not & names), (sorted(must - names), sorted(must_not & names))
    _compare(lambda: _trainer(mode, switches), _standard_script(data), what=route)


def test_replayed_steps_equal_eager_steps_from_waveforms():
    """The form ``bench.py --graph`` replays: the mel front end runs inside the captured step (from_wave=True).  Protects
    the waveform path of the graph -- static WAVEFORM tensors, the front end's launches on the capture stream, its
    lazily built tables made in the warm-up -- which the dB-mel cases never enter."""
    from bsed_amd.features import MelConfig, MelFrontEnd
    fe = MelFrontEnd(MelConfig())
    n = 127 * fe.cfg.hop_size
    assert fe.num_frames(n) == T0
    g = torch.Generator(device="cuda").manual_seed(5)
    data = [(torch.randn(B0, n, device="cuda", generator=g) * 0.1,
             torch.from_numpy(seeded.strong_targets(90 + k, B0, T0 // 4)).cuda()) for k in range(4)]
    _compare(lambda: _trainer(frontend=fe), _standard_script(data), from_wave=True, what="from_wave")


# ------------------------------------------------------------------------------------------------------------------
# b. the masks really advance
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_replays_of_one_batch_draw_new_masks(mode):
    """lr = 0: the parameters never move, so the SAME batch replayed three times gives three different losses only
    because every replay draws new dropout masks.  A change that froze the seed in the eager path and in the graph
    alike would keep case a green; here the three losses would coincide.  They also equal the eager trainer's at the
    same global steps."""
    data = _batches(2)
    script = [("capture", *data[0], 3)] + [("replay", *data[1])] * 3
    start = _trainer(mode, lr=0.0)
    eager, graph = _compare(lambda: _trainer(mode, lr=0.0), script, what=f"lr=0 {mode}")
    for snaps in (eager, graph):
        assert torch.equal(snaps[-1]["crnn.flat"], start.crnn.flat) and torch.equal(snaps[-1]["pred.flat"], start.predictor.flat)
        losses = [s["loss"] for s in snaps]
        assert len(set(losses)) == 3, losses
    assert [s["global_step"] for s in graph] == [4, 5, 6]


# ------------------------------------------------------------------------------------------------------------------
# c. eager steps mixed into replays
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
def test_eager_steps_between_replays_release_and_recapture(mode):
    """capture, replay x2, train_step on a SMALLER batch (the last batch of an epoch), replay x2, release, train_step x2,
    capture again, replay x2: equal to the all-eager trainer after every step.  An eager step that ran with the graph's
    device addends on top of the host's counters would be K steps ahead in its Adam bias correction and its masks, and
    one that did not advance the device state would leave every later replay one step behind."""
    d = _batches(9)
    small = _batches(1, B=2, base=40)[0]
    script = [("capture", *d[0], 3), ("replay", *d[1]), ("replay", *d[2]), ("eager", *small), ("replay", *d[3]),
              ("replay", *d[4]), ("release",), ("eager", *d[5]), ("eager", *d[6]),
              ("capture", *d[0], 0), ("replay", *d[7]), ("replay", *d[8])]
    eager, graph = _compare(lambda: _trainer(mode), script, what=f"mixed {mode}")
    assert [s["global_step"] for s in graph] == [4, 5, 6, 7, 8, 9, 10, 11, 12]
    assert [s["step_count"] for s in graph] == [4, 5, 6, 7, 8, 9, 10, 11, 12]


def test_release_graph_frees_what_the_captured_step_owned():
    """The static inputs and the device-resident step state belong to the captured step: release_graph drops them with
    the graph (not the next capture, not the death of the trainer).  Weak references to the three tensors are dead after
    the release and a collection.  The eager step after it equals the third step of the all-eager trainer: the freed
    state took nothing the trainer steps on with it."""
    import weakref
    d = _batches(4)
    script = _standard_script(d[:3]) + [("release",), ("eager", *d[3])]
    eager = _run(_trainer(), script, graph=False)
    tr = _trainer()
    try:
        for entry in script[:3]:                        # capture, replay, replay
            _apply(tr, entry, graph=True)
        refs = [weakref.ref(t) for t in (tr._graph.x, tr._graph.y, tr._graph.state)]
        assert all(r() is not None for r in refs)
        tr.release_graph()
        gc.collect()
        assert all(r() is None for r in refs) and tr._graph is None
        _assert_same(_apply(tr, script[4], graph=True), eager[2], "the eager step after the release")
    finally:
        tr.release_graph()


# ------------------------------------------------------------------------------------------------------------------
# d. learning-rate schedule
# ------------------------------------------------------------------------------------------------------------------
def test_replayed_steps_follow_the_learning_rate_schedule():
    """The reference sets the rate before every iteration (adjust_learning_rate, src/main_baseline.py:53-88).  A replay
    that kept the rate baked at capture would train at 1e-3 for ever.  Ramp values: rising, back to a value used before
    (0.6), to the capture-time rate itself (2.0 * 0.0005 = 1e-3) and away from it again; one eager step of the armed
    trainer in between takes the rate of ITS step."""
    d = _batches(8)
    small = _batches(1, B=2, base=40)[0]
    script = [("capture", *d[0], 3)]
    for k, ramp in enumerate((0.2, 0.6, 1.0, 0.6, 2.0, 0.35)):
        script += [("lr", ramp), ("replay", *d[1 + k])]
        if k == 2:
            script += [("lr", 0.8), ("eager", *small)]
    eager, graph = _compare(lambda: _trainer(), script, what="lr schedule")
    # the schedule matters at all: the same steps at the constant capture-time rate end elsewhere
    const = _run(_trainer(), [e for e in script if e[0] != "lr"], graph=False)
    assert not torch.equal(const[-1]["crnn.flat"], eager[-1]["crnn.flat"])


# ------------------------------------------------------------------------------------------------------------------
# e. what a held graph must not touch
# ------------------------------------------------------------------------------------------------------------------
def test_second_trainer_steps_eagerly_beside_an_armed_one():
    """Two trainers, each with a graph of its own.  The library is pointed at a trainer's device-resident step state only
    while that trainer captures, so B's eager steps beside A's graph equal the same steps with no graph anywhere in the
    process, B captures while A holds a graph, and their replays and eager steps (A's on the smaller last batch of an
    epoch, B's at its captured shape) alternate: after EVERY step the stepping trainer equals the same trainer run alone,
    all eager, through the same sequence.  A capture that left the library pointed at B's state would give A's eager step
    B's addends; graphs that shared one state would advance each other's seeds and step counts."""
    da, db = _batches(5), _batches(7, base=30)
    small = _batches(1, B=2, base=40)[0]
    a_script = [("capture", *da[0], 3), ("replay", *da[1]), ("eager", *small), ("replay", *da[2]), ("replay", *da[3])]
    b_script = [("eager", *db[0]), ("eager", *db[1]), ("capture", *db[2], 2), ("replay", *db[3]), ("replay", *db[4]),
                ("eager", *db[5]), ("replay", *db[6])]
    # both references before any graph exists: B's first two steps are its steps with no graph anywhere in the process
    want = {"A": _run(_trainer(), a_script, graph=False), "B": _run(_trainer(weights=21, seed=5), b_script, graph=False)}
    A, B = _trainer(), _trainer(weights=21, seed=5)
    todo = {"A": (A, iter(a_script)), "B": (B, iter(b_script))}
    done = {"A": 0, "B": 0}

    def step(who):
        tr, entries = todo[who]
        snap = _apply(tr, next(entries), graph=True)
        if snap is not None:
            _assert_same(snap, want[who][done[who]], f"trainer {who} step {done[who] + 1} beside the other trainer")
            done[who] += 1
    try:
        step("A")                                       # A captures
        step("B")                                       # B steps eagerly beside A's graph, twice
        step("B")
        assert A._graph is not None and B._graph is None
        step("B")                                       # B captures while A holds a graph
        assert A._graph is not None and B._graph is not None
        for _ in range(4):                              # A replay, B replay, A eager (B = 2), B replay,
            step("A")                                   # A replay, B eager, A replay, B replay
            step("B")
        assert done == {"A": len(want["A"]), "B": len(want["B"])} == {"A": 4, "B": 6}
    finally:
        A.release_graph()
        B.release_graph()


def test_direct_op_calls_do_not_see_a_held_graphs_step_state():
    """ops.dropout and ops.adam_step called directly while a trainer holds a graph whose device addends are both non-zero
    (two replays) give the bits of the same calls made before the trainer existed: the mask of (rng_stream, seed) alone,
    the bias correction of ``step`` alone.  With the library still pointed at the graph's state they would run with
    seed + 2 steps' worth of addend and step + 2.  The replay after them equals the all-eager trainer's step: the direct
    calls did not disturb the graph either.  3 x 1000 elements: not a multiple of the wave size."""
    from bsed_amd import ops
    from bsed_amd.engine import SEDTrainer
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 1000, generator=g).cuda()
    adam_in = [torch.randn(1000, generator=g).cuda() for _ in range(3)] + [torch.rand(1000, generator=g).cuda()]

    def direct():
        p, grad, m, v = [t.clone() for t in adam_in]
        ops.adam_step(p, grad, m, v, 1e-3, 3)
        out = {"dropout": ops.dropout(x, 0.5, 200, 1234567), "p": p, "m": m, "v": v}
        torch.cuda.synchronize()
        return out
    before = direct()
    assert 0.3 < float((before["dropout"] == 0).float().mean()) < 0.7 and not torch.equal(before["p"], adam_in[0])
    d = _batches(4)
    eager = _run(_trainer(), _standard_script(d), graph=False)
    tr = _trainer()
    try:
        tr.capture_step(*d[0], warmup=3)
        for k in (1, 2):
            _assert_same(_snap(tr, SEDTrainer.loss_value(tr.replay_step(*d[k]))), eager[k - 1], f"replay {k}")
        step = tr._graph
        assert bool((step.state[[step.SEED, step.STEP]] != 0).all())       # seed addend, step addend
        during = direct()
        for k, w in before.items():
            assert torch.equal(during[k], w), f"{k} of a direct call differs in {int((during[k] != w).sum())} of " \
                                              f"{w.numel()} entries while a graph is held"
        _assert_same(_snap(tr, SEDTrainer.loss_value(tr.replay_step(*d[3]))), eager[2], "the replay after the direct calls")
    finally:
        tr.release_graph()


def test_a_trainer_dropped_without_release_leaves_nothing_behind():
    """A trainer that captured and replayed is garbage-collected WITHOUT release_graph: its step state is freed device
    memory.  The library must not be pointing at it: two eager steps of a fresh trainer afterwards equal the same steps
    taken before any graph existed in the process."""
    d, db = _batches(2), _batches(2, base=30)
    b_script = [("eager", *db[0]), ("eager", *db[1])]
    b_alone = _run(_trainer(weights=21, seed=5), b_script, graph=False)       # no graph exists yet
    A = _trainer()
    A.capture_step(*d[0], warmup=3)
    A.replay_step(*d[1])
    del A
    gc.collect()
    torch.cuda.synchronize()
    b_after = _run(_trainer(weights=21, seed=5), b_script, graph=False)
    assert len(b_after) == len(b_alone) == 2
    for i, (g, w) in enumerate(zip(b_after, b_alone)):
        _assert_same(g, w, f"trainer B step {i + 1} after trainer A was dropped unreleased")


# ------------------------------------------------------------------------------------------------------------------
# f. input checking
# ------------------------------------------------------------------------------------------------------------------
def test_replay_step_refuses_inputs_that_differ_from_the_captured_ones():
    """``static.copy_(batch)`` broadcasts: a batch of ONE clip would silently fill the captured batch of four, a float64
    batch would be converted.  Every such call must raise BsedError before anything is copied or launched: the trainer's
    state is unchanged and the next good replay equals the eager step."""
    from bsed_amd._lib import BsedError
    from bsed_amd.engine import SEDTrainer
    d = _batches(3)
    eager = _run(_trainer(), _standard_script(d), graph=False)
    tr = _trainer()
    try:
        tr.capture_step(*d[0], warmup=3)
        first = _snap(tr, SEDTrainer.loss_value(tr.replay_step(*d[1])))
        _assert_same(first, eager[0], "first replay")
        x, y = d[2]
        bad = {"batch of one (would broadcast)": (x[:1].contiguous(), y[:1].contiguous()),
               "x of one clip only": (x[:1].contiguous(), y),
               "y of one clip only": (x, y[:1].contiguous()),
               "fewer frames": (x[:, :, :T0 // 2].contiguous(), y[:, :T0 // 8].contiguous()),
               "x float64": (x.double(), y), "y float64": (x, y.double()), "x bfloat16": (x.bfloat16(), y),
               "x not a tensor": (None, y)}
        for what, (bx, by) in bad.items():
            before = _snap(tr)
            with pytest.raises(BsedError):
                tr.replay_step(bx, by)
                pytest.fail(f"replay_step accepted: {what}")
            _assert_same(_snap(tr), before, f"after the refused replay ({what})")
        second = _snap(tr, SEDTrainer.loss_value(tr.replay_step(x, y)))
        _assert_same(second, eager[1], "the replay after the refused ones")
    finally:
        tr.release_graph()


def test_replay_step_needs_a_captured_graph():
    """before capture_step and after release_graph there is nothing to replay: BsedError (not an AttributeError, and not
    a replay of a dropped graph), state unchanged, and the trainer still steps eagerly"""
    from bsed_amd._lib import BsedError
    d = _batches(2)
    tr = _trainer()
    with pytest.raises(BsedError):
        tr.replay_step(*d[0])
    assert tr.global_step == 0 and tr.optimizer.step_count == 0
    tr.capture_step(*d[0], warmup=2)
    try:
        tr.replay_step(*d[1])
    finally:
        tr.release_graph()
    before = _snap(tr)
    with pytest.raises(BsedError):
        tr.replay_step(*d[1])
    _assert_same(_snap(tr), before, "after the refused replay")
    tr.release_graph()                      # releasing twice is harmless
    tr.train_step(*d[1])
    assert tr.global_step == 4 and tr.optimizer.step_count == 4


@pytest.mark.parametrize("what", ["ema", "discriminator", "multi-rank", "sgd"])
def test_capture_step_refuses_steps_it_cannot_replay(what):
    """EMA teacher, discriminator, data-parallel group: per-step host decisions that are not graph nodes.  An optimizer
    other than FlatAdam: its per-step scalars (FlatSGD's first-step flag, its rate) are not device-resident.  BsedError
    before any step runs; the trainer then still steps eagerly."""
    from bsed_amd._lib import BsedError
    from bsed_amd.engine import FlatAdam, FlatSGD, SEDTrainer
    d = _batches(1)
    ocrnn, opred = _oracle(0.5, 9)
    crnn, pred = _mine(0.5, ocrnn, opred)
    kw = {"optimizer": FlatAdam([crnn, pred], lr=1e-3)}
    if what == "ema":
        ema_c, ema_p = _mine(0.5, ocrnn, opred)
        kw.update(ema_crnn=ema_c, ema_predictor=ema_p)
    elif what == "discriminator":
        from bsed_amd.disc import Clip_Discriminator, ConditionalDomainAdversarialLoss
        kw.update(domain_loss=ConditionalDomainAdversarialLoss(Clip_Discriminator()))
    elif what == "sgd":
        kw["optimizer"] = FlatSGD([crnn, pred], lr=1e-3)
    tr = SEDTrainer(crnn, pred, seed=11, **kw)
    if what == "multi-rank":
        tr.world = 2        # what a trainer built inside a two-rank process group carries
    with pytest.raises(BsedError):
        tr.capture_step(*d[0], warmup=1)
    assert tr.global_step == 0 and tr.optimizer.step_count == 0
    with pytest.raises(BsedError):
        tr.replay_step(*d[0])
    if what == "multi-rank":
        tr.world = 1
    tr.train_step(*d[0])
    torch.cuda.synchronize()
    assert tr.global_step == 1
