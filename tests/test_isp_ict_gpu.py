"""The interpolation consistency (mixup) passes of the ISP iteration: ``SEDTrainer.train_step_isp(..., ict=IctPlan)``
(reference src/main.py:366-372,385-392,425-432,451-470,483).

Yardstick: the CPU oracle, ``co.train_losses_isp(...)`` (pinned to the reference's own modules by tests/golden/isp.npz)
plus ``ict_reference.ict_losses(...)`` on the same oracle modules.  The latter is in the reference's ``mixup_criterion``
form, lam * bce(p, y_a) + (1 - lam) * bce(p, y_b), the step computes BCE against the mixed target: agreement also checks
the linearity argument end to end.  No fixture pins the mixup terms to a run of the reference's ``train()`` (main.py cannot
be imported).  Bars: those of tests/test_isp_ada_gpu.py -- loss 3e-5 relative, CRNN / Predictor gradients
3e-4 ||ref|| + 1e-7 per tensor, widened to 2 e32 ||ref|| from the oracle alone where its own float32 run is no sharper.
"""
import numpy as np
import pytest
import torch

import ict_reference as R
from oracle import crnn_oracle as co
from oracle import mel_oracle as mo
from oracle import seeded
from test_isp_ada_gpu import SHIFT_BINS, SHIFT_FRAMES, _inputs, _kw, _oracle_models, _skip, _state, _trainer

pytestmark = pytest.mark.gpu

CC = 0.6


def _plan4():
    from bsed_amd.engine import IctPlan
    return IctPlan(0.3, [1, 0], 0.7, [2, 0, 3, 1], 0.55, [1, 0])


def _tensors(out):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}


def _assert_same_step(a, b):
    (oa, ga), (ob, gb) = a, b
    assert set(oa) == set(ob)
    for k, v in oa.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, ob[k]), k
        else:
            assert v == ob[k], k
    assert float(ga.abs().max()) > 0 and torch.equal(ga, gb)


def test_ict_step_matches_oracle():
    """loss, the four mixup terms and every CRNN / Predictor gradient of the ISP + ICT step against the oracle
    composition, at 4 + 4 clips of 256 frames, dropout 0, exact-fp32 contractions, lr = 0.  The widening rule is the one
    of test_isp_adversarial_step_matches_oracle: bar[k] = max(fixed bar, 2 e32[k] ||ref||) with e32 the float32 oracle's
    own relative L2 error against its float64 run; only the Predictor's dense_softmax.bias may need it."""
    from bsed_amd.engine import SEDTrainer
    seed, B, T = 43, 4, 256
    rng = np.random.default_rng(seed)
    xs = seeded.db_like_input(seed + 1, B, T); xr = seeded.db_like_input(seed + 2, B, T)
    xe = xr + rng.normal(0, 1.0, xr.shape).astype(np.float32)
    y = seeded.strong_targets(seed + 3, B, T // 4)
    yw = (rng.random((B, 20)) < 0.2).astype(np.float32)
    plan = _plan4()

    def oracle_step(dtype):
        models = _oracle_models(seed)
        state = _state(models)
        ocrnn, opred, oema_c, oema_p, _ = models
        for m in models:
            m.to(dtype).train()
        t = lambda a: torch.from_numpy(a).to(dtype)
        loss_isp = co.train_losses_isp(ocrnn, opred, (oema_c, oema_p), t(xs), t(y), t(xr), t(yw), t(xe), SHIFT_FRAMES,
                                       SHIFT_BINS, consistency_cost=CC)
        loss_ict, parts = R.ict_losses(ocrnn, opred, (oema_c, oema_p), t(xs), t(y), t(xr), t(yw), plan, CC)
        (loss_isp + loss_ict).backward()
        grads = {}
        for tag, omod in (("crnn", ocrnn), ("pred", opred)):
            for k, p in omod.named_parameters():
                key = k.replace("cnn.cnn.", "cnn.", 1)
                if not _skip(key):
                    grads[(tag, key)] = p.grad.double()
        return float(loss_isp.detach()), float(loss_ict.detach()), {k: float(v.detach()) for k, v in parts.items()}, grads, state

    l_isp, l_ict, parts, g32, state = oracle_step(torch.float32)
    _, _, _, g64, _ = oracle_step(torch.float64)
    e32 = {k: float((g32[k] - g64[k]).norm() / g64[k].norm()) for k in g64}

    tr, _ = _trainer(state, adversarial=False)
    tt = lambda a: torch.from_numpy(a).cuda()
    out = tr.train_step_isp(tt(xs), tt(y), tt(xr), tt(yw), tt(xe), SHIFT_FRAMES, SHIFT_BINS, consistency_cost=CC, ict=plan)
    loss = SEDTrainer.isp_loss_value(out)
    terms = SEDTrainer.ict_loss_terms(out)
    print(f"ISP + ICT step: loss {loss:.6f}; oracle {l_isp:.6f} + {l_ict:.6f}")
    print("ict terms:", terms, "oracle:", parts)
    assert out["ict"] == (0.3, 0.7, 0.55) and tr.global_step == 1
    assert abs(loss - (l_isp + l_ict)) < 3e-5 * abs(loss), (loss, l_isp + l_ict)
    assert set(terms) == {"mixup_weak_class_loss", "mixup_strong_class_loss", "mixup_cons_weak_loss", "mixup_cons_strong_loss"}
    for k, want in parts.items():
        assert abs(terms[k] - want) < 3e-5 * abs(want), (k, terms[k], want)
    mods = {"crnn": tr.crnn, "pred": tr.predictor}
    widened, bad = [], []
    for (tag, key), ref in g32.items():
        got = mods[tag].P(key).grad.cpu().double()
        err, rn = float((got - ref).norm()), float(ref.norm())
        fixed = 3e-4 * rn + 1e-7
        if err <= fixed:
            continue
        if err <= 2.0 * e32[(tag, key)] * rn:
            widened.append((tag, key, f"err {err / rn:.2e}", f"fixed {fixed / rn:.2e}", f"e32 {e32[(tag, key)]:.2e}"))
        else:
            bad.append((tag, key, err / rn, fixed / rn, e32[(tag, key)]))
    print("tensors that needed the widened bar max(fixed, 2 x e32):", widened)
    assert not bad, bad
    assert {(t_, k) for t_, k, *_ in widened} <= {("pred", "dense_softmax.bias")}, widened


def test_three_classes_and_an_odd_half():
    """6 + 6 clips of 128 frames, half = 3, perms with a fixed point, nclass = 3: label rows of 3 floats take the 4-byte
    path of the mix.  Loss against the oracle (3e-5), finite loss and gradients."""
    from bsed_amd.engine import FlatSGD, IctPlan, SEDTrainer
    from bsed_amd.models import CRNN, Predictor
    seed, B, T, C = 61, 6, 128, 3
    ck, pk = dict(co.CRNN_KWARGS), dict(co.PREDICTOR_KWARGS)
    ck["nclass"] = pk["nclass"] = C
    ck["dropout"] = 0.0
    rng = np.random.default_rng(seed)
    xs = seeded.db_like_input(seed + 1, B, T); xr = seeded.db_like_input(seed + 2, B, T)
    xe = xr + rng.normal(0, 1.0, xr.shape).astype(np.float32)
    y = seeded.strong_targets(seed + 3, B, T // 4, C=C)
    yw = (rng.random((B, C)) < 0.3).astype(np.float32)
    frames, bins = [-8, 12, 0, 40, 4, -20], [3, -2, 0, -4, 1, 2]
    plan = IctPlan(0.3137, [0, 2, 1], 0.8, [0, 5, 1, 2, 3, 4], 0.45, [2, 1, 0])
    omods = []
    for s in (seed, seed + 5):
        oc, op = co.CRNN(**ck), co.Predictor(**pk)
        seeded.load_seeded(oc, s); seeded.load_seeded(op, s + 1)
        omods += [oc.train(), op.train()]
    mine = []
    for om, cls, kw in zip(omods, (CRNN, Predictor, CRNN, Predictor), (ck, pk, ck, pk)):
        m = cls(**kw)
        m.load_state_dict(om.state_dict())
        mine.append(m)
    t = torch.from_numpy
    with torch.no_grad():
        want = float(co.train_losses_isp(omods[0], omods[1], omods[2:], t(xs), t(y), t(xr), t(yw), t(xe), frames, bins,
                                         consistency_cost=CC)
                     + R.ict_losses(omods[0], omods[1], omods[2:], t(xs), t(y), t(xr), t(yw), plan, CC)[0])
    tr = SEDTrainer(*mine, optimizer=FlatSGD(mine[:2], lr=0.0, momentum=0.0, weight_decay=0.0))
    tt = lambda a: torch.from_numpy(a).cuda()
    out = tr.train_step_isp(tt(xs), tt(y), tt(xr), tt(yw), tt(xe), frames, bins, consistency_cost=CC, ict=plan)
    loss = SEDTrainer.isp_loss_value(out)
    print(f"nclass 3, half 3: loss {loss:.6f}; oracle {want:.6f}")
    assert out["isp"] == (CC, 3) and out["ict_weak"].shape[1] == 6
    assert np.isfinite(loss) and bool(torch.isfinite(tr.arena.flat).all()) and float(tr.arena.flat.abs().max()) > 0
    assert abs(loss - want) < 3e-5 * abs(want), (loss, want)


def test_two_fresh_trainers_give_the_same_bits():
    seed, B, T = 47, 4, 256
    state = _state(_oracle_models(seed, 0.5))
    xs, y, xr, yw, xe = _inputs(seed, B, T)
    runs = []
    for _ in range(2):
        tr, _ = _trainer(state, dropout=0.5, adversarial=False, fp32=False)
        out = tr.train_step_isp(xs, y, xr, yw, xe, SHIFT_FRAMES, SHIFT_BINS, consistency_cost=CC, ict=_plan4())
        runs.append((_tensors(out), tr.arena.flat.clone()))
    assert {"ict_weak", "ict_strong", "ict_unl"} <= set(runs[0][0])
    _assert_same_step(*runs)


def test_lam_one_and_identity_perms_feed_the_unmixed_input():
    """with lam = 1 and identity perms the mixed synthetic batch IS the synthetic batch: the loss part of ict_strong equals,
    bit for bit, that of a plain strong-BCE pass of syn_x under the same dropout seed slot (7)"""
    from bsed_amd import parallel
    from bsed_amd.engine import IctPlan
    seed, B, T = 49, 4, 256
    state = _state(_oracle_models(seed, 0.5))
    xs, y, xr, yw, xe = _inputs(seed, B, T)
    plan = IctPlan(1.0, [0, 1], 1.0, [0, 1, 2, 3], 1.0, [0, 1])
    tr, _ = _trainer(state, dropout=0.5, adversarial=False, fp32=False, seed=91)
    out = tr.train_step_isp(xs, y, xr, yw, xe, SHIFT_FRAMES, SHIFT_BINS, consistency_cost=CC, ict=plan)
    plain, _ = _trainer(state, dropout=0.5, adversarial=False, fp32=False, seed=91)
    plain.crnn.train(); plain.predictor.train()
    plain.crnn.set_seed(parallel.rank_seed(91, 0, 0) * 16 + 7)
    enc, _ = plain.crnn.run_forward(xs, save=True)
    _, lp = plain.predictor.run_backward(enc, plain.predictor.run_forward(enc), y_strong=y)
    assert float(lp[:, 0].sum()) > 0 and torch.equal(lp, out["ict_strong"])
    # and under another slot the masks, so the bits, differ: the comparison above can tell
    plain.crnn.set_seed(parallel.rank_seed(91, 0, 0) * 16 + 6)
    enc, _ = plain.crnn.run_forward(xs, save=True)
    _, lp6 = plain.predictor.run_backward(enc, plain.predictor.run_forward(enc), y_strong=y)
    assert not torch.equal(lp6, out["ict_strong"])


@pytest.mark.parametrize("dropout", [0.0, 0.5])
def test_waveform_path_equals_tensor_path_bitwise_with_ict(dropout):
    """the construction of test_waveform_path_equals_tensor_path_bitwise, with a plan: from waveforms the mixes read the
    dB-mel tensors the mel stage wrote"""
    from bsed_amd import parallel
    from bsed_amd.features import MelConfig, MelFrontEnd
    seed, B = 51, 4
    fe = MelFrontEnd(MelConfig(sr=22050))
    wav_s = torch.from_numpy(np.stack([mo.synth_clip(i, sr=22050, seconds=3.0)[0] for i in range(B)])).cuda()
    wav_r = torch.from_numpy(np.stack([mo.synth_clip(10 + i, sr=22050, seconds=3.0)[0] for i in range(B)])).cuda()
    T = fe.num_frames(wav_s.shape[1])
    rng = np.random.default_rng(seed)
    y = torch.from_numpy(seeded.strong_targets(seed, B, T // 4)).cuda()
    yw = torch.from_numpy((rng.random((B, 20)) < 0.2).astype(np.float32)).cuda()
    state = _state(_oracle_models(seed, dropout))
    res = []
    for from_wave in (True, False):
        tr, _ = _trainer(state, dropout=dropout, frontend=fe, it=3, fp32=False, seed=77)
        if from_wave:
            out = tr.train_step_isp(wav_s, y, wav_r, yw, shift_frames=SHIFT_FRAMES, shift_bins=SHIFT_BINS, from_wave=True,
                                    ict=_plan4())
        else:
            xs = fe.transform(wav_s, max_frames=T)
            xr, xe = fe.transform(wav_r, max_frames=T, noisy=True, seed=parallel.rank_seed(77, 0, 0))
            out = tr.train_step_isp(xs, y, xr, yw, xe, SHIFT_FRAMES, SHIFT_BINS, ict=_plan4())
        res.append((out, tr.arena.flat.clone()))
    assert "domain" in res[0][0] and "ict_unl" in res[0][0]
    _assert_same_step(*res)


def test_guard_rails_leave_the_step_counter_alone():
    from bsed_amd import _lib as L
    from bsed_amd.engine import IctPlan
    seed, T = 59, 128
    state = _state(_oracle_models(seed))
    tr, _ = _trainer(state, adversarial=False, fp32=False)
    one = IctPlan(0.5, [0], 0.5, [0], 0.5, [0])
    xs, y, xr, yw, xe = _inputs(seed, 1, T)
    with pytest.raises(L.BsedError, match="both need a clip"):       # one real clip: no weakly labelled half
        tr.train_step_isp(xs, y, xr, yw, xe, [0], [0], ict=one)
    xs, y, xr, yw, xe = _inputs(seed, 2, T)
    with pytest.raises(L.BsedError, match="both need a clip"):       # weak targets for 4 clips: no unlabelled half of 2
        tr.train_step_isp(xs, y, xr, torch.cat([yw, yw]), xe, [0, 0], [0, 0], ict=IctPlan(0.5, [0, 1], 0.5, [0, 1], 0.5, [0]))
    for bad in (IctPlan(0.5, [1, 0], 0.5, [0, 1], 0.5, [0]), IctPlan(0.5, [0], 0.5, [0, 2, 1], 0.5, [0]),
                IctPlan(0.5, [0], 0.5, [0, 1], 0.5, [1, 0])):
        with pytest.raises(L.BsedError, match="IctPlan"):            # a perm that does not fit its batch
            tr.train_step_isp(xs, y, xr, yw, xe, [0, 0], [0, 0], ict=bad)
    assert tr.global_step == 0
    # without a plan the step runs and has none of the new keys
    out = tr.train_step_isp(xs, y, xr, yw, xe, [0, 0], [0, 0])
    assert tr.global_step == 1 and not [k for k in out if k.startswith("ict")]


def test_realistic_size_from_waveforms_with_ict():
    """12 + 12 clips of 10 s at 22.05 kHz from waveforms, dropout 0.5, the adversarial loss on, plans from draw_ict"""
    from bsed_amd.disc import Clip_Discriminator, ConditionalDomainAdversarialLoss
    from bsed_amd.engine import FlatSGD, SEDTrainer, draw_ict
    from bsed_amd.features import MelConfig, MelFrontEnd
    from bsed_amd.models import CRNN, Predictor, weights_init
    B, sr = 12, 22050
    torch.manual_seed(5)
    fe = MelFrontEnd(MelConfig(sr=sr))
    g = torch.Generator(device="cuda").manual_seed(9)
    wav_s = (torch.rand(B, 10 * sr, device="cuda", generator=g) - 0.5) * 0.2
    wav_r = (torch.rand(B, 10 * sr, device="cuda", generator=g) - 0.5) * 0.2
    T = fe.num_frames(10 * sr)
    y = torch.from_numpy(seeded.strong_targets(3, B, T // 4)).cuda()
    yw = y.max(1)[0].contiguous()
    crnn, pred = CRNN(**_kw(0.5)), Predictor(**co.PREDICTOR_KWARGS)
    ema_c, ema_p = CRNN(**_kw(0.5)), Predictor(**co.PREDICTOR_KWARGS)
    weights_init(crnn); weights_init(pred)
    ema_c.load_state_dict(crnn.state_dict()); ema_p.load_state_dict(pred.state_dict())
    disc = Clip_Discriminator()
    tr = SEDTrainer(crnn, pred, ema_c, ema_p, frontend=fe,
                    optimizer=FlatSGD([crnn, pred], lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True),
                    domain_loss=ConditionalDomainAdversarialLoss(disc),
                    optimizer_d=FlatSGD([disc], lr=1e-4, momentum=0.9, weight_decay=1e-4, nesterov=True))
    rng = np.random.default_rng(1)
    for step in range(2):
        frames = [int(v) * 4 for v in rng.integers(-64, 65, B)]
        bins = [int(v) for v in rng.integers(-4, 5, B)]
        plan = draw_ict(rng, B // 2, B, B - B // 2)
        out = tr.train_step_isp(wav_s, y, wav_r, yw, shift_frames=frames, shift_bins=bins, from_wave=True, ict=plan)
        loss = SEDTrainer.isp_loss_value(out)
        assert np.isfinite(loss) and loss >= 0, loss
        assert min(SEDTrainer.ict_loss_terms(out).values()) >= 0 and out["ict"] == plan.lams
        assert bool(torch.isfinite(tr.arena.flat).all())
    assert tr.global_step == 2 and tr.domain_loss.iter_num == 2
