"""Host restatement of interpolation consistency training (mixup) as the reference's ISP iteration runs it
(src/main.py:127-156, 366-372, 385-392, 425-432, 451-470, 483), in this project's own text.

  mix(x, perm, lam)   the row mix of ``bsed_mix_rows`` in numpy float32, with its rounding rule (include/bsed.h)
  ict_losses(...)     the four mixup terms on ``oracle.crnn_oracle`` modules, in the reference's ``mixup_criterion``
                      form  lam * bce(p, y_a) + (1 - lam) * bce(p, y_b)  -- NOT bce against the mixed target, which is
                      what the GPU step computes: a test that compares the two also checks that BCE is linear in its target.

No fixture pins this file to a run of the reference's ``train()``: main.py needs its datasets and its command line and
cannot be imported.  What is held against the reference is the arithmetic of its mixing expression (test_ict_reference_cpu.py).
"""
import numpy as np
import torch
from torch import nn


def mix(x, perm, lam):
    """out[r] = fl32(fl32(lam32 * x[r]) + fl32(oml32 * x[perm[r]])) over the rows (axis 0) of a float32 array;
    lam32 = float32(lam), oml32 = float32(1.0 - lam) with the subtraction in double.  Each product is rounded to float32
    on its own and then the sum: numpy's float32 array arithmetic does exactly that."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    perm = np.asarray(perm, dtype=np.int64)
    assert perm.shape == (x.shape[0],)
    lam32, oml32 = np.float32(lam), np.float32(1.0 - float(lam))
    a = np.multiply(x, lam32, dtype=np.float32)
    b = np.multiply(x[perm], oml32, dtype=np.float32)
    return np.add(a, b, dtype=np.float32)


def ict_losses(crnn, pred, ema, x_syn, y_syn, x_real, y_weak_real, plan, cc):
    """The mixup terms of one ISP iteration on the batches of ``co.train_losses_isp``: the synthetic batch is the
    strongly labelled one, ``x_real[:half]`` the weakly labelled half and ``x_real[half:]`` the unlabelled half
    (half = len(y_weak_real) // 2).  plan: anything with lam_weak / perm_weak / lam_strong / perm_strong / lam_unl /
    perm_unl.  Returns (sum of the terms as they enter the loss, main.py:483; dict of the four parts as the reference logs
    them: the consistency parts before the multiplication by cc, main.py:464-470)."""
    bce, mse = nn.BCELoss(), nn.MSELoss()
    half = y_weak_real.shape[0] // 2
    idx = lambda p: torch.as_tensor(list(p), dtype=torch.long)
    # weakly labelled half: mixup_data_sup + mixup_criterion on the weak prediction (main.py:387-391)
    lam, p = plan.lam_weak, idx(plan.perm_weak)
    x, y = x_real[:half], y_weak_real[:half]
    _, weak = pred(crnn(lam * x + (1 - lam) * x[p])[0])
    weak_class = lam * bce(weak, y) + (1 - lam) * bce(weak, y[p])
    # strongly labelled batch: the same on the strong prediction (main.py:427-431)
    lam, p = plan.lam_strong, idx(plan.perm_strong)
    strong, _ = pred(crnn(lam * x_syn + (1 - lam) * x_syn[p])[0])
    strong_class = lam * bce(strong, y_syn) + (1 - lam) * bce(strong, y_syn[p])
    # unlabelled half: the teacher on the unmixed clips, its two outputs mixed like the input (main.py:453-465)
    lam, p = plan.lam_unl, idx(plan.perm_unl)
    x = x_real[half:]
    with torch.no_grad():
        t_strong, t_weak = ema[1](ema[0](x)[0])
    strong, weak = pred(crnn(lam * x + (1 - lam) * x[p])[0])
    cons_weak = mse(weak, lam * t_weak + (1 - lam) * t_weak[p])
    cons_strong = mse(strong, lam * t_strong + (1 - lam) * t_strong[p])
    parts = {"mixup_weak_class_loss": weak_class, "mixup_strong_class_loss": strong_class,
             "mixup_cons_weak_loss": cons_weak, "mixup_cons_strong_loss": cons_strong}
    return weak_class + strong_class + cc * cons_weak + cc * cons_strong, parts
