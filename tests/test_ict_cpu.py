"""Interpolation consistency (mixup), the part that needs no GPU: the C ABI of ``bsed_mix_rows`` (declared, exported,
every refusal before any HIP call) and the host-side plan (``engine.IctPlan``, ``engine.draw_ict``)."""
import ctypes

import numpy as np
import pytest

from bsed_amd import _lib as L
from bsed_amd.engine import IctPlan, draw_ict


def test_entry_point_and_job_limit_are_declared_and_exported():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 18
    assert "bsed_mix_rows" in L.header_symbols() and hasattr(lib, "bsed_mix_rows")
    assert L.CONSTANTS["BSED_MIX_MAX_JOBS"] == 8
    assert len(L.FUNCTIONS["bsed_mix_rows"][1]) == 9


def _call(n=2, njobs=None, tables=True, **k):
    """bsed_mix_rows on n well-formed jobs of dummy device pointers (never dereferenced: every refusal comes before
    the first HIP call), except for what the keyword arguments break in job 1"""
    job = dict(in_=0x100000, out=0x200000, perm=0x300000, lam=0.3, oml=0.7, rows=4, row_len=20)
    jobs = [dict(job) for _ in range(n)]
    if n > 1:
        jobs[1].update(k)
    arr = lambda t, key: (t * max(n, 1))(*[j[key] for j in jobs])
    args = [arr(ctypes.c_void_p, "in_"), arr(ctypes.c_void_p, "out"), arr(ctypes.c_void_p, "perm"),
            arr(ctypes.c_float, "lam"), arr(ctypes.c_float, "oml"), arr(ctypes.c_int, "rows"), arr(ctypes.c_long, "row_len")]
    if tables is not True:
        args[tables] = None
    return L.lib().bsed_mix_rows(*args, n if njobs is None else njobs, None)


def test_mix_rows_refuses_bad_arguments_before_any_hip_call():
    lib = L.lib()

    def refused(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and msg.startswith("bsed_mix_rows:") and word in msg, (rc, msg)

    for table in range(7):
        refused(_call(tables=table), "null")
    for name in ("in_", "out", "perm"):
        refused(_call(**{name: None}), "null")
    refused(_call(njobs=0), "jobs")
    refused(_call(njobs=-1), "jobs")
    refused(_call(n=9), "jobs")
    refused(_call(rows=0), "rows")
    refused(_call(rows=-3), "rows")
    refused(_call(row_len=0), "row_len")
    refused(_call(row_len=-1), "row_len")
    refused(_call(rows=1 << 20, row_len=1 << 14), "too large")           # 2^32 chunks of 4 elements
    refused(_call(out=0x100000), "overlap")                              # in place
    refused(_call(out=0x100000 + 4 * 4 * 20 - 4), "overlap")             # out begins in in's last element
    refused(_call(in_=0x200000 + 4 * 4 * 20 - 4), "overlap")             # in begins in out's last element
    refused(_call(in_=0x100002), "misaligned")
    refused(_call(out=0x200001), "misaligned")
    refused(_call(perm=0x300002), "misaligned")
    with pytest.raises(L.BsedError, match="bsed_mix_rows"):              # the convention of every caller: L.call raises
        L.call("bsed_mix_rows", None, None, None, None, None, None, None, 1, None)


def test_ict_plan_validates_on_the_host():
    plan = IctPlan(0.3, [1, 0], 0.7, [2, 0, 3, 1], 0.55, np.array([1, 0]))
    assert plan.lams == (0.3, 0.7, 0.55) and plan.perm_strong == (2, 0, 3, 1) and plan.perm_unl == (1, 0)
    assert plan.check_sizes(2, 4, 2) is plan
    IctPlan(0.0, [0], 1.0, [0], 1, [0])                                  # the ends of [0, 1], single clips
    good = dict(lam_weak=0.3, perm_weak=[1, 0], lam_strong=0.7, perm_strong=[2, 0, 3, 1], lam_unl=0.55, perm_unl=[1, 0])
    for bad in (dict(perm_weak=[1, 1]), dict(perm_strong=[1, 2, 3, 4]), dict(perm_unl=[0, -1]), dict(perm_unl=[]),
                dict(perm_weak=["a", 0]),
                dict(lam_weak=-1e-9), dict(lam_strong=1.0000001), dict(lam_unl=float("nan")), dict(lam_unl=None)):
        with pytest.raises(L.BsedError, match="IctPlan"):
            IctPlan(**{**good, **bad})
    for sizes in ((3, 4, 2), (2, 3, 2), (2, 4, 1)):                      # a perm of the wrong length for the batch
        with pytest.raises(L.BsedError, match="IctPlan"):
            plan.check_sizes(*sizes)


def test_draw_ict_is_deterministic_and_follows_the_reference_order():
    a, b = draw_ict(np.random.default_rng(5), 6, 12, 6), draw_ict(np.random.default_rng(5), 6, 12, 6)
    for name, n in (("weak", 6), ("strong", 12), ("unl", 6)):
        assert getattr(a, "lam_" + name) == getattr(b, "lam_" + name) and 0.0 <= getattr(a, "lam_" + name) <= 1.0
        assert getattr(a, "perm_" + name) == getattr(b, "perm_" + name)
        assert sorted(getattr(a, "perm_" + name)) == list(range(n))
    assert draw_ict(np.random.default_rng(6), 6, 12, 6).perm_strong != a.perm_strong
    # weak, strong, unlabelled; beta(alpha, alpha) then permutation(n); alpha 1.0, 1.0, 2.0
    rng = np.random.default_rng(5)
    want = [(float(rng.beta(al, al)), tuple(int(v) for v in rng.permutation(n))) for n, al in ((6, 1.0), (12, 1.0), (6, 2.0))]
    assert [(a.lam_weak, a.perm_weak), (a.lam_strong, a.perm_strong), (a.lam_unl, a.perm_unl)] == want
    # alpha <= 0 draws no beta: lam = 1, and the perms are the generator's first three permutations
    z = draw_ict(np.random.default_rng(5), 3, 5, 2, sup_alpha=0.0, usup_alpha=0)
    rng = np.random.default_rng(5)
    assert z.lams == (1.0, 1.0, 1.0)
    assert [z.perm_weak, z.perm_strong, z.perm_unl] == [tuple(int(v) for v in rng.permutation(n)) for n in (3, 5, 2)]
    half = draw_ict(np.random.default_rng(5), 3, 5, 2, sup_alpha=0.0)
    assert half.lams[:2] == (1.0, 1.0) and 0.0 < half.lam_unl < 1.0
    with pytest.raises(L.BsedError, match="draw_ict"):
        draw_ict(np.random.default_rng(5), 0, 4, 2)
