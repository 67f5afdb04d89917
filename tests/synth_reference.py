"""Float64 restatement of the soundscape mix (include/bsed.h, bsed_synth_mix), the reference of tests/test_synth_cpu.py
and tests/test_synth_gpu.py:

    ref[b, j] = bank[bg_off + (bg_phase + j) % bg_len] * bg_gain + sum_k bank[src_k + i] * w_k(i) * g_k,   i = j - on_k

over the events k < n_ev[b] with 0 <= i < len_k.  The samples, the gains and the fade weight w are the fp32 values the
kernel sees (w is two fp32 products and three minima, which numpy float32 arithmetic reproduces bit for bit), all
promoted to float64; the products and the sum are float64.  It differs from the kernel by the
kernel's fp32 roundings alone: per event one for the product x * w and one for the fma, one for the background product,
which is what the bound

    |out - ref| <= (2 * K[j] + 2) * 2^-24 * S[j],     S[j] = |bg * bg_gain| + sum_k |x * w * g|,   K[j] = events over j

allows (one unit of slack; it holds for any order of the sum).  Also here: the hand-built bank and plans both test files
use."""
import numpy as np

U24 = 2.0 ** -24


def fade_weight(length, inv_fade):
    """w(i), i = 0 .. length - 1, in float32 arithmetic"""
    i = np.arange(length, dtype=np.int64)
    f, one = np.float32(inv_fade), np.float32(1.0)
    up = np.minimum(one, (i + 1).astype(np.float32) * f)
    down = np.minimum(one, (length - i).astype(np.float32) * f)
    w = np.minimum(up, down)
    assert w.dtype == np.float32
    return w


def mix_ref(bank, plan):
    """bank: (N,) float32 numpy; plan: a SoundscapePlan (or anything with its arrays) -> (ref, S, K): float64, float64,
    int64, each (B, n)"""
    bank = np.asarray(bank)
    assert bank.dtype == np.float32
    b64 = bank.astype(np.float64)
    B, n = plan.B, plan.n
    ref, S, K = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n), np.int64)
    j = np.arange(n, dtype=np.int64)
    for b in range(B):
        if plan.bg_len[b] > 0:
            bg = b64[plan.bg_off[b] + (plan.bg_phase[b] + j) % plan.bg_len[b]] * np.float64(plan.bg_gain[b])
            ref[b] += bg
            S[b] += np.abs(bg)
        for k in range(int(plan.n_ev[b])):
            on, ln, src = int(plan.on[b, k]), int(plan.len[b, k]), int(plan.src[b, k])
            w = fade_weight(ln, plan.inv_fade[b, k]).astype(np.float64)
            term = b64[src:src + ln] * w * np.float64(plan.g[b, k])
            ref[b, on:on + ln] += term
            S[b, on:on + ln] += np.abs(term)
            K[b, on:on + ln] += 1
    return ref, S, K


# ---- the hand-built case: seven items, three clips of n = 20011 samples -------------------------------------------------
# n is prime: the last tile is ragged and rows 1 and 2 of the (B, n) output start 3 and 2 samples off a 16-byte boundary.
# The kernel's tile is 4096 samples, so the clip spans five tiles.
N_HAND = 20011
ITEM_LEN = [1, 7, 1000, 5003, 30000, 997, 25000]           # five snippets (30000 > n), two backgrounds
ITEM_CLASS = [0, 1, 2, 3, 2, -1, -1]                        # items 2 and 4 share a class
ITEM_OFF = np.concatenate([[0], np.cumsum(ITEM_LEN)[:-1]]).astype(np.int64)


def hand_bank_samples(seed=5):
    rng = np.random.default_rng(seed)
    return [(0.25 * rng.standard_normal(ln)).astype(np.float32) for ln in ITEM_LEN]


def hand_rows():
    """per clip: (background (item, phase, gain) or None, [(item, start inside the item, on, len, g, inv_fade), ...])"""
    n, f = N_HAND, 1.0 / 320.0
    clip0 = ((5, 123, 0.5), [                               # the 997-sample background wraps about 20 times
        (2, 0, 0, 1000, 0.7, f),                            # onset 0
        (3, 0, n - 5003, 5003, 1.3, f),                     # ends exactly at n
        (2, 0, 3001, 1000, 0.9, f),                         # two events over the same samples, same class,
        (4, 777, 3001, 1000, 0.4, 1.0),                     # src - on odd for both
        (0, 0, 10000, 1, 2.0, 1.0),                         # one sample
        (1, 0, 5000, 7, 0.0, f),                            # gain 0
        (4, 5, 0, n, 0.2, f),                               # a snippet longer than the clip, cut to it
    ])
    clip1 = ((6, 24999, 1.0), [])                           # no events; the background wraps after one sample
    ev2 = [(3, 100 * k + 1, 1000 + 500 * k, 4000, 0.1 * (k + 1), f if k % 2 else 1.0) for k in range(8)]    # 8 deep
    ev2 += [(1, 0, on, 7, 1.0, 1.0) for on in (0, 7, 14, n - 7)]
    ev2 += [(2, k, 12000 + 1001 * k, 1000 - k, 0.5, f) for k in range(4)]
    clip2 = (None, ev2)                                     # 16 events over silence
    return [clip0, clip1, clip2]


def hand_plan(synth, labels, rows=None, sr=32000, K=16, n=N_HAND, **kw):
    """the SoundscapePlan of the given rows (default: all three clips)"""
    rows = hand_rows() if rows is None else rows
    B = len(rows)
    P = dict(bg_off=np.zeros(B, np.int64), bg_len=np.zeros(B, np.int64), bg_phase=np.zeros(B, np.int64),
             bg_gain=np.zeros(B, np.float32), n_ev=np.zeros(B, np.int32), src=np.zeros((B, K), np.int64),
             on=np.zeros((B, K), np.int64), length=np.ones((B, K), np.int64), g=np.zeros((B, K), np.float32),
             inv_fade=np.ones((B, K), np.float32), cls=np.zeros((B, K), np.int32))
    for b, (bg, events) in enumerate(rows):
        if bg is not None:
            P["bg_off"][b], P["bg_len"][b], P["bg_phase"][b], P["bg_gain"][b] = ITEM_OFF[bg[0]], ITEM_LEN[bg[0]], bg[1], bg[2]
        P["n_ev"][b] = len(events)
        for k, (item, start, on, ln, g, f) in enumerate(events):
            P["src"][b, k], P["on"][b, k], P["length"][b, k] = ITEM_OFF[item] + start, on, ln
            P["g"][b, k], P["inv_fade"][b, k], P["cls"][b, k] = g, f, ITEM_CLASS[item]
    return synth.SoundscapePlan(n, sr, labels, **P, **kw)


# sample onsets at which sample // (hop * pooling) is NOT the encoder's frame int(t * sr // hop // pooling)
BOUNDARY_ONSETS = {32000: [129540, 256020, 259080], 22050: [1020, 2040, 4080, 8160]}
