"""Recording-level detection, the part that needs no GPU: the window plan against values worked by hand, the argument
checks of the new C entry points (they run before any HIP call), and numpy restatements of the stitch and of the
rank-paired, chunked region decode that the GPU kernels implement -- checked here against
``labels_oracle.find_contiguous_regions`` and imported by tests/test_detect_gpu.py as the kernels' reference."""
import numpy as np
import pytest

from bsed_amd import _lib as L
from bsed_amd.evaluation import window_plan
from oracle import labels_oracle as lo

CHUNK = 64          # BSED_DECODE_LONG_FRAMES


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements
# ---------------------------------------------------------------------------------------------------------------------
def stitch_np(p, starts, weighting="triangular"):
    """(W, Tp, C) window probabilities + starts in output frames -> ((T_total, C) float64 weighted mean over the
    covering windows in ascending window order, (T_total,) number of windows covering each frame)"""
    p = np.asarray(p, dtype=np.float64)
    W, Tp, C = p.shape
    j = np.arange(Tp)
    wgt = np.minimum(j + 1, Tp - j).astype(np.float64) if weighting == "triangular" else np.ones(Tp)
    T_total = int(starts[-1]) + Tp
    acc, wsum, cover = np.zeros((T_total, C)), np.zeros(T_total), np.zeros(T_total, dtype=np.int64)
    for w in range(W):
        s = int(starts[w])
        acc[s:s + Tp] += wgt[:, None] * p[w]
        wsum[s:s + Tp] += wgt
        cover[s:s + Tp] += 1
    assert cover.min() >= 1, "a frame that no window covers"
    return acc / wsum[:, None], cover


def decode_long_np(mask, scale, max_len, chunk=CHUNK):
    """The kernels' algorithm on the host: (T, C) 0/1 mask -> (clip, class, frames (E,2), seconds (E,2)).  Frame t opens
    a region iff on[t] and not on[t-1] and closes one (offset frame t + 1) iff on[t] and not on[t+1]; per (class, chunk)
    counts of onsets, exclusive prefix in class-major order, every chunk writes its onsets at offset + rank and its ends
    at the same ranks less one if a region is open across its first frame.  No state passes between chunks."""
    on = np.asarray(mask) != 0
    T, C = on.shape
    nchunks = -(-T // chunk)
    prev = np.vstack([np.zeros((1, C), bool), on[:-1]])
    nxt = np.vstack([on[1:], np.zeros((1, C), bool)])
    onset, end = on & ~prev, on & ~nxt
    counts = np.zeros((C, nchunks), np.int64)
    for k in range(nchunks):
        counts[:, k] = onset[k * chunk:(k + 1) * chunk].sum(0)
    flat = counts.ravel()
    offsets = (np.cumsum(flat) - flat).reshape(C, nchunks)
    E = int(flat.sum())
    ev_class, ev_frames = np.full(E, -1, np.int32), np.full((E, 2), -1, np.int32)
    for k in range(nchunks):
        t0 = k * chunk
        for c in range(C):
            is_open = t0 > 0 and on[t0 - 1, c] and on[t0, c]
            ts = np.nonzero(onset[t0:t0 + chunk, c])[0] + t0
            te = np.nonzero(end[t0:t0 + chunk, c])[0] + t0
            ko = offsets[c, k] + np.arange(len(ts))
            ke = offsets[c, k] - int(is_open) + np.arange(len(te))
            ev_class[ko] = c
            ev_frames[ko, 0] = ts
            ev_frames[ke, 1] = te + 1
    sec = np.minimum(np.maximum(ev_frames.astype(np.float64) * scale, 0.0), max_len)
    return np.zeros(E, np.int32), ev_class, ev_frames, sec


def regions_oracle(mask):
    """[(class, onset, offset)] by labels_oracle.find_contiguous_regions, class then time"""
    return [(c, int(a), int(b)) for c in range(mask.shape[1]) for a, b in lo.find_contiguous_regions(mask[:, c])]


def crafted_masks():
    """(name, (T, C) float32 mask) cases of the long decode: densities, edges of the recording, edges of the chunks"""
    rng = np.random.default_rng(11)
    out = []
    for dens in (0.01, 0.5, 0.99):
        out.append((f"random{dens}", (rng.random((1000, 20)) < dens).astype(np.float32)))
    out.append(("all_on", np.ones((300, 20), np.float32)))
    out.append(("all_off", np.zeros((300, 20), np.float32)))
    m = np.zeros((4 * CHUNK + 7, 20), np.float32)
    m[0:5, 0] = 1                                   # an event from frame 0
    m[-3:, 1] = 1                                   # an event to frame T
    m[CHUNK - 1:CHUNK + 9, 2] = 1                   # starts on the last frame of a chunk
    m[10:CHUNK + 1, 3] = 1                          # ends on the first frame of the next chunk
    m[CHUNK - 5:3 * CHUNK + 5, 4] = 1               # spans three chunk boundaries
    m[CHUNK - 1, 5] = 1; m[CHUNK, 6] = 1            # single frames at either side of a boundary
    m[0:CHUNK, 7] = 1; m[CHUNK:2 * CHUNK, 8] = 1    # exactly one chunk, on
    m[::2, 9] = 1                                   # alternating: one event per two frames
    m[:, 10] = 1
    out.append(("crafted", m))
    for T in (1, CHUNK, CHUNK + 1):
        for C in (20, 1):
            out.append((f"T{T}_C{C}", (rng.random((T, C)) < 0.5).astype(np.float32)))
            out.append((f"T{T}_C{C}_on", np.ones((T, C), np.float32)))
    return out


def long_mask(T=113000, C=20, dens=0.01, seed=5):
    return (np.random.default_rng(seed).random((T, C)) < dens).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# window_plan
# ---------------------------------------------------------------------------------------------------------------------
def test_window_plan_values_worked_by_hand():
    s, Tp, T_total = window_plan(320000)
    assert s.dtype == np.int32 and s.tolist() == [0] and (Tp, T_total) == (313, 313)
    # 30 s: 156 * 1020 = 159120 samples per hop; 4 * 159120 + 320000 = 956480 <= 960000 < 5 * 159120 + 320000, so the
    # regular starts are 0 .. 624; the end-aligned one is (960000 - 320000) // 1020 = 627
    s, Tp, T_total = window_plan(960000, hop_frames=156)
    assert s.tolist() == [0, 156, 312, 468, 624, 627] and (Tp, T_total) == (313, 940)
    assert window_plan(960000)[0].tolist() == s.tolist()                     # hop_frames defaults to Tp // 2 = 156
    # the last window lies inside the recording and leaves less than one output frame (1020 samples) uncovered
    assert 627 * 1020 + 320000 <= 960000 < 628 * 1020 + 320000
    # end-aligned start == last regular start: (638240 - 320000) // 1020 = 312 = 2 * 156 -> not duplicated
    s, _, T_total = window_plan(320000 + 2 * 156 * 1020, hop_frames=156)
    assert s.tolist() == [0, 156, 312] and T_total == 625
    # ... and one output frame more moves the last window
    assert window_plan(320000 + 2 * 156 * 1020 + 1020, hop_frames=156)[0].tolist() == [0, 156, 312, 313]
    # hop_frames = Tp: no overlap; n = two hops plus one window
    s, _, T_total = window_plan(2 * 313 * 1020 + 320000, hop_frames=313)
    assert s.tolist() == [0, 313, 626] and T_total == 939


def test_window_plan_at_22050_hz_and_short_recordings():
    # win = 220500 samples, ceil(220500 / 255) = 865 STFT frames, 865 // 4 = 216 output frames
    s, Tp, T_total = window_plan(220500, sr=22050)
    assert s.tolist() == [0] and (Tp, T_total) == (216, 216)
    # 30 s: (661500 - 220500) // (108 * 1020) = 4 -> regular 0 .. 432; end-aligned 441000 // 1020 = 432: the same window
    s, Tp, T_total = window_plan(661500, sr=22050)
    assert s.tolist() == [0, 108, 216, 324, 432] and T_total == 648
    s, Tp, T_total = window_plan(700000, sr=22050, hop_frames=216)
    assert s.tolist() == [0, 216, 432, 470] and T_total == 686              # (700000 - 220500) // 1020 = 470
    # shorter than one window: one clip, padded by the clip path
    for n in (1, 1019, 100000, 319999):
        s, Tp, T_total = window_plan(n)
        assert s.tolist() == [0] and (Tp, T_total) == (313, 313)


def test_window_plan_refuses_a_hop_outside_1_to_Tp():
    for bad in (0, -1, 314):
        with pytest.raises(L.BsedError):
            window_plan(960000, hop_frames=bad)
    with pytest.raises(L.BsedError):
        window_plan(661500, sr=22050, hop_frames=217)
    assert window_plan(960000, hop_frames=313)[1] == 313 and window_plan(960000, hop_frames=1)[0][1] == 1


def test_every_window_is_on_the_frame_grid_and_inside_the_recording():
    rng = np.random.default_rng(0)
    for n in [int(v) for v in rng.integers(320000, 5_000_000, 40)] + [320001, 321019, 321020, 321021]:
        for hop in (None, 100, 313, 1):
            if hop == 1 and n > 400000:
                continue
            s, Tp, T_total = window_plan(n, hop_frames=hop)
            h = 156 if hop is None else hop
            assert s[0] == 0 and np.all(np.diff(s) > 0) and np.all(np.diff(s) <= h)
            assert np.all(np.diff(s)[:-1] == h)
            assert int(s[-1]) * 1020 + 320000 <= n < (int(s[-1]) + 1) * 1020 + 320000
            assert T_total == s[-1] + Tp


# ---------------------------------------------------------------------------------------------------------------------
# the restatements against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mask", crafted_masks(), ids=[n for n, _ in crafted_masks()])
def test_rank_paired_decode_restatement_matches_find_contiguous_regions(name, mask):
    scale = 4 / (32000 / 255)
    max_len = mask.shape[0] * scale * 0.9          # clips the late events
    clip, cls, frames, sec = decode_long_np(mask, scale, max_len)
    want = regions_oracle(mask)
    assert [(int(c), int(f[0]), int(f[1])) for c, f in zip(cls, frames)] == want
    assert not clip.any() and sec.dtype == np.float64
    ref = np.clip(np.asarray([[a, b] for _, a, b in want], np.float64).reshape(-1, 2) * scale, 0, max_len)
    assert np.array_equal(sec, ref)
    if mask.shape[0] > 3:                           # the chunk length is a free parameter of the algorithm
        for chunk in (1, 3, 1000):
            assert np.array_equal(decode_long_np(mask, scale, max_len, chunk)[2], frames)


def test_rank_paired_decode_restatement_on_a_long_mask():
    mask = long_mask(20000, 20, 0.01)
    _, cls, frames, _ = decode_long_np(mask, 1.0, 1e9)
    assert [(int(c), int(f[0]), int(f[1])) for c, f in zip(cls, frames)] == regions_oracle(mask)


def test_stitch_restatement():
    rng = np.random.default_rng(2)
    Tp, C = 313, 20
    # windows cut from one time line: any weighted mean gives the time line back
    starts, _, T_total = window_plan(35 * 32000, hop_frames=100)
    line = rng.random((T_total, C))
    p = np.stack([line[s:s + Tp] for s in starts])
    for weighting in ("uniform", "triangular"):
        out, cover = stitch_np(p, starts, weighting)
        assert np.abs(out - line).max() < 1e-15 and cover.max() == 4 and cover.min() == 1
    # no overlap: a concatenation
    starts, _, T_total = window_plan(2 * 313 * 1020 + 320000, hop_frames=313)
    p = rng.random((3, Tp, C))
    out, cover = stitch_np(p, starts, "triangular")
    assert cover.max() == 1 and np.abs(out - p.reshape(-1, C)).max() < 1e-15
    # two windows, by hand: frame 200 is local frame 200 of window 0 (weight min(201, 113) = 113) and local frame 44 of
    # window 1 (weight 45)
    starts = np.asarray([0, 156], np.int32)
    p = rng.random((2, Tp, C))
    tri, _ = stitch_np(p, starts, "triangular")
    uni, _ = stitch_np(p, starts, "uniform")
    assert np.allclose(tri[200], (113 * p[0, 200] + 45 * p[1, 44]) / 158, rtol=0, atol=1e-15)
    assert np.allclose(uni[200], (p[0, 200] + p[1, 44]) / 2, rtol=0, atol=1e-15)
    assert np.array_equal(uni[100], p[0, 100]) and np.array_equal(uni[400], p[1, 244])


# ---------------------------------------------------------------------------------------------------------------------
# argument checks of the new entry points: all before the first HIP call
# ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_refuse_bad_arguments_before_any_hip_call():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 4
    for name in ("bsed_gather_windows", "bsed_stitch_windows", "bsed_decode_long_count", "bsed_decode_long_write"):
        assert name in L.header_symbols()
    assert L.CONSTANTS["BSED_DECODE_LONG_FRAMES"] == CHUNK
    assert (L.CONSTANTS["BSED_STITCH_UNIFORM"], L.CONSTANTS["BSED_STITCH_TRIANGULAR"]) == (0, 1)
    d = 0x1000                                      # non-null, 16-byte aligned, never dereferenced on the host

    def refused(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(lib.bsed_gather_windows(None, 960000, d, 6, 320000, 1020, d, None), "null")
    refused(lib.bsed_gather_windows(d, 960000, d, 6, 320002, 1020, d, None), "multiples of 4")      # win % 4 != 0
    refused(lib.bsed_gather_windows(d, 960000, d, 6, 320000, 1022, d, None), "multiples of 4")      # frame % 4 != 0
    refused(lib.bsed_gather_windows(d + 4, 960000, d, 6, 320000, 1020, d, None), "aligned")
    refused(lib.bsed_gather_windows(d, 1000, d, 1, 320000, 1020, d, None), "bad shape")             # win > n
    refused(lib.bsed_stitch_windows(d, d, 6, 313, 20, 0, 940, 1, d + 0x1000, None), "hop_frames")
    refused(lib.bsed_stitch_windows(d, d, 6, 313, 20, 314, 940, 1, d + 0x1000, None), "hop_frames")
    refused(lib.bsed_stitch_windows(d, d, 6, 313, 20, 156, 940, 2, d + 0x1000, None), "weighting")
    refused(lib.bsed_stitch_windows(d, d, 6, 313, 20, 156, 1200, 1, d + 0x1000, None), "does not fit")   # a gap
    refused(lib.bsed_stitch_windows(d, d, 6, 313, 20, 156, 900, 1, d + 0x1000, None), "does not fit")    # last <= W-2
    refused(lib.bsed_stitch_windows(d, None, 6, 313, 20, 156, 940, 1, d + 0x1000, None), "null")
    refused(lib.bsed_decode_long_count(d, 0, 20, d, None), "bad shape")
    refused(lib.bsed_decode_long_count(d, 100, 513, d, None), "bad shape")
    refused(lib.bsed_decode_long_write(d, d, 100, 20, 1.0, 10.0, d, None, d, None), "null")


def test_python_wrappers_refuse_bad_layouts_before_any_gpu_call():
    import torch
    from bsed_amd import evaluation as ev
    p = torch.zeros((3, 313, 20))                                   # a CPU tensor: any GPU call would raise on it
    for starts in ([0, 100, 250], [1, 157, 313], [0, 400, 800], [0, 156, 156]):
        with pytest.raises(L.BsedError, match="starts|apart"):
            ev.stitch_windows(p, starts)
    with pytest.raises(L.BsedError, match="weighting"):
        ev.stitch_windows(p, [0, 156, 312], weighting="hann")
    with pytest.raises(L.BsedError, match="hop_frames"):
        ev.detect_recording(torch.nn.Identity(), np.zeros(960000, np.float32), _Enc().decode_strong,
                            predictor=torch.nn.Identity(), hop_frames=400, mel=_Mel())
    with pytest.raises(NotImplementedError):
        ev.detect_recording(torch.nn.Identity(), np.zeros(960000, np.float32), _Enc().decode_strong)


class _Enc:
    labels = lo.BIRD_LIST

    def decode_strong(self, y):
        return lo.decode_strong(y)


class _Mel:
    class cfg:
        sr, hop_size, max_len_seconds = 32000, 255, 10.0
