"""The segmented true-peak ceiling on the GPU (csrc/ceiling.hip: the need, apply, peak and trim
launches over all tracks of a batch, every track with its own ceiling) against the host
restatement mm_ceiling_host run on every track alone: equal samples, every mm_ceiling field
equal.  The shapes are the smallest at which a halo, a plane mask, a span count or the
workgroup -> track search can go wrong: tracks of 0, 1, 11, 12 and 13 frames, on both sides of
the need grid's span less its 11-frame tail and of the apply grid's span, and one of several
spans, in one batch; a quiet track between loud neighbours whose loudest frames touch it; the
three branches (under, limited, trimmed) in one batch."""
import ctypes

import numpy as np
import pytest

from test_ceiling import ONE, ceiling_stats, host_ceiling, q28

pytestmark = pytest.mark.gpu

RATE = 44100


def to_i16(raw):
    if raw.dtype == np.int16:
        return raw
    k = raw * np.float32(32768)
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max(initial=0) <= 32768  # still on the int16 grid
    return k.astype(np.int16)


def batch_ceiling(tracks, Cs, W, f32=False, device=False):
    """mm_batch_ceiling_pcm on copies of int16 `tracks` (or of tracks / 32768 as f32), or
    mm_batch_ceiling_device on torch copies of them: (the tracks afterwards as int16, their raw
    copies, the statistics of every track)."""
    from mastering_amd import engine, native
    ctx = native.context(0)
    n = len(tracks)
    xs = [np.ascontiguousarray(t, np.int16) for t in tracks]
    ch = 1 if xs[0].ndim == 1 else xs[0].shape[1]
    host = [x.astype(np.float32) / np.float32(32768) if f32 else x.copy() for x in xs]
    frames = (ctypes.c_int64 * n)(*[x.shape[0] for x in xs])
    C = (ctypes.c_int32 * n)(*Cs)
    out = (native.MMCeiling * n)()
    kind = native.MM_OUT_F32 if f32 else native.MM_OUT_I16
    if device:
        import torch
        d = [torch.from_numpy(h).cuda() for h in host]
        torch.cuda.current_stream().synchronize()  # the copies are on torch's stream, the library uses its own
        ctx.check(ctx.lib.mm_batch_ceiling_device(ctx.ptr, engine._pointers([t.data_ptr() for t in d]), kind, frames, n, ch,
                                                  C, W, out), "mm_batch_ceiling_device")
        host = [t.cpu().numpy() for t in d]
    else:
        ctx.check(ctx.lib.mm_batch_ceiling_pcm(ctx.ptr, engine._pointers([h.ctypes.data for h in host]), kind, frames, n, ch,
                                               C, W, out), "mm_batch_ceiling_pcm")
    return [to_i16(h) for h in host], host, [ceiling_stats(m) for m in out]


def check(tracks, Cs, W, **kw):
    """The batch against mm_ceiling_host of every track alone; returns the host's results."""
    got, _, stats = batch_ceiling(tracks, Cs, W, **kw)
    want = [host_ceiling(t, C, W) for t, C in zip(tracks, Cs)]
    for i, ((y, st), g, gst) in enumerate(zip(want, got, stats)):
        assert gst == st, (i, gst, st)
        assert np.array_equal(g, y), i
    return want


def timed(fn):
    from mastering_amd import native
    ctx = native.context(0)
    ctx.timing(True)
    try:
        res = fn()
        return res, ctx.kernel_stats()
    finally:
        ctx.timing(False)


@pytest.fixture(scope="module")
def spans():
    from mastering_amd import native
    lib = native.load()
    return lib.mm_meter_span(), lib.mm_ceiling_span()


def seam_lengths(spans):
    ms, cs = spans
    return [0, 1, 11, 12, 13, ms - 11, ms - 10, cs - 1, cs, cs + 1, 3 * cs + 5]


def seam_tracks(spans, ch):
    """Pink noise at -6 dBFS rms (test_ceiling's `trimmed` level: limited at -1 dBTP), one seed a track."""
    from mastering_amd.synth import pink_noise_pcm16
    return [pink_noise_pcm16(n, RATE, ch, track=40 + i, level_dbfs=-6.0) for i, n in enumerate(seam_lengths(spans))]


@pytest.mark.parametrize("W", [1, 220, 1024])
@pytest.mark.parametrize("ch", [1, 2])
def test_seams(spans, ch, W):
    tracks = seam_tracks(spans, ch)
    Cs = [q28(-1.0) if i % 2 == 0 else q28(-6.0) for i in range(len(tracks))]
    want = check(tracks, Cs, W)
    assert want[0][1]["frames"] == 0 and want[0][1]["tp_out_q28"] == 0
    for (y, st), C in list(zip(want, Cs))[5:]:  # every track of a span or so is limited, at either ceiling
        assert st["tp_in_q28"] > C >= st["tp_out_q28"] and st["limited_frames"] > 0
    assert len({st["ceiling_q28"] for _, st in want}) == 2


def test_a_quiet_track_between_loud_neighbours():
    """Three tracks packed with no padding between them (every byte count a multiple of 16).  The
    outer two sit at -1 dBFS with their loudest bursts in the 12 frames that touch the middle
    track, which sits at -30 dBFS: a read that runs from one track into the next (a halo, a
    plane, a window of W = 1024) limits frames of the middle track."""
    rng = np.random.default_rng(7)
    peak = int(round(32768 * 10 ** (-1 / 20)))
    outer = []
    for n in (8192, 8192):
        x = rng.integers(-peak, peak + 1, (n, 2)).astype(np.int16)
        x[:12] = np.where(np.arange(12)[:, None] % 2 == 0, 32767, -32768)
        x[-12:] = np.where(np.arange(12)[:, None] % 2 == 0, -32768, 32767)
        outer.append(x)
    quiet = rng.integers(-1036, 1037, (4096, 2)).astype(np.int16)
    tracks = [outer[0], quiet, outer[1]]
    assert all(t.nbytes % 16 == 0 for t in tracks)
    C = q28(-1.0)
    for f32 in (False, True):
        before = quiet.astype(np.float32) / np.float32(32768) if f32 else quiet
        got, raw, stats = batch_ceiling(tracks, [C] * 3, 1024, f32=f32)
        assert raw[1].tobytes() == before.tobytes()
        st = stats[1]
        assert st["limited_frames"] == 0 and st["tp_in_q28"] == st["tp_out_q28"] and st["min_gain_q16"] == ONE
        for i in (0, 2):
            y, hst = host_ceiling(tracks[i], C, 1024)
            assert stats[i] == hst and np.array_equal(got[i], y)
            assert hst["tp_in_q28"] > C >= hst["tp_out_q28"]


@pytest.fixture(scope="module")
def branches():
    """test_ceiling.branch_inputs' three signals."""
    from mastering_amd.synth import pink_noise_pcm16
    return [pink_noise_pcm16(20000, RATE, 2, track=3, level_dbfs=-18.0),
            pink_noise_pcm16(20000, RATE, 2, track=2, level_dbfs=-12.0),
            pink_noise_pcm16(20000, RATE, 2, track=1, level_dbfs=-6.0)]


@pytest.mark.parametrize("W,trim", [(1, 65254), (16, 65514), (220, ONE)])
def test_every_branch_in_one_batch(branches, W, trim):
    """under, limited and trimmed in one call: the trims are those tests/test_gpu_ceiling.py pins,
    and the trim launch appears exactly when a track is trimmed."""
    C = q28(-1.0)
    want, stats = timed(lambda: check(branches, [C] * 3, W, device=True))
    (_, under), (_, limited), (_, trimmed) = want
    assert under["limited_frames"] == 0 and under["tp_out_q28"] == under["tp_in_q28"] <= C
    assert limited["limited_frames"] > 0 and limited["trim_q16"] == ONE
    assert trimmed["trim_q16"] == trim and trimmed["tp_out_q28"] <= C < trimmed["tp_in_q28"]
    assert ("ceil_tracks_trim" in stats) == (trim != ONE)
    n_peak = 2 if trim != ONE else 1
    assert stats["ceil_tracks_need"][1] == stats["ceil_tracks_apply"][1] == 1 and stats["ceil_tracks_peak"][1] == n_peak
    assert not [k for k in stats if k in ("ceil_need", "ceil_apply", "ceil_trim", "meter_i16")], stats.keys()


def test_f32_equals_int16_and_a_second_run_is_identical(spans):
    tracks = seam_tracks(spans, 2)
    Cs = [q28(-1.0) if i % 2 == 0 else q28(-6.0) for i in range(len(tracks))]
    a, raw_a, st_a = batch_ceiling(tracks, Cs, 220, device=True)
    b, raw_b, st_b = batch_ceiling(tracks, Cs, 220, device=True)
    f, _, st_f = batch_ceiling(tracks, Cs, 220, f32=True, device=True)
    p, _, st_p = batch_ceiling(tracks, Cs, 220)
    assert st_a == st_b == st_f == st_p
    for x, y, z, w in zip(raw_a, raw_b, f, p):
        assert x.tobytes() == y.tobytes() and np.array_equal(x, z) and np.array_equal(x, w)


def test_the_python_entry(branches):
    from mastering_amd import ceiling_batch_pcm
    before = [b.copy() for b in branches]
    outs, ds = ceiling_batch_pcm(branches, RATE, [-1.0, -3.0, -1.0])
    for x, b, y, d, db in zip(branches, before, outs, ds, (-1.0, -3.0, -1.0)):
        want, st = host_ceiling(x, q28(db), 220)
        assert np.array_equal(x, b) and np.array_equal(y, want)  # new arrays: the inputs are not touched
        assert {k: d[k] for k in st} == st and d["window"] == 220
    assert [d["ceiling_q28"] for d in ds] == [q28(-1.0), q28(-3.0), q28(-1.0)]
    outs1, ds1 = ceiling_batch_pcm(branches, RATE, -1.0, window=16)
    assert [d["window"] for d in ds1] == [16] * 3 and ds1[2]["trim_q16"] == 65514


def test_refusals_name_the_track_and_leave_the_context_usable(branches):
    pcm = np.zeros((64, 2), np.int16)
    ok = 2 ** 27
    for Cs, W, words in (([ok, 2 ** 24 - 1], 16, "track 1: ceiling_q28 out of range"),
                         ([2 ** 28 + 1, ok], 16, "track 0: ceiling_q28 out of range"),
                         ([ok, ok, 0], 16, "track 2: ceiling_q28 out of range"),
                         ([ok, ok], 0, "track 0: ceiling window out of range"),
                         ([ok, ok], 1025, "track 0: ceiling window out of range")):
        with pytest.raises(ValueError, match=words):
            batch_ceiling([pcm] * len(Cs), Cs, W)
        with pytest.raises(ValueError, match=words):
            batch_ceiling([pcm] * len(Cs), Cs, W, device=True)
    from mastering_amd import native
    ctx, lib = native.context(0), native.load()
    out = (native.MMCeiling * 1)()
    fr, C = (ctypes.c_int64 * 1)(64), (ctypes.c_int32 * 1)(ok)
    ptr = (ctypes.c_void_p * 1)(pcm.ctypes.data)
    for n in (0, 257):
        assert lib.mm_batch_ceiling_pcm(ctx.ptr, ptr, 0, fr, n, 2, C, 16, out) == native.MM_ERR_ARG
        assert b"tracks out of range [1, 256]" in lib.mm_last_error(ctx.ptr)
    assert lib.mm_batch_ceiling_pcm(ctx.ptr, ptr, 0, fr, 1, 3, C, 16, out) == native.MM_ERR_ARG
    assert b"track 0: channels must be 1 or 2" in lib.mm_last_error(ctx.ptr)
    assert lib.mm_batch_ceiling_pcm(ctx.ptr, ptr, 7, fr, 1, 2, C, 16, out) == native.MM_ERR_ARG
    fr2, C2 = (ctypes.c_int64 * 2)(2 ** 30, 2 ** 30), (ctypes.c_int32 * 2)(ok, ok)
    ptr2 = (ctypes.c_void_p * 2)(pcm.ctypes.data, pcm.ctypes.data)
    out2 = (native.MMCeiling * 2)()
    assert lib.mm_batch_ceiling_pcm(ctx.ptr, ptr2, 0, fr2, 2, 2, C2, 16, out2) == native.MM_ERR_ARG
    assert b"track 1: 2^31 frames or more in all" in lib.mm_last_error(ctx.ptr)
    # an empty batch of one empty track is valid; and the context still works
    got, _, st = batch_ceiling([np.zeros((0, 2), np.int16)], [ok], 16)
    assert st[0]["frames"] == 0 and st[0]["tp_out_q28"] == 0 and got[0].shape == (0, 2)
    check(branches, [q28(-1.0)] * 3, 220)
