"""The converter over a batch on the GPU (mm_batch_resample_device / _pcm): no numerics are new,
so every track's samples and statistics are compared with the numpy definition of that track
ALONE (tests/test_resample.py: ref_resample), at the sizes where the launch over all tracks can
go wrong: tracks of 0, 1, K, S - 1, S, S + 1 and 3 S + 5 output frames (S = mm_resample_span())
in one batch, empty tracks in front, in the middle and at the end (the track search), tracks
packed back to back in one allocation (a neighbour's frames must never be read or written),
statistics that must stay with their track, spans staged in pieces, the launch count, refused
arguments and the taps cache shared with the single-track entry.  All comparisons are
equalities on integers."""
import ctypes

import numpy as np
import pytest

from test_gpu_resample import planned, seam_signal, smallest_input
from test_resample import ONE, host_resample, ref_resample, resample_stats, resampler

pytestmark = pytest.mark.gpu

PAIRS = [(96000, 44100), (44100, 48000), (96000, 48000)]  # L = 147 down, up, L = 1
GUARD = 64  # sentinel frames in front of and behind the packed outputs


@pytest.fixture(scope="module")
def span():
    from mastering_amd import native
    return native.load().mm_resample_span()


def _frames_out(n, rs):
    return -(-n * rs.L // rs.M)


def _pointers(addresses):
    return (ctypes.c_void_p * len(addresses))(*[ctypes.c_void_p(int(a)) for a in addresses])


def _as_int16(raw, f32):
    if not f32:
        return raw
    k = raw * np.float32(32768)
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max(initial=0) <= 32768  # on the int16 grid
    return k.astype(np.int16)


def batch_device(tracks, rs, f32=False, kind=None, ch=None, n=None):
    """mm_batch_resample_device on tracks packed back to back, without a gap, in ONE device
    allocation (pointers into it), the outputs likewise packed between two guards and pre-filled
    with the sentinel 77: ([output of track t as int16], [statistics]).  Asserts that no frame of
    the guards was written; a write outside a track's frames_out inside the packed outputs lands
    in a neighbour and shows there."""
    import torch
    from mastering_amd import native
    xs = [np.ascontiguousarray(t, np.int16) for t in tracks]
    tail = xs[0].shape[1:]
    host = np.concatenate(xs) if xs else np.zeros((0,) + tail, np.int16)
    host = host.astype(np.float32) / np.float32(32768) if f32 else host
    outs = [_frames_out(x.shape[0], rs) for x in xs]
    d = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    o = torch.full((2 * GUARD + sum(outs),) + tail, 77, dtype=d.dtype, device="cuda")
    torch.cuda.current_stream().synchronize()  # the copies are on torch's stream, the library uses its own
    fb = host.dtype.itemsize * (tail[0] if tail else 1)
    in_at = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).astype(np.int64)
    out_at = GUARD + np.concatenate([[0], np.cumsum(outs)]).astype(np.int64)
    count = len(xs) if n is None else n
    frames = (ctypes.c_int64 * max(count, 1))(*[x.shape[0] for x in xs][:count])
    ms = (native.MMResample * max(count, 1))()
    ctx = native.context(0)
    ctx.check(ctx.lib.mm_batch_resample_device(
        ctx.ptr, _pointers([d.data_ptr() + int(a) * fb for a in in_at[:-1]]),
        (native.MM_OUT_F32 if f32 else native.MM_OUT_I16) if kind is None else kind, frames, count,
        (tail[0] if tail else 1) if ch is None else ch, ctypes.byref(rs),
        _pointers([o.data_ptr() + int(a) * fb for a in out_at[:-1]]), ms), "mm_batch_resample_device")
    raw = o.cpu().numpy()
    assert np.all(raw[:GUARD] == 77) and np.all(raw[len(raw) - GUARD:] == 77), "a frame outside the outputs was written"
    got = [_as_int16(raw[out_at[t]:out_at[t + 1]], f32) for t in range(len(xs))]
    for m in ms[:len(xs)]:
        assert (m.rate_in, m.rate_out) == (rs.rate_in, rs.rate_out)
    return got, [resample_stats(m) for m in ms[:len(xs)]]


def batch_pcm(tracks, rs, f32=False):
    """mm_batch_resample_pcm on host arrays, every output followed by a guard of the sentinel."""
    from mastering_amd import native
    xs = [np.ascontiguousarray(t, np.int16) for t in tracks]
    xs = [x.astype(np.float32) / np.float32(32768) for x in xs] if f32 else xs
    tail = xs[0].shape[1:]
    outs = [np.full((_frames_out(x.shape[0], rs) + 8,) + tail, 77, x.dtype) for x in xs]
    n = len(xs)
    frames = (ctypes.c_int64 * n)(*[x.shape[0] for x in xs])
    ms = (native.MMResample * n)()
    ctx = native.context(0)
    ctx.check(ctx.lib.mm_batch_resample_pcm(ctx.ptr, _pointers([x.ctypes.data for x in xs]),
                                            native.MM_OUT_F32 if f32 else native.MM_OUT_I16, frames, n,
                                            tail[0] if tail else 1, ctypes.byref(rs),
                                            _pointers([o.ctypes.data for o in outs]), ms), "mm_batch_resample_pcm")
    for o in outs:
        assert np.all(o[len(o) - 8:] == 77), "a frame behind a track's frames_out was written"
    return [_as_int16(o[:len(o) - 8], f32) for o in outs], [resample_stats(m) for m in ms]


def check_batch(tracks, rs, table, want=None, f32s=(False, True), paths=("pcm", "device")):
    """Every track of the batch against ref_resample of that track alone."""
    want = [ref_resample(t, *table) for t in tracks] if want is None else want
    for path in paths:
        for f32 in f32s:
            got, st = (batch_pcm if path == "pcm" else batch_device)(tracks, rs, f32)
            for t, (w, wst) in enumerate(want):
                assert st[t] == wst, (path, "f32" if f32 else "i16", t, st[t], wst)
                assert got[t].shape == w.shape and np.array_equal(got[t], w), (path, "f32" if f32 else "i16", t)
    return want


# ------------------------------------------------------------------ 1. seams and the track search
_SEAMS = {}


def seam_batch(span, pair, ch):
    """The batch of test 1 and its reference, computed once per (pair, ch) and left unchanged."""
    if (pair, ch) not in _SEAMS:
        rs, table = planned(*pair)
        L, M, K, _ = table
        tracks = []
        for i, size in enumerate((0, 1, K, span - 1, 0, span, span + 1, 3 * span + 5, 0)):
            n = smallest_input(size, L, M)[0] if size else 0
            tracks.append(seam_signal(n, ch, span, L, M, 100 * i + 10 * ch + L) if n
                          else np.zeros((0, 2) if ch == 2 else (0,), np.int16))
        _SEAMS[(pair, ch)] = (rs, table, tracks, [ref_resample(t, *table) for t in tracks])
    return _SEAMS[(pair, ch)]


@pytest.mark.parametrize("path", ["pcm", "device"])
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("pair", PAIRS)
def test_seams_and_the_track_search(span, pair, ch, kind, path):
    rs, table, tracks, want = seam_batch(span, pair, ch)
    outs = [st["frames_out"] for _, st in want]
    assert outs[0] == outs[4] == outs[8] == 0 and outs[1] >= 1 and outs[3] >= span - 1 and outs[7] >= 3 * span + 5
    if pair[0] > pair[1]:  # going down every length is reachable
        assert outs == [0, 1, table[2], span - 1, 0, span, span + 1, 3 * span + 5, 0]
    check_batch(tracks, rs, table, want, f32s=(kind == "f32",), paths=(path,))
    assert max(max(st["peak"]) for _, st in want) > 1036


# ------------------------------------------------------------------ 2. no frame of a neighbour
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("pair", [(96000, 44100), (44100, 48000)])
def test_no_frame_of_a_neighbour_is_read_or_written(span, pair, ch, kind):
    """Silent tracks between full-scale square waves that end and begin at their borders, all
    packed back to back in one allocation: a silent track's output is all zero, and the loud
    tracks' ends are the zero-padded definition's, not a continuation into the neighbour."""
    rs, table = planned(*pair)
    L, M, K, _ = table

    def square(n):
        sq = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
        return np.stack([sq, -1 - sq], axis=1) if ch == 2 else sq

    def silent(n):
        return np.zeros((n, 2) if ch == 2 else (n,), np.int16)

    n_loud = smallest_input(span + 9, L, M)[0]
    tracks = [square(n_loud), silent(5), square(n_loud), silent(smallest_input(span + 3, L, M)[0]), square(n_loud)]
    got, st = batch_device(tracks, rs, kind == "f32")
    want = [ref_resample(t, *table) for t in tracks]
    for t in (1, 3):
        assert not got[t].any() and st[t]["peak"] == st[t]["clipped"] == [0] * ch, t
        assert st[t] == want[t][1]
    for t in (0, 2, 4):
        assert np.array_equal(got[t][:K // 2], want[t][0][:K // 2]), t
        assert np.array_equal(got[t][-(K // 2):], want[t][0][-(K // 2):]), t
        assert np.array_equal(got[t], want[t][0]) and st[t] == want[t][1], t
        assert max(st[t]["peak"]) == 32768


# ------------------------------------------------------------------ 3. statistics stay per track
@pytest.mark.parametrize("path", ["pcm", "device"])
@pytest.mark.parametrize("pair", [(96000, 44100), (44100, 48000)])
def test_statistics_stay_per_track(span, pair, path):
    rs, table = planned(*pair)
    rng = np.random.default_rng(pair[1])
    n = 3 * span
    sq = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    quiet = [rng.integers(-1036, 1037, (m, 2)).astype(np.int16) for m in (2 * span + 11, span + 1)]
    for ch in (1, 2):  # (stereo: the clipping track's left channel is silent)
        loud = np.stack([np.zeros(n, np.int16), sq], axis=1) if ch == 2 else sq
        tracks = [quiet[0] if ch == 2 else quiet[0][:, 0], loud, quiet[1] if ch == 2 else quiet[1][:, 1]]
        want = check_batch(tracks, rs, table, f32s=(False,), paths=(path,))
        assert want[1][1]["clipped"][ch - 1] > 0 and want[1][1]["peak"][ch - 1] == 32768
        assert want[0][1]["clipped"] == want[2][1]["clipped"] == [0] * ch
        assert max(want[0][1]["peak"] + want[2][1]["peak"]) < 2000
        if ch == 2:
            assert want[1][1]["clipped"][0] == 0 and want[1][1]["peak"][0] == 0


# ------------------------------------------------------------------ 4. spans staged in pieces
@pytest.mark.parametrize("ch", [1, 2])
def test_spans_staged_in_pieces(span, ch):
    """A ratio steeper than 8: a workgroup stages its span in several pieces, in every track."""
    L, M, K = 3, 40, 6
    rng = np.random.default_rng(L * M + K)
    c = rng.integers(-(1 << 20), 1 << 20, (L, K))
    c[:, 0] += ONE - c.sum(axis=1)
    rs = resampler(1000 * M, 1000 * L, L, M, K, c)
    tracks = []
    for size in (2 * span + 3, 1, span + 1):
        pcm = rng.integers(-32768, 32768, (smallest_input(size, L, M)[0], ch)).astype(np.int16)
        tracks.append(pcm if ch == 2 else pcm[:, 0])
    want = check_batch(tracks, rs, (L, M, K, c), f32s=(False,))
    assert [st["frames_out"] for _, st in want] == [2 * span + 3, 1, span + 1]
    h, hst = host_resample(tracks[2], rs)  # the library's host restatement agrees with the reference
    assert np.array_equal(h, want[2][0]) and hst == want[2][1]


# ------------------------------------------------------------------ 5. launch structure
def test_one_launch_whatever_the_track_count(span):
    from mastering_amd import native
    rs, table = planned(96000, 44100)
    rng = np.random.default_rng(5)
    ctx = native.context(0)

    def launches(tracks):
        ctx.timing(False)
        ctx.timing(True)
        batch_device(tracks, rs)
        stats = ctx.kernel_stats()
        ctx.timing(False)
        return stats

    for n in (2, 9):
        stats = launches([rng.integers(-3000, 3000, (700 + 400 * t, 2)).astype(np.int16) for t in range(n)])
        assert stats["resample_tracks"][1] == 1 and "resample" not in stats, (n, stats)
    stats = launches([np.zeros((0, 2), np.int16)] * 3)
    assert "resample_tracks" not in stats and "resample" not in stats, stats


# ------------------------------------------------------------------ 6. arguments
def test_arguments(span):
    from mastering_amd import engine, native
    rs, table = planned(96000, 44100)
    L, M, K, c = table
    pcm = np.zeros((64, 2), np.int16)
    with pytest.raises(ValueError, match=r"0 tracks out of range \[1, 256\]"):
        batch_device([pcm], rs, n=0)
    with pytest.raises(ValueError, match=r"257 tracks out of range \[1, 256\]"):
        batch_device([pcm] * 257, rs)
    with pytest.raises(ValueError, match="kind 7"):
        batch_device([pcm, pcm], rs, kind=7)
    with pytest.raises(ValueError, match="track 0"):
        batch_device([pcm, pcm], rs, ch=3)
    for bad in (resampler(96000, 44100, L, M, K - 1, c), resampler(96000, 96000, L, L, K, c),
                resampler(96000, 48000, L, M, K, c), resampler(96000, 44100, L, M, K, c.astype(np.int64) * 8)):
        with pytest.raises(ValueError, match="resampler"):
            batch_device([pcm, pcm], bad)
        with pytest.raises(ValueError, match="resampler"):
            batch_pcm([pcm, pcm], bad)
    with pytest.raises(ValueError, match="1 to 256 tracks, not 0"):
        engine.resample_batch_pcm([], 96000, 44100)
    with pytest.raises(ValueError, match="one channel count"):
        engine.resample_batch_pcm([pcm, pcm[:, 0]], 96000, 44100)
    with pytest.raises(ValueError):
        engine.resample_batch_pcm([pcm], 96000, 44101)
    # the context is still usable: an ordinary conversion right afterwards is correct
    x = np.random.default_rng(6).integers(-20000, 20000, (3000, 2)).astype(np.int16)
    out, d = engine.resample_pcm(x, 96000, 44100)
    want, st = ref_resample(x, *table)
    assert np.array_equal(out, want) and {k: d[k] for k in st} == st


def test_resample_batch_pcm_is_the_reference():
    from mastering_amd import design, engine
    from mastering_amd.synth import pink_noise_pcm16
    tracks = [pink_noise_pcm16(n, 48000, 2, track=7 + i, level_dbfs=-9.0) for i, n in enumerate((5000, 1, 2600))]
    tracks.insert(1, np.zeros((0, 2), np.int16))
    table = design.resample_taps(48000, 44100)
    outs, ds = engine.resample_batch_pcm(tracks, 48000, 44100)
    outs_f, ds_f = engine.resample_batch_pcm([t.astype(np.float32) / np.float32(32768) for t in tracks], 48000, 44100)
    for t, x in enumerate(tracks):
        want, st = ref_resample(x, *table)
        assert outs[t].dtype == np.int16 and outs[t].shape == want.shape and np.array_equal(outs[t], want)
        assert {k: ds[t][k] for k in st} == st and (ds[t]["rate_in"], ds[t]["rate_out"]) == (48000, 44100)
        assert outs_f[t].dtype == np.float32 and np.array_equal(outs_f[t] * np.float32(32768), want) and ds_f[t] == ds[t]
        if len(x):
            single, d1 = engine.resample_pcm(x, 48000, 44100)
            assert np.array_equal(single, outs[t]) and d1 == ds[t]


# ------------------------------------------------------------------ 7. the taps cache
def test_taps_cache_is_shared_with_the_single_track_entry(span):
    """A batch call after a single-track call of another pair is right, and so is the
    single-track call after the batch; a table without a key is uploaded every time."""
    from test_gpu_resample import dev_resample
    from mastering_amd.synth import pink_noise_pcm16
    tracks = [pink_noise_pcm16(n, 96000, 2, track=5 + i, level_dbfs=-12.0) for i, n in enumerate((4000, 2500))]
    a, ta = planned(96000, 44100)
    b, tb = planned(96000, 48000)
    got, st = dev_resample(tracks[0], a)
    assert np.array_equal(got, ref_resample(tracks[0], *ta)[0])
    check_batch(tracks, b, tb, f32s=(False,), paths=("device",))       # another pair than the cached one
    got, st = dev_resample(tracks[0], a)                               # and the first pair after the batch
    assert np.array_equal(got, ref_resample(tracks[0], *ta)[0])
    check_batch(tracks, a, ta, f32s=(False,), paths=("device",))       # the cached pair, from the single-track call
    L, M, K, c = tb
    flipped = np.ascontiguousarray(c[:, ::-1])  # another table of the same geometry, no key
    check_batch(tracks, resampler(96000, 48000, L, M, K, flipped), (L, M, K, flipped), f32s=(False,), paths=("device",))
    check_batch(tracks, b, tb, f32s=(False,), paths=("device",))
