"""An album levelled as one programme, on the GPU: the segmented K-weighting pass's hop energies
(mm_op_r128_album_hops) against the host restatement and, bit for bit, against the single-track
pass on every track alone, at the sizes where the layout can go wrong (a partial tile, a track
of one frame, a track of exactly one workgroup and one frame more, a predecessor whose filter
state is far from zero at its end); the album level against mm_album_level_host on the albums
whose decision margins tests/test_album.py asserts; the launch count; the album at the end of
a batch and of the file path; the refusals."""
import ctypes

import numpy as np
import pytest

from test_album import NAMES, RATE, STATUS, case_inputs, host_album_level
from test_gpu_r128 import TOL, gpu_hops, long_carry
from test_r128 import design_rate, host_r128, stepped_noise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def span():
    from mastering_amd import native
    return native.load().mm_r128_span()


def album_hops(tracks, rate, f32=False):
    """The segmented pass's hop energies of int16 `tracks` (or of tracks / 32768 as MM_OUT_F32
    buffers), one array a track."""
    from mastering_amd import engine, native
    xs = [np.ascontiguousarray(t, np.int16) for t in tracks]
    host = [x.astype(np.float32) / np.float32(32768) if f32 else x for x in xs]
    n = len(xs)
    H = [10 * x.shape[0] // rate for x in xs]
    e = np.full(sum(H) + 1, -1.0)
    ptrs = (ctypes.c_void_p * n)(*[ctypes.c_void_p(h.ctypes.data) for h in host])
    frames = (ctypes.c_int64 * n)(*[x.shape[0] for x in xs])
    ctx = native.context(0)
    got = ctx.check(ctx.lib.mm_op_r128_album_hops(ctx.ptr, ptrs, native.MM_OUT_F32 if f32 else native.MM_OUT_I16, frames, n,
                                                  1 if xs[0].ndim == 1 else xs[0].shape[1], rate,
                                                  engine.kweight_sos(design_rate(rate)), e.ctypes.data_as(native.c_double_p),
                                                  sum(H)), "mm_op_r128_album_hops")
    assert got == sum(H) and e[sum(H)] == -1.0
    return np.split(e[:sum(H)], np.cumsum(H)[:-1])


def hop_albums(span):
    tile = span // 256
    floor = [tile - 1, 1, 6001, span, span + 1, 800, 799]
    return {
        "floor-stereo": (2000, [stepped_noise(n, 2000, 2, seed=11 + t) for t, n in enumerate(floor)]),
        "floor-mono": (2000, [stepped_noise(n, 2000, 1, seed=11 + t) for t, n in enumerate(floor)]),
        "44k": (44100, [stepped_noise(n, 44100, 2, seed=21 + t) for t, n in enumerate([321987, 30000, 44100])]),
        "carry": (44100, [long_carry(2 * span + 17, 44100), stepped_noise(span + 5, 44100, 2)]),
    }


@pytest.mark.parametrize("name", ["floor-stereo", "floor-mono", "44k", "carry"])
def test_segmented_hops(span, name):
    rate, tracks = hop_albums(span)[name]
    e = album_hops(tracks, rate)
    assert [len(x) for x in e] == [10 * len(t) // rate for t in tracks]
    for t, (pcm, et) in enumerate(zip(tracks, e)):
        ref, _ = host_r128(pcm, rate)
        dev = float(np.max(np.abs(et - ref) / ref)) if len(et) else 0.0
        print(f"album hop energies {name} track {t}: {len(pcm)} frames, {len(et)} hops, largest relative deviation {dev:.3e}")
        assert np.all(np.isfinite(et)) and dev <= TOL, t
        # the layout's promise: a track's hops are the single-track pass's of that track alone
        assert np.array_equal(et, gpu_hops(pcm, rate)), t
    again = album_hops(tracks, rate)
    assert all(np.array_equal(a, b) for a, b in zip(again, e))  # two runs are bit-identical (no atomics)
    if name == "floor-stereo":  # the decoded doubles of the f32 buffers are equal
        f = album_hops(tracks, rate, f32=True)
        assert all(np.array_equal(a, b) for a, b in zip(f, e))


def test_album_r128_pcm_pools_the_tracks(span):
    from mastering_amd import album_r128_pcm, engine, native
    from test_album import album_from_hops
    rate, tracks = hop_albums(span)["44k"]
    d = album_r128_pcm(tracks, rate)
    want = engine.r128_dict(album_from_hops(album_hops(tracks, rate), rate))
    assert d == want and d["hops"] == sum(10 * len(t) // rate for t in tracks)
    rs = engine.r128s(native.context(0), len(tracks))
    assert [engine.r128_dict(r) for r in rs] == [engine.r128_pcm(t, rate) for t in tracks]
    assert [(r.frames, r.channels) for r in rs] == [(len(t), 2) for t in tracks]


# ------------------------------------------------------------------ the album level against the host
@pytest.fixture(scope="module")
def host_results():
    """mm_album_level_host of every case (shared, read-only); the decision margins of the cases
    are asserted in tests/test_album.py."""
    out = {}
    for name, (tracks, T, C, W, status, passes) in case_inputs().items():
        y, m, alb, tr, ce = host_album_level(tracks, RATE, T, C, W)
        assert m.status == STATUS[status] and m.passes == passes, name
        out[name] = ((tracks, T, C, W), y, m, alb, tr, ce)
    return out


def check_r128(got, want):
    """A report dict of the device against the host's struct: counts equal, figures within 1e-6."""
    from mastering_amd import engine
    w = engine.r128_dict(want)
    for k, v in w.items():
        if isinstance(v, int):
            assert got[k] == v, k
        else:
            assert (got[k] is None and v is None) or abs(got[k] - v) <= 1e-6, k


@pytest.mark.parametrize("name", NAMES)
def test_album_level_pcm_is_the_host_restatement(host_results, name):
    from mastering_amd import album_level_pcm, engine, native
    (tracks, T, C, W), want, hm, halb, htr, hce = host_results[name]
    got, d = album_level_pcm(tracks, RATE, T, ceiling_dbtp=-1.0 if C else None, window=W)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    hd = engine.level_dict(hm)
    for k in ("frames", "channels", "rate", "target_clu", "ceiling_q28", "window", "passes", "gain_q16", "min_gain_q16",
              "clipped", "limited_frames", "status", "pass_gain_q16"):
        assert d[k] == hd[k], k
    for a, b in zip(d["pass_lufs"], hd["pass_lufs"]):
        assert abs(a - b) <= 1e-6
    for k in ("source_lufs", "loudness"):
        assert (d[k] is None and hd[k] is None) or abs(d[k] - hd[k]) <= 1e-6, k
    check_r128(d["r128"], halb)
    assert len(d["tracks"]) == len(tracks)
    for t, rep in enumerate(d["tracks"]):
        check_r128(rep["r128"], htr[t])
        assert ("ceiling" in rep) == bool(C)
        if C:
            assert all(rep["ceiling"][f] == getattr(hce[t], f) for f, _ in native.MMCeiling._fields_), t
            assert rep["ceiling"]["tp_out_q28"] <= C
    again, d2 = album_level_pcm(tracks, RATE, T, ceiling_dbtp=-1.0 if C else None, window=W)
    assert all(np.array_equal(a, g) for a, g in zip(again, got)) and d2 == d  # a second run: bit for bit


@pytest.fixture(scope="module")
def fates_host():
    """mm_album_level_host of the album of tests/test_album.py's album_fates (shared, read-only);
    what the album is made of and its decision margins are asserted there."""
    from test_album import album_fates
    tracks, rate, T, C, W = album_fates()
    return (tracks, rate, T, C, W), host_album_level(tracks, rate, T, C, W)


@pytest.mark.parametrize("f32", [False, True], ids=["i16", "f32"])
def test_tracks_of_different_fates_in_one_pass(fates_host, f32):
    """Through the segmented ceilings in one launch: a track the inner ceiling limits, one it
    does not touch (ceil_tracks_peak skips it), one with a span seam three frames before its
    end, one without a window of its own and an empty one, in every pass of a boosting album."""
    from mastering_amd import album_level_pcm, engine, native
    from test_gpu_level import as_kind, to_i16
    (tracks, rate, T, C, W), (want, hm, halb, htr, hce) = fates_host
    got, d = album_level_pcm([as_kind(t, f32) for t in tracks], rate, T, ceiling_dbtp=-1.0, window=W)
    assert all(np.array_equal(to_i16(g), w) for g, w in zip(got, want))
    hd = engine.level_dict(hm)
    for k in ("frames", "channels", "rate", "target_clu", "ceiling_q28", "window", "passes", "gain_q16", "min_gain_q16",
              "clipped", "limited_frames", "status", "pass_gain_q16"):
        assert d[k] == hd[k], k
    for a, b in zip(d["pass_lufs"], hd["pass_lufs"]):
        assert abs(a - b) <= 1e-6
    assert abs(d["source_lufs"] - hd["source_lufs"]) <= 1e-6 and abs(d["loudness"] - hd["loudness"]) <= 1e-6
    check_r128(d["r128"], halb)
    assert len(d["tracks"]) == len(tracks) == 5
    for t, rep in enumerate(d["tracks"]):
        check_r128(rep["r128"], htr[t])
        assert all(rep["ceiling"][f] == getattr(hce[t], f) for f, _ in native.MMCeiling._fields_), t


@pytest.mark.parametrize("name,track", [("cut", 0), ("boost-2", 0), ("no-ceiling", 2), ("unmeasurable", 0)])
def test_one_track_is_level_pcm(host_results, name, track):
    from mastering_amd import album_level_pcm, engine
    (tracks, T, C, W), *_ = host_results[name]
    pcm = tracks[track]
    want, dw = engine.level_pcm(pcm, RATE, T, ceiling_dbtp=-1.0 if C else None, window=W)
    got, d = album_level_pcm([pcm], RATE, T, ceiling_dbtp=-1.0 if C else None, window=W)
    assert np.array_equal(got[0], want)
    assert {k: d[k] for k in dw} == dw  # every mm_level field, bit for bit
    assert d["r128"] == d["tracks"][0]["r128"] == engine.r128_pcm(want, RATE)


def test_the_balance_between_the_tracks_is_kept(host_results):
    """Case "cut": the limiter is idle, so every track moves by the one gain."""
    from mastering_amd import album_level_pcm, engine
    (tracks, T, C, W), _, hm, *_ = host_results["cut"]
    assert hm.limited_frames == 0
    before = [engine.r128_pcm(t, RATE)["integrated_lufs"] for t in tracks[:3]]
    _, d = album_level_pcm(tracks, RATE, T, ceiling_dbtp=-1.0, window=W)
    after = [t["r128"]["integrated_lufs"] for t in d["tracks"][:3]]
    assert d["tracks"][3]["r128"]["integrated_lufs"] is None  # (0.3 s: no window of its own)
    for a in range(3):
        for b in range(a):
            assert abs((after[a] - after[b]) - (before[a] - before[b])) <= 0.01, (a, b)
    assert abs(before[0] - before[1]) > 5.0  # (a loud opener and a quiet interlude)


def album_launches(tracks, T, W):
    """(album dict, kernel name -> launches) of one warm album_level_pcm under -1 dBTP."""
    from mastering_amd import album_level_pcm, native
    ctx = native.context(0)
    album_level_pcm(tracks, RATE, T, ceiling_dbtp=-1.0, window=W)  # (buffers and tables in place)
    ctx.timing(True)
    try:
        before = ctx.kernel_stats()
        _, d = album_level_pcm(tracks, RATE, T, ceiling_dbtp=-1.0, window=W)
        after = ctx.kernel_stats()
    finally:
        ctx.timing(False)
    return d, {k: v[1] - before.get(k, (0.0, 0))[1] for k, v in after.items() if v[1] != before.get(k, (0.0, 0))[1]}


def test_launch_count(host_results):
    """One segmented measuring launch for the source and one a pass; the per-track reports come
    from the same hop energies, so the single-track pass is never launched.  Nor is any other
    kernel of the single-track path, and no kernel is launched more often for more tracks: the
    album with every track listed twice launches what the album launches."""
    (tracks, T, C, W), *_ = host_results["boost-3"]
    d, count = album_launches(tracks, T, W)
    assert d["passes"] == 3
    assert count["r128_album_kweight"] == d["passes"] + 1 == count["r128_album_reduce"]
    for k in ("level_gain", "ceil_need", "ceil_apply", "ceil_trim", "meter_i16", "r128_kweight"):
        assert k not in count, k
    d2, count2 = album_launches(tracks + tracks, T, W)
    assert d2["passes"] == d["passes"]  # (twice the album has the album's loudness)
    print(count)
    for k in ("r128_album_kweight", "r128_album_reduce", "level_tracks_gain", "ceil_tracks_need", "ceil_tracks_apply",
              "ceil_tracks_peak"):
        assert count[k] == count2[k] > 0, k
    assert count == count2
    # what a pass queues, whatever n: the keep, then a pass's gain and its ceiling at C, and for a
    # boost the copy back and the inner ceiling before them
    boosts = sum(g > 65536 for g in d["pass_gain_q16"])
    assert boosts == d["passes"] and count["level_tracks_gain"] == 1 + d["passes"] + boosts
    assert count["ceil_tracks_need"] == count["ceil_tracks_apply"] == d["passes"] + boosts <= count["ceil_tracks_peak"]


# ------------------------------------------------------------------ at the end of a batch
P = {"multiband": True, "lufs": -14.0, "saturation": 20}


def test_master_album_is_the_batch_then_the_album_level():
    import torch
    from mastering_amd import Job, album_level_pcm, engine, master_album, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcms = [pink_noise_pcm16(30000, rate, 2, track=1), pink_noise_pcm16(41000, rate, 2, track=2, level_dbfs=-6.0)]

    def plan():
        jobs = [Job(len(p), rate, 2, P) for p in pcms]
        for j in jobs:
            j.job.in_kind = native.MM_IN_I16
        return jobs

    xs = [torch.from_numpy(p).cuda() for p in pcms]
    ctx = native.context(0)

    def outs_of(jobs):
        return [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]

    jobs = plan()
    plain = outs_of(jobs)
    torch.cuda.current_stream().synchronize()
    master_batch(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in plain])
    want, dw = album_level_pcm([o.cpu().numpy() for o in plain], rate, -16.0, ceiling_dbtp=-1.0)
    jobs = plan()
    outs = outs_of(jobs)
    torch.cuda.current_stream().synchronize()
    res, d = master_album(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs], -16.0, -1.0)
    assert len(res) == 2 and d == dw
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs, want))
    assert [engine.r128_dict(r) for r in engine.r128s(ctx, 2)] == [t["r128"] for t in d["tracks"]]
    assert [c.tp_out_q28 for c in engine.ceilings(ctx, 2)] == [t["ceiling"]["tp_out_q28"] for t in d["tracks"]]


def test_process_album_writes_the_levelled_files(tmp_path):
    from mastering_amd import album_r128_pcm, process_album, wavio
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcms = [pink_noise_pcm16(2 * rate, rate, 2, track=1), pink_noise_pcm16(rate, rate, 2, track=2, level_dbfs=-9.0)]
    ins, outs = [str(tmp_path / f"in{i}.wav") for i in range(2)], [str(tmp_path / f"out{i}.wav") for i in range(2)]
    for p, path in zip(pcms, ins):
        wavio.write_wav(path, p, rate)
    infos, album = process_album(ins, outs, dict(P, deliver_lufs=-16.0, ceiling_dbtp=-1.0))
    got = [wavio.read_wav(path) for path in outs]
    assert [r for _, r in got] == [rate, rate] and [len(y) for y, _ in got] == [i["frames"] for i in infos]
    assert album["r128"] == album_r128_pcm([y for y, _ in got], rate)
    assert album["status"] in ("reached", "saturated", "passes") and album["target_lufs"] == -16.0
    assert [i["output_path"] for i in infos] == outs and len(album["tracks"]) == 2


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable():
    from mastering_amd import Job, album_level_pcm, album_r128_pcm, engine, master_album, native
    ctx = native.context(0)
    st, mono = np.zeros((1000, 2), np.int16), np.zeros(1000, np.int16)
    jobs = [Job(44100, 44100, 2, P), Job(48000, 48000, 2, P)]
    with pytest.raises(ValueError, match="one sample rate"):
        master_album(ctx, jobs, [0, 0], [0, 0], -14.0)
    with pytest.raises(ValueError, match="one channel count"):
        album_level_pcm([st, mono], RATE, -14.0)
    with pytest.raises(ValueError, match="1 to 256 tracks, not 0"):
        album_level_pcm([], RATE, -14.0)
    with pytest.raises(ValueError, match="1 to 256 tracks, not 257"):
        album_level_pcm([st] * 257, RATE, -14.0)
    with pytest.raises(ValueError, match="outside"):
        album_level_pcm([st], RATE, -4.0)
    # the library's own sentences, raised before anything is queued
    sos, m = engine.kweight_sos(RATE), native.MMR128()
    ptrs, fr = (ctypes.c_void_p * 2)(st.ctypes.data, st.ctypes.data), (ctypes.c_int64 * 2)(1000, 1000)
    I16 = native.MM_OUT_I16
    for call, words in (
            (lambda: ctx.lib.mm_album_level_pcm(ctx.ptr, ptrs, I16, fr, 0, 2, RATE, sos, -1400, 0, 220), "0 tracks out of range"),
            (lambda: ctx.lib.mm_album_level_pcm(ctx.ptr, ptrs, I16, fr, 257, 2, RATE, sos, -1400, 0, 220), "257 tracks out of range"),
            (lambda: ctx.lib.mm_album_level_pcm(ctx.ptr, ptrs, I16, fr, 2, 2, RATE, sos, -400, 0, 220), "level_clu out of range"),
            (lambda: ctx.lib.mm_album_level_pcm(ctx.ptr, ptrs, I16, fr, 2, 3, RATE, sos, -1400, 0, 220), "track 0: channels must be 1 or 2"),
            (lambda: ctx.lib.mm_album_level_pcm(ctx.ptr, ptrs, I16, fr, 2, 2, 1999, sos, -1400, 0, 220), "rate below 2000"),
            (lambda: ctx.lib.mm_album_level_pcm(ctx.ptr, ptrs, 7, fr, 2, 2, RATE, sos, -1400, 0, 220), "kind 7"),
            (lambda: ctx.lib.mm_album_level_pcm(ctx.ptr, ptrs, I16, fr, 2, 2, RATE, sos, -1400, 1, 220), "track 0: ceiling_q28 out of range"),
            (lambda: ctx.lib.mm_album_r128_pcm(ctx.ptr, ptrs, I16, (ctypes.c_int64 * 2)(1000, -1), 2, 2, RATE, sos, ctypes.byref(m)),
             "track 1: frames out of range")):
        with pytest.raises(ValueError, match=words):
            ctx.check(call(), "album")
    with pytest.raises(RuntimeError, match="levelled no album"):
        ctx.check(ctx.lib.mm_album_r128_pcm(ctx.ptr, ptrs, I16, fr, 2, 2, RATE, sos, ctypes.byref(m)), "mm_album_r128_pcm")
        ctx.check(ctx.lib.mm_last_album(ctx.ptr, ctypes.byref(native.MMLevel()), ctypes.byref(m)), "mm_last_album")
    # the next call on the same context succeeds
    tracks = case_inputs()["cut"][0]
    _, d = album_level_pcm(tracks, RATE, -15.0, ceiling_dbtp=-1.0)
    assert d["status"] == "reached" and d["passes"] == 1
    assert album_r128_pcm(tracks, RATE)["hops"] == sum(10 * len(t) // RATE for t in tracks)
