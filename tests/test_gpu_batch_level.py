"""The batch level on the GPU (csrc/tracks.hip: mm_batch_level_*): every track of a batch to its
own R 128 target under its own ceiling, the passes of all tracks in lockstep and every launch
over all tracks, against the host restatement mm_level_host run on every track alone
(bit-identical samples, equal integers) and against level_pcm on that track alone (the whole
mm_level, bit for bit).  The inputs are the cases of tests/test_level.py, whose decision margins
(at least 1e-3 LU, slopes at least 0.01) are asserted there on the numpy reference, so that no
decision of the rule can turn on the 1e-6 LU by which two correct meters may differ."""
import ctypes

import numpy as np
import pytest

from test_ceiling import ceiling_stats, q28
from test_gpu_level import dev_level, to_i16
from test_level import STATUS, TOL, case_inputs, host_level, level_ints

pytestmark = pytest.mark.gpu

RATE = 44100
STEREO = ["down", "up-idle", "stepped", "saturated", "capped", "no-ceiling"]
P = {"multiband": True, "lufs": -14.0, "saturation": 20}


def raw(m):
    return ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m))


def batch_level(tracks, rate, Ts, Cs, W, f32=False):
    """mm_batch_level_pcm on copies of int16 `tracks` (or of tracks / 32768 as f32): (the tracks
    afterwards as int16, [mm_level], [mm_ceiling] or None, [mm_r128])."""
    from mastering_amd import design, engine, native
    ctx = native.context(0)
    n = len(tracks)
    xs = [np.ascontiguousarray(t, np.int16) for t in tracks]
    ch = 1 if xs[0].ndim == 1 else xs[0].shape[1]
    host = [x.astype(np.float32) / np.float32(32768) if f32 else x.copy() for x in xs]
    frames = (ctypes.c_int64 * n)(*[x.shape[0] for x in xs])
    clu = (ctypes.c_int32 * n)(*[design.level_clu(T) for T in Ts])
    C = (ctypes.c_int32 * n)(*Cs)
    ctx.check(ctx.lib.mm_batch_level_pcm(ctx.ptr, engine._pointers([h.ctypes.data for h in host]),
                                         native.MM_OUT_F32 if f32 else native.MM_OUT_I16, frames, n, ch, rate,
                                         engine.kweight_sos(rate), clu, C, W), "mm_batch_level_pcm")
    return ([to_i16(h) for h in host], engine.levels(ctx, n), engine.ceilings(ctx, n) if any(Cs) else None,
            engine.r128s(ctx, n))


def close(a, b):
    return (a == b) or (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-6


def check_track(got, m, ce, want, hm, hce, C):
    """One track of a batch against mm_level_host of that track alone."""
    assert np.array_equal(got, want)
    assert level_ints(m) == level_ints(hm)
    assert close(m.source_lufs, hm.source_lufs) and close(m.loudness, hm.loudness)
    for k in range(m.passes):
        assert close(m.pass_lufs[k], hm.pass_lufs[k])
    if C:
        assert ceiling_stats(ce) == ceiling_stats(hce) and ce.tp_out_q28 <= C
    elif ce is not None:
        assert ce.frames == 0 and ce.ceiling_q28 == 0 and ce.channels == m.channels  # a cleared entry


@pytest.fixture(scope="module")
def inputs():
    from mastering_amd.synth import pink_noise_pcm16
    c = case_inputs()
    c["short"] = (pink_noise_pcm16(17000, RATE, 1, track=5, level_dbfs=-12.0), RATE, -14.0, q28(-1.0), 220, "unmeasurable", 0)
    return c


@pytest.fixture(scope="module")
def host(inputs):
    """mm_level_host of every case used here, and of the mono cases at W = 1 (shared, read-only)."""
    from mastering_amd import native
    out = {}
    for name in STEREO + ["mono-boost", "short"]:
        for W in ((220, 1) if name in ("mono-boost", "short") else (220,)):
            pcm, rate, T, C, _, status, passes = inputs[name]
            ce = native.MMCeiling()
            y, m = host_level(pcm, rate, T, C, W, ce)
            assert m.status == STATUS[status] and (W == 1 or passes is None or m.passes == passes), name
            out[name, W] = (y, m, ce)
    return out


@pytest.fixture(scope="module")
def stereo_run(inputs):
    """The stereo batch, levelled once with timing on: (results, kernel statistics)."""
    from mastering_amd import native
    ctx = native.context(0)
    ctx.timing(True)
    try:
        res = batch_level([inputs[k][0] for k in STEREO], RATE, [inputs[k][2] for k in STEREO],
                          [inputs[k][3] for k in STEREO], 220)
        return res, ctx.kernel_stats()
    finally:
        ctx.timing(False)


def test_the_stereo_batch_is_the_host_restatement_per_track(inputs, host, stereo_run):
    """A cut, a boost reached in one pass, a track of two passes, saturated, capped under a ceiling
    and capped without one in ONE call: tracks leave after pass 1 and after pass 2, and cut-branch
    and boost-branch tracks share a pass."""
    (got, lv, ce, rs), _ = stereo_run
    for i, name in enumerate(STEREO):
        want, hm, hce = host[name, 220]
        check_track(got[i], lv[i], ce[i], want, hm, hce, inputs[name][3])
    assert [m.passes for m in lv] == [1, 1, 2, 2, 1, 1]
    assert [m.status for m in lv] == [STATUS[s] for s in ("reached", "reached", "reached", "saturated", "capped", "capped")]
    assert lv[0].gain_q16 < 65536 < lv[1].gain_q16  # a cut and a boost in pass 1


@pytest.mark.parametrize("f32", [False, True], ids=["i16", "f32"])
@pytest.mark.parametrize("W", [220, 1])
def test_the_mono_batch(inputs, host, W, f32):
    """Three passes next to a track too short to measure, which only gets its ceiling."""
    names = ["mono-boost", "short"]
    got, lv, ce, rs = batch_level([inputs[k][0] for k in names], RATE, [inputs[k][2] for k in names],
                                  [inputs[k][3] for k in names], W, f32)
    for i, name in enumerate(names):
        want, hm, hce = host[name, W]
        check_track(got[i], lv[i], ce[i], want, hm, hce, inputs[name][3])
    assert lv[1].status == STATUS["unmeasurable"] and lv[1].passes == 0 and rs[1].hops == 3
    if W == 220:
        assert lv[0].passes == 3


def test_every_track_is_level_pcm_on_that_track_alone(inputs, stereo_run):
    """A track's result does not depend on its neighbours in the launch: the whole mm_level and
    level_dict bit for bit, and the R 128 report of the delivered samples, against the same driver
    run on that track alone.  (The oracle is the host comparison in check_track.)"""
    from mastering_amd import engine, level_batch_pcm
    (got, lv, ce, rs), _ = stereo_run
    dbs = [None if inputs[k][3] == 0 else -1.0 for k in STEREO]
    outs, ds = level_batch_pcm([inputs[k][0] for k in STEREO], RATE, [inputs[k][2] for k in STEREO], dbs)
    for i, name in enumerate(STEREO):
        pcm, rate, T, C, W, _, _ = inputs[name]
        y, m, c1 = dev_level(pcm, rate, T, C, W)
        assert np.array_equal(got[i], y) and np.array_equal(outs[i], y)
        assert raw(lv[i]) == raw(m)
        if C:
            assert raw(ce[i]) == raw(c1)
        d = dict(ds[i])
        r128, ceiling = d.pop("r128"), d.pop("ceiling", None)
        assert d == engine.level_dict(m)
        assert r128 == engine.r128_dict(rs[i]) == engine.r128_pcm(y, rate)
        assert (ceiling is not None) == bool(C) and (not C or ceiling == engine.ceiling_dict(c1))


def test_launches_do_not_depend_on_n(inputs, host, stereo_run):
    """The same batch with every track listed twice: every kernel is launched as often, and no
    per-track kernel of the single-track path is launched at all."""
    from mastering_amd import native
    (got, _, _, _), stats = stereo_run
    names = STEREO + STEREO
    ctx = native.context(0)
    ctx.timing(True)
    try:
        got2, lv2, ce2, rs2 = batch_level([inputs[k][0] for k in names], RATE, [inputs[k][2] for k in names],
                                          [inputs[k][3] for k in names], 220)
        stats2 = ctx.kernel_stats()
    finally:
        ctx.timing(False)
    print({k: v[1] for k, v in stats.items()})
    assert {k: v[1] for k, v in stats.items()} == {k: v[1] for k, v in stats2.items()}
    for k in ("ceil_need", "ceil_apply", "ceil_trim", "level_gain", "r128_kweight", "meter_i16"):
        assert k not in stats and k not in stats2
    for k in ("ceil_tracks_need", "ceil_tracks_apply", "ceil_tracks_peak", "level_tracks_gain", "r128_album_kweight"):
        assert stats[k][1] > 0
    for i, name in enumerate(names):  # and a second run, as twice the batch, gives the same bits
        assert np.array_equal(got2[i], got[i % len(STEREO)])
        check_track(got2[i], lv2[i], ce2[i], *host[name, 220], inputs[name][3])


def test_misaligned_views():
    """mm_batch_level_device on torch views one sample past a 16-byte boundary (the kept sources
    then sit at that offset too): the head and tail single samples of the segmented gain, which a
    track's own first workgroup handles.  5 samples, mm_level_span() + 3 samples and a 3 s track, mono
    at 8 kHz, where the middle one is long enough to be measured.  (A source that does not share its
    destination's offset cannot be reached through the batch level; that path of the shared body is
    covered by tests/test_gpu_level.py on level_gain.)"""
    import torch
    from mastering_amd import design, engine, native
    from mastering_amd.synth import pink_noise_pcm16
    rate, W, C = 8000, 40, q28(-1.0)
    span = native.load().mm_level_span()
    tracks = [pink_noise_pcm16(n, rate, 1, track=60 + i, level_dbfs=-18.0) for i, n in enumerate((5, span + 3, 3 * rate))]
    Ts = [-14.0, -15.0, -13.0]
    bufs = [torch.zeros(len(t) + 16, dtype=torch.int16, device="cuda") for t in tracks]
    views = [b[1:1 + len(t)] for b, t in zip(bufs, tracks)]
    for v, t in zip(views, tracks):
        v.copy_(torch.from_numpy(t))
        assert v.data_ptr() % 16 == 2
    torch.cuda.current_stream().synchronize()
    ctx = native.context(0)
    n = len(tracks)
    ctx.check(ctx.lib.mm_batch_level_device(ctx.ptr, engine._pointers([v.data_ptr() for v in views]), native.MM_OUT_I16,
                                            (ctypes.c_int64 * n)(*[len(t) for t in tracks]), n, 1, rate,
                                            engine.kweight_sos(rate), (ctypes.c_int32 * n)(*[design.level_clu(T) for T in Ts]),
                                            (ctypes.c_int32 * n)(*[C] * n), W), "mm_batch_level_device")
    lv, ce = engine.levels(ctx, n), engine.ceilings(ctx, n)
    for i, t in enumerate(tracks):
        hce = native.MMCeiling()
        want, hm = host_level(t, rate, Ts[i], C, W, hce)
        check_track(views[i].cpu().numpy(), lv[i], ce[i], want, hm, hce, C)
        b = bufs[i].cpu().numpy()
        assert b[0] == 0 and not b[1 + len(t):].any()  # nothing outside the view is written
    assert lv[0].status == STATUS["unmeasurable"] and lv[1].passes >= 1 and lv[2].passes >= 1


@pytest.fixture(scope="module")
def delivered():
    """Three 3 s pink tracks mastered as a batch and delivered to three targets under -1 dBTP."""
    import torch
    from mastering_amd import Job, deliver_batch, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16
    pcms = [pink_noise_pcm16(3 * RATE, RATE, 2, track=20 + i) for i in range(3)]
    targets = (-14.0, -16.0, -11.0)
    ctx = native.context(0)

    def run(deliver):
        jobs = [Job(len(p), RATE, 2, P) for p in pcms]
        for j in jobs:
            j.job.in_kind = native.MM_IN_I16
        xs = [torch.from_numpy(p).cuda() for p in pcms]
        outs = [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]
        torch.cuda.current_stream().synchronize()
        ins, ptrs = [x.data_ptr() for x in xs], [o.data_ptr() for o in outs]
        lv = None
        if deliver:
            lv = deliver_batch(ctx, jobs, ins, ptrs, targets, -1.0)[1]
        else:
            master_batch(ctx, jobs, ins, ptrs)
        return [o.cpu().numpy() for o in outs], lv

    plain, _ = run(False)
    outs, lv = run(True)
    return pcms, targets, plain, outs, lv


def test_deliver_batch_is_master_batch_then_the_batch_level(delivered):
    from mastering_amd import level_batch_pcm, meter_pcm
    pcms, targets, plain, outs, lv = delivered
    want, ds = level_batch_pcm(plain, RATE, targets, -1.0)
    for y, w, d, e, T in zip(outs, want, lv, ds, targets):
        assert y.tobytes() == w.tobytes() and d == e
        assert d["status"] != "unmeasurable" and (abs(d["loudness"] - T) <= TOL or d["status"] != "reached")
        assert d["r128"]["integrated_lufs"] == d["loudness"] and d["ceiling"]["tp_out_q28"] <= q28(-1.0)
        assert max(meter_pcm(y, RATE, loudness=False)["true_peak_q28"]) <= q28(-1.0)
    assert [d["target_lufs"] for d in lv] == list(targets)


def test_process_batch_writes_the_same_samples(delivered, tmp_path):
    from mastering_amd import process_batch, wavio
    pcms, targets, plain, outs, lv = delivered
    ins = [str(tmp_path / f"in{i}.wav") for i in range(3)]
    dst = [str(tmp_path / f"out{i}.wav") for i in range(3)]
    for p, x in zip(ins, pcms):
        wavio.write_wav(p, x, RATE)
    infos = process_batch(ins, dst, dict(P, deliver_lufs=list(targets), ceiling_dbtp=-1.0))
    for p, y, info, d in zip(dst, outs, infos, lv):
        got, rate = wavio.read_wav(p)
        assert rate == RATE and np.array_equal(got, y) and info["level"] == d


def test_refusals_name_the_track_and_leave_the_context_usable(inputs, host):
    from mastering_amd import native
    pcm = inputs["down"][0]
    C = q28(-1.0)
    for Ts, Cs, W, words in (([-14.0, -4.0], [C, C], 220, None), ([-14.0, -14.0], [C, 2 ** 28 + 1], 220, "track 1: ceiling_q28"),
                             ([-14.0, -14.0], [C, 0], 0, "track 0: ceiling window")):
        with pytest.raises(ValueError, match=words):
            batch_level([pcm, pcm], RATE, Ts, Cs, W)
    ctx, lib = native.context(0), native.load()
    from mastering_amd import engine
    fr, clu, Cq = (ctypes.c_int64 * 2)(100, 100), (ctypes.c_int32 * 2)(-1400, -400), (ctypes.c_int32 * 2)(C, C)
    ptr = (ctypes.c_void_p * 2)(pcm.ctypes.data, pcm.ctypes.data)
    sos = engine.kweight_sos(RATE)
    assert lib.mm_batch_level_pcm(ctx.ptr, ptr, 0, fr, 2, 2, RATE, sos, clu, Cq, 220) == native.MM_ERR_ARG
    assert b"batch: track 1: level_clu out of range" in lib.mm_last_error(ctx.ptr)
    clu[1] = -1400
    for n in (0, 257):
        assert lib.mm_batch_level_pcm(ctx.ptr, ptr, 0, fr, n, 2, RATE, sos, clu, Cq, 220) == native.MM_ERR_ARG
        assert b"tracks out of range [1, 256]" in lib.mm_last_error(ctx.ptr)
    assert lib.mm_batch_level_pcm(ctx.ptr, ptr, 0, fr, 2, 2, 1999, sos, clu, Cq, 220) == native.MM_ERR_ARG
    assert b"track 0: rate below 2000 Hz" in lib.mm_last_error(ctx.ptr)
    fr[0] = fr[1] = 2 ** 30
    assert lib.mm_batch_level_pcm(ctx.ptr, ptr, 0, fr, 2, 2, RATE, sos, clu, Cq, 220) == native.MM_ERR_ARG
    assert b"track 1: 2^31 frames or more in all" in lib.mm_last_error(ctx.ptr)
    # the context still works
    got, lv, ce, rs = batch_level([pcm], RATE, [inputs["down"][2]], [inputs["down"][3]], 220)
    check_track(got[0], lv[0], ce[0], *host["down", 220], inputs["down"][3])
