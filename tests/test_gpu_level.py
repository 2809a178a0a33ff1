"""Delivery to an R 128 loudness target on the GPU: the gain kernel against numpy at the
sizes where it can go wrong (its workgroup span and seams, fewer samples than one vector,
views that start off a 16-byte boundary, full-scale input at the ends of the gain range),
the whole stage against the host restatement mm_level_host (bit-identical samples, equal
integers) on the inputs whose decision margins tests/test_level.py asserts, and the stage
at the end of every master entry point."""
import ctypes
import math

import numpy as np
import pytest

from test_ceiling import ONE, q28
from test_level import PASSES, STATUS, TOL, case_inputs, host_level, level_ints, pink, ref_gain, ref_level

pytestmark = pytest.mark.gpu

RATE = 44100
P = {"bass_boost": 2.0, "treble_boost": 1.5, "saturation": 20, "width": 1.2, "multiband": True, "lufs": -14.0}


@pytest.fixture(scope="module")
def span():
    from mastering_amd import native
    return native.load().mm_level_span()


def as_kind(x, f32):
    return x.astype(np.float32) / np.float32(32768) if f32 else x


def to_i16(raw):
    if raw.dtype == np.int16:
        return raw
    k = raw * np.float32(32768)
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max(initial=0) <= 32768  # still on the int16 grid
    return k.astype(np.int16)


def op_gain(x, g, f32, src_off=0, dst_off=0):
    """mm_op_level_gain on int16 `x` (or x / 32768 as f32): (samples as int16, clipped, peak)."""
    from mastering_amd import native
    ctx = native.context(0)
    host = np.ascontiguousarray(as_kind(x, f32))
    out = np.empty_like(host)
    clipped, peak = ctypes.c_int64(-1), ctypes.c_int32(-1)
    ctx.check(ctx.lib.mm_op_level_gain(ctx.ptr, host.ctypes.data_as(ctypes.c_void_p),
                                       native.MM_OUT_F32 if f32 else native.MM_OUT_I16, host.size, src_off, dst_off, g,
                                       out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(clipped), ctypes.byref(peak)),
              "mm_op_level_gain")
    return to_i16(out), clipped.value, peak.value


@pytest.mark.parametrize("f32", [False, True], ids=["i16", "f32"])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("size", ["1", "7", "8", "9", "S-1", "S", "S+1", "3S+5"])
def test_gain_kernel(span, size, ch, f32):
    """Random samples with both full-scale values at the ends of the line, of every vector and
    of every workgroup's share; every view: aligned, both offset by one sample (and by three),
    in place on an offset view, and a source that does not share the destination's offset."""
    n = {"1": 1, "7": 7, "8": 8, "9": 9, "S-1": span - 1, "S": span, "S+1": span + 1, "3S+5": 3 * span + 5}[size] * ch
    x = np.random.default_rng(7 * n + ch).integers(-32768, 32768, n).astype(np.int16)
    for at in (0, 7, 8, span - 1, span, span + 1, n - 2, n - 1):
        if 0 <= at < n:
            x[at] = 32767 if at % 2 else -32768
    for g in (1 << 8, ONE - 1, ONE, ONE + 1, 1 << 21):
        want, clipped = ref_gain(x, g)
        peak = int(np.abs(want.astype(np.int64)).max())
        for src_off, dst_off in ((0, 0), (1, 1), (3, 3), (1, -1), (0, 1), (2, 0)):
            got, gc, gp = op_gain(x, g, f32, src_off, dst_off)
            assert np.array_equal(got, want), (g, src_off, dst_off)
            assert (gc, gp) == (clipped, peak), (g, src_off, dst_off)
        if g == ONE:
            assert np.array_equal(want, x) and clipped == 0
        if g == 1 << 21 and n > 8:
            assert clipped > n // 2


def test_gain_kernel_refusals():
    from mastering_amd import native
    ctx = native.context(0)
    x = np.zeros(16, np.int16)
    c, p = ctypes.c_int64(), ctypes.c_int32()
    call = lambda kind, n, so, do, g: ctx.lib.mm_op_level_gain(  # noqa: E731
        ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, n, so, do, g, x.ctypes.data_as(ctypes.c_void_p),
        ctypes.byref(c), ctypes.byref(p))
    for args in ((7, 16, 0, 0, ONE), (0, -1, 0, 0, ONE), (0, 16, 8, 0, ONE), (0, 16, 0, 8, ONE), (0, 16, -1, 0, ONE),
                 (0, 16, 0, 0, 255), (0, 16, 0, 0, (1 << 21) + 1)):
        assert call(*args) == native.MM_ERR_ARG, args
    assert call(0, 16, 0, 0, ONE) == 0 and call(0, 0, 0, 0, ONE) == 0


# ------------------------------------------------------------------ the stage against the host
def dev_level(pcm, rate, T, C, W, f32=False):
    """mm_level_pcm: (samples as int16, mm_level, mm_ceiling)."""
    from mastering_amd import design, engine, native
    x = np.ascontiguousarray(as_kind(np.asarray(pcm), f32)).copy()
    ctx = native.context(0)
    m, ce = native.MMLevel(), native.MMCeiling()
    ctx.check(ctx.lib.mm_level_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p),
                                   native.MM_OUT_F32 if f32 else native.MM_OUT_I16, x.shape[0],
                                   1 if x.ndim == 1 else x.shape[1], rate, engine.kweight_sos(rate), design.level_clu(T),
                                   C, W, ctypes.byref(m), ctypes.byref(ce)), "mm_level_pcm")
    return to_i16(x), m, ce


def all_cases():
    c = case_inputs()
    c["mono-48k"] = (pink(3, 1, -18.0, 7, rate=48000), 48000, -14.0, q28(-1.0), 240, "reached", None)
    return c


CASES = ["down", "up-idle", "stepped", "mono-boost", "saturated", "capped", "no-ceiling", "window-1", "mono-48k"]


@pytest.fixture(scope="module")
def host_results():
    """mm_level_host of every case (shared, read-only).  The decision margins of the cases of
    tests/test_level.py are asserted there; those of the 48 kHz case here."""
    from mastering_amd import native
    cases = all_cases()
    pcm, rate, T, C, W, status, _ = cases["mono-48k"]
    _, st = ref_level(pcm, rate, T, C, W)
    assert st["status"] == status and min(st["margins"]) >= 1e-3 and min(st["slopes"], default=1.0) >= 0.01
    out = {}
    for name, (pcm, rate, T, C, W, status, passes) in cases.items():
        ce = native.MMCeiling()
        y, m = host_level(pcm, rate, T, C, W, ce)
        assert m.status == STATUS[status] and (passes is None or m.passes == passes), name
        out[name] = (cases[name], y, m, ce)
    return out


@pytest.mark.parametrize("f32", [False, True], ids=["i16", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_level_pcm_is_the_host_restatement(host_results, name, f32):
    (pcm, rate, T, C, W, _, _), want, hm, hce = host_results[name]
    got, m, ce = dev_level(pcm, rate, T, C, W, f32)
    assert np.array_equal(got, want)
    assert level_ints(m) == level_ints(hm)
    for k in range(PASSES):
        assert (math.isnan(m.pass_lufs[k]) and math.isnan(hm.pass_lufs[k])) or abs(m.pass_lufs[k] - hm.pass_lufs[k]) <= 1e-6
    assert abs(m.source_lufs - hm.source_lufs) <= 1e-6 and abs(m.loudness - hm.loudness) <= 1e-6
    if C:
        from mastering_amd import native
        assert all(getattr(ce, f) == getattr(hce, f) for f, _ in native.MMCeiling._fields_)
        assert ce.tp_out_q28 <= C
    if not f32:  # a second run: the same bytes and the same struct, bit for bit
        again, m2, _ = dev_level(pcm, rate, T, C, W)
        assert np.array_equal(again, got) and bytes(m2) == bytes(m)


@pytest.mark.parametrize("what", ["short", "silence", "empty"])
def test_level_pcm_unmeasurable(what):
    pcm = {"short": pink(1, 2, -3.0, 6)[:17000], "silence": np.zeros((RATE, 2), np.int16),
           "empty": np.zeros((0, 2), np.int16)}[what]
    C = q28(-1.0)
    want, hm = host_level(pcm, RATE, -14.0, C, 220)
    got, m, ce = dev_level(pcm, RATE, -14.0, C, 220)
    assert np.array_equal(got, want) and level_ints(m) == level_ints(hm)
    assert m.status == STATUS["unmeasurable"] and m.passes == 0 and math.isnan(m.loudness)
    assert ce.tp_out_q28 <= C and (what == "short") == (m.limited_frames > 0)


def test_engine_level_pcm(host_results):
    from mastering_amd import engine
    (pcm, rate, T, C, W, _, _), want, hm, _ = host_results["stepped"]
    out, d = engine.level_pcm(pcm, rate, T, ceiling_dbtp=-1.0)
    assert np.array_equal(out, want) and d["status"] == "reached" and d["passes"] == hm.passes == len(d["pass_lufs"])
    assert d["pass_gain_q16"] == [hm.pass_gain_q16[k] for k in range(hm.passes)] and abs(d["loudness"] - T) <= TOL
    assert d["window"] == 220 and d["ceiling_q28"] == C and d["limited_frames"] == hm.limited_frames
    (pcm, rate, T, C, W, _, _), want, hm, _ = host_results["no-ceiling"]
    out, d = engine.level_pcm(pcm, rate, T)
    assert np.array_equal(out, want) and d["status"] == "capped" and d["clipped"] == 0 and d["ceiling_q28"] == 0


# ------------------------------------------------------------------ at the end of a master call
@pytest.fixture(scope="module")
def track():
    return pink(4, 2, -20.0, 8)


def check_delivered(out, info, plain, rate, target, ceiling):
    from mastering_amd import design, engine
    want, d = engine.level_pcm(plain, rate, target, ceiling_dbtp=ceiling)
    lv = info["level"]
    assert np.array_equal(out, want)
    assert {k: lv[k] for k in ("status", "passes", "gain_q16", "pass_gain_q16", "clipped", "limited_frames")} == \
        {k: d[k] for k in ("status", "passes", "gain_q16", "pass_gain_q16", "clipped", "limited_frames")}
    assert lv["loudness"] == d["loudness"] == info["r128"]["integrated_lufs"]
    print("level:", lv["status"], lv["passes"], lv["pass_gain_db"], lv["pass_lufs"])
    if lv["status"] == "reached":
        assert abs(lv["loudness"] - target) <= TOL
    assert max(info["report"]["true_peak_q28"]) <= design.ceiling_q28(ceiling) == info["ceiling"]["ceiling_q28"]
    assert info["ceiling"]["tp_out_q28"] == max(info["report"]["true_peak_q28"])
    assert lv["rate"] == rate and lv["frames"] == len(out) == info["report"]["frames"]


def test_master_pcm_delivers_to_the_target(track):
    from mastering_amd import engine, native
    plain, pinfo = engine.master_pcm(track, RATE, P)
    out, info = engine.master_pcm(track, RATE, dict(P, deliver_lufs=-14.0, ceiling_dbtp=-1.0, report=True, r128=True))
    check_delivered(out, info, plain, RATE, -14.0, -1.0)
    assert info["level"]["status"] == "reached" and "resample" not in info and "rate" not in info
    assert {k: info[k] for k in pinfo} == pinfo  # the chain's own figures are the plain call's
    with pytest.raises(RuntimeError, match="did not resample"):
        m = native.MMResample()
        ctx = native.context(0)
        ctx.check(ctx.lib.mm_last_resample(ctx.ptr, ctypes.byref(m)), "mm_last_resample")
    # the float output carries the same samples
    outf, infof = engine.master_pcm(track, RATE, dict(P, deliver_lufs=-14.0, ceiling_dbtp=-1.0), native.MM_OUT_F32)
    assert np.array_equal(to_i16(outf), out) and infof["level"]["pass_gain_q16"] == info["level"]["pass_gain_q16"]
    # and without a ceiling the level alone
    out0, info0 = engine.master_pcm(track, RATE, dict(P, deliver_lufs=-16.0))
    want0, d0 = engine.level_pcm(plain, RATE, -16.0)
    assert np.array_equal(out0, want0) and "ceiling" not in info0 and info0["level"]["status"] == d0["status"]


def test_master_pcm_delivers_at_another_rate(track):
    from mastering_amd import engine
    plain, _ = engine.master_pcm(track, RATE, dict(P, output_rate=48000))
    out, info = engine.master_pcm(track, RATE, dict(P, deliver_lufs=-14.0, ceiling_dbtp=-1.0, report=True, r128=True,
                                                    output_rate=48000))
    check_delivered(out, info, plain, 48000, -14.0, -1.0)
    assert info["rate"] == 48000 and info["resample"]["frames_out"] == len(out) and info["level"]["window"] == 240


def test_process_delivers_to_the_target(track, tmp_path):
    from mastering_amd import engine, wavio
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    wavio.write_wav(src, track, RATE)
    plain, _ = engine.master_pcm(track, RATE, P)
    info = engine.process(src, dst, dict(P, deliver_lufs=-14.0, ceiling_dbtp=-1.0, report=True, r128=True))
    out, rate = wavio.read_wav(dst)
    assert rate == RATE
    check_delivered(out, info, plain, RATE, -14.0, -1.0)


def test_without_the_key_nothing_changes(track):
    from mastering_amd import engine, native
    ctx = native.context(0)
    params = dict(P, ceiling_dbtp=-1.0, report=True, r128=True)
    ctx.timing(True)
    try:
        ctx.kernel_stats()
        a, ia = engine.master_pcm(track, RATE, params)
        names = set(ctx.kernel_stats())
        assert "ceil_tracks_need" in names and "r128_album_kweight" in names and "level_tracks_gain" not in names
        with pytest.raises(RuntimeError, match="no loudness target"):
            engine.levels(ctx)
        b, ib = engine.master_pcm(track, RATE, dict(params, deliver_lufs=None))
        assert np.array_equal(a, b) and ia == ib and "level" not in ia
        assert "level_tracks_gain" not in set(ctx.kernel_stats())
        job = engine.Job(len(track), RATE, 2, P, ceiling_dbtp=-1.0, report=True, r128=True)
        assert job.delivery is None  # the plain entry point, as before
        engine.master_pcm(track, RATE, dict(params, deliver_lufs=-14.0))
        assert "level_tracks_gain" in set(ctx.kernel_stats()) and engine.levels(ctx)[0].status == STATUS["reached"]
    finally:
        ctx.timing(False)


def test_refusals_leave_the_context_usable(track, host_results):
    from mastering_amd import engine, native
    ctx = native.context(0)
    x = np.ascontiguousarray(track[:8000]).copy()
    m, sos, C = native.MMLevel(), engine.kweight_sos(RATE), q28(-1.0)
    p = x.ctypes.data_as(ctypes.c_void_p)
    call = lambda kind, ch, rate, s, clu, c, w: ctx.lib.mm_level_pcm(  # noqa: E731
        ctx.ptr, p, kind, 4000, ch, rate, s, clu, c, w, ctypes.byref(m), None)
    for args, words in (((0, 2, RATE, sos, -300, C, 220), "level_clu"), ((0, 2, RATE, sos, -4001, C, 220), "level_clu"),
                        ((0, 2, RATE, sos, 0, C, 220), "level_clu"), ((7, 2, RATE, sos, -1400, C, 220), "kind"),
                        ((0, 3, RATE, sos, -1400, C, 220), "channels"), ((0, 2, 1999, sos, -1400, C, 220), "rate"),
                        ((0, 2, RATE, None, -1400, C, 220), "bad arguments"),
                        ((0, 2, RATE, sos, -1400, 2 ** 24 - 1, 220), "ceiling"),
                        ((0, 2, RATE, sos, -1400, C, 1025), "window")):
        with pytest.raises(ValueError, match=words):
            ctx.check(call(*args), "mm_level_pcm")
    assert np.array_equal(x, track[:8000])
    # a loudness target without the `loud` job is refused before the chain runs
    job = engine.Job(len(track), RATE, 2, P, deliver_lufs=-14.0)
    job.delivery.loud = None
    out = np.empty_like(track)
    res = native.MMResult()
    with pytest.raises(ValueError, match="loud"):
        ctx.check(ctx.lib.mm_deliver(ctx.ptr, ctypes.byref(job.job), ctypes.byref(job.delivery),
                                     track.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.byref(res)), "mm_deliver")
    with pytest.raises(ValueError):
        ctx.check(ctx.lib.mm_deliver(ctx.ptr, ctypes.byref(job.job), None, track.ctypes.data_as(ctypes.c_void_p),
                                     out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(res)), "mm_deliver")
    with pytest.raises(ValueError):
        engine.master_pcm(track, RATE, dict(P, deliver_lufs=-3.0))
    # and the context goes on working
    (pcm, rate, T, C, W, _, _), want, hm, _ = host_results["down"]
    y, d = engine.level_pcm(pcm, rate, T, ceiling_dbtp=-1.0)
    assert np.array_equal(y, want) and d["passes"] == hm.passes and d["status"] == native.LEVEL_STATUS[hm.status]
