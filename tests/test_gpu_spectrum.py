"""The spectrum report on the GPU (csrc/spectrum.hip): the frames kernel (one
complex 8192-point FFT a frame in registers and LDS, float64 accumulators), its records and the
fold against the host restatement mm_spectrum_host, within the tolerance derived below, at the
lengths where the groups of frames can go wrong, for both buffer kinds, mono and stereo, on
signals that reach every output position of the FFT; a file whose lows are in phase and whose
highs are out of phase; and what is bitwise: the same call twice, a batch on tracks side by side
in one allocation against single calls, and the report through the master call and
deliver_batch against spectrum_pcm on what they delivered."""
import ctypes

import numpy as np
import pytest

from test_spectrum import BINS, H, N, host_spectrum, tail

pytestmark = pytest.mark.gpu

RATE = 44100
G0 = 16  # SPEC_G0 of csrc/spectrum.h: the frames of a whole group
P = {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0,
     "saturation": 30, "width": 1.3, "multiband": True, "lufs": -9.0}
INFO_KEYS = {"loudness", "gain_db", "gain_linear", "frames", "comp_iters", "comp_walked", "comp_jumped", "comp_active",
             "chunks", "tile"}

# The tolerance.  For a column Q of {S_L, S_R, C} and a bin k the GPU is held to
#   |Q_gpu[k] - Q_ref[k]| <= TAU * sqrt(M * P[k]) + TAU^2 * M,   P = S_L + S_R of the reference, M = mean P,
# the shape an amplitude error of TAU * rms(X) an output gives a power.  TAU is not taken from
# the kernel: TAU_32 is the smallest value with which ref_spectrum's own lines, evaluated in
# single precision (float32 window and samples, scipy.fft.fft on complex64 input), satisfy the
# criterion against their float64 evaluation on the signals of this file (every entry of
# cases(), stereo and mono): 3.52e-6, set by "sine on bin 1235" in mono (the sines on bins 1 and
# N/2 - 1 read 2.87e-6; the noises 1.0e-7 to 8.7e-7, the impulses up to 5.6e-7, R = +-L 4.7e-7).
# That is 4.6 times eps * log2 N = 7.7e-7, the most a sound single-precision FFT should read, and
# the sines alone pass it: a twiddle's rounding is an error relative to the peak it multiplies,
# 52 times rms(X) for a full-scale tone on a bin, where the criterion allows TAU * 0.019 of the
# peak's own power, so 2 * 3e-8 / 0.019 = 3e-6 is what eps / 2 a factor gives.  The measurement
# stands as made.  TAU = 4 * TAU_32: two bits for another butterfly order and the stereo unpacking.
TAU_32 = 3.52e-6
TAU = 4 * TAU_32


def smallest_tau(got, want):
    """The smallest tau with which `got` satisfies the criterion against `want` (0 for equal tables)."""
    P = want[:, 0] + want[:, 1]
    M = float(P.mean())
    e = np.abs(got - want).max(axis=1)
    if M == 0.0:
        return 0.0 if e.max() == 0.0 else np.inf
    b = np.sqrt(M * P)
    den = b + np.sqrt(b * b + 4.0 * M * e)  # (0 only where P[k] == 0 and e == 0: nothing to allow for)
    return float(np.max(2.0 * e / np.where(den > 0.0, den, 1.0)))


def as_kind(x, f32):
    return x.astype(np.float32) / np.float32(32768) if f32 else x


def gpu_spectrum(pcm, rate=RATE, f32=False):
    """(struct, bands, bins) of mm_spectrum_pcm on int16 `pcm` (or on pcm / 32768 as an MM_OUT_F32 buffer)."""
    from mastering_amd import native
    x = np.ascontiguousarray(pcm, np.int16)
    host = np.ascontiguousarray(as_kind(x, f32))
    ctx = native.context(0)
    m = native.MMSpectrum()
    bins = np.full((BINS + 1, 3), -7.0)
    bands = np.full((native.SPECTRUM_MAX_BANDS + 1, 4), -7.0)
    ctx.check(ctx.lib.mm_spectrum_pcm(ctx.ptr, host.ctypes.data_as(ctypes.c_void_p), native.MM_OUT_F32 if f32 else native.MM_OUT_I16,
                                      x.shape[0], 1 if x.ndim == 1 else x.shape[1], rate, ctypes.byref(m),
                                      bands.ctypes.data_as(native.c_double_p), bins.ctypes.data_as(native.c_double_p)),
              "mm_spectrum_pcm")
    assert (bins[-1] == -7.0).all() and (bands[m.n_bands:] == -7.0).all()  # nothing past the tables
    return m, bands[:m.n_bands].copy(), bins[:-1].copy()


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check(pcm, rate=RATE):
    """The device within TAU of the host restatement, both kinds bit-equal; returns (struct, bands, bins)."""
    hm, hbands, hbins = host_spectrum(pcm, rate)
    m, bands, bins = gpu_spectrum(pcm, rate)
    m32, bands32, bins32 = gpu_spectrum(pcm, rate, f32=True)
    assert same_bits(bins, bins32) and same_bits(bands, bands32)
    for s in (m, m32):
        assert (s.frames, s.channels, s.rate, s.n_fft, s.hop, s.n_frames, s.n_bands) == \
               (hm.frames, hm.channels, hm.rate, N, H, hm.n_frames, hm.n_bands)
    if hm.n_frames == 0:
        assert np.isnan(bins).all() and np.isnan(bands[:, :3]).all() and np.isnan(m.total_ms[0])
        return m, bands, bins
    tau = smallest_tau(bins, hbins)
    print(f"tau {tau:.3e} of {TAU:.3e}")
    assert tau <= TAU, tau
    if hm.channels == 1:
        assert (bins[:, 1:] == 0).all()
    # the tail is the host's own: the bands of the device's table, bit for bit
    assert same_bits(tail(bins, hm.frames, hm.channels, rate)[1], bands)
    return m, bands, bins


def noise(n, seed=1, amp=20000):
    return np.random.default_rng(seed).integers(-amp, amp, (n, 2)).astype(np.int16)


def sine(k, frames=N + H):
    t = np.arange(frames)
    return np.stack([np.rint(32767 * np.cos(2 * np.pi * k * t / N)), np.rint(32767 * np.sin(2 * np.pi * k * t / N + 0.3))],
                    axis=1).astype(np.int16)


def impulse(n0):
    x = np.zeros((N, 2), np.int16)
    x[n0] = (-32768, 32767)
    return x


def cases():
    """(name, stereo int16 signal) of every signal the device is held against the host on."""
    a = noise(2 * N + 9, seed=7)
    out = [(f"noise of {n} frames", noise(n, seed=n)) for n in
           (N - 1, N, N + H - 1, N + H, G0 * H + N - H, G0 * H + N, 3 * G0 * H + N)]  # 0, 1, 1, 2, G0, G0 + 1, 3 G0 + 1 frames
    out += [(f"impulse at {n0}", impulse(n0)) for n0 in (1, N // 2, N - 1)]
    out += [(f"sine on bin {k}", sine(k)) for k in (1, N // 2 - 1, 1235)]
    out += [("R = L", np.stack([a[:, 0], a[:, 0]], axis=1)), ("R = -L", np.stack([a[:, 0], -a[:, 0]], axis=1)),
            ("R = 0", np.stack([a[:, 0], 0 * a[:, 0]], axis=1)), ("full scale", np.full((N + H, 2), -32768, np.int16))]
    return out


@pytest.mark.parametrize("name,x", cases(), ids=[c[0] for c in cases()])
def test_device_against_host(name, x):
    m, bands, bins = check(x)
    check(np.ascontiguousarray(x[:, 0]))  # and as a mono signal
    if name.startswith("impulse"):
        w = 0.5 - 0.5 * np.cos(2 * np.pi * int(name.split()[-1]) / N)
        assert np.allclose(bins[:, 0], w * w, rtol=1e-5, atol=0) and np.allclose(bins[:, 2], -w * w * 32767 / 32768, rtol=1e-5, atol=0)
    if name == "R = L":
        assert np.allclose(bins[:, 2], bins[:, 0], rtol=1e-5) and np.allclose(bins[:, 1], bins[:, 0], rtol=1e-5)
    if name == "R = -L":
        assert np.allclose(bins[:, 2], -bins[:, 0], rtol=1e-5)
    if name == "R = 0":
        assert bins[:, 1].max() <= TAU ** 2 * bins[:, 0].mean() and m.total_ms[1] <= TAU ** 2 * m.total_ms[0]
    if name == "full scale":  # DC at full scale: bin 0 holds (N/2)^2, bin 1 a quarter of it
        assert bins[0, 0] == pytest.approx((N / 2) ** 2, rel=1e-6) and bins[1, 0] == pytest.approx((N / 4) ** 2, rel=1e-6)
        assert bins[0, 2] == pytest.approx(bins[0, 0], rel=1e-6)


def band_split(frames=6 * H + N, seed=3):
    """L = a + b, R = a - b: a below 1 kHz, b above 4 kHz, at equal power (FFT masks on noise)."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfftfreq(frames, 1.0 / RATE)
    A, B = np.fft.rfft(rng.normal(size=frames)), np.fft.rfft(rng.normal(size=frames))
    a, b = np.fft.irfft(A * (f < 1000.0), frames), np.fft.irfft(B * (f > 4000.0), frames)
    a, b = a / np.sqrt(np.mean(a * a)), b / np.sqrt(np.mean(b * b))
    return np.rint(3000.0 * np.stack([a + b, a - b], axis=1)).astype(np.int16)


def test_band_split_phase():
    """In phase below 1 kHz, out of phase above 4 kHz: the overall correlation reads about 0, the
    bands say which part of the spectrum a mono fold-down loses.  (The limits: every band that ends
    below 800 Hz and every band that begins above 5 kHz, clear of the masks' edges; ref_spectrum and
    ref_qc on the CPU read +1.000 and -1.000 there and 0.000 overall.)"""
    from mastering_amd import qc_pcm, spectrum_pcm
    x = band_split()
    d = spectrum_pcm(x, RATE)
    low = [b for b in d["bands"] if b["hi_hz"] < 800.0]
    high = [b for b in d["bands"] if b["lo_hz"] > 5000.0]
    assert len(low) >= 10 and len(high) >= 5
    assert all(b["correlation"] > 0.99 for b in low), [b["correlation"] for b in low]
    assert all(b["correlation"] < -0.99 for b in high), [b["correlation"] for b in high]
    assert abs(qc_pcm(x, RATE)["correlation"]) < 0.1
    assert all(b["side_dbfs"] < b["mid_dbfs"] - 20 for b in low) and all(b["mid_dbfs"] < b["side_dbfs"] - 20 for b in high)


def test_twice_is_bitwise():
    x = noise(3 * G0 * H + N, seed=11)
    first, second = gpu_spectrum(x), gpu_spectrum(x)
    assert same_bits(first[2], second[2]) and same_bits(first[1], second[1])
    assert bytes(first[0]) == bytes(second[0])


def batch_tracks():
    """Six tracks cut from ONE array at odd frame offsets: one shorter than a frame, one frame,
    a group's seam and several groups."""
    lens = [N + H + 2, N - 2, G0 * H + N + 4, N, 2 * G0 * H + N + 6, 3 * H + N + 8]  # (even: every offset stays odd)
    x = noise(1 + sum(lens), seed=6)
    off = 1 + np.concatenate([[0], np.cumsum(lens)])
    assert all(int(o) % 2 == 1 for o in off[:-1])
    return x, lens, off


@pytest.mark.parametrize("f32", [False, True], ids=["i16", "f32"])
def test_batch_side_by_side(f32):
    import torch
    from mastering_amd import engine, native
    x, lens, off = batch_tracks()
    ctx = native.context(0)
    d = torch.from_numpy(np.ascontiguousarray(as_kind(x, f32))).cuda()
    torch.cuda.current_stream().synchronize()
    step = d.element_size() * 2
    n = len(lens)
    out = (native.MMSpectrum * n)()
    ctx.check(ctx.lib.mm_batch_spectrum_device(ctx.ptr, engine._pointers([d.data_ptr() + int(o) * step for o in off[:-1]]),
                                               native.MM_OUT_F32 if f32 else native.MM_OUT_I16, (ctypes.c_int64 * n)(*lens), n, 2,
                                               RATE, out), "mm_batch_spectrum_device")
    last = engine.spectra(ctx, n)
    for t in range(n):
        track = x[off[t]:off[t + 1]]
        m, bands, bins = gpu_spectrum(track, f32=f32)  # (the single call replaces the context's results: read before)
        assert bytes(out[t]) == bytes(m) == bytes(last[t]), t
    ctx.check(ctx.lib.mm_batch_spectrum_device(ctx.ptr, engine._pointers([d.data_ptr() + int(o) * step for o in off[:-1]]),
                                               native.MM_OUT_F32 if f32 else native.MM_OUT_I16, (ctypes.c_int64 * n)(*lens), n, 2,
                                               RATE, out), "mm_batch_spectrum_device")
    tables = [engine.spectrum_bins(ctx, t) for t in range(n)]
    for t in range(n):
        m, bands, bins = gpu_spectrum(x[off[t]:off[t + 1]], f32=f32)
        assert same_bits(tables[t], bins), t
    assert out[1].n_frames == 0 and np.isnan(tables[1]).all() and out[3].n_frames == 1 and out[4].n_frames == 2 * G0 + 1


def test_batch_python_entry():
    from mastering_amd import spectrum_batch_pcm, spectrum_pcm
    x, lens, off = batch_tracks()
    tracks = [np.ascontiguousarray(x[off[t]:off[t + 1]]) for t in range(len(lens))]
    for f32 in (False, True):
        got = spectrum_batch_pcm([as_kind(t, f32) for t in tracks], RATE, curve=True)
        for (d, bins), t in zip(got, tracks):
            want, want_bins = spectrum_pcm(as_kind(t, f32), RATE, curve=True)
            assert same_bits(bins, want_bins) and repr(d) == repr(want)  # (repr: NaN-free dicts compare, None stays None)
    assert got[1][0]["n_frames"] == 0 and got[1][0]["bands"][0]["level_dbfs"] == [None, None]
    mono = spectrum_batch_pcm([t[:, 0] for t in tracks[:3]], RATE)
    assert repr(mono[0]) == repr(spectrum_pcm(tracks[0][:, 0], RATE)) and mono[0]["channels"] == 1
    with pytest.raises(ValueError, match="one channel count"):
        spectrum_batch_pcm([tracks[2], tracks[2][:, 0]], RATE)
    with pytest.raises(ValueError, match="track 0: rate below 2000"):
        spectrum_batch_pcm(tracks[:3], 1999)
    with pytest.raises(ValueError, match="spectrum: rate below 2000"):
        spectrum_pcm(tracks[0], 1999)


@pytest.fixture(scope="module")
def hot():
    from mastering_amd.synth import pink_noise_pcm16
    return pink_noise_pcm16(int(1.5 * RATE), RATE, 2, track=31, level_dbfs=-6.0)


def test_master_call_reports_what_it_delivered(hot):
    from mastering_amd import engine, master_pcm, native, spectrum_pcm
    ctx = native.context(0)
    plain, info_plain = master_pcm(hot, RATE, P)
    assert set(info_plain) == INFO_KEYS  # without the key: the call of before
    with pytest.raises(RuntimeError, match="made no spectrum report"):
        engine.spectra(ctx, 1)
    m = native.MMSpectrum()
    assert ctx.lib.mm_last_spectrum(ctx.ptr, 1, ctypes.byref(m)) == -4  # MM_ERR_STATE
    out, info = master_pcm(hot, RATE, dict(P, spectrum=True, qc=True))
    table = engine.spectrum_bins(ctx, 0)
    assert np.array_equal(out, plain) and set(info) == INFO_KEYS | {"spectrum", "qc"}
    want, want_bins = spectrum_pcm(out, RATE, curve=True)
    assert repr(info["spectrum"]) == repr(want) and same_bits(table, want_bins)
    assert info["spectrum"]["frames"] == len(out) and info["spectrum"]["rate"] == RATE and info["spectrum"]["n_frames"] == 15
    out, info = master_pcm(hot, RATE, dict(P, spectrum=True))  # alone: no other report is made
    assert np.array_equal(out, plain) and set(info) == INFO_KEYS | {"spectrum"} and repr(info["spectrum"]) == repr(want)
    with pytest.raises(RuntimeError):
        engine.qcs(ctx, 1)
    out, info = master_pcm(hot, RATE, dict(P, spectrum=True, report=True, output_rate=48000, ceiling_dbtp=-1.0))
    table = engine.spectrum_bins(ctx, 0)
    want, want_bins = spectrum_pcm(out, 48000, curve=True)  # of what was delivered, at its rate
    assert info["rate"] == 48000 and repr(info["spectrum"]) == repr(want) and same_bits(table, want_bins)
    assert info["spectrum"]["n_bands"] == 32 and info["spectrum"]["frames"] == len(out)
    ref, info_ref = master_pcm(hot, RATE, dict(P, report=True, output_rate=48000, ceiling_dbtp=-1.0))
    assert np.array_equal(out, ref) and {k: v for k, v in info.items() if k != "spectrum"} == info_ref
    out, info = master_pcm(hot, RATE, dict(P, spectrum=True, deliver_lufs=-16.0))
    assert repr(info["spectrum"]) == repr(spectrum_pcm(out, RATE)) and "level" in info
    mono, info = master_pcm(np.ascontiguousarray(hot[:, 0]), RATE, dict(P, spectrum=True), out_kind=native.MM_OUT_F32)
    assert repr(info["spectrum"]) == repr(spectrum_pcm(mono, RATE)) and info["spectrum"]["channels"] == 1
    assert "correlation" not in info["spectrum"]["bands"][0]


def test_deliver_batch_with_spectrum():
    import torch
    from mastering_amd import Job, deliver_batch, native, spectrum_pcm
    from mastering_amd.synth import pink_noise_pcm16
    pcms = [pink_noise_pcm16(int(1.2 * RATE) + 100 * i, RATE, 2, track=40 + i, level_dbfs=-10.0) for i in range(3)]
    ctx = native.context(0)

    def run(**kw):
        jobs = [Job(len(p), RATE, 2, P) for p in pcms]
        for j in jobs:
            j.job.in_kind = native.MM_IN_I16
        xs = [torch.from_numpy(p).cuda() for p in pcms]
        outs = [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]
        torch.cuda.current_stream().synchronize()
        lv = deliver_batch(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs], (-14.0, -16.0, -11.0), -1.0,
                           **kw)[1]
        return [o.cpu().numpy() for o in outs], lv

    plain, lv_plain = run()
    outs, lv = run(spectrum=True)
    for a, b, d, e in zip(outs, plain, lv, lv_plain):
        assert np.array_equal(a, b) and "spectrum" not in e
        assert {k: v for k, v in d.items() if k != "spectrum"} == e  # the level dicts are otherwise what they were
        assert repr(d["spectrum"]) == repr(spectrum_pcm(a, RATE))
