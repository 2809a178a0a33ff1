"""The spectrum report on CPU: the library's host restatement (mm_spectrum_host: its own
radix-2 FFT in double) and its tail (mm_spectrum_from_bins) against a few dozen lines of numpy
written from the definition in include/mastering.h (ref_spectrum, ref_bands), known answers of
the tail and of the whole, the refusals, the mm_spectrum layout and the Python plumbing that
needs no GPU.  The FFT is float arithmetic: the two restatements agree to 1e-9 relative on every
bin that holds 1e-12 of the largest, not bit for bit."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

N, H = 8192, 4096
BINS = N // 2 + 1
NORM = N * (3 * N / 8)
REL, FLOOR = 1e-9, 1e-12  # host against numpy: relative, on bins that hold FLOOR of the largest


def n_frames(frames):
    return 0 if frames < N else (frames - N) // H + 1


def ref_spectrum(pcm, dtype=np.float64, rfft=np.fft.rfft):
    """The bin table [N/2 + 1, 3] of mm_spectrum's steps 1 and 2 in numpy (`dtype`, `rfft`: the
    arithmetic; the GPU tests evaluate the same lines in single precision to measure it)."""
    x = np.asarray(pcm, np.int16).astype(dtype) / dtype(32768)
    x = x[:, None] if x.ndim == 1 else x
    F = n_frames(x.shape[0])
    bins = np.zeros((BINS, 3), np.float64)
    if F == 0:
        return bins * np.nan
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(dtype)
    for j in range(F):
        X = rfft(w[:, None] * x[j * H:j * H + N], axis=0).astype(np.complex128)
        bins[:, 0] += np.abs(X[:, 0]) ** 2
        if x.shape[1] == 2:
            bins[:, 1] += np.abs(X[:, 1]) ** 2
            bins[:, 2] += (X[:, 0] * np.conj(X[:, 1])).real
    return bins / F


def ref_edges(rate):
    """[n_bands, 3] of lower edge, centre, upper edge."""
    rows, m = [], -17
    while 1000.0 * 10.0 ** ((2 * m - 1) / 20.0) < rate / 2:
        rows.append((1000.0 * 10.0 ** ((2 * m - 1) / 20.0), 1000.0 * 10.0 ** (m / 10.0),
                     min(1000.0 * 10.0 ** ((2 * m + 1) / 20.0), rate / 2)))
        m += 1
    return np.array(rows)


def ref_bands(bins, rate):
    """[n_bands, 4] of step 3 another way: the power below f as a piecewise linear function over
    the bins' rectangles, a band the difference at its two edges."""
    df = rate / N
    ck = np.full(BINS, 2.0)
    ck[0] = ck[-1] = 1.0
    bounds = np.concatenate([[0.0], (np.arange(1, BINS) - 0.5) * df, [rate / 2]])
    e = ref_edges(rate)
    out = np.zeros((len(e), 4))
    for q in range(3):
        below = np.concatenate([[0.0], np.cumsum(ck * bins[:, q])])
        out[:, q] = (np.interp(e[:, 2], bounds, below) - np.interp(e[:, 0], bounds, below)) / NORM
    out[:, 3] = (e[:, 2] - e[:, 0]) / df
    return out


def host_spectrum(pcm, rate):
    """(struct, bands [n_bands, 4], bins) of mm_spectrum_host; the buffers carry a guard row."""
    from mastering_amd import native
    lib = native.load()
    x = np.ascontiguousarray(pcm, np.int16)
    m = native.MMSpectrum()
    bins = np.full((BINS + 1, 3), -7.0)
    bands = np.full((native.SPECTRUM_MAX_BANDS + 1, 4), -7.0)
    rc = lib.mm_spectrum_host(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), x.shape[0], 1 if x.ndim == 1 else x.shape[1],
                              rate, ctypes.byref(m), bands.ctypes.data_as(native.c_double_p),
                              bins.ctypes.data_as(native.c_double_p))
    assert rc == 0, rc
    assert (bins[-1] == -7.0).all() and (bands[m.n_bands:] == -7.0).all()  # nothing past the tables
    return m, bands[:m.n_bands].copy(), bins[:-1].copy()


def tail(bins, frames, ch, rate):
    from mastering_amd import native
    m = native.MMSpectrum()
    bands = np.full((native.SPECTRUM_MAX_BANDS, 4), -7.0)
    b = np.ascontiguousarray(bins, np.float64)
    rc = native.load().mm_spectrum_from_bins(b.ctypes.data_as(native.c_double_p), frames, ch, rate, ctypes.byref(m),
                                             bands.ctypes.data_as(native.c_double_p))
    assert rc == 0, rc
    return m, bands[:m.n_bands].copy()


def bins_close(got, want, rel=REL):
    """Every bin and column within `rel` of its scale (S: itself; C: the mean of S_L and S_R), the
    bins below FLOOR of the largest within `rel` of that floor.  Returns the worst ratio."""
    if np.isnan(want).all():
        return 0.0 if np.isnan(got).all() else np.inf
    P = want[:, 0] + want[:, 1]
    scale = np.stack([np.abs(want[:, 0]), np.abs(want[:, 1]), P / 2], axis=1)
    return float(np.max(np.abs(got - want) / (rel * np.maximum(scale, FLOOR * P.max()) + 1e-300)))


def signal(kind, n, ch, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "noise":
        x = rng.integers(-20000, 20000, (n, 2))
    elif kind == "sine":
        x = np.stack([np.rint(30000 * np.sin(2 * np.pi * 0.01234 * t)), np.rint(12000 * np.cos(2 * np.pi * 0.2101 * t + 1.0))], axis=1)
    elif kind == "impulse":
        x = np.zeros((n, 2))
        if n:
            x[min(n - 1, 5000), 0] = -32768
            x[n // 3, 1] = 32767
    else:
        x = np.zeros((n, 2))
    x = x.astype(np.int16)
    return np.ascontiguousarray(x if ch == 2 else x[:, 0])


LENGTHS = (0, 1, N - 1, N, N + H - 1, N + H, 3 * N + 5)


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("kind", ["noise", "sine", "impulse", "zeros"])
def test_host_against_numpy(kind, ch):
    for i, n in enumerate(LENGTHS):
        rate = (2000, 44100, 192000)[i % 3]
        x = signal(kind, n, ch, seed=n)
        m, bands, bins = host_spectrum(x, rate)
        want = ref_spectrum(x)
        assert (m.frames, m.channels, m.rate, m.n_fft, m.hop, m.n_frames) == (n, ch, rate, N, H, n_frames(n))
        assert bins_close(bins, want) <= 1.0, (n, bins_close(bins, want))
        e = ref_edges(rate)
        assert m.n_bands == len(e) == bands.shape[0]
        if m.n_frames == 0:
            assert np.isnan(bins).all() and np.isnan(bands[:, :3]).all() and math.isnan(m.total_ms[0]) and math.isnan(m.total_ms[1])
            continue
        if ch == 1:
            assert (bins[:, 1:] == 0).all() and (bands[:, 1:3] == 0).all() and m.total_ms[1] == 0.0
        wb = ref_bands(want, rate)
        total = max(float((want[:, 0] + want[:, 1]).sum() * 2 / NORM), 1e-300)
        assert np.max(np.abs(bands[:, :3] - wb[:, :3])) <= 1e-9 * total
        assert np.allclose(bands[:, 3], wb[:, 3], rtol=1e-12, atol=0)
        ck = np.full(BINS, 2.0)
        ck[0] = ck[-1] = 1.0
        for c in range(ch):
            assert m.total_ms[c] == pytest.approx(float((ck * want[:, c]).sum() / NORM), rel=1e-9, abs=1e-300)


@pytest.mark.parametrize("rate", [2000, 44100, 48000, 192000])
def test_band_geometry(rate):
    from mastering_amd import engine
    e = engine.spectrum_bands(rate)
    want = ref_edges(rate)
    assert e.shape == want.shape and np.allclose(e, want, rtol=1e-14, atol=0)
    assert e[0, 1] == pytest.approx(19.9526, abs=1e-3) and e[0, 0] == pytest.approx(17.7828, abs=1e-3)
    assert (e[1:, 0] == e[:-1, 2]).all()              # the bands partition: an upper edge IS the next lower edge
    assert e[-1, 2] == rate / 2 and e[-1, 0] < rate / 2  # the last band is clipped at rate / 2
    assert e[-2, 1] * 10 ** 0.05 <= rate / 2             # and only the last
    assert {2000: 18, 44100: 31, 48000: 32, 192000: 38}[rate] == len(e)
    with pytest.raises(ValueError):
        engine.spectrum_bands(1999)


@pytest.mark.parametrize("rate", [2000, 44100, 192000])
def test_tail_on_a_flat_table(rate):
    """S = 1 everywhere: a band's mean square is its width * 2 N / rate / NORM (every bin, the
    half-width ones at 0 and N/2 with their weight 1 too, holds 2 / df a hertz), and bins_in_band
    its width in bins; the 20 Hz band at 192 kHz rests on a fifth of a bin."""
    flat = np.ones((BINS, 3))
    m, bands = tail(flat, 3 * N, 2, rate)
    e = ref_edges(rate)
    width = e[:, 2] - e[:, 0]
    assert np.allclose(bands[:, 3], width * N / rate, rtol=1e-12, atol=0)
    for q in range(3):
        assert np.allclose(bands[:, q], 2.0 * width * N / rate / NORM, rtol=1e-12, atol=0)
    assert (bands[:, 3] > 0).all()  # no band is empty
    if rate == 192000:
        assert bands[0, 3] == pytest.approx(0.1965, abs=1e-3)
    assert m.total_ms[0] == pytest.approx(2.0 * (N / 2) / NORM, rel=1e-12)


@pytest.mark.parametrize("rate", [2000, 44100, 192000])
def test_tail_partitions_the_power(rate):
    rng = np.random.default_rng(rate)
    bins = rng.random((BINS, 3)) ** 4  # (some bins hold nearly nothing)
    bins[:, 2] -= 0.3
    m, bands = tail(bins, 3 * N, 2, rate)
    df, lo = rate / N, ref_edges(rate)[0, 0]
    k = np.arange(BINS)
    bl, bh = np.maximum(0.0, (k - 0.5) * df), np.minimum(rate / 2, (k + 0.5) * df)
    inside = np.clip((bh - np.maximum(bl, lo)) / (bh - bl), 0.0, 1.0)  # of a bin above the 20 Hz band's lower edge
    ck = np.where((k == 0) | (k == N // 2), 1.0, 2.0)
    for q in range(3):
        want = float((inside * ck * bins[:, q]).sum() / NORM)
        scale = float((inside * ck * np.abs(bins[:, q])).sum() / NORM)
        assert abs(bands[:, q].sum() - want) <= 1e-12 * scale
    assert bands[:, 3].sum() == pytest.approx((rate / 2 - lo) / df, rel=1e-12)


def test_rolloff_and_occupied_on_one_bin():
    from mastering_amd import engine, native
    rate, k0 = 48000, 1234
    bins = np.zeros((BINS, 3))
    bins[k0, :2] = (N / 4 * 0.5) ** 2  # the centre bin of a sine of amplitude 0.5 on bin k0, in both channels
    level = 10 * math.log10(0.25 * 2 / 3)  # (without its two side bins: 2/3 of the windowed sine's power)
    m, bands = tail(bins, 2 * N, 2, rate)
    d = engine.spectrum_dict(m, bands, bins)
    f0 = k0 * rate / N
    assert d["rolloff_hz"] == {"95": f0, "99": f0, "99.9": f0}
    assert engine.occupied_hz(bins, rate, -3.1) == f0 and engine.occupied_hz(bins, rate, -2.9) is None  # 2 * 0.25: -3.01 dB
    assert d["occupied_hz"] == {"-60": f0, "-90": f0}
    b = [x for x in d["bands"] if x["lo_hz"] <= f0 < x["hi_hz"]]
    assert len(b) == 1 and b[0]["level_dbfs"][0] == pytest.approx(level, abs=1e-9)
    assert b[0]["correlation"] == 0.0 and b[0]["cross_ms"] == 0.0  # (C is 0 in this table)
    bins[:, 2] = -bins[:, 0]
    m, bands = tail(bins, 2 * N, 2, rate)
    d = engine.spectrum_dict(m, bands, bins)
    b = [x for x in d["bands"] if x["lo_hz"] <= f0 < x["hi_hz"]][0]
    assert b["correlation"] == pytest.approx(-1.0, abs=1e-12) and b["mid_dbfs"] == -math.inf
    assert b["side_dbfs"] == pytest.approx(level, abs=1e-9)
    assert d["total_dbfs"][0] == pytest.approx(level, abs=1e-9)
    spread = np.zeros((BINS, 3))
    spread[100:200, 0] = 1.0  # 100 equal bins: 95 % at the 95th, 99 % at the 99th, 99.9 % at the last
    m, bands = tail(spread, 2 * N, 1, rate)
    d = engine.spectrum_dict(m, bands, spread)
    assert d["rolloff_hz"] == {"95": 194 * rate / N, "99": 198 * rate / N, "99.9": 199 * rate / N}
    m, bands = tail(np.full((BINS, 3), np.nan), N - 1, 2, rate)  # unmeasurable: None throughout
    d = engine.spectrum_dict(m, bands, np.full((BINS, 3), np.nan))
    assert d["n_frames"] == 0 and d["rolloff_hz"]["95"] is None and d["occupied_hz"]["-60"] is None
    assert d["bands"][3]["level_dbfs"] == [None, None] and d["bands"][3]["correlation"] is None and d["total_dbfs"] == [None, None]
    assert native.SPECTRUM_BINS == BINS


def level_db(S):
    return 10 * np.log10(16 * S / N ** 2)


def test_sine_on_a_bin():
    """Amplitude 16384 exactly on bin k0: -6.02 dBFS there and 6.02 dB less at k0 +- 1 (the Hann
    window's two side bins), nothing but rounding noise elsewhere."""
    k0 = 777
    x = np.rint(16384 * np.cos(2 * np.pi * k0 * np.arange(N + H) / N)).astype(np.int16)
    m, bands, bins = host_spectrum(x, 44100)
    db = level_db(bins[:, 0])
    assert db[k0] == pytest.approx(-6.0206, abs=2e-3)
    assert db[k0 - 1] == pytest.approx(db[k0] - 6.0206, abs=2e-3) and db[k0 + 1] == pytest.approx(db[k0] - 6.0206, abs=2e-3)
    rest = np.delete(db, [k0 - 1, k0, k0 + 1])
    assert rest.max() < -110
    assert 10 * math.log10(2 * m.total_ms[0]) == pytest.approx(-6.0206, abs=2e-3)


def test_impulse_fills_every_bin():
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
    for n0, v in ((1, 32767), (N // 2, -32768), (N - 1, 12345), (3001, -77)):
        x = np.zeros((N, 2), np.int16)
        x[n0, 0] = v
        x[n0, 1] = -v if v != -32768 else 32767
        m, bands, bins = host_spectrum(x, 48000)
        want_l, want_r = (w[n0] * v / 32768) ** 2, (w[n0] * int(x[n0, 1]) / 32768) ** 2
        assert np.allclose(bins[:, 0], want_l, rtol=1e-11, atol=0) and np.allclose(bins[:, 1], want_r, rtol=1e-11, atol=0)
        assert np.allclose(bins[:, 2], -math.sqrt(want_l * want_r), rtol=1e-11, atol=0)


def test_equal_and_opposite_channels():
    rng = np.random.default_rng(5)
    a = rng.integers(-16000, 16000, 2 * N + 17).astype(np.int16)
    m, bands, bins = host_spectrum(np.stack([a, a], axis=1), 44100)
    assert np.allclose(bins[:, 1], bins[:, 0], rtol=1e-12, atol=0) and np.allclose(bins[:, 2], bins[:, 0], rtol=1e-12, atol=0)
    m, bands, bins = host_spectrum(np.stack([a, -a], axis=1), 44100)
    assert np.allclose(bins[:, 1], bins[:, 0], rtol=1e-12, atol=0) and np.allclose(bins[:, 2], -bins[:, 0], rtol=1e-12, atol=0)
    assert np.allclose(bands[:, 2], -bands[:, 0], rtol=1e-12, atol=0)
    mono, _, bins1 = host_spectrum(a, 44100)
    assert np.allclose(bins1[:, 0], bins[:, 0], rtol=1e-12, atol=0) and mono.channels == 1


def test_refusals():
    from mastering_amd import native
    lib = native.load()
    x = np.zeros((16, 2), np.int16)
    p = x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))
    m = native.MMSpectrum()
    bins = np.zeros((BINS, 3))
    pb = bins.ctypes.data_as(native.c_double_p)

    def rc(frames=16, ch=2, rate=2000, out=ctypes.byref(m), pcm=p):
        return lib.mm_spectrum_host(pcm, frames, ch, rate, out, None, None)
    assert rc() == 0 and m.n_frames == 0 and m.n_bands == 18
    for bad in (dict(ch=0), dict(ch=3), dict(frames=-1), dict(frames=2 ** 31), dict(rate=1999), dict(out=None), dict(pcm=None)):
        assert rc(**bad) == native.MM_ERR_ARG, bad
    assert rc(frames=0, pcm=None) == 0 and m.frames == 0
    assert lib.mm_spectrum_from_bins(pb, 16, 2, 2000, ctypes.byref(m), None) == 0
    for args in ((None, 16, 2, 2000, ctypes.byref(m), None), (pb, 16, 2, 2000, None, None), (pb, 16, 3, 2000, ctypes.byref(m), None),
                 (pb, -1, 2, 2000, ctypes.byref(m), None), (pb, 16, 2, 1999, ctypes.byref(m), None)):
        assert lib.mm_spectrum_from_bins(*args) == native.MM_ERR_ARG, args
    assert lib.mm_spectrum_bands(1999, 0, None) == native.MM_ERR_ARG and lib.mm_spectrum_bands(2000, 1, None) == native.MM_ERR_ARG
    assert lib.mm_spectrum_bands(2000, -1, None) == native.MM_ERR_ARG and lib.mm_spectrum_bands(44100, 0, None) == 31


def test_spectrum_layout_matches_c(tmp_path):
    from mastering_amd import native
    fl = [f[0] for f in native.MMSpectrum._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mastering.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(mm_spectrum));']
    lines += [f'printf("{f} %zu\\n", offsetof(mm_spectrum, {f}));' for f in fl]
    lines += ['printf("bit %d\\n", MM_REPORT_SPECTRUM);', 'printf("abi %d\\n", MM_ABI_VERSION);',
              'printf("max %d\\n", MM_SPECTRUM_MAX_BANDS);', "return 0;}"]
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(native.MMSpectrum)
    for f in fl:
        assert int(got[f]) == getattr(native.MMSpectrum, f).offset, f
    assert int(got["bit"]) == native.REPORT_SPECTRUM == 8 and int(got["abi"]) == native.ABI_VERSION == 5
    assert int(got["max"]) == native.SPECTRUM_MAX_BANDS


def test_planning():
    from mastering_amd import engine
    job = engine.Job(44100, 44100, 2, {}, spectrum=True)
    assert job.job.meter_on == 8 and job.delivery is None
    assert engine.Job(44100, 44100, 2, {}, spectrum=True, qc=True, report=True, r128=True).job.meter_on == 15
    assert engine.Job(44100, 44100, 2, {}).job.meter_on == 0
    job = engine.Job(44100, 44100, 2, {}, spectrum=True, output_rate=48000)
    assert job.job.meter_on == 0 and job.delivery.meter_on == 8
    assert job.delivery.loud.contents.rate == 48000  # the report reads its rate there
    job = engine.Job(44100, 44100, 2, {}, spectrum=True, qc=True, deliver_lufs=-16.0)
    assert job.job.meter_on == 0 and job.delivery.meter_on == 12
    with pytest.raises(ValueError, match="spectrum report needs the whole track"):
        engine.Job(44100, 44100, 2, {}, spectrum=True, seg_bounds=[0, 44100])


def test_refused_where_qc_is():
    from mastering_amd import distributed, engine, legacy
    with pytest.raises(ValueError, match="spectrum report needs the whole track: not available on the time-sharded path"):
        distributed.master_time_sharded(None, None, {"spectrum": True}, None, None, None)
    with pytest.raises(ValueError, match="spectrum report belongs to the mastering chain's delivery"):
        legacy.master_pcm(np.zeros((10, 2), np.int16), 44100, {"spectrum": True})
    for fn in (engine.process_batch, engine.process_album):
        with pytest.raises(ValueError, match=r"takes no params\['spectrum'\]"):
            fn([], [], {"deliver_lufs": -14.0, "spectrum": True})
