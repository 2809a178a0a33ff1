"""The linear-phase FIR and the reference match on CPU: the library's host restatement
(mm_fir_host) against a numpy restatement of the definition in include/mastering.h (mm_fir),
refused tables, the design of the taps (design.match_taps) judged by the response of the
integer taps, the match rule (engine.match_gains) on hand-made spectra, the match end to end in
numpy, and the trim that keeps it from clipping.  Comparisons of samples and statistics are
equalities on integers; the design and end-to-end bounds are twice what this file measured on
the CPU, with the measured value beside each."""
import ctypes
import math

import numpy as np
import pytest

ONE = 1 << 22
RATES = (44100, 48000, 96000, 192000)
LENGTHS = {44100: 2047, 48000: 2227, 96000: 4457, 192000: 8191}


def ref_fir(pcm, taps):
    """The definition in numpy int64, vectorised over n with a loop over k: (out int16, stats)."""
    pcm = np.asarray(pcm)
    x = (pcm[:, None] if pcm.ndim == 1 else pcm).astype(np.int64)
    N, ch = x.shape
    c = np.asarray(taps, np.int64)
    K = c.size
    H = (K - 1) // 2
    z = np.concatenate([np.zeros((K, ch), np.int64), x, np.zeros((K, ch), np.int64)])  # z[i] = s[i - K]
    acc = np.zeros((N, ch), np.int64)
    for k in range(K):
        lo = H - k + K  # sample n + H - k of output n = 0
        acc += c[k] * z[lo:lo + N]
    y = (acc + (1 << 21)) >> 22
    out = np.clip(y, -32768, 32767)
    st = dict(frames=N, channels=ch, K=K, clipped=[int(v) for v in (y != out).sum(axis=0)],
              peak=[int(v) for v in np.abs(out).max(axis=0, initial=0)],
              peak_unclipped=[int(v) for v in np.abs(y).max(axis=0, initial=0)])
    return out.astype(np.int16).reshape(pcm.shape), st


def fir_stats(d):
    """A fir_dict cut to ref_fir's statistics."""
    return {k: d[k] for k in ("frames", "channels", "K", "clipped", "peak", "peak_unclipped")}


def host_fir(pcm, taps, rate=44100):
    """mm_fir_host, raw: (rc, out filled with 77 beforehand, the struct)."""
    from mastering_amd import native
    x = np.ascontiguousarray(pcm, np.int16)
    ch = 1 if x.ndim == 1 else x.shape[1]
    c = np.ascontiguousarray(taps, np.int32)
    f = native.MMFir()
    f.rate, f.K, f.taps_key = rate, c.size, 0
    f.taps = c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out = np.full(x.shape, 77, np.int16)
    m = native.MMFirResult()
    p16 = ctypes.POINTER(ctypes.c_int16)
    rc = native.load().mm_fir_host(x.ctypes.data_as(p16), x.shape[0], ch, ctypes.byref(f), out.ctypes.data_as(p16),
                                   ctypes.byref(m))
    return rc, out, m


def random_taps(K, seed, total=0.99):
    """Symmetric int32 taps of both signs with sum |c| = about `total` * 2^24 and a DC gain of
    about half of that (so that the rails and hot signals clip at `total` 0.99)."""
    rng = np.random.default_rng(seed)
    H = (K - 1) // 2
    half = (rng.standard_normal(H + 1) + 0.8) * np.hanning(2 * H + 3)[1:H + 2]
    c = np.concatenate([half, half[:H][::-1]])
    c = np.rint(c / np.abs(c).sum() * total * (1 << 24)).astype(np.int64)
    c[:H] = c[:H:-1]
    assert np.array_equal(c, c[::-1]) and np.abs(c).sum() < 1 << 24
    return c.astype(np.int32)


def signals(N, ch, seed):
    """Noise, hard-clipped noise, a full-scale square and constants at both rails, [N, ch] each
    (mono: [N]); the channels differ, and none is symmetric in time."""
    rng = np.random.default_rng(seed)
    shape = (N,) if ch == 1 else (N, ch)
    noise = np.clip(rng.standard_normal(shape) * 6000, -32768, 32767)
    hot = np.clip(rng.standard_normal(shape) * 40000, -32768, 32767)
    n = np.arange(N)
    sq = np.where((n // 37) % 2 == 0, 32767, -32768)
    sq = sq if ch == 1 else np.stack([sq, -1 - sq], axis=1)
    return {"noise": noise.astype(np.int16), "clipped noise": hot.astype(np.int16), "square": sq.astype(np.int16),
            "top rail": np.full(shape, 32767, np.int16), "bottom rail": np.full(shape, -32768, np.int16)}


# ------------------------------------------------------------------ the host restatement
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("K", [3, 5, 129, 2047, 8191])
def test_host_restatement_is_the_definition(K, ch):
    """mm_fir_host equals ref_fir, samples and statistics, at every length around the half
    length and on signals that clip; the noise cases are the check of the indexing (symmetric
    taps hide a reversed index on a symmetric signal only)."""
    H = (K - 1) // 2
    taps = random_taps(K, K)
    clipped = 0
    for N in (0, 1, H, H + 1, K, 5000):
        for name, x in signals(N, ch, 100 * K + N).items():
            rc, out, m = host_fir(x, taps)
            assert rc == 0, (N, name)
            want, st = ref_fir(x, taps)
            assert np.array_equal(out, want), (N, name)
            assert m.rate == 44100
            got = dict(frames=int(m.frames), channels=int(m.channels), K=int(m.K),
                       clipped=[int(m.clipped[c]) for c in range(ch)], peak=[int(m.peak[c]) for c in range(ch)],
                       peak_unclipped=[int(m.peak_unclipped[c]) for c in range(ch)])
            assert got == st, (N, name)
            clipped += sum(st["clipped"])
    assert clipped > 0  # (the clip and its count were exercised)


def test_an_off_centre_impulse_comes_out_as_the_taps():
    from mastering_amd import engine
    K, N, p, A = 129, 400, 37, 1 << 12
    H = (K - 1) // 2
    taps = random_taps(K, 7, total=0.2)
    x = np.zeros(N, np.int16)
    x[p] = A
    out, st = engine.fir_host(x, 48000, taps)
    want = np.zeros(N, np.int64)
    for n in range(N):
        k = n + H - p  # the tap that meets the impulse at output n
        if 0 <= k < K:
            want[n] = (int(taps[k]) * A + (1 << 21)) >> 22
    assert np.array_equal(out, want) and st["clipped"] == [0] and st["rate"] == 48000
    assert np.flatnonzero(out)[-1] <= p + H < N and want[p] == (int(taps[H]) * A + (1 << 21)) >> 22
    assert np.array_equal(out, ref_fir(x, taps)[0])


def test_refused_tables_and_signals_write_nothing():
    x = np.arange(-50, 50, dtype=np.int16)
    good = random_taps(9, 1)
    assert host_fir(x, good)[0] == 0
    off = good.copy()
    off[1] += 1
    full = np.zeros(5, np.int32)
    full[[0, 4]] = 1 << 22
    full[2] = 1 << 23  # sum |c| = 2^24 exactly
    under = full.copy()
    under[2] -= 1
    assert host_fir(x, under)[0] == 0
    cases = {"even K": random_taps(9, 1)[:8], "K = 1": np.array([ONE], np.int32), "K = 8193": np.ones(8193, np.int32),
             "one tap off symmetry": off, "sum |c| = 2^24": full}
    for name, taps in cases.items():
        rc, out, _ = host_fir(x, taps)
        assert rc == -1 and np.all(out == 77), name
    rc, out, _ = host_fir(np.zeros((40, 3), np.int16), good)
    assert rc == -1 and np.all(out == 77)
    from mastering_amd import engine
    with pytest.raises(ValueError):
        engine.fir_host(x, 44100, off)


def test_struct_layouts_match_c(tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    from mastering_amd import native
    classes = {"mm_fir": native.MMFir, "mm_fir_result": native.MMFirResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mastering.h"', "int main(void){"]
    for st, cls in classes.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for st, cls in classes.items():
        assert int(got[st]) == ctypes.sizeof(cls), st
        for f, _ in cls._fields_:
            assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"


# ------------------------------------------------------------------ the design
TILT_MEASURED_DB = 0.0277  # worst |realised - asked| of the tilt over the four rates, measured here
TILT_BOUND_DB = 0.056      # twice that


def tilt(rate):
    from mastering_amd import engine
    centres = engine.spectrum_bands(rate)[:, 1]
    return centres, np.linspace(6.0, -6.0, centres.size)


@pytest.mark.parametrize("rate", RATES)
def test_a_tilt_is_realised_by_the_integer_taps(rate):
    """+6 ... -6 dB linear over the band index, at every band centre from 100 Hz up to rate / 2 (the
    last band's nominal centre lies above rate / 2 at 48, 96 and 192 kHz: no frequency of the signal)."""
    from mastering_amd import design
    assert design.match_length(rate) == LENGTHS[rate]
    centres, g = tilt(rate)
    taps = design.match_taps(rate, g)
    assert taps.dtype == np.int32 and taps.size == LENGTHS[rate]
    assert np.array_equal(taps, taps[::-1])
    assert int(np.abs(taps.astype(np.int64)).sum()) < 1 << 24
    judged = (centres >= 100.0) & (centres <= rate / 2)
    err = np.abs(design.fir_response_db(taps, rate, centres) - g)[judged]
    print(f"tilt at {rate} Hz: worst {err.max():.4f} dB over {judged.sum()} bands")
    assert err.max() <= TILT_BOUND_DB
    assert np.array_equal(design.match_taps(rate, g, trim=1.0), taps)
    half = design.match_taps(rate, g, trim=0.5)
    assert np.array_equal(half, half[::-1]) and np.abs(2 * half.astype(np.int64) - taps).max() <= 1
    assert design.match_key(taps) == design.match_key(taps.copy()) != design.match_key(half) and design.match_key(taps)


def test_match_taps_refusals_and_limits():
    from mastering_amd import design
    centres, g = tilt(44100)
    for K in (2, 1, 8193, 2048):
        with pytest.raises(ValueError):
            design.match_taps(44100, g, K)
    with pytest.raises(ValueError):
        design.match_taps(44100, g[:-1])
    with pytest.raises(ValueError):
        design.match_taps(44100, np.full(centres.size, 30.0))  # a flat +30 dB: sum |c| >= 2^24


def test_tap_sums_stay_under_the_limit_with_the_headroom_trim():
    """sum |c| < 2^24 for curves within +-12 dB.  2^24 is 4 * 2^22, a tap sum of 4, and a curve
    whose boosts and cuts alternate has a sum far above its largest gain: measured here at trim 1,
    in units of 2^22, a flat +12 dB has 3.98, a smooth +-6 dB sine 4.24 / 4.26 (44.1 / 192 kHz), a
    6-band +12 dB bump 7.59 / 7.56, a -12 / +12 dB step 10.9 / 11.0, bands alternating +-12 dB 15.2
    / 18.7.  So match_taps refuses
    those at trim 1, and the match designs every table under design.match_headroom's trim, with
    which the bound holds by construction; that is what is asserted, with the table still using
    the room it has."""
    from mastering_amd import design
    rng = np.random.default_rng(3)
    for rate in RATES:
        n = tilt(rate)[0].size
        i = np.arange(n)
        curves = {"flat": np.full(n, 12.0), "sine": 6.0 * np.sin(i * (2 * np.pi / 20.0)),
                  "bump": np.where(np.abs(i - 17) < 3, 12.0, -2.0), "step": np.where(i < 15, -12.0, 12.0),
                  "alternating": np.where(i % 2, 12.0, -12.0), "random": rng.uniform(-12, 12, n)}
        for name, curve in curves.items():
            fit = design.match_headroom(rate, curve)
            taps = design.match_taps(rate, curve, trim=fit)
            total = int(np.abs(taps.astype(np.int64)).sum())
            assert total < 1 << 24 and 0.0 < fit <= 1.0, (rate, name)
            if name == "flat":
                assert fit == 1.0 and np.array_equal(taps, design.match_taps(rate, curve))
            else:
                assert fit < 1.0 and total > (1 << 24) - 2 * taps.size, (rate, name)
                with pytest.raises(ValueError):
                    design.match_taps(rate, curve)


def test_realised_db_reports_what_the_design_cannot_follow():
    """A 24 dB step between neighbouring bands and a jagged curve are not promised; the match_dict's
    realised_db is fir_response_db of the taps, so the caller sees the deviation."""
    from mastering_amd import design, engine
    centres, _ = tilt(44100)
    n = centres.size
    for curve in (np.where(np.arange(n) < 15, -12.0, 12.0), np.where(np.arange(n) % 2, 9.0, -9.0)):
        gains = {"status": "matched", "amount": 1.0, "max_db": 12.0, "gains_db": list(curve),
                 "bands": [{"centre_hz": float(c), "gain_db": float(g)} for c, g in zip(centres, curve)]}
        seen = []
        d = engine.match_apply(lambda taps: (seen.append(taps), ref_fir(np.zeros(8, np.int16), taps)[1])[1], gains, 44100)
        fit = design.match_headroom(44100, curve)
        want = design.fir_response_db(seen[0], 44100, centres) - 20 * math.log10(fit)  # (trim excluded)
        assert np.array_equal(seen[0], design.match_taps(44100, curve, trim=fit))
        assert [b["realised_db"] for b in d["bands"]] == [float(v) for v in want]
        assert d["passes"] == 1 and d["trim_db"] == 20 * math.log10(fit) < 0.0 and d["K"] == 2047
        assert np.abs(want - curve).max() > 0.5  # (the deviation is there to be seen)


# ------------------------------------------------------------------ the match rule
def spectrum(rate, levels_db, channels=1, n_frames=10, bins=None):
    """A hand-made spectrum_dict: `levels_db` (10 log10 ms) a band, the same in every channel
    unless a band's entry is a tuple; None: a band without a bin."""
    from mastering_amd import engine
    bands = []
    for i, (lo, centre, hi) in enumerate(engine.spectrum_bands(rate)):
        lv = levels_db[i] if i < len(levels_db) else -200.0
        lv = lv if isinstance(lv, tuple) else (lv,) * channels
        bands.append({"centre_hz": float(centre), "lo_hz": float(lo), "hi_hz": float(hi),
                      "bins_in_band": 0.0 if bins is not None and i in bins else 4.0,
                      "ms": [0.0 if v == -math.inf else 10.0 ** (v / 10.0) for v in lv]})
    return {"rate": rate, "channels": channels, "n_frames": n_frames, "bands": bands}


def test_match_rule_mean_clip_and_amount():
    from mastering_amd import engine
    n = len(engine.spectrum_bands(44100))
    src = spectrum(44100, [-40.0] * n)
    d_true = np.array([3.0 + 0.5 * i for i in range(n)])
    ref = spectrum(44100, list(-40.0 + d_true))
    g = engine.match_gains(src, ref)
    assert g["status"] == "matched" and g["comparable"] == n and all(b["comparable"] for b in g["bands"])
    assert np.allclose(g["gains_db"], d_true - d_true.mean(), atol=1e-9) and abs(sum(g["gains_db"])) < 1e-9
    g = engine.match_gains(src, ref, max_db=4.0)
    assert np.allclose(g["gains_db"], np.clip(d_true - d_true.mean(), -4.0, 4.0), atol=1e-9)
    g = engine.match_gains(src, ref, amount=0.25, max_db=4.0)
    assert np.allclose(g["gains_db"], 0.25 * np.clip(d_true - d_true.mean(), -4.0, 4.0), atol=1e-9)
    assert engine.match_gains(src, ref, amount=0.0)["gains_db"] == [0.0] * n
    assert g["bands"][3]["source_dbfs"] == pytest.approx(-40.0) and g["bands"][3]["reference_dbfs"] == pytest.approx(-35.5)
    for bad in (dict(amount=1.5), dict(amount=-0.1), dict(max_db=-1.0)):
        with pytest.raises(ValueError):
            engine.match_gains(src, ref, **bad)


def test_match_rule_fills_from_the_nearest_comparable_band():
    from mastering_amd import engine
    n = len(engine.spectrum_bands(44100))
    lv = [-40.0] * n
    ref_lv = [-40.0 + (6.0 if i >= 10 else 0.0) for i in range(n)]
    for i in (0, 1, 2):
        lv[i] = -95.0  # below the floor in the source
    ref_lv[12] = -120.0  # below the floor in the reference: between 11 and 13, the tie goes to 11
    ref_lv[11], ref_lv[13] = -38.0, -30.0
    src, ref = spectrum(44100, lv, bins={20}), spectrum(44100, ref_lv, bins={n - 1})
    g = engine.match_gains(src, ref)
    out = {0, 1, 2, 12, 20, n - 1}
    assert [not b["comparable"] for b in g["bands"]] == [i in out for i in range(n)]
    gains = g["gains_db"]
    d = {i: ref_lv[i] - lv[i] for i in range(n) if i not in out}
    mean = sum(d.values()) / len(d)
    for i in d:
        assert gains[i] == pytest.approx(d[i] - mean)
    assert gains[0] == gains[1] == gains[2] == gains[3]
    assert gains[12] == gains[11] != gains[13]
    assert gains[20] == gains[19] and gains[n - 1] == gains[n - 2]  # (19 and 21 hold the same gain or not: the lower)


def test_match_rule_mixed_rates_and_channel_counts():
    """A 44.1 kHz stereo source against a 96 kHz mono reference: the bands of equal edges are
    compared (the source's Nyquist-clipped band has other edges there), one curve for both channels
    from the mean of their ms."""
    from mastering_amd import engine
    b44, b96 = engine.spectrum_bands(44100), engine.spectrum_bands(96000)
    n = len(b44)
    assert b44[-1][2] == 22050.0 and b96[n - 1][2] != 22050.0
    src = spectrum(44100, [(-43.0, -37.0)] * n, channels=2)
    mean_db = 10 * math.log10((10 ** -4.3 + 10 ** -3.7) / 2)
    ref = spectrum(96000, [-30.0 + (i % 3) for i in range(len(b96))])
    g = engine.match_gains(src, ref)
    assert [b["comparable"] for b in g["bands"]] == [True] * (n - 1) + [False]
    d = np.array([-30.0 + (i % 3) - mean_db for i in range(n - 1)])
    assert np.allclose(g["gains_db"][:-1], d - d.mean(), atol=1e-9) and g["gains_db"][-1] == g["gains_db"][-2]
    assert g["bands"][0]["source_dbfs"] == pytest.approx(mean_db)
    assert g["bands"][-1]["reference_dbfs"] is None


def test_match_rule_unmeasurable():
    from mastering_amd import engine
    n = len(engine.spectrum_bands(44100))
    ref = spectrum(44100, [-30.0] * n)
    two = spectrum(44100, [-40.0, -41.0] + [-math.inf] * (n - 2))
    g = engine.match_gains(two, ref)
    assert g["status"] == "unmeasurable" and g["comparable"] == 2 and g["gains_db"] == [0.0] * n
    three = spectrum(44100, [-40.0, -41.0, -42.0] + [-math.inf] * (n - 3))
    assert engine.match_gains(three, ref)["status"] == "matched"
    for a, b in ((spectrum(44100, [-40.0] * n, n_frames=0), ref), (ref, spectrum(44100, [-40.0] * n, n_frames=0))):
        g = engine.match_gains(a, b)
        assert g["status"] == "unmeasurable" and g["comparable"] == 0
    d = engine.match_apply(lambda taps: pytest.fail("an unmeasurable match filters nothing"), g, 44100)
    assert d["status"] == "unmeasurable" and d["passes"] == 0 and d["fir"] is None and d["trim_db"] == 0.0


# ------------------------------------------------------------------ end to end in numpy
def host_spectrum(pcm, rate):
    """spectrum_dict of the library's host restatement (mm_spectrum_host; no GPU)."""
    from mastering_amd import engine, native
    x = np.ascontiguousarray(pcm, np.int16)
    ch = 1 if x.ndim == 1 else x.shape[1]
    m = native.MMSpectrum()
    bands = np.zeros((native.SPECTRUM_MAX_BANDS, 4), np.float64)
    bins = np.zeros((native.SPECTRUM_BINS, 3), np.float64)
    rc = native.load().mm_spectrum_host(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), x.shape[0], ch, rate, ctypes.byref(m),
                                        bands.ctypes.data_as(native.c_double_p), bins.ctypes.data_as(native.c_double_p))
    assert rc == 0
    return engine.spectrum_dict(m, bands[:m.n_bands], bins)


def band_levels(spec):
    return np.array([10 * math.log10(sum(b["ms"]) / len(b["ms"])) for b in spec["bands"]])


E2E_SAME_MEASURED_DB, E2E_SAME_BOUND_DB = 0.190, 0.380    # reference: the source itself through the curve
E2E_OTHER_MEASURED_DB, E2E_OTHER_BOUND_DB = 0.203, 0.406  # reference: an independent noise through the curve


def test_match_end_to_end_in_numpy():
    """2 s of white noise (sigma 3000, 44.1 kHz) is matched to a reference that is noise through a
    known smooth +-6 dB curve: after match_gains -> match_taps -> ref_fir the band levels of the
    result minus the reference's, mean removed, stay small at every centre from 200 Hz up.  Bounds:
    twice what this composition measured here."""
    from mastering_amd import design, engine
    rate, N = 44100, 88200
    centres, _ = tilt(rate)
    curve = 6.0 * np.sin(np.arange(centres.size) * (2 * np.pi / 20.0))
    shape = design.match_taps(rate, curve, trim=design.match_headroom(rate, curve))  # (its level does not matter)
    src = np.rint(np.random.default_rng(11).standard_normal(N) * 3000).astype(np.int16)
    other = np.rint(np.random.default_rng(12).standard_normal(N) * 3000).astype(np.int16)
    s_src = host_spectrum(src, rate)
    judged = centres >= 200.0
    for name, noise, bound in (("same", src, E2E_SAME_BOUND_DB), ("other", other, E2E_OTHER_BOUND_DB)):
        s_ref = host_spectrum(ref_fir(noise, shape)[0], rate)
        gains = engine.match_gains(s_src, s_ref)
        assert gains["status"] == "matched"
        outs = []
        d = engine.match_apply(lambda taps: (outs.append(ref_fir(src, taps)), outs[-1][1])[1], gains, rate)
        assert d["passes"] == 1 and d["fir"]["clipped"] == [0] and d["trim_db"] <= 0.0
        diff = band_levels(host_spectrum(outs[-1][0], rate)) - band_levels(s_ref)
        comparable = np.array([b["comparable"] for b in d["bands"]])
        diff = (diff - diff[comparable].mean())[judged & comparable]
        print(f"match end to end ({name} noise as reference): worst {np.abs(diff).max():.4f} dB over {diff.size} bands")
        assert np.abs(diff).max() <= bound


# ------------------------------------------------------------------ the trim
def test_trim_keeps_the_second_pass_from_clipping():
    """A 1 kHz square at +-32000 under a curve with +12 dB at 1 kHz clips in pass one; the taps are
    redesigned with design.match_trim and applied from the untouched source: no clip, and the largest
    |y| obeys |y'| <= trim P + (trim + 1) K / 256 + 1 <= 32767 with P the first pass's."""
    from mastering_amd import design, engine
    rate = 44100
    centres, _ = tilt(rate)
    n = np.arange(6000)
    x = np.where((n * 1000 * 2 // rate) % 2 == 0, 32000, -32000).astype(np.int16)
    x = np.stack([x, np.roll(x, 7)], axis=1)
    curve = np.where(np.abs(np.log2(centres / 1000.0)) < 0.7, 12.0, -2.0)
    gains = {"status": "matched", "amount": 1.0, "max_db": 12.0, "gains_db": list(curve),
             "bands": [{"centre_hz": float(c), "gain_db": float(g)} for c, g in zip(centres, curve)]}
    passes = []
    d = engine.match_apply(lambda taps: (passes.append((taps, ref_fir(x, taps)[1])), passes[-1][1])[1], gains, rate)
    K = d["K"]
    assert len(passes) == 2 and d["passes"] == 2 and d["trim_db"] < 0.0
    first, second = passes[0][1], passes[1][1]
    assert sum(first["clipped"]) > 0 and second["clipped"] == [0, 0] and d["fir"] == second
    P = max(first["peak_unclipped"])
    fit, trim = design.match_headroom(rate, curve), design.match_trim(K, P)  # (the table's own trim, and the clip's)
    assert d["trim_db"] == 20 * math.log10(fit * trim) and trim == (32767 - K / 128 - 1) / P
    assert np.array_equal(passes[0][0], design.match_taps(rate, curve, K, fit))
    assert np.array_equal(passes[1][0], design.match_taps(rate, curve, K, fit * trim))
    assert max(second["peak_unclipped"]) <= trim * P + (trim + 1) * K / 256 + 1 <= 32767
    assert max(second["peak_unclipped"]) >= 32767 - K / 64 - 2  # (the same bound from below: no headroom wasted)
    realised = design.fir_response_db(passes[0][0], rate, centres) - 20 * math.log10(fit)
    assert [b["realised_db"] for b in d["bands"]] == [float(v) for v in realised]  # (trim excluded)


# ------------------------------------------------------------------ where the match does not run
def test_match_is_refused_before_any_device_work(tmp_path):
    """Every refusal names the key and comes before a file is read or the device touched (no GPU
    here): the batch, album, time-sharded, staged and legacy paths, which plan with Job or check
    their params first, and a reference that is not a 16-bit PCM WAV."""
    from mastering_amd import distributed, engine, legacy, wavio
    n = len(engine.spectrum_bands(44100))
    M = {"reference": spectrum(44100, [-40.0] * n)}
    x = np.zeros((4410, 2), np.int16)
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(ValueError, match="match"):
        engine.Job(4410, 44100, 2, {"match": M})  # what master_batch, deliver_batch, master_album and a staged job plan with
    for call in (engine.process_batch, engine.process_album):
        with pytest.raises(ValueError, match=r"params\['match'\]"):
            call([missing], [str(tmp_path / "o.wav")], {"deliver_lufs": -14.0, "match": M})
    with pytest.raises(ValueError, match="match"):
        distributed.master_time_sharded(None, None, {"match": M}, None, None, None)
    with pytest.raises(ValueError, match="match"):
        legacy.master_pcm(x, 44100, {"match": M})
    with pytest.raises(ValueError, match="match"):
        legacy.process(missing, str(tmp_path / "o.wav"), {"match": M})
    wide = str(tmp_path / "float.wav")
    wavio.write_wav(wide, np.zeros((9000, 2), np.float32), 44100)
    for run in (lambda m: engine.master_pcm(x, 44100, {"match": m}),
                lambda m: engine.process(missing, str(tmp_path / "o.wav"), {"match": m})):
        with pytest.raises(ValueError, match="16-bit"):
            run({"reference": wide})
        for bad in ({"amount": 0.5}, M["reference"], dict(M, strength=1.0), dict(M, amount=2.0), dict(M, max_db=-3.0)):
            with pytest.raises(ValueError, match="match"):
                run(bad)


def test_worker_resolves_a_reference_inside_its_object_tree(tmp_path):
    """A queue message names a reference as an object of the tree, never as a path of the worker's
    own file system: what object_path refuses is refused before anything is read, and an object
    that is there is the file the match opens (here one it then refuses: float, not 16-bit PCM)."""
    from mastering_amd import wavio, worker
    root = tmp_path / "root"
    (root / "b").mkdir(parents=True)
    wavio.write_wav(str(root / "b" / "ref.wav"), np.zeros((9000, 2), np.float32), 44100)
    outside = tmp_path / "outside.wav"
    wavio.write_wav(str(outside), np.zeros((9000, 2), np.float32), 44100)
    for bad in (str(outside), "gs://b/../../outside.wav", "gs://../outside.wav", "ref.wav"):
        with pytest.raises(ValueError, match="object URI|escapes|bucket"):
            worker.process_audio_from_gcs("gs://b/in.wav", {"match": {"reference": bad}}, root=str(root))
    with pytest.raises(ValueError, match="16-bit"):
        worker.process_audio_from_gcs("gs://b/in.wav", {"match": {"reference": "gs://b/ref.wav"}}, root=str(root))
    spec = {"match": {"reference": {"bands": []}}}
    assert worker._resolve_match(spec, str(root)) is spec
