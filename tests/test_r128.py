"""The EBU R 128 report on CPU: the library's host restatement (mm_r128_host) and its tail
(mm_r128_from_hops) against a short numpy/scipy restatement of the definition in
include/mastering.h, the EBU Tech 3341 / 3342 known answers, the mm_r128 layout and the
Python planning that needs no GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIGURES = ("integrated", "relative_gate", "momentary_max", "short_term_max", "lra", "lra_low", "lra_high")


# ------------------------------------------------------------ the definition, in numpy
def bounds(hops, rate):
    return np.arange(hops + 1, dtype=np.int64) * rate // 10


def design_rate(rate):
    """The rate whose K-weighting sections a test passes for a signal at `rate`: its own,
    except below 3.1 kHz, where design.kweight_sections is no filter to measure with (its
    shelf at 1500 Hz lies at or above Nyquist and its poles outside the unit circle: the
    outputs overflow within a second).  The sections are the caller's, and what the cases
    at the library's floor of 2000 Hz are about is the hop geometry (hops of 200 frames),
    so they run with the stable sections of 8 kHz."""
    return rate if rate > 3100 else 8000


def ref_hops(pcm, rate):
    """Steps 1-2: lfilter per channel in f64 from a zero state, squares summed per hop."""
    import scipy.signal
    from mastering_amd import design
    y = np.asarray(pcm).reshape(len(pcm), -1).astype(np.float64) / 32768.0
    for b0, b1, b2, a1, a2 in design.kweight_sections(design_rate(rate)):
        y = scipy.signal.lfilter([b0, b1, b2], [1.0, a1, a2], y, axis=0)
    B = bounds(10 * len(y) // rate, rate)
    return np.array([np.sum(y[B[i]:B[i + 1]] ** 2) for i in range(len(B) - 1)])


def level(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def windows(e, rate, w):
    H, B = len(e), bounds(len(e), rate)
    z = np.array([np.sum(e[j:j + w]) / (B[j + w] - B[j]) for j in range(max(H - w + 1, 0))])
    return z, level(z)


def ref_r128(e, rate):
    """Steps 3-7 by plain slicing; also the block levels and gates, for the tests' margins."""
    e = np.asarray(e, np.float64)
    r = {f: math.nan for f in FIGURES}
    r.update(hops=len(e), lra_blocks=0, levels=[], gates=[])
    if len(e) >= 4:
        z, l = windows(e, rate, 4)
        r["momentary_max"] = l.max()
        r["levels"] += list(l)
        r["integrated"] = -math.inf
        if (l > -70).any():
            gate = level(z[l > -70].mean()) - 10.0
            r["relative_gate"] = gate
            r["integrated"] = level(z[(l > -70) & (l > gate)].mean())
            r["gates"].append(gate)
    if len(e) >= 30:
        z, l = windows(e, rate, 30)
        r["short_term_max"] = l.max()
        r["levels"] += list(l)
        r["lra"] = 0.0
        if (l > -70).any():
            gate = level(z[l > -70].mean()) - 20.0
            r["gates"].append(gate)
            k = np.sort(l[(l > -70) & (l > gate)])
            n = r["lra_blocks"] = len(k)
            r["lra_low"], r["lra_high"] = k[((n - 1) * 10 + 50) // 100], k[((n - 1) * 95 + 50) // 100]
            r["lra"] = r["lra_high"] - r["lra_low"]
    return r


def gate_margin(r):
    """The smallest distance of a finite block level from -70 or from a relative gate."""
    l = np.array([v for v in r["levels"] if math.isfinite(v)])
    return min(np.abs(l - g).min() for g in [-70.0] + r["gates"])


# ------------------------------------------------------------ the library
def host_r128(pcm, rate):
    """(hop energies, mm_r128) of mm_r128_host."""
    from mastering_amd import engine, native
    lib = native.load()
    x = np.ascontiguousarray(pcm, np.int16)
    H = 10 * x.shape[0] // rate
    e = np.zeros(H + 1)
    m = native.MMR128()
    rc = lib.mm_r128_host(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), x.shape[0], 1 if x.ndim == 1 else x.shape[1],
                          rate, engine.kweight_sos(design_rate(rate)), e.ctypes.data_as(native.c_double_p), H, ctypes.byref(m))
    assert rc == 0
    assert m.frames == x.shape[0] and m.hops == H and m.rate == rate and e[H] == 0.0
    return e[:H], m


def from_hops(e, rate):
    from mastering_amd import native
    e = np.ascontiguousarray(e, np.float64)
    m = native.MMR128()
    assert native.load().mm_r128_from_hops(e.ctypes.data_as(native.c_double_p), len(e), rate, ctypes.byref(m)) == 0
    assert m.hops == len(e)
    return m


def same(a, b, tol=0.0):
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= tol


# ------------------------------------------------------------ signals
def stepped_noise(n, rate, channels, seed=11):
    """Pink noise with level steps: -12 dBFS, then 9 dB lower, 15 dB lower and 4 dB lower,
    a quarter of the signal each."""
    from signals import _layout, _pink
    cols = _pink(n, rate, seed, -12.0)
    for c in cols:
        for q, db in enumerate((0.0, -9.0, -15.0, -4.0)):
            c[q * n // 4:(q + 1) * n // 4 if q < 3 else n] *= 10.0 ** (db / 20.0)
    return _layout(cols, channels)


def sine(parts, rate, channels=2):
    """1 kHz sine, in phase on every channel: (dBFS peak, seconds) parts back to back."""
    amp = np.concatenate([np.full(int(round(s * rate)), 32768.0 * 10.0 ** (db / 20.0)) for db, s in parts])
    s = np.round(amp * np.sin(2 * np.pi * 1000.0 * np.arange(len(amp)) / rate)).astype(np.int16)
    return s if channels == 1 else np.ascontiguousarray(np.stack([s, s], axis=1))


EBU_3341 = {  # Tech 3341 cases 1-4: signal, required integrated loudness (+- 0.1 LU)
    "3341-1": ([(-23.0, 20)], -23.0),
    "3341-2": ([(-33.0, 20)], -33.0),
    "3341-3": ([(-36.0, 10), (-23.0, 60), (-36.0, 10)], -23.0),
    "3341-4": ([(-72.0, 10), (-36.0, 10), (-23.0, 60), (-36.0, 10), (-72.0, 10)], -23.0),
}
EBU_3342 = {  # Tech 3342 cases 1-3: signal, required loudness range (+- 1 LU)
    "3342-1": ([(-20.0, 20), (-30.0, 20)], 10.0),
    "3342-2": ([(-20.0, 20), (-15.0, 20)], 5.0),
    "3342-3": ([(-40.0, 20), (-20.0, 20)], 20.0),
}


# ------------------------------------------------------------ tests
@pytest.mark.parametrize("rate,n,ch", [(44100, 321987, 2), (44100, 321987, 1), (2000, 6001, 2), (192000, 250003, 1),
                                       (48000, 1, 2), (48000, 4799, 1), (48000, 4800, 2)])
def test_host_hop_energies_are_the_definitions(rate, n, ch):
    """Both sides sum the same non-negative f64 squares of bit-identical filter outputs in
    another order: relative 2 m 2^-53 per hop of m = frames x channels terms.  A larger
    difference means the host filter was contracted into FMAs."""
    pcm = stepped_noise(n, rate, ch)
    e, m = host_r128(pcm, rate)
    ref = ref_hops(pcm, rate)
    assert len(e) == len(ref) == 10 * n // rate
    B = bounds(len(e), rate)
    for i in range(len(e)):
        assert abs(e[i] - ref[i]) <= 2.0 * (B[i + 1] - B[i]) * ch * 2.0 ** -53 * ref[i], i
    r = ref_r128(ref, rate)
    assert m.lra_blocks == r["lra_blocks"]
    for f in FIGURES:
        assert same(getattr(m, f), r[f], 1e-9), f


@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("case", sorted(EBU_3341))
def test_ebu_tech_3341(case, rate):
    parts, want = EBU_3341[case]
    _, m = host_r128(sine(parts, rate), rate)
    assert abs(m.integrated - want) <= 0.1
    if case == "3341-1":
        assert abs(m.momentary_max - want) <= 0.1 and abs(m.short_term_max - want) <= 0.1


@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("case", sorted(EBU_3342))
def test_ebu_tech_3342(case, rate):
    parts, want = EBU_3342[case]
    _, m = host_r128(sine(parts, rate), rate)
    assert abs(m.lra - want) <= 1.0
    assert m.lra == m.lra_high - m.lra_low and m.lra_blocks > 0


def test_channels_are_summed_not_averaged():
    """A centred stereo signal reads 10 log10 2 above one channel of it alone (which is also
    what the channel-mean measure of the meter reads for the stereo file)."""
    st = sine([(-23.0, 20)], 48000)
    _, m2 = host_r128(st, 48000)
    _, m1 = host_r128(np.ascontiguousarray(st[:, 0]), 48000)
    assert abs((m2.integrated - m1.integrated) - 10.0 * math.log10(2.0)) <= 1e-3
    assert abs(m1.integrated - (-26.05)) <= 0.05


@pytest.mark.parametrize("hops", [0, 3, 4, 29, 30])
def test_short_signals_have_nan_figures(hops):
    m = from_hops(np.full(hops, 4.8), 48000)  # 1e-3 per frame: -30.691 LUFS
    has_m, has_s = hops >= 4, hops >= 30
    assert m.momentary_blocks == max(hops - 3, 0) and m.short_term_blocks == max(hops - 29, 0)
    for f in ("integrated", "relative_gate", "momentary_max"):
        assert math.isnan(getattr(m, f)) != has_m, f
    for f in ("short_term_max", "lra", "lra_low", "lra_high"):
        assert math.isnan(getattr(m, f)) != has_s, f
    if has_m:
        assert abs(m.integrated - (-30.691)) < 1e-9 and abs(m.relative_gate - (-40.691)) < 1e-9
    if has_s:
        assert m.lra == 0.0 and m.lra_blocks == 1


def test_silence():
    m = from_hops(np.zeros(40), 48000)
    assert m.integrated == -math.inf and m.momentary_max == -math.inf and m.short_term_max == -math.inf
    assert math.isnan(m.relative_gate)
    assert m.lra == 0.0 and m.lra_blocks == 0 and math.isnan(m.lra_low) and math.isnan(m.lra_high)


def test_lra_percentiles_are_list_elements():
    """400 hops whose 371 short-term levels all pass both gates and are distinct, in an
    order that is not sorted: the bounds are elements 37 and 352 of the sorted list."""
    rate, H = 48000, 400
    i = np.arange(H)
    e = 4.8 * (1.0 + 0.3 * np.sin(i * 0.013) + 0.001 * ((i * 7) % 13))
    levels = []
    for j in range(H - 29):  # the definition's own order of operations, in Python floats
        acc = float(e[j])
        for k in range(1, 30):
            acc += float(e[j + k])
        levels.append(-0.691 + 10.0 * math.log10(acc / float(30 * 4800)))
    assert len(set(levels)) == 371 and levels != sorted(levels)
    assert max(levels) - min(levels) < 20.0 and min(levels) > -70.0
    m = from_hops(e, rate)
    k = sorted(levels)
    assert m.lra_blocks == 371 and m.lra_low == k[37] and m.lra_high == k[352] and m.lra == k[352] - k[37]
    assert m.short_term_max == k[-1]


def test_absolute_gate_is_strict():
    """One momentary block at exactly -70 LUFS is excluded; the next double above it is not."""
    frames = 4 * 4800
    a = 10.0 ** ((-70.0 + 0.691) / 10.0) * frames
    lv = lambda v: -0.691 + 10.0 * math.log10(v / frames)  # noqa: E731
    while lv(a) > -70.0:
        a = math.nextafter(a, 0.0)
    while lv(a) < -70.0:
        a = math.nextafter(a, math.inf)
    assert lv(a) == -70.0
    m = from_hops([a, 0.0, 0.0, 0.0], 48000)
    assert m.momentary_max == -70.0 and m.integrated == -math.inf and math.isnan(m.relative_gate)
    b = a
    while lv(b) == -70.0:
        b = math.nextafter(b, math.inf)
    m = from_hops([b, 0.0, 0.0, 0.0], 48000)
    assert m.integrated == m.momentary_max > -70.0


def test_host_refusals_and_empty_signal():
    from mastering_amd import engine, native
    lib = native.load()
    sos, m = engine.kweight_sos(48000), native.MMR128()
    x = np.zeros((100, 2), np.int16)
    p = x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))
    assert lib.mm_r128_host(p, 100, 3, 48000, sos, None, 0, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_host(p, 100, 2, 1999, sos, None, 0, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_host(p, 2 ** 31, 2, 48000, sos, None, 0, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_host(None, 100, 2, 48000, sos, None, 0, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_host(p, 100, 2, 48000, None, None, 0, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_host(p, 100, 2, 48000, sos, None, 0, None) == native.MM_ERR_ARG
    assert lib.mm_r128_from_hops(None, 5, 48000, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_host(None, 0, 2, 48000, sos, None, 0, ctypes.byref(m)) == 0
    assert m.frames == 0 and m.channels == 2 and m.hops == 0 and all(math.isnan(getattr(m, f)) for f in FIGURES)
    assert lib.mm_r128_host(p, 100, 2, 2000, sos, None, 0, ctypes.byref(m)) == 0  # the floor itself is accepted
    assert lib.mm_r128_span() % 256 == 0 and 1 <= lib.mm_r128_span() // 256 <= 200


def test_r128_layout_matches_c(tmp_path):
    from mastering_amd import native
    fl = [f[0] for f in native.MMR128._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mastering.h"', "int main(void){",
             'printf("mm_r128 %zu\\n", sizeof(mm_r128));']
    lines += [f'printf("mm_r128.{f} %zu\\n", offsetof(mm_r128, {f}));' for f in fl]
    lines += ['printf("abi %d\\n", MM_ABI_VERSION);', 'printf("bits %d\\n", MM_REPORT_METER | MM_REPORT_R128 << 4);',
              "return 0;}"]
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["mm_r128"]) == ctypes.sizeof(native.MMR128)
    for f in fl:
        assert int(got[f"mm_r128.{f}"]) == getattr(native.MMR128, f).offset, f
    assert int(got["abi"]) == native.ABI_VERSION == native.load().mm_version() == 5
    assert int(got["bits"]) == native.REPORT_METER | native.REPORT_R128 << 4 == 33


def test_job_plans_the_report():
    from mastering_amd import design, engine, native
    p = {"multiband": True, "lufs": -14.0}
    assert engine.Job(44100, 44100, 2, p).job.meter_on == 0
    assert engine.Job(44100, 44100, 2, p, r128=True).job.meter_on == 2
    assert engine.Job(44100, 44100, 2, p, report=True, r128=True).job.meter_on == 3
    # alone it plans the K-weighting sections and nothing else of the loudness tail
    j = engine.Job(4000, 48000, 2, {}, r128=True)
    assert j.job.meter_on == 2 and j.job.lufs_on == 0 and j.job.n_blocks == 0 and j.job.kweight.nsec == 2
    assert [tuple(j.job.kweight.sos[s]) for s in range(2)] == [tuple(map(float, s)) for s in design.kweight_sections(48000)]
    assert engine.Job(4000, 48000, 2, {}).job.kweight.nsec == 0
    # with a delivery at another rate the bits sit on the delivery, with the output rate's sections
    for report, bits in ((False, 2), (True, 3)):
        j = engine.Job(4000, 44100, 2, {}, report=report, r128=True, output_rate=48000)
        assert j.job.meter_on == 0 and j.delivery.meter_on == bits
        loud = j.delivery.loud.contents
        assert loud.rate == 48000 and loud.kweight.nsec == 2
        assert tuple(loud.kweight.sos[1]) == tuple(map(float, design.kweight_sections(48000)[1]))
    assert engine.Job(4000, 44100, 2, {}, report=True, output_rate=48000).delivery.meter_on == 1
    assert native.REPORT_METER == 1 and native.REPORT_R128 == 2


def test_paths_without_the_whole_track_refuse_the_key():
    from mastering_amd import distributed, engine, legacy
    with pytest.raises(ValueError, match="R 128"):
        engine.Job(44100, 44100, 2, {"lufs": -14.0}, seg_bounds=[0, 4410, 44100], check_length=False, r128=True)
    with pytest.raises(ValueError, match="R 128"):
        distributed.master_time_sharded(None, None, {"r128": True}, None, None, None)
    with pytest.raises(ValueError, match="R 128"):
        legacy.master_pcm(np.zeros((100, 2), np.int16), 44100, {"r128": True})


def test_r128_dict():
    from mastering_amd import engine, native
    m = native.MMR128()
    m.hops, m.lra_blocks = 12, 0
    m.integrated, m.relative_gate, m.momentary_max = -14.2, -24.2, -12.0
    m.short_term_max = m.lra = m.lra_low = m.lra_high = math.nan
    assert engine.r128_dict(m) == {"integrated_lufs": -14.2, "momentary_max_lufs": -12.0, "short_term_max_lufs": None,
                                   "lra_lu": None, "lra_low_lufs": None, "lra_high_lufs": None,
                                   "relative_gate_lufs": -24.2, "hops": 12, "lra_blocks": 0}


def test_master_pcm_pops_the_key_before_planning(monkeypatch):
    """`r128` is a report switch like `report`, not a chain setting: it reaches Job as the
    argument and the worker / GUI pass it through untouched."""
    from mastering_amd import engine, gui_compat
    seen = {}

    class Stop(Exception):
        pass

    def job(*a, **kw):
        seen.update(kw, params=a[3])
        raise Stop

    monkeypatch.setattr(engine, "Job", job)
    with pytest.raises(Stop):
        engine.master_pcm(np.zeros((10, 2), np.int16), 44100, {"r128": 1, "report": True, "width": 1.2})
    assert seen["r128"] is True and seen["report"] is True and seen["params"] == {"width": 1.2}
    assert gui_compat.chain_settings({"r128": True, "input_file": "a"}) == {"r128": True}
