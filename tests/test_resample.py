"""The sample-rate converter on CPU: the taps of design.resample_taps and the library's
host restatement (mm_resample_host) against a numpy restatement of the definition in
include/mastering.h (mm_resampler), the quality of the designed filters computed from the
integer taps, tones through the converter, refused tables, the struct layouts and the
Python plumbing that needs no GPU.  All comparisons are equalities on integers, except
the design-quality and tone conditions, whose bounds and measured values are stated."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ONE = 1 << 22
PAIRS = [(96000, 44100), (48000, 44100), (44100, 48000), (96000, 48000), (192000, 44100), (44100, 96000)]
GEOMETRY = {(96000, 44100): (147, 320, 280), (48000, 44100): (147, 160, 140), (44100, 48000): (160, 147, 128),
            (96000, 48000): (1, 2, 256), (192000, 44100): (147, 640, 558), (44100, 96000): (320, 147, 128)}
STATS = ("frames_in", "frames_out", "channels", "rate_in", "rate_out", "L", "M", "K")


def ref_taps(rate_in, rate_out):
    """The taps of the definition, phase by phase: (L, M, K, c int64 [L][K])."""
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    K = 2 * ((64 * max(L, M) + L - 1) // L)
    fc = 0.475 * min(1, L / M)
    c = np.zeros((L, K), np.int64)
    for p in range(L):
        d = p + (np.arange(K) - K // 2) * L
        t = d / L
        u = t / (K // 2)
        w = np.where(np.abs(u) <= 1, np.i0(10 * np.sqrt(np.maximum(1 - u ** 2, 0))) / np.i0(10), 0.0)
        h = 2 * fc * np.sinc(2 * fc * t) * w
        h = h / h.sum()
        row = np.rint(h * 2 ** 22).astype(np.int64)
        row[np.argmax(np.abs(row))] += 2 ** 22 - row.sum()
        c[p] = row
    return L, M, K, c


def ref_resample(pcm, L, M, K, c):
    """The definition in numpy int64, vectorised over n with a loop over k: (out int16, stats)."""
    pcm = np.asarray(pcm)
    x = (pcm[:, None] if pcm.ndim == 1 else pcm).astype(np.int64)
    N, ch = x.shape
    n_out = -(-N * L // M)
    q = np.arange(n_out, dtype=np.int64) * M
    b, p = q // L, q % L
    z = np.concatenate([np.zeros((K, ch), np.int64), x, np.zeros((K, ch), np.int64)])  # z[i] = s[i - K]
    c = np.asarray(c, np.int64)
    acc = np.zeros((n_out, ch), np.int64)
    for k in range(K):
        acc += c[p, k, None] * z[b + K // 2 - k + K]
    y = (acc + (1 << 21)) >> 22
    out = np.clip(y, -32768, 32767)
    st = dict(frames_in=N, frames_out=n_out, channels=ch, L=L, M=M, K=K,
              clipped=[int(v) for v in (y != out).sum(axis=0)],
              peak=[int(v) for v in np.abs(out).max(axis=0, initial=0)])
    return out.astype(np.int16).reshape((n_out,) + pcm.shape[1:]), st


def resampler(rate_in, rate_out, L, M, K, c, key=0):
    """An mm_resampler over the table c (the array is kept alive on the struct)."""
    from mastering_amd import native
    rs = native.MMResampler()
    rs.rate_in, rs.rate_out, rs.L, rs.M, rs.K, rs.taps_key = rate_in, rate_out, L, M, K, key
    rs._c = np.ascontiguousarray(c, np.int32)
    rs.taps = rs._c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return rs


def resample_stats(m, rates=False):
    d = {f: int(getattr(m, f)) for f in STATS if rates or not f.startswith("rate")}
    ch = int(m.channels)
    d["clipped"], d["peak"] = [int(m.clipped[i]) for i in range(ch)], [int(m.peak[i]) for i in range(ch)]
    return d


def host_resample(pcm, rs):
    from mastering_amd import native
    lib = native.load()
    x = np.ascontiguousarray(pcm, np.int16)
    ch = 1 if x.ndim == 1 else x.shape[1]
    n_out = -(-x.shape[0] * rs.L // rs.M)
    out = np.full((n_out,) + x.shape[1:], 77, np.int16)
    m = native.MMResample()
    i16p = ctypes.POINTER(ctypes.c_int16)
    rc = lib.mm_resample_host(x.ctypes.data_as(i16p), x.shape[0], ch, ctypes.byref(rs), out.ctypes.data_as(i16p),
                              ctypes.byref(m))
    assert rc == 0
    assert (m.rate_in, m.rate_out) == (rs.rate_in, rs.rate_out)
    return out, resample_stats(m)


@pytest.fixture(scope="module")
def tables():
    """ref_taps of the six pairs (shared, read-only)."""
    return {pair: ref_taps(*pair) for pair in PAIRS}


# ------------------------------------------------------------------ the taps
@pytest.mark.parametrize("pair", PAIRS)
def test_taps_are_the_definition(tables, pair):
    from mastering_amd import design
    L, M, K, c = design.resample_taps(*pair)
    rL, rM, rK, rc = tables[pair]
    assert (L, M, K) == (rL, rM, rK) == GEOMETRY[pair]
    assert c.dtype == np.int32 and c.shape == (L, K) and np.array_equal(c, rc)
    assert np.all(c.astype(np.int64).sum(axis=1) == ONE)
    worst = int(np.abs(c.astype(np.int64)).sum(axis=1).max())
    print(f"{pair}: L {L} M {M} K {K}, {L * K} taps, worst row sum|c| = {worst / ONE:.3f} * 2^22")
    assert worst < 1 << 24
    assert design.resample_geometry(*pair) == (L, M, K) and design.resample_key(*pair) != 0
    assert design.resample_taps(*pair)[3] is c and not c.flags.writeable  # cached and read-only


def test_every_studio_pair_fits_the_limits():
    from mastering_amd import design
    rates = (44100, 48000, 88200, 96000, 176400, 192000)
    biggest = max((design.resample_geometry(a, b) for a in rates for b in rates if a != b), key=lambda g: g[0] * g[2])
    assert biggest == (147, 640, 558) and biggest[0] * biggest[2] == 82026


def response_db(L, c, rate_in, freqs):
    """|H(f)| in dB of the prototype filter the phases interleave (h[k * L + p] = c[p][k], the
    filter run at L * rate_in between zero-stuffing and decimation), unity = 0 dB."""
    h = np.asarray(c, np.float64).T.reshape(-1) / ONE  # index k * L + p
    i = np.arange(len(h))
    H = np.array([np.sum(h * np.exp(-2j * np.pi * f / (L * rate_in) * i)) for f in freqs]) / L
    return 20 * np.log10(np.maximum(np.abs(H), 1e-300))


@pytest.mark.parametrize("pair", PAIRS)
def test_design_quality(pair):
    """Passband to 20 kHz within +-0.01 dB (measured worst over the pairs 0.0084 dB), stopband
    from the lower Nyquist upward at most -98 dB (measured worst -99.77 dB, the 2:1 pairs)."""
    from mastering_amd import design
    L, M, K, c = design.resample_taps(*pair)
    rate_in, rate_out = pair
    top = L * rate_in / 2
    pb = response_db(L, c, rate_in, np.linspace(0, 20000, 201))
    sb = response_db(L, c, rate_in, np.linspace(min(pair) / 2, top, 1200))
    print(f"{pair}: passband {np.abs(pb).max():.4f} dB, stopband {sb.max():.2f} dB")
    assert np.abs(pb).max() <= 0.01
    assert sb.max() <= -98.0


# ------------------------------------------------------------------ the host restatement
def signals(n, ch, seed):
    rng = np.random.default_rng(seed)
    shape = (n, ch) if ch == 2 else (n,)
    noise = rng.integers(-32768, 32768, shape).astype(np.int16)
    hot = np.clip(rng.normal(0, 30000, shape), -32768, 32767).astype(np.int16)
    square = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    square = np.stack([square, -1 - square], axis=1) if ch == 2 else square
    return {"noise": noise, "hot": hot, "square": square,
            "c12345": np.full(shape, 12345, np.int16), "cmin": np.full(shape, -32768, np.int16)}


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("pair", PAIRS)
def test_host_restatement(tables, pair, ch):
    L, M, K, c = tables[pair]
    rs = resampler(*pair, L, M, K, c)
    for n in (0, 1, K // 2, K, 5000):
        for name, pcm in signals(n, ch, 17 * n + ch).items():
            want, st = ref_resample(pcm, L, M, K, c)
            got, gst = host_resample(pcm, rs)
            assert gst == st, (name, n, gst, st)
            assert np.array_equal(got, want), (name, n)
            assert got.shape[0] == st["frames_out"] == -(-n * L // M)
            if name == "square" and n == 5000:
                assert min(st["clipped"]) > 0 and max(st["peak"]) == 32768
            if name in ("c12345", "cmin") and n == 5000:  # DC gain exactly 2^22: unchanged away from the ends
                lo = -(-K * L // M)
                assert np.all(got[lo:len(got) - lo] == pcm.flat[0]) and len(got) > 2 * lo


def test_resample_frames_and_span():
    from mastering_amd import design, native
    lib = native.load()
    out = ctypes.c_int64()
    for n, L, M in ((0, 147, 320), (1, 147, 320), (320, 147, 320), (321, 147, 320), (2 ** 31 - 1, 1, 2), (5, 320, 147)):
        assert lib.mm_resample_frames(n, L, M, ctypes.byref(out)) == 0
        assert out.value == -(-n * L // M) == design.resample_frames(n, L, M)
    assert lib.mm_resample_frames(-1, 1, 2, ctypes.byref(out)) == native.MM_ERR_ARG
    assert lib.mm_resample_frames(5, 641, 2, ctypes.byref(out)) == native.MM_ERR_ARG
    assert lib.mm_resample_span() >= 256


# ------------------------------------------------------------------ tones
def test_sine_comes_through():
    """1 kHz at amplitude 20000, 96 -> 44.1 kHz: the least-squares fit of the output on the
    tone is within 0.001 dB of 20000 and leaves a residual of at most 0.5 LSB rms over the
    interior (measured 0.00003 dB and 0.36 LSB: the two roundings to the int16 grid)."""
    from mastering_amd import design
    L, M, K, c = design.resample_taps(96000, 44100)
    n = 30000
    x = np.rint(20000 * np.sin(2 * np.pi * 1000 * np.arange(n) / 96000)).astype(np.int16)
    y, st = ref_resample(x, L, M, K, c)
    lo = -(-K * L // M)
    t = np.arange(len(y))[lo:-lo] / 44100
    A = np.stack([np.sin(2 * np.pi * 1000 * t), np.cos(2 * np.pi * 1000 * t)], axis=1)
    coef, *_ = np.linalg.lstsq(A, y[lo:-lo].astype(np.float64), rcond=None)
    amp_db = 20 * np.log10(np.hypot(*coef) / 20000)
    rms = np.sqrt(np.mean((y[lo:-lo] - A @ coef) ** 2))
    print(f"1 kHz: amplitude {amp_db:+.5f} dB, residual {rms:.3f} LSB rms")
    assert abs(amp_db) <= 0.001 and rms <= 0.5 and st["clipped"] == [0]


def test_tone_above_the_new_nyquist_is_removed():
    """25.05 kHz at amplitude 20000, 96 -> 44.1 kHz (it would alias to 19.05 kHz): |y| <= 1
    over the interior (measured 0)."""
    from mastering_amd import design
    L, M, K, c = design.resample_taps(96000, 44100)
    x = np.rint(20000 * np.sin(2 * np.pi * 25050 * np.arange(30000) / 96000)).astype(np.int16)
    y, _ = ref_resample(x, L, M, K, c)
    lo = -(-K * L // M)
    print("25.05 kHz: max |y| in the interior", int(np.abs(y[lo:-lo]).max()))
    assert np.abs(y[lo:-lo]).max() <= 1


# ------------------------------------------------------------------ arguments, layouts, plumbing
def test_host_refuses_bad_tables(tables):
    from mastering_amd import native
    lib = native.load()
    L, M, K, c = tables[(96000, 48000)]
    x = np.zeros(64, np.int16)
    out = np.zeros(64 * 640, np.int16)  # room for the steepest accepted ratio
    m = native.MMResample()
    i16p = ctypes.POINTER(ctypes.c_int16)

    def rc(rs, frames=64, ch=1):
        return lib.mm_resample_host(x.ctypes.data_as(i16p), frames, ch, ctypes.byref(rs), out.ctypes.data_as(i16p),
                                    ctypes.byref(m))

    assert rc(resampler(96000, 48000, L, M, K, c)) == 0
    flat = np.zeros((2, 4), np.int32)
    flat[:, 1] = ONE
    assert rc(resampler(48000, 96000, 2, 1, 4, flat)) == 0
    assert rc(resampler(48000, 48000, 1, 1, 4, flat[:1])) == native.MM_ERR_ARG            # L = M
    assert rc(resampler(48000, 96000, 2, 2, 4, flat)) == native.MM_ERR_ARG                # L = M, not coprime
    assert rc(resampler(48000, 96000, 4, 2, 4, np.tile(flat, (2, 1)))) == native.MM_ERR_ARG  # gcd 2
    big = np.zeros((641, 2), np.int32)
    big[:, 1] = ONE
    assert rc(resampler(1000, 641000, 641, 1, 2, big)) == native.MM_ERR_ARG               # L above 640
    assert rc(resampler(641000, 1000, 1, 641, 2, big[:1])) == native.MM_ERR_ARG           # M above 640
    assert rc(resampler(1000, 640000, 640, 1, 2, big[:640])) == 0
    assert rc(resampler(48000, 96000, 2, 1, 3, np.full((2, 3), 5, np.int32))) == native.MM_ERR_ARG  # odd K
    assert rc(resampler(48000, 96000, 2, 1, 0, flat)) == native.MM_ERR_ARG
    assert rc(resampler(48000, 96000, 2, 1, 1026, np.zeros((2, 1026), np.int32))) == native.MM_ERR_ARG
    heavy = flat.copy()
    heavy[1] = [1 << 23, -(1 << 22), 1 << 22, 0]                                          # sum |c| = 2^24
    assert rc(resampler(48000, 96000, 2, 1, 4, heavy)) == native.MM_ERR_ARG
    heavy[1, 0] -= 1
    heavy[1, 3] += 1                                                                      # 2^24 - 1 + 1: still 2^24
    assert rc(resampler(48000, 96000, 2, 1, 4, heavy)) == native.MM_ERR_ARG
    heavy[1, 3] = 0                                                                       # 2^24 - 1
    assert rc(resampler(48000, 96000, 2, 1, 4, heavy)) == 0
    assert rc(resampler(48000, 44100, 2, 1, 4, flat)) == native.MM_ERR_ARG                # rates do not match L / M
    assert rc(resampler(48000, 96000, 2, 1, 4, flat), ch=3) == native.MM_ERR_ARG
    assert rc(resampler(48000, 96000, 2, 1, 4, flat), frames=-1) == native.MM_ERR_ARG


def test_resample_layouts_match_c(tmp_path):
    from mastering_amd import native
    fields = {"mm_resampler": native.MMResampler, "mm_resample": native.MMResample, "mm_delivery": native.MMDelivery,
              "mm_job": native.MMJob}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mastering.h"', "int main(void){"]
    for st, cls in fields.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        if st != "mm_job":
            lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("abi %d\\n", MM_ABI_VERSION);')
    lines.append("return 0;}")
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for st, cls in fields.items():
        assert int(got[st]) == ctypes.sizeof(cls), st
        if st != "mm_job":
            for f, _ in cls._fields_:
                assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"
    assert int(got["abi"]) == native.ABI_VERSION == native.load().mm_version() == 5


def test_design_refuses_pairs_outside_the_limits():
    from mastering_amd import design
    for a, b in ((44100, 44100), (96000, 44101), (44100, 5000), (384000, 44100), (0, 44100), (44100, -1)):
        with pytest.raises(ValueError):
            design.resample_taps(a, b)
    assert design.resample_geometry(384000, 48000) == (1, 8, 1024)  # the steepest ratio that fits


def test_job_plans_a_delivery():
    from mastering_amd import design, engine
    params = {"multiband": True, "lufs": -14.0}
    plain = engine.Job(96000, 96000, 2, params, report=True, ceiling_dbtp=-1.0)
    assert plain.delivery is None and plain.frames_out == plain.frames_proc and plain.output_rate is None
    same = engine.Job(96000, 96000, 2, params, report=True, ceiling_dbtp=-1.0, output_rate=96000)
    assert same.delivery is None and bytes(same.job)[:64] == bytes(plain.job)[:64]
    assert (same.job.meter_on, same.job.ceiling_q28) == (1, design.ceiling_q28(-1.0))
    job = engine.Job(96000, 96000, 2, params, report=True, ceiling_dbtp=-1.0, output_rate=44100)
    d = job.delivery
    assert (job.job.meter_on, job.job.ceiling_q28) == (0, 0) and job.job.lufs_on == 1 and job.job.rate == 96000
    assert (d.meter_on, d.ceiling_q28, d.window) == (1, design.ceiling_q28(-1.0), design.ceiling_window(44100))
    rs = d.rs.contents
    assert (rs.rate_in, rs.rate_out, rs.L, rs.M, rs.K) == (96000, 44100, 147, 320, 280)
    assert rs.taps_key == design.resample_key(96000, 44100) != 0
    assert np.array_equal(np.ctypeslib.as_array(rs.taps, (147, 280)), design.resample_taps(96000, 44100)[3])
    assert job.frames_out == -(-job.frames_proc * 147 // 320) and job.output_rate == 44100
    loud = d.loud.contents
    assert (loud.frames_proc, loud.rate, loud.channels, loud.kweight.tpb) == (job.frames_out, 44100, 2, 256)
    bare = engine.Job(96000, 96000, 1, params, output_rate=48000).delivery
    assert (bare.meter_on, bare.ceiling_q28) == (0, 0) and not bare.loud
    short = engine.Job(9600, 96000, 1, {}, report=True, output_rate=48000).delivery  # under one 0.4 s block
    assert short.meter_on == 1 and not short.loud
    with pytest.raises(ValueError):
        engine.Job(96000, 96000, 2, params, output_rate=44101)
    with pytest.raises(ValueError):
        engine.Job(96000, 96000, 2, params, seg_bounds=[0, 38400, 96000], check_length=False, output_rate=44100)


def test_master_pcm_refuses_a_bad_output_rate_before_any_device_work():
    from mastering_amd import distributed, engine
    pcm = np.zeros((4800, 2), np.int16)
    for bad in (44101, 1000, 0):
        with pytest.raises(ValueError):
            engine.master_pcm(pcm, 96000, {"multiband": False, "output_rate": bad})
    with pytest.raises(ValueError):
        engine.resample_pcm(pcm, 96000, 44101)
    with pytest.raises(ValueError, match="rate"):
        distributed.master_time_sharded(None, None, {"lufs": -14.0, "output_rate": 44100}, 0, 0, None)


def test_resample_dict():
    from mastering_amd import engine, native
    m = native.MMResample()
    m.frames_in, m.frames_out, m.channels, m.rate_in, m.rate_out, m.L, m.M, m.K = 320, 147, 2, 96000, 44100, 147, 320, 280
    m.clipped[0], m.clipped[1], m.peak[0], m.peak[1] = 3, 0, 32768, 16384
    d = engine.resample_dict(m)
    assert {k: d[k] for k in STATS} == {k: int(getattr(m, k)) for k in STATS}
    assert d["clipped"] == [3, 0] and d["peak"] == [32768, 16384] and d["peak_dbfs"] == 0.0
