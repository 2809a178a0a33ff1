"""The delivery QC report on CPU: the library's sequential host restatement (mm_qc_host) and
its tail (mm_qc_from_hops) against about fifty lines of numpy written from the definition in
include/mastering.h (ref_qc), known answers of the correlation, the refusals, the mm_qc
layout, and the Python plumbing that needs no GPU."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INTS = ("frames", "channels", "rate", "hops", "silence_lsb", "min_run", "cross", "lead_silence", "trail_silence",
        "silent_frames", "silence_longest", "silence_longest_at", "corr_windows", "corr_negative", "corr_min_hop")
PAIRS = ("sum", "sq", "smin", "smax", "or_bits", "clip_samples", "clip_runs", "clip_longest", "clip_longest_at")


def _runs(v):
    """The maximal stretches of equal non-zero values of v: [(start, length)], in order."""
    if len(v) == 0:
        return []
    edges = np.flatnonzero(np.diff(v) != 0) + 1
    starts, ends = np.concatenate([[0], edges]), np.concatenate([edges, [len(v)]])
    return [(int(s), int(e - s)) for s, e in zip(starts, ends) if v[s] != 0]


def _longest(runs):
    """(length, start) of the longest run, the first among equals; none: (0, -1)."""
    if not runs:
        return 0, -1
    best = max(n for _, n in runs)
    return best, next(s for s, n in runs if n == best)


def ref_qc(pcm, rate, q=1, r=3):
    """The definition of mm_qc in numpy int64 (both channels of every pair; a mono signal's
    second entries are 0, its longest-at -1): (fields, the [H, 3] hop table)."""
    pcm = np.asarray(pcm)
    x = pcm.reshape(len(pcm), 1 if pcm.ndim == 1 else pcm.shape[1]).astype(np.int64)
    N, ch = x.shape
    H = 10 * N // rate
    B = [i * rate // 10 for i in range(H + 1)]
    o = {"frames": N, "channels": ch, "rate": rate, "hops": H, "silence_lsb": q, "min_run": r}
    for f in PAIRS:
        o[f] = [0, 0]
    o["clip_longest_at"] = [-1, -1]
    for c in range(ch):
        s = x[:, c]
        o["sum"][c], o["sq"][c] = int(s.sum()), int((s * s).sum())
        o["smin"][c], o["smax"][c] = (int(s.min()), int(s.max())) if N else (0, 0)
        o["or_bits"][c] = int(np.bitwise_or.reduce(s & 0xFFFF)) if N else 0
        rail = np.where(s == 32767, 1, np.where(s <= -32767, -1, 0))
        runs = _runs(rail)
        o["clip_samples"][c] = int((rail != 0).sum())
        o["clip_runs"][c] = sum(n >= r for _, n in runs)
        o["clip_longest"][c], o["clip_longest_at"][c] = _longest(runs)
    o["cross"] = int((x[:, 0] * x[:, 1]).sum()) if ch == 2 else 0
    silent = (np.abs(x) <= q).all(axis=1)
    loud = np.flatnonzero(~silent)
    o["lead_silence"] = int(loud[0]) if len(loud) else N
    o["trail_silence"] = N - 1 - int(loud[-1]) if len(loud) else N
    o["silent_frames"] = int(silent.sum())
    o["silence_longest"], o["silence_longest_at"] = _longest(_runs(silent.astype(np.int64)))
    table = np.zeros((H, 3), np.int64)
    for i in range(H):
        seg = x[B[i]:B[i + 1]]
        table[i, 0] = (seg[:, 0] ** 2).sum()
        if ch == 2:
            table[i, 1], table[i, 2] = (seg[:, 1] ** 2).sum(), (seg[:, 0] * seg[:, 1]).sum()
    o.update(corr_windows=0, corr_negative=0, corr_min=math.nan, corr_min_hop=-1)
    if ch == 2:
        o.update(ref_corr(table, rate))
    return o, table


def ref_corr(table, rate):
    """Step 5 on a hop table, the window loop in np.float64."""
    H = len(table)
    o = {"corr_windows": 0, "corr_negative": 0, "corr_min": math.nan, "corr_min_hop": -1}
    for j in range(H - 3):
        A, Bw, X = (int(v) for v in np.asarray(table[j:j + 4], np.int64).sum(axis=0))
        if A + Bw < 2048 * ((j + 4) * rate // 10 - j * rate // 10):
            continue
        o["corr_windows"] += 1
        o["corr_negative"] += X < 0
        rho = np.float64(0.0) if A == 0 or Bw == 0 else np.float64(X) / np.sqrt(np.float64(A) * np.float64(Bw))
        if o["corr_min_hop"] < 0 or rho < o["corr_min"]:
            o["corr_min"], o["corr_min_hop"] = float(rho), j
    return o


def qc_fields(m):
    """Every field of an MMQc as ref_qc's dict."""
    o = {f: int(getattr(m, f)) for f in INTS}
    o.update({f: [int(getattr(m, f)[c]) for c in range(2)] for f in PAIRS})
    o["corr_min"] = float(m.corr_min)
    return o


def same_qc(got, want):
    """All fields equal; corr_min bit-equal, or both NaN.  Returns the names that differ."""
    bad = [f for f in want if f != "corr_min" and got[f] != want[f]]
    a, b = got["corr_min"], want["corr_min"]
    if not ((math.isnan(a) and math.isnan(b)) or struct.pack("<d", a) == struct.pack("<d", b)):
        bad.append("corr_min")
    return bad


def host_qc(pcm, rate, q=1, r=3):
    """(fields, hop table) of mm_qc_host."""
    from mastering_amd import native
    lib = native.load()
    x = np.ascontiguousarray(pcm, np.int16)
    m = native.MMQc()
    table = np.full((10 * x.shape[0] // rate + 1, 3), -7, np.int64)
    rc = lib.mm_qc_host(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), x.shape[0], 1 if x.ndim == 1 else x.shape[1],
                        rate, q, r, ctypes.byref(m), table.ctypes.data_as(native.c_int64_p))
    assert rc == 0
    assert (table[-1] == -7).all()  # nothing past H rows
    return qc_fields(m), table[:-1]


R = 3  # the default min_run


def signal(kind, n, ch, seed=0):
    rng = np.random.default_rng(seed)
    shape = (n,) if ch == 1 else (n, ch)
    if kind == "noise":
        return rng.integers(-20000, 20000, shape).astype(np.int16)
    if kind == "clipped":  # hard-clipped noise: rail runs of every short length, both signs
        return np.clip(rng.normal(0.0, 40000.0, shape), -32768, 32767).astype(np.int16)
    if kind == "square":  # full-scale squares of period 14, channels out of step
        t = np.arange(n)
        cols = [np.where(((t + 3 * c) // 7) % 2 == 0, 32767, -32768) for c in range(ch)]
        return (cols[0] if ch == 1 else np.stack(cols, axis=1)).astype(np.int16)
    value = {"rail+": 32767, "rail-": -32767, "min": -32768, "zero": 0}[kind]
    return np.full(shape, value, np.int16)


KINDS = ("noise", "clipped", "square", "rail+", "rail-", "min", "zero")


def sizes(rate):
    hop = rate // 10
    return sorted({0, 1, 2, R - 1, R, hop - 1, hop, hop + 1, 4 * hop - 1, 4 * hop, 4 * hop + 1, 5000})


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate", [2000, 11025, 44100])
def test_host_equals_numpy(rate, ch):
    for kind in KINDS:
        for n in sizes(rate) + ([4 * 1102 + 2, 4 * 1103] if rate == 11025 else []):  # (hop 1102.5: B[4] = 4410)
            x = signal(kind, n, ch, seed=n)
            want, want_table = ref_qc(x, rate)
            got, got_table = host_qc(x, rate)
            assert same_qc(got, want) == [], (kind, n, same_qc(got, want))
            assert np.array_equal(got_table, want_table), (kind, n)


def test_parameters_and_runs():
    """q and r are honoured; runs of both rails, equal longest runs, runs at either end."""
    x = np.zeros(40, np.int16)
    x[2:5] = 32767        # 3 at +rail
    x[5:8] = -32768       # 3 at -rail, adjacent: a run of its own
    x[10:12] = 32767      # 2
    x[20:24] = -32767     # 4: the longest
    x[30:34] = 32767      # 4 again: the first wins
    x[38:40] = -32768     # 2, at the end
    x[15] = 1
    x[16] = -2
    for q, r in ((0, 1), (1, 3), (2, 4), (32767, 65535)):
        want, _ = ref_qc(x, 2000, q, r)
        got, _ = host_qc(x, 2000, q, r)
        assert same_qc(got, want) == [], (q, r)
    got, _ = host_qc(x, 2000, 1, 3)
    assert got["clip_samples"][0] == 18 and got["clip_runs"][0] == 4
    assert (got["clip_longest"][0], got["clip_longest_at"][0]) == (4, 20)
    assert got["lead_silence"] == 2 and got["trail_silence"] == 0
    assert (got["silence_longest"], got["silence_longest_at"]) == (6, 24)  # 24..29 (12..15 is 4 long: 16 is -2)
    got, _ = host_qc(x, 2000, 2, 3)
    assert (got["silence_longest"], got["silence_longest_at"]) == (8, 12)  # 12..19


def _corr(x, rate=2000):
    got, table = host_qc(x, rate)
    assert same_qc(got, ref_qc(x, rate)[0]) == []
    return got, table


def test_correlation_known_answers():
    rng = np.random.default_rng(5)
    L = rng.integers(-20000, 20000, 2500).astype(np.int16)
    got, _ = _corr(np.stack([L, L], axis=1))  # R = L
    assert got["corr_min"] == 1.0 and got["corr_negative"] == 0 and got["corr_windows"] == 9
    assert got["sq"][0] + got["sq"][1] - 2 * got["cross"] == 0
    got, _ = _corr(np.stack([L, -L], axis=1))  # R = -L (no -32768 in L)
    assert got["corr_min"] == -1.0 and got["corr_negative"] == got["corr_windows"] == 9 and got["corr_min_hop"] == 0
    got, _ = _corr(np.stack([L, np.zeros_like(L)], axis=1))  # one channel zero
    assert got["corr_min"] == 0.0 and got["corr_negative"] == 0 and got["corr_windows"] == 9


def test_gate_and_ties():
    """A window below the gate is left out (the comparison is exact); ties take the smallest j."""
    rate, hop = 2000, 200
    x = np.zeros((8 * hop, 2), np.int16)
    x[:, 0], x[:, 1] = 32, -32  # mean square exactly 32^2 a channel: every window sits ON the gate
    got, _ = _corr(x)
    assert got["corr_windows"] == 5 and got["corr_negative"] == 5 and got["corr_min"] == -1.0 and got["corr_min_hop"] == 0
    x[4 * hop, 1] = -31  # windows 1..4 now lie below it by 63
    got, _ = _corr(x)
    assert got["corr_windows"] == 1 and got["corr_min_hop"] == 0
    x[:4 * hop] = 0      # the only window that passed is silent: none is gated
    got, _ = _corr(x)
    assert got["corr_windows"] == 0 and math.isnan(got["corr_min"]) and got["corr_min_hop"] == -1
    y = np.zeros((7 * hop, 2), np.int16)  # loud and in phase, hop 3 out of phase: windows 0..3 tie
    y[:, 0] = y[:, 1] = 1000
    y[3 * hop:4 * hop, 1] = -1000
    got, _ = _corr(y)
    assert got["corr_windows"] == 4 and got["corr_min"] == 0.5 and got["corr_min_hop"] == 0


def test_from_hops_alone():
    from mastering_amd import native
    lib = native.load()
    rng = np.random.default_rng(9)
    for H in (0, 3, 4, 5, 40):
        a, b = rng.integers(0, 2 ** 46, H), rng.integers(0, 2 ** 46, H)
        table = np.ascontiguousarray(np.stack([a, b, rng.integers(-2 ** 45, 2 ** 45, H)], axis=1), np.int64)
        if H > 4:
            table[1] = 0
        m = native.MMQc()
        m.frames = 77  # (not touched)
        assert lib.mm_qc_from_hops(table.ctypes.data_as(native.c_int64_p), H, 48000, ctypes.byref(m)) == 0
        want = ref_corr(table, 48000)
        assert same_qc(qc_fields(m), want) == [], H  # (the four fields of step 5)
        assert m.hops == H and m.rate == 48000 and m.frames == 77
    assert lib.mm_qc_from_hops(None, 1, 48000, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_qc_from_hops(table.ctypes.data_as(native.c_int64_p), 1, 1999, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_qc_from_hops(table.ctypes.data_as(native.c_int64_p), -1, 48000, ctypes.byref(m)) == native.MM_ERR_ARG


def test_refusals():
    from mastering_amd import native
    lib = native.load()
    x = np.zeros((16, 2), np.int16)
    p = x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))
    m = native.MMQc()

    def rc(frames=16, ch=2, rate=2000, q=1, r=3, out=ctypes.byref(m), pcm=p):
        return lib.mm_qc_host(pcm, frames, ch, rate, q, r, out, None)
    assert rc() == 0
    for bad in (dict(ch=0), dict(ch=3), dict(frames=-1), dict(frames=2 ** 31), dict(rate=1999), dict(q=-1),
                dict(q=32768), dict(r=0), dict(r=65536), dict(out=None), dict(pcm=None)):
        assert rc(**bad) == native.MM_ERR_ARG, bad
    assert rc(frames=0, pcm=None) == 0 and m.frames == 0 and m.silence_longest_at == -1


def test_qc_layout_matches_c(tmp_path):
    from mastering_amd import native
    fl = [f[0] for f in native.MMQc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mastering.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(mm_qc));']
    lines += [f'printf("{f} %zu\\n", offsetof(mm_qc, {f}));' for f in fl]
    lines += ['printf("bit %d\\n", MM_REPORT_QC);', 'printf("abi %d\\n", MM_ABI_VERSION);', "return 0;}"]
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(native.MMQc)
    for f in fl:
        assert int(got[f]) == getattr(native.MMQc, f).offset, f
    assert int(got["bit"]) == native.REPORT_QC == 4 and int(got["abi"]) == native.ABI_VERSION == 5


def test_planning():
    from mastering_amd import engine, native
    job = engine.Job(44100, 44100, 2, {}, qc=True)
    assert job.job.meter_on == 4 and job.delivery is None
    assert engine.Job(44100, 44100, 2, {}, qc=True, report=True, r128=True).job.meter_on == 7
    assert engine.Job(44100, 44100, 2, {}).job.meter_on == 0
    job = engine.Job(44100, 44100, 2, {}, qc=True, output_rate=48000)
    assert job.job.meter_on == 0 and job.delivery.meter_on == 4
    assert job.delivery.loud.contents.rate == 48000  # the report reads its rate there
    job = engine.Job(44100, 44100, 2, {}, qc=True, r128=True, deliver_lufs=-16.0)
    assert job.job.meter_on == 0 and job.delivery.meter_on == 6
    with pytest.raises(ValueError, match="QC report needs the whole track"):
        engine.Job(44100, 44100, 2, {}, qc=True, seg_bounds=[0, 44100])


def test_refused_where_r128_is():
    from mastering_amd import distributed, engine, legacy
    with pytest.raises(ValueError, match="QC report needs the whole track: not available on the time-sharded path"):
        distributed.master_time_sharded(None, None, {"qc": True}, None, None, None)
    with pytest.raises(ValueError, match="QC report belongs to the mastering chain's delivery"):
        legacy.master_pcm(np.zeros((10, 2), np.int16), 44100, {"qc": True})
    for fn in (engine.process_batch, engine.process_album):
        with pytest.raises(ValueError, match=r"takes no params\['qc'\]"):
            fn([], [], {"deliver_lufs": -14.0, "qc": True})


def test_qc_dict_derived_figures():
    from mastering_amd import engine, native
    m = native.MMQc()
    m.frames, m.channels, m.rate, m.hops, m.silence_lsb, m.min_run = 1000, 2, 1000, 10, 1, 3
    m.sum[0], m.sum[1] = 32768 * 10, -32768 * 1000
    m.sq[0], m.sq[1], m.cross = 400, 100, -100
    m.or_bits[0], m.or_bits[1] = 0xFFF0, 0x8000
    m.lead_silence, m.trail_silence, m.silent_frames = 100, 250, 550
    m.silence_longest, m.silence_longest_at = 200, 300
    m.corr_min, m.corr_min_hop, m.corr_windows, m.corr_negative = -0.25, 3, 5, 2
    for c in range(2):
        m.clip_longest_at[c] = -1
    d = engine.qc_dict(m)
    assert d["dc_offset"] == [0.01, -1.0]
    assert d["correlation"] == -0.5
    assert d["mono_fold_db"] == pytest.approx(10 * math.log10(300 / 1000), abs=1e-12)
    assert d["side_mid_db"] == pytest.approx(10 * math.log10(700 / 300), abs=1e-12)
    assert d["dual_mono"] is False and d["effective_bits"] == [12, 1]
    assert d["lead_silence_seconds"] == 0.1 and d["trail_silence_seconds"] == 0.25 and d["silence_longest_seconds"] == 0.2
    assert d["dropout"] == (300, 200) and d["corr_min"] == -0.25 and d["corr_min_seconds"] == 0.3
    assert d["clip_longest_at"] == [-1, -1] and d["sum"] == [327680, -32768000]
    m.silence_longest_at = 0  # touches the head: no dropout
    assert engine.qc_dict(m)["dropout"] is None
    m.silence_longest_at, m.silence_longest = 800, 200  # touches the tail
    assert engine.qc_dict(m)["dropout"] is None
    m.sq[0], m.sq[1], m.cross = 400, 400, 400  # L == R
    d = engine.qc_dict(m)
    assert d["dual_mono"] is True and d["correlation"] == 1.0 and d["mono_fold_db"] == 0.0 and d["side_mid_db"] == -math.inf
    m.sq[0] = m.sq[1] = m.cross = 0  # digital zero
    m.or_bits[0] = m.or_bits[1] = 0
    d = engine.qc_dict(m)
    assert d["correlation"] is None and d["mono_fold_db"] is None and d["side_mid_db"] is None
    assert d["dual_mono"] is True and d["effective_bits"] == [0, 0]
    m.channels = 1
    m.corr_min, m.corr_min_hop = math.nan, -1
    d = engine.qc_dict(m)
    assert d["correlation"] is None and d["dual_mono"] is False and d["corr_min"] is None and d["corr_min_seconds"] is None
    assert len(d["sum"]) == 1
