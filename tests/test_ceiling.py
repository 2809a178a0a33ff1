"""The true-peak ceiling on CPU: the library's host restatement (mm_ceiling_host) against
thirty lines of numpy written from the definition in include/mastering.h (mm_ceiling),
the three branches (untouched, limited, limited and trimmed), the properties the
definition promises, its boundaries, the struct layouts and the Python plumbing that
needs no GPU.  All comparisons are equalities on integers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from conftest import ROOT
from test_meter import TAPS, ref_meter

ONE = 1 << 16
GUARD = 8286
STATS = ("frames", "channels", "window", "ceiling_q28", "tp_in_q28", "tp_limited_q28", "tp_out_q28",
         "min_gain_q16", "trim_q16", "limited_frames")
RATE = 44100


def linked_need(x):
    """P[m] = max over channels and phases of |Y_c[m][p]|, m in [0, N + 11) (ref_meter's convolution)."""
    P = np.zeros(len(x) + 11, np.int64)
    for s in x.T:
        z = np.concatenate([np.zeros(11, np.int64), s, np.zeros(11, np.int64)])  # z[i] = s[i - 11]
        Y = sum(TAPS[:, k, None] * z[None, 11 - k:11 - k + len(s) + 11] for k in range(12))
        P = np.maximum(P, np.abs(Y).max(axis=0))
    return P


def ref_ceiling(pcm, C, W, detail=None):
    """The definition of mm_ceiling in numpy int64: (out, stats).  `detail` (a dict)
    receives the gains g and the per-sample need R of a limited signal."""
    pcm = np.asarray(pcm)
    x = pcm.reshape(len(pcm), -1).astype(np.int64)
    N, Ct, D = len(x), C - GUARD, 2 * W + 1
    P = linked_need(x)
    tp0 = int(P.max())
    st = dict(frames=N, channels=x.shape[1], window=W, ceiling_q28=C, tp_in_q28=tp0, tp_limited_q28=tp0,
              tp_out_q28=tp0, min_gain_q16=ONE, trim_q16=ONE, limited_frames=0)
    if tp0 <= C:
        return pcm.copy(), st
    r = np.where(P <= Ct, ONE, (Ct << 16) // np.maximum(P, 1))
    R = sliding_window_view(r, 12).min(axis=1)                                   # R[n], n in [0, N)
    Rp = np.concatenate([np.full(2 * W, ONE), R, np.full(2 * W, ONE)])           # R = ONE outside
    h = sliding_window_view(Rp, D).min(axis=1)                                   # h[k] at k + W
    g = sliding_window_view(h, D).sum(axis=1) // D                               # g[n], n in [0, N)
    y = np.where(g[:, None] == ONE, x, (x * g[:, None] + (1 << 15)) >> 16)
    st["limited_frames"], st["min_gain_q16"] = int((g < ONE).sum()), int(g.min())
    st["tp_limited_q28"] = st["tp_out_q28"] = tp1 = int(linked_need(y).max())
    if tp1 > C:
        st["trim_q16"] = gt = (Ct << 16) // tp1
        y = (y * gt + (1 << 15)) >> 16
        st["tp_out_q28"] = int(linked_need(y).max())
    if detail is not None:
        detail.update(g=g, R=R)
    return y.astype(np.int16).reshape(pcm.shape), st


def ceiling_stats(m):
    return {f: int(getattr(m, f)) for f in STATS}


def host_ceiling(pcm, C, W):
    from mastering_amd import native
    lib = native.load()
    x = np.array(pcm, np.int16, order="C")  # a copy: the call works in place
    m = native.MMCeiling()
    rc = lib.mm_ceiling_host(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), x.shape[0],
                             1 if x.ndim == 1 else x.shape[1], C, W, ctypes.byref(m))
    assert rc == 0
    return x, ceiling_stats(m)


def q28(db):
    from mastering_amd import design
    return design.ceiling_q28(db)


@pytest.fixture(scope="module")
def branch_inputs():
    """The three branch inputs: 20 000 stereo frames of pink noise at 44.1 kHz."""
    from mastering_amd.synth import pink_noise_pcm16
    return {"under": pink_noise_pcm16(20000, RATE, 2, track=3, level_dbfs=-18.0),
            "limited": pink_noise_pcm16(20000, RATE, 2, track=2, level_dbfs=-12.0),
            "trimmed": pink_noise_pcm16(20000, RATE, 2, track=1, level_dbfs=-6.0)}


@pytest.fixture(scope="module")
def branch_refs(branch_inputs):
    """ref_ceiling of every branch input at C = -1 dBTP and W in {1, 16, 220, 1024} (shared, read-only)."""
    C = q28(-1.0)
    out = {}
    for name, pcm in branch_inputs.items():
        for W in (1, 16, 220, 1024):
            d = {}
            y, st = ref_ceiling(pcm, C, W, d)
            out[name, W] = (y, st, d)
    return out


def check_properties(pcm, y, st, d):
    C = st["ceiling_q28"]
    assert st["tp_out_q28"] <= C or st["tp_in_q28"] <= C
    assert st["tp_out_q28"] == max(ref_meter(y)["true_peak_q28"])
    assert np.all(np.abs(y.astype(np.int64)) <= np.abs(np.asarray(pcm).astype(np.int64)))
    if d:
        assert np.all(d["g"] <= d["R"])


@pytest.mark.parametrize("W", [1, 16, 1024])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n", [1, 11, 12, 13, 1000])
def test_host_restatement_random(n, ch, W):
    pcm = np.random.default_rng(1000 * n + 10 * ch + W).integers(-32768, 32768, (n, ch) if ch == 2 else (n,)).astype(np.int16)
    C = q28(-1.0)
    d = {}
    want, st = ref_ceiling(pcm, C, W, d)
    got, gst = host_ceiling(pcm, C, W)
    assert gst == st
    assert np.array_equal(got, want)
    check_properties(pcm, want, st, d)
    assert st["tp_out_q28"] <= C


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n", [1, 11, 12, 13, 500])
def test_host_tp_in_is_the_meters_linked_peak(n, ch):
    """mm_ceiling_host and mm_true_peak_host share one host FIR: on full-scale noise (the
    LCG of tools/diag/ceiling_host_check.cpp) tp_in_q28 == max_c true_peak_q28[c]."""
    from test_meter import host_meter
    W = 16
    s, v = n * 31 + W * 7 + ch, np.empty(n * ch, np.int64)
    for i in range(n * ch):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        v[i] = s >> 16
    pcm = v.astype(np.uint16).view(np.int16).reshape((n, ch) if ch == 2 else (n,))
    _, st = host_ceiling(pcm, 1 << 27, W)
    assert st["tp_in_q28"] == max(host_meter(pcm)["true_peak_q28"])


@pytest.mark.parametrize("W", [1, 16, 220, 1024])
@pytest.mark.parametrize("name", ["under", "limited", "trimmed"])
def test_host_restatement_branch_inputs(branch_inputs, branch_refs, name, W):
    want, st, d = branch_refs[name, W]
    got, gst = host_ceiling(branch_inputs[name], st["ceiling_q28"], W)
    assert gst == st
    assert np.array_equal(got, want)
    check_properties(branch_inputs[name], want, st, d)


def test_branch_under_the_ceiling(branch_inputs, branch_refs):
    for W in (1, 16, 220, 1024):
        y, st, _ = branch_refs["under", W]
        assert round(20 * np.log10(st["tp_in_q28"] / 2 ** 28), 2) == -5.34
        assert np.array_equal(y, branch_inputs["under"])
        assert st["limited_frames"] == 0 and st["trim_q16"] == ONE and st["min_gain_q16"] == ONE
        assert st["tp_out_q28"] == st["tp_limited_q28"] == st["tp_in_q28"]


def test_branch_limited_without_a_trim(branch_inputs, branch_refs):
    share = {}
    for W in (1, 16, 220, 1024):
        y, st, _ = branch_refs["limited", W]
        assert round(20 * np.log10(st["tp_in_q28"] / 2 ** 28), 2) == 0.21
        assert st["trim_q16"] == ONE and st["tp_limited_q28"] == st["tp_out_q28"] <= st["ceiling_q28"]
        assert 0 < st["limited_frames"] and st["min_gain_q16"] < ONE
        assert not np.array_equal(y, branch_inputs["limited"])
        share[W] = st["limited_frames"] / 20000
    print("limited share of frames by window:", share)
    assert 0.004 <= share[1] <= 0.006 and 0.78 <= share[1024] <= 0.82  # 0.5 % and 80 %
    assert share[1] < share[16] < share[220] < share[1024]


def test_branch_trimmed(branch_refs):
    C = q28(-1.0)
    for W, trim in ((1, 65254), (16, 65514)):
        _, st, _ = branch_refs["trimmed", W]
        assert st["trim_q16"] == trim and st["tp_limited_q28"] > C >= st["tp_out_q28"]
    over = {W: 20 * np.log10(branch_refs["trimmed", W][1]["tp_limited_q28"] / C) for W in (1, 16)}
    print("limiter alone ends over the ceiling by (dB):", over)
    assert round(over[1], 3) == 0.037 and round(over[16], 4) == 0.0025
    for W in (220, 1024):
        _, st, _ = branch_refs["trimmed", W]
        assert st["trim_q16"] == ONE and st["limited_frames"] > 0 and st["tp_out_q28"] <= C


def test_boundary_lone_impulse():
    """P of a lone impulse of 20000 is 7964 * 20000: a ceiling of exactly that leaves it
    alone, one less limits it."""
    pcm = np.zeros(64, np.int16)
    pcm[30] = 20000
    peak = 7964 * 20000
    y, st = host_ceiling(pcm, peak, 4)
    assert np.array_equal(y, pcm) and st["limited_frames"] == 0 and st["tp_in_q28"] == st["tp_out_q28"] == peak
    assert st == ref_ceiling(pcm, peak, 4)[1]
    y, st = host_ceiling(pcm, peak - 1, 4)
    want, wst = ref_ceiling(pcm, peak - 1, 4)
    assert st == wst and np.array_equal(y, want)
    assert st["limited_frames"] > 0 and y[30] < 20000 and st["tp_out_q28"] <= peak - 1


@pytest.mark.parametrize("W", [1, 16])
def test_boundary_need_at_the_guarded_ceiling(W):
    """Two impulses further apart than 2W + 12, the larger over the ceiling: the smaller
    one keeps r = ONE when its P equals C_t exactly, and loses it at C_t + 1."""
    small = 15000
    Ct = 7964 * small
    pcm = np.zeros(400, np.int16)
    pcm[50], pcm[50 + 2 * W + 13 + 100] = 32767, small
    at = 50 + 2 * W + 13 + 100
    limited = {}
    for C, kept in ((Ct + GUARD, True), (Ct + GUARD - 1, False)):  # C_t = P, then C_t = P - 1
        d = {}
        y, st = host_ceiling(pcm, C, W)
        want, wst = ref_ceiling(pcm, C, W, d)
        assert st == wst and np.array_equal(y, want)
        assert st["tp_in_q28"] == 7964 * 32767 > C and y[50] < 32767
        assert (d["R"][at] == ONE) == kept and d["R"][at] >= ONE - 1
        # its peak 7964 * s stands at Y[at + 5] (phase 3) and Y[at + 6] (phase 0): samples
        # at-6 .. at+6 feed one of them, and the ramps reach 2W further
        assert np.all(d["g"][at - 6 - 2 * W:at + 6 + 2 * W + 1] < ONE) == (not kept)
        assert np.all(d["g"][at + 6 + 2 * W + 1:] == ONE)
        limited[kept] = st["limited_frames"]
    assert limited[False] == limited[True] + 4 * W + 13  # the hold of 13 frames and both ramps


def test_host_rejects_bad_arguments():
    from mastering_amd import native
    lib = native.load()
    x = np.zeros(16, np.int16)
    m = native.MMCeiling()
    p = x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))
    assert lib.mm_ceiling_max_window() == 1024
    for C, W in ((2 ** 24 - 1, 16), (2 ** 28 + 1, 16), (2 ** 27, 0), (2 ** 27, 1025)):
        assert lib.mm_ceiling_host(p, 16, 1, C, W, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_ceiling_host(p, 16, 1, 2 ** 24, 1024, ctypes.byref(m)) == 0
    assert lib.mm_ceiling_host(p, 16, 3, 2 ** 27, 16, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_ceiling_host(p, 2 ** 31, 1, 2 ** 27, 16, ctypes.byref(m)) == native.MM_ERR_ARG


def test_ceiling_span_is_a_launch_constant():
    from mastering_amd import native
    s = native.load().mm_ceiling_span()
    assert s >= 12 and s < 63488  # the uint32 box sums: (span + 2 * 1024) * 2^16 < 2^32


def test_ceiling_layouts_match_c(tmp_path):
    from mastering_amd import native
    fields = {"mm_ceiling": ([f[0] for f in native.MMCeiling._fields_], native.MMCeiling),
              "mm_job": (["ceiling_q28", "meter_on"], native.MMJob)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mastering.h"', "int main(void){"]
    for st, (fl, _) in fields.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fl]
    lines.append('printf("abi %d\\n", MM_ABI_VERSION);')
    lines.append("return 0;}")
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for st, (fl, cls) in fields.items():
        assert int(got[st]) == ctypes.sizeof(cls), st
        for f in fl:
            assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"
    assert int(got["mm_job.ceiling_q28"]) == int(got["mm_job.meter_on"]) + 4
    assert int(got["mm_job.ceiling_q28"]) + 4 == int(got["mm_job"])  # the former trailing pad: the size is kept
    assert int(got["abi"]) == native.ABI_VERSION == 5


def test_design_ceiling_q28():
    from mastering_amd import design
    assert design.ceiling_q28(0) == 2 ** 28
    assert design.ceiling_q28(-1.0) == int(np.floor(10 ** (-1 / 20) * 2 ** 28)) == 239243351
    assert design.ceiling_q28(-24) == int(np.floor(10 ** (-24 / 20) * 2 ** 28)) >= 2 ** 24
    for bad in (0.01, -24.01, float("nan"), 3):
        with pytest.raises(ValueError):
            design.ceiling_q28(bad)


def test_design_ceiling_window():
    from mastering_amd import design
    assert [design.ceiling_window(r) for r in (8000, 44100, 192000, 384000)] == [40, 220, 960, 1024]
    assert design.ceiling_window(100) == 1 and design.ceiling_window(48000) == 240


def test_job_ceiling_field():
    from mastering_amd import design, engine
    params = {"multiband": True, "lufs": -14.0}
    assert engine.Job(44100, 44100, 2, params).job.ceiling_q28 == 0
    assert engine.Job(44100, 44100, 2, params, ceiling_dbtp=-1.0).job.ceiling_q28 == design.ceiling_q28(-1.0)
    assert engine.Job(44100, 44100, 2, params, ceiling_dbtp=0).job.ceiling_q28 == 2 ** 28
    with pytest.raises(ValueError):
        engine.Job(44100, 44100, 2, params, ceiling_dbtp=1.0)
    with pytest.raises(ValueError):
        engine.Job(44100, 44100, 2, params, seg_bounds=[0, 17640, 44100], check_length=False, ceiling_dbtp=-1.0)


def test_time_sharded_path_refuses_the_ceiling():
    from mastering_amd import distributed
    with pytest.raises(ValueError, match="ceiling"):
        distributed.master_time_sharded(None, None, {"lufs": -14.0, "ceiling_dbtp": -1.0}, 0, 0, None)


def test_ceiling_dict():
    from mastering_amd import engine, native
    m = native.MMCeiling()
    m.frames, m.channels, m.window, m.ceiling_q28 = 100, 2, 220, 2 ** 27
    m.tp_in_q28, m.tp_limited_q28, m.tp_out_q28 = 2 ** 28, 2 ** 27, 2 ** 27
    m.min_gain_q16, m.trim_q16, m.limited_frames = 2 ** 15, ONE, 7
    d = engine.ceiling_dict(m)
    assert {k: d[k] for k in STATS} == ceiling_stats(m)
    assert d["tp_in_dbtp"] == 0.0 and d["tp_out_dbtp"] == d["ceiling_dbtp"] == 20 * np.log10(0.5)
    assert d["max_reduction_db"] == -20 * np.log10(0.5) and d["trimmed"] is False
    m.trim_q16 = 65254
    assert engine.ceiling_dict(m)["trimmed"] is True


def test_gui_and_worker_pass_the_ceiling_through(tmp_path, monkeypatch):
    import json
    from mastering_amd import engine, gui_compat
    from mastering_amd.worker import process_audio_from_gcs
    ceiling = {"ceiling_dbtp": -1.0, "tp_in_dbtp": 4.76, "tp_out_dbtp": -1.02, "max_reduction_db": 5.78,
               "trimmed": False}
    seen = []

    def process(src, dst, params, device=0, verbose=False):
        seen.append(dict(params))
        with open(dst, "wb") as f:
            f.write(b"RIFF")
        return {"loudness": -20.0, "ceiling": dict(ceiling)} if "ceiling_dbtp" in params else {"loudness": -20.0}

    monkeypatch.setattr(engine, "process", process)
    said = []
    s = {"input_file": str(tmp_path / "a.wav"), "output_file": str(tmp_path / "b.wav"), "lufs": -14.0}
    gui_compat.process_audio(dict(s, ceiling_dbtp=-1.0), said.append)
    assert seen[-1]["ceiling_dbtp"] == -1.0
    assert said[-2] == "Ceiling -1.00 dBTP: true peak +4.76 -> -1.02 dBTP, up to 5.78 dB reduction"
    said.clear()
    gui_compat.process_audio(s, said.append)
    assert not any(m.startswith("Ceiling") for m in said)
    (tmp_path / "b").mkdir()
    (tmp_path / "b" / "x.wav").write_bytes(b"")
    out = tmp_path / "b" / "processed" / "mastered_x.wav"
    process_audio_from_gcs("gs://b/x.wav", {"lufs": -14.0}, root=str(tmp_path))
    assert out.exists() and not os.path.exists(str(out) + ".ceiling.json")
    process_audio_from_gcs("gs://b/x.wav", {"lufs": -14.0, "ceiling_dbtp": -1.0}, root=str(tmp_path))
    assert json.loads(open(str(out) + ".ceiling.json").read()) == ceiling
    assert os.path.exists(str(out) + ".complete") and not list((tmp_path / "b" / "processed").glob("*.part"))
