"""The mastering report on CPU: the BS.1770-4 Annex 2 tap table, the library's host
restatement of the integer meter (mm_true_peak_host) against ten lines of numpy
written from the definition in include/mastering.h, the mm_meter / mm_job.meter_on
layouts, and the Python plumbing that needs no GPU."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

C0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
C1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
TAPS = np.array([C0, C1, C1[::-1], C0[::-1]], dtype=np.int64)  # H * 8192
FIELDS = ("sample_peak", "clipped", "true_peak_q28", "true_peak_frame", "overs")


def ref_meter(pcm):
    """The definition, in numpy int64: Y[m][p] = sum_k C[p][k] s[m-k] over the full
    convolution m in [0, N + 11), s = 0 outside [0, N)."""
    x = np.asarray(pcm).reshape(len(pcm), -1).astype(np.int64)
    out = {f: [] for f in FIELDS}
    for s in x.T:
        z = np.concatenate([np.zeros(11, np.int64), s, np.zeros(11, np.int64)])  # z[i] = s[i - 11]
        Y = sum(TAPS[:, k, None] * z[None, 11 - k:11 - k + len(s) + 11] for k in range(12))  # [4][N + 11]
        A = np.abs(Y).max(axis=0)
        out["sample_peak"].append(int(np.abs(s).max()))
        out["clipped"].append(int((np.abs(s) >= 32767).sum()))
        out["true_peak_q28"].append(int(A.max()))
        out["true_peak_frame"].append(int(np.argmax(A)))  # first occurrence
        out["overs"].append(int((A > 2 ** 28).sum()))
    return out


def meter_fields(m):
    return {f: [int(getattr(m, f)[c]) for c in range(m.channels)] for f in FIELDS}


def worst_case(n=64, at=30):
    """Every tap of phase 1 meets a full-scale sample of its own sign at m = `at`."""
    s = np.full(n, 32767, np.int16)
    for k in range(12):
        if C1[k] > 0:
            s[at - k] = -32768
    return s


def host_meter(pcm):
    from mastering_amd import native
    lib = native.load()
    x = np.ascontiguousarray(pcm, np.int16)
    m = native.MMMeter()
    rc = lib.mm_true_peak_host(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), x.shape[0],
                               1 if x.ndim == 1 else x.shape[1], ctypes.byref(m))
    assert rc == 0
    assert m.frames == x.shape[0] and math.isnan(m.loudness)
    return meter_fields(m)


def test_tap_table():
    from mastering_amd import design
    H = design.TRUE_PEAK_TAPS
    assert H.shape == (4, 12) and H.dtype == np.float64
    C = H * 8192
    assert np.array_equal(C[0], C0) and np.array_equal(C[1], C1)
    assert H[0][0] == 0.0017089843750 and H[0][1] == 0.0109863281250 and H[0][-1] == -0.0083007812500
    assert H[1][0] == -0.0291748046875 and H[1][1] == 0.0292968750000 and H[1][-1] == -0.0189208984375
    assert np.array_equal(H[3], H[0][::-1]) and np.array_equal(H[2], H[1][::-1])
    assert np.abs(C).sum(axis=1).tolist() == [11749, 16571, 16571, 11749]
    assert np.array_equal(C, TAPS)


def test_reference_is_upfirdn():
    """The numpy reference is the full convolution scipy computes: on int16-grid input
    max|y| * 2^28 equals the integer peak exactly."""
    import scipy.signal
    from mastering_amd import design
    pcm = np.random.default_rng(7).integers(-32768, 32768, (5000, 2)).astype(np.int16)
    h = design.TRUE_PEAK_TAPS.T.reshape(-1)  # h[4k + p] = H[p][k]
    ref = ref_meter(pcm)
    for c in range(2):
        y = scipy.signal.upfirdn(h, pcm[:, c] / 32768.0, up=4)
        assert len(y) == 4 * (5000 + 11)
        assert np.max(np.abs(y)) * 2.0 ** 28 == ref["true_peak_q28"][c]
        assert int(np.argmax(np.abs(y).reshape(-1, 4).max(axis=1))) == ref["true_peak_frame"][c]


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n", [1, 11, 12, 13, 1000])
def test_host_restatement_random(n, ch):
    pcm = np.random.default_rng(100 * n + ch).integers(-32768, 32768, (n, ch) if ch == 2 else (n,)).astype(np.int16)
    assert host_meter(pcm) == ref_meter(pcm)


def test_host_restatement_silence():
    got = host_meter(np.zeros((50, 2), np.int16))
    assert got == ref_meter(np.zeros((50, 2), np.int16))
    assert got["true_peak_q28"] == [0, 0] and got["true_peak_frame"] == [0, 0]


def test_host_restatement_tail_impulse():
    pcm = np.zeros(100, np.int16)
    pcm[99] = -32768
    got = host_meter(pcm)
    assert got == ref_meter(pcm)
    assert got["true_peak_q28"] == [260964352] and got["true_peak_frame"] == [104]  # past the last input frame
    assert got["sample_peak"] == [32768] and got["clipped"] == [1]


def test_host_restatement_worst_case():
    pcm = worst_case()
    got = host_meter(pcm)
    assert got == ref_meter(pcm)
    assert got["true_peak_q28"] == [542994228] and got["true_peak_q28"][0] < 2 ** 31
    assert got["overs"][0] >= 1


def test_meter_layouts_match_c(tmp_path):
    from mastering_amd import native
    fields = {"mm_meter": ([f[0] for f in native.MMMeter._fields_], native.MMMeter),
              "mm_job": (["meter_on", "sat_key"], native.MMJob)}
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
    assert int(got["abi"]) == native.ABI_VERSION == 5
    assert native.MMJob.meter_on.offset > native.MMJob.sat_key.offset  # trailing: older fields keep their place


def test_job_meter_flag():
    from mastering_amd import engine
    params = {"multiband": True, "lufs": -14.0}
    assert engine.Job(44100, 44100, 2, params).job.meter_on == 0
    assert engine.Job(44100, 44100, 2, params, report=True).job.meter_on == 1
    # report alone plans the loudness geometry (for the meter) but no normalisation...
    j = engine.Job(44100, 44100, 2, {}, report=True)
    assert j.job.lufs_on == 0 and j.job.n_blocks >= 1 and j.job.kweight.nsec == 2
    # ...and none on a track shorter than one 0.4 s block, which is not an error
    j = engine.Job(4000, 44100, 2, {}, report=True)
    assert j.job.meter_on == 1 and j.job.n_blocks == 0
    assert engine.Job(44100, 44100, 2, {}).job.n_blocks == 0


def test_meter_span_is_a_launch_constant():
    from mastering_amd import native
    s = native.load().mm_meter_span()
    assert s >= 12 and s % 2 == 0


def test_report_dict():
    from mastering_amd import engine, native
    m = native.MMMeter()
    m.frames, m.channels = 100, 2
    m.sample_peak[0], m.sample_peak[1] = 32768, 0
    m.true_peak_q28[0], m.true_peak_q28[1] = 2 ** 28, 0
    m.true_peak_frame[0], m.clipped[0], m.overs[0] = 104, 3, 2
    m.loudness = float("nan")
    r = engine.report_dict(m, -14.0)
    assert r["sample_peak_dbfs"] == [0.0, -math.inf] and r["true_peak_dbtp"] == [0.0, -math.inf]
    assert r["true_peak_frame"] == [104, 0] and r["clipped"] == [3, 0] and r["overs"] == [2, 0]
    assert r["sample_peak"] == [32768, 0] and r["true_peak_q28"] == [2 ** 28, 0]
    assert r["max_true_peak_dbtp"] == 0.0 and r["output_loudness"] is None and "loudness_error" not in r
    m.loudness = -14.5
    r = engine.report_dict(m, -14.0)
    assert r["output_loudness"] == -14.5 and r["loudness_error"] == -0.5
    assert "loudness_error" not in engine.report_dict(m)


def test_true_peak_rejects_int_input():
    from mastering_amd import ops
    with pytest.raises(TypeError):
        ops.true_peak(np.zeros(16, np.int16))


REPORT = {"output_loudness": -14.21, "max_true_peak_dbtp": -0.42, "true_peak_dbtp": [-0.42, -math.inf]}


@pytest.fixture
def fake_process(monkeypatch):
    from mastering_amd import engine
    seen = []

    def process(src, dst, params, device=0, verbose=False):
        seen.append(dict(params))
        with open(dst, "wb") as f:
            f.write(b"RIFF")
        info = {"loudness": -20.0}
        if params.get("report"):
            info["report"] = dict(REPORT)
        return info

    monkeypatch.setattr(engine, "process", process)
    return seen


def test_gui_status_line(tmp_path, fake_process):
    from mastering_amd import gui_compat
    said = []
    s = {"input_file": str(tmp_path / "a.wav"), "output_file": str(tmp_path / "b.wav"), "lufs": -14.0}
    gui_compat.process_audio(dict(s, report=True), said.append)
    assert said[-2] == "Output: -14.21 LUFS, true peak -0.42 dBTP" and "complete" in said[-1]
    assert fake_process[-1]["report"] is True
    said.clear()
    gui_compat.process_audio(s, said.append)
    assert not any(m.startswith("Output:") for m in said) and "report" not in fake_process[-1]


def test_worker_report_file(tmp_path, fake_process):
    from mastering_amd.worker import process_audio_from_gcs
    (tmp_path / "b").mkdir()
    (tmp_path / "b" / "x.wav").write_bytes(b"")
    process_audio_from_gcs("gs://b/x.wav", {"lufs": -14.0}, root=str(tmp_path))
    out = tmp_path / "b" / "processed" / "mastered_x.wav"
    assert out.exists() and not (tmp_path / "b" / "processed" / "mastered_x.wav.report.json").exists()
    process_audio_from_gcs("gs://b/x.wav", {"lufs": -14.0, "report": True}, root=str(tmp_path))
    rep = json.loads((tmp_path / "b" / "processed" / "mastered_x.wav.report.json").read_text())
    assert rep["output_loudness"] == -14.21 and rep["true_peak_dbtp"] == [-0.42, None]  # strict JSON: no -Infinity
    assert (tmp_path / "b" / "processed" / "mastered_x.wav.complete").exists()
    assert not list((tmp_path / "b" / "processed").glob("*.part"))
