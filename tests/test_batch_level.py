"""The batch level on CPU: the names import, the C entries are declared, exported and bound,
and what is not a batch is refused in Python before any context is touched (the device side is
tests/test_gpu_batch_ceiling.py and tests/test_gpu_batch_level.py; the layout arithmetic of
csrc/tracks.h is checked by tools/diag/tracks_layout_host_check.cpp, built and run here too)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

RATE = 44100
ENTRIES = ("mm_batch_ceiling_device", "mm_batch_ceiling_pcm", "mm_batch_level_device", "mm_batch_level_pcm")


def test_the_names_are_exported():
    import mastering_amd
    for name in ("ceiling_batch_pcm", "level_batch_pcm", "deliver_batch", "process_batch"):
        assert callable(getattr(mastering_amd, name)) and name in mastering_amd.__all__


def test_the_c_entries_are_declared_exported_and_bound():
    from mastering_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mastering.h")).read(), flags=re.S)
    lib = native.load()
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert name in native.EXPORTS and getattr(lib, name).argtypes is not None
    assert lib.mm_version() == native.ABI_VERSION == 5  # additive: the ABI stays


def test_the_c_entries_refuse_without_a_context():
    """(MM_ERR_ARG before anything else: no device is touched)"""
    from mastering_amd import native
    lib = native.load()
    assert lib.mm_batch_level_device(None, None, 0, None, 1, 2, RATE, None, None, None, 220) == native.MM_ERR_ARG
    assert lib.mm_batch_ceiling_device(None, None, 0, None, 1, 2, None, 220, None) == native.MM_ERR_ARG


def test_python_refusals_need_no_gpu(tmp_path, monkeypatch):
    from mastering_amd import ceiling_batch_pcm, deliver_batch, engine, level_batch_pcm, native, process_batch, wavio

    def no_context(device=0):
        raise AssertionError("a refused batch must not reach the device")

    monkeypatch.setattr(native, "context", no_context)
    st, mono, f32 = np.zeros((100, 2), np.int16), np.zeros(100, np.int16), np.zeros((100, 2), np.float32)
    for fn, tail in ((level_batch_pcm, (RATE, -14.0)), (ceiling_batch_pcm, (RATE, -1.0))):
        with pytest.raises(ValueError, match="1 to 256 tracks, not 0"):
            fn([], *tail)
        with pytest.raises(ValueError, match="1 to 256 tracks, not 257"):
            fn([st] * 257, *tail)
        with pytest.raises(ValueError, match="one channel count"):
            fn([st, mono], *tail)
        with pytest.raises(ValueError, match="one sample type"):
            fn([st, f32], *tail)
    # a sequence whose length is not the track count
    with pytest.raises(ValueError, match="target_lufs: 3 values for 2 tracks"):
        level_batch_pcm([st, st], RATE, [-14.0, -16.0, -11.0])
    with pytest.raises(ValueError, match="ceiling_dbtp: 1 values for 2 tracks"):
        level_batch_pcm([st, st], RATE, -14.0, [-1.0])
    with pytest.raises(ValueError, match="ceiling_dbtp: 3 values for 2 tracks"):
        ceiling_batch_pcm([st, st], RATE, (-1.0, -2.0, -3.0))
    # a target outside [-40, -5], alone and as one of several; a ceiling outside [-24, 0]
    with pytest.raises(ValueError, match=r"loudness target -4.0 LUFS outside \[-40, -5\]"):
        level_batch_pcm([st], RATE, -4.0)
    with pytest.raises(ValueError, match=r"loudness target -41.0 LUFS outside \[-40, -5\]"):
        level_batch_pcm([st, st], RATE, [-14.0, -41.0])
    with pytest.raises(ValueError, match="ceiling"):
        level_batch_pcm([st, st], RATE, -14.0, [None, 1.0])
    with pytest.raises(ValueError, match="ceiling"):
        ceiling_batch_pcm([st], RATE, 1.0)
    # deliver_batch: the jobs of a batch to deliver
    p = {"lufs": -14.0}
    job = lambda **kw: engine.Job(kw.pop("n", 44100), kw.pop("rate", 44100), kw.pop("ch", 2), p, **kw)  # noqa: E731
    for jobs, words in (([], "1 to 256 tracks, not 0"), ([job()] * 257, "1 to 256 tracks, not 257"),
                        ([job(), job(ceiling_dbtp=-1.0)], "without ceiling_dbtp"),
                        ([job(deliver_lufs=-14.0)], "without a delivery"), ([job(output_rate=48000)], "without a delivery"),
                        ([job(), job(report=True)], "without report or r128"), ([job(r128=True)], "without report or r128"),
                        ([job(), job(rate=48000)], "one sample rate"), ([job(), job(ch=1)], "one channel count"),
                        ([job(), job(out_kind=native.MM_OUT_F32)], "one output kind")):
        with pytest.raises(ValueError, match=words):
            deliver_batch(None, jobs, [0] * len(jobs), [0] * len(jobs), -14.0, -1.0)
    with pytest.raises(ValueError, match="outside"):
        deliver_batch(None, [job()], [0], [0], -4.0)
    with pytest.raises(ValueError, match="deliver_lufs: 1 values for 2 tracks"):
        deliver_batch(None, [job(), job()], [0, 0], [0, 0], [-14.0])
    with pytest.raises(ValueError, match="ceiling_dbtp: 3 values for 2 tracks"):
        deliver_batch(None, [job(), job()], [0, 0], [0, 0], -14.0, [-1.0, None, -1.0])
    # process_batch: the keys and the files
    a, b, m = str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), str(tmp_path / "m.wav")
    wavio.write_wav(a, np.zeros((44100, 2), np.int16), 44100)
    wavio.write_wav(b, np.zeros((48000, 2), np.int16), 48000)
    wavio.write_wav(m, np.zeros(44100, np.int16), 44100)
    with pytest.raises(ValueError, match="deliver_lufs"):
        process_batch([a], [a + ".out"], {"lufs": -14.0})
    with pytest.raises(ValueError, match=r"delivery at another rate \(output_rate\) is not available for a batch"):
        process_batch([a], [a + ".out"], {"deliver_lufs": -14.0, "output_rate": 48000})
    for key in ("report", "r128"):
        with pytest.raises(ValueError, match=f"takes no params\\['{key}'\\]"):
            process_batch([a], [a + ".out"], {"deliver_lufs": -14.0, key: True})
    with pytest.raises(ValueError, match="one output path"):
        process_batch([a, b], [a + ".out"], {"deliver_lufs": -14.0})
    with pytest.raises(ValueError, match="deliver_lufs: 3 values for 2 tracks"):
        process_batch([a, a], [a + ".1", a + ".2"], {"deliver_lufs": [-14.0, -15.0, -16.0]})
    with pytest.raises(ValueError, match="one sample rate"):
        process_batch([a, b], [a + ".out", b + ".out"], {"deliver_lufs": -14.0})
    with pytest.raises(ValueError, match="one channel count"):
        process_batch([a, m], [a + ".out", m + ".out"], {"deliver_lufs": -14.0})
    with pytest.raises(ValueError, match="1 to 256 tracks, not 0"):
        process_batch([], [], {"deliver_lufs": -14.0})
    assert not [f for f in os.listdir(tmp_path) if ".out" in f or f[-2:] in (".1", ".2")]  # nothing was written
    # master_batch keeps its refusal of a job planned with deliver_lufs, word for word
    with pytest.raises(ValueError, match="a loudness target \\(deliver_lufs\\) re-measures one delivered track pass by "
                                         "pass: not available for a batch"):
        engine.master_batch(None, [job(deliver_lufs=-14.0)], [0], [0])


def test_the_layout_header_stand_alone(tmp_path):
    """tools/diag/tracks_layout_host_check.cpp: csrc/tracks.h alone, on the CPU, a stand-alone program
    (its header comment gives the build line with the sanitizers; here it is built plainly)."""
    exe = str(tmp_path / "tracks_layout_host_check")
    subprocess.check_call(["c++", "-O1", "-std=c++17", os.path.join(ROOT, "tools", "diag", "tracks_layout_host_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().endswith("tracks_layout_host_check: 0 failure(s)")
