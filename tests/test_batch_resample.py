"""A batch or an album at another rate on CPU: the names import, the C entries are declared,
exported and bound with the signature a C caller compiles against, what is not such a call is
refused in Python before any context is touched, an `output_rate` equal to the jobs' rate plans
nothing, and the layout arithmetic of the converter's grid (csrc/tracks.h) passes its
stand-alone check (the device side is tests/test_gpu_batch_resample.py and
tests/test_gpu_batch_deliver_rate.py)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = ("mm_batch_resample_device", "mm_batch_resample_pcm")


def test_the_names_are_exported():
    import mastering_amd
    assert callable(mastering_amd.resample_batch_pcm) and "resample_batch_pcm" in mastering_amd.__all__
    for fn, kws in ((mastering_amd.deliver_batch, ("output_rate", "d_mids")), (mastering_amd.master_album, ("output_rate", "d_mids")),
                    (mastering_amd.process_batch, ("output_rate",)), (mastering_amd.process_album, ("output_rate",))):
        par = inspect.signature(fn).parameters
        for kw in kws:
            assert kw in par and par[kw].default is None, (fn.__name__, kw)
        assert "output_rate" in fn.__doc__ and "refused" in fn.__doc__  # the params key stays refused, and says so
    assert "output_rate" in mastering_amd.master_batch.__doc__ and "refused" in mastering_amd.master_batch.__doc__


def test_the_c_entries_are_declared_exported_and_bound():
    from mastering_amd import native
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mastering.h")).read(), flags=re.S)
    lib = native.load()
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert name in native.EXPORTS and getattr(lib, name).argtypes is not None
    assert lib.mm_version() == native.ABI_VERSION == 5  # additive: the ABI stays
    # refused without a context, before anything else
    assert lib.mm_batch_resample_device(None, None, 0, None, 1, 2, None, None, None) == native.MM_ERR_ARG
    assert lib.mm_batch_resample_pcm(None, None, 0, None, 1, 2, None, None, None) == native.MM_ERR_ARG


def test_layouts_and_signatures_match_c(tmp_path):
    """mm_resampler and mm_resample field by field, and the two entries assigned to function
    pointers of the types native.py binds (a mismatch of the header is a compile error)."""
    from mastering_amd import native
    fields = {"mm_resampler": native.MMResampler, "mm_resample": native.MMResample}
    inc = ["-I", os.path.join(ROOT, "include")]
    sig = tmp_path / "signature.c"  # compiled only: the types must agree, nothing is linked or run
    sig.write_text("\n".join([
        '#include "mastering.h"',
        "typedef int (*batch_fn)(mm_ctx *, const void *const *, int, const int64_t *, int, int, const mm_resampler *,",
        "                        void *const *, mm_resample *);",
        "batch_fn entries[2] = {mm_batch_resample_device, mm_batch_resample_pcm};", ""]))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", *inc, "-c", str(sig), "-o", str(tmp_path / "signature.o")])
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mastering.h"', "int main(void){"]
    for st, cls in fields.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines += ['printf("tracks %d\\n", MM_ALBUM_TRACKS);', 'printf("abi %d\\n", MM_ABI_VERSION);', "return 0;}"]
    prog = tmp_path / "layout.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", *inc, str(prog), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for st, cls in fields.items():
        assert int(got[st]) == ctypes.sizeof(cls), st
        for f, _ in cls._fields_:
            assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"
    assert int(got["tracks"]) == native.ALBUM_TRACKS and int(got["abi"]) == native.ABI_VERSION == 5
    vp, P = ctypes.c_void_p, ctypes.POINTER
    want = [vp, P(vp), ctypes.c_int, P(ctypes.c_int64), ctypes.c_int, ctypes.c_int, P(native.MMResampler), P(vp),
            P(native.MMResample)]
    lib = native.load()
    for name in ENTRIES:
        assert list(getattr(lib, name).argtypes) == want and getattr(lib, name).restype is ctypes.c_int, name


def test_python_refusals_need_no_gpu(tmp_path, monkeypatch):
    from mastering_amd import deliver_batch, engine, master_album, native, process_album, process_batch, resample_batch_pcm, wavio

    def no_context(device=0):
        raise AssertionError("a refused call must not reach the device")

    monkeypatch.setattr(native, "context", no_context)
    st, mono, f32 = np.zeros((100, 2), np.int16), np.zeros(100, np.int16), np.zeros((100, 2), np.float32)
    with pytest.raises(ValueError, match="1 to 256 tracks, not 0"):
        resample_batch_pcm([], 96000, 44100)
    with pytest.raises(ValueError, match="1 to 256 tracks, not 257"):
        resample_batch_pcm([st] * 257, 96000, 44100)
    with pytest.raises(ValueError, match="one channel count"):
        resample_batch_pcm([st, mono], 96000, 44100)
    with pytest.raises(ValueError, match="one sample type"):
        resample_batch_pcm([st, f32], 96000, 44100)
    for a, b in ((44100, 44100), (96000, 44101), (44100, 5000)):
        with pytest.raises(ValueError):
            resample_batch_pcm([st], a, b)
    p = {"lufs": -14.0}
    job = lambda **kw: engine.Job(kw.pop("n", 96000), kw.pop("rate", 96000), 2, p, **kw)  # noqa: E731
    calls = ((lambda jobs, **kw: deliver_batch(None, jobs, [0] * len(jobs), [0] * len(jobs), -14.0, -1.0, **kw)),
             (lambda jobs, **kw: master_album(None, jobs, [0] * len(jobs), [0] * len(jobs), -14.0, -1.0, **kw)))
    for call in calls:
        with pytest.raises(ValueError, match="d_mids"):  # output_rate without d_mids
            call([job(), job()], output_rate=44100)
        with pytest.raises(ValueError, match="d_mids: 1 buffers for 2 jobs"):  # a wrong d_mids length
            call([job(), job()], output_rate=44100, d_mids=[0])
        with pytest.raises(ValueError, match="d_mids: 3 buffers for 2 jobs"):
            call([job(), job()], output_rate=44100, d_mids=[0, 0, 0])
        for bad in (44101, 5000, 0):  # a pair design.resample_geometry refuses
            with pytest.raises(ValueError):
                call([job(), job()], output_rate=bad, d_mids=[0, 0])
        with pytest.raises(ValueError, match="one sample rate"):  # mixed rates
            call([job(), job(rate=48000)], output_rate=44100, d_mids=[0, 0])
        with pytest.raises(ValueError, match="without a delivery"):  # a job's own plan stays refused
            call([job(output_rate=44100)], output_rate=44100, d_mids=[0])
    # the files: a rate pair is refused before the device, and the params key stays refused
    a = str(tmp_path / "a.wav")
    wavio.write_wav(a, np.zeros((96000, 2), np.int16), 96000)
    for fn in (process_batch, process_album):
        with pytest.raises(ValueError):
            fn([a], [a + ".out"], {"deliver_lufs": -14.0}, output_rate=44101)
        with pytest.raises(ValueError, match=r"delivery at another rate \(output_rate\) is not available for a batch"):
            fn([a], [a + ".out"], {"deliver_lufs": -14.0, "output_rate": 44100}, output_rate=44100)
    assert not [f for f in os.listdir(tmp_path) if ".out" in f]  # nothing was written
    with pytest.raises(ValueError, match=r"delivery at another rate \(output_rate\) is not available for a batch"):
        engine.master_batch(None, [job(output_rate=44100)], [0], [0])


def test_output_rate_equal_to_the_rate_plans_nothing(monkeypatch):
    """None and the jobs' own rate: no converter is planned, d_mids is not looked at, and the
    batch is mastered into d_outs as before."""
    from mastering_amd import deliver_batch, engine, master_album
    jobs = [engine.Job(96000, 96000, 2, {"lufs": -14.0}) for _ in range(2)]
    assert engine._batch_resampler(jobs, None, None, "a batch") is None
    assert engine._batch_resampler(jobs, 96000, None, "a batch") is None
    assert engine._batch_resampler(jobs, 96000.0, [0], "a batch") is None
    rs = engine._batch_resampler(jobs, 44100, [1, 2], "a batch")
    assert (rs.L, rs.M, rs.K, rs.rs.rate_in, rs.rs.rate_out) == (147, 320, 280, 96000, 44100)
    assert rs.frames_out(jobs[0].frames_proc) == -(-jobs[0].frames_proc * 147 // 320)
    seen = []

    class Reached(Exception):
        pass

    def fake_master_batch(ctx, js, d_ins, d_outs, with_results=True):
        seen.append(list(d_outs))
        raise Reached

    monkeypatch.setattr(engine, "master_batch", fake_master_batch)
    for fn in (deliver_batch, master_album):
        for kw in ({}, {"output_rate": None}, {"output_rate": 96000}, {"output_rate": 96000, "d_mids": [7, 8]}):
            with pytest.raises(Reached):
                fn(None, jobs, [1, 2], [3, 4], -14.0, -1.0, **kw)
            assert seen.pop() == [3, 4]
        with pytest.raises(Reached):
            fn(None, jobs, [1, 2], [3, 4], -14.0, -1.0, output_rate=44100, d_mids=[7, 8])
        assert seen.pop() == [7, 8]  # at another rate the batch is mastered into the mids


def test_the_layout_check_covers_the_converter_grid(tmp_path):
    """tools/diag/tracks_layout_host_check.cpp walks the converter's grid too (built plainly here;
    its header comment gives the build line with the sanitizers)."""
    src = os.path.join(ROOT, "tools", "diag", "tracks_layout_host_check.cpp")
    assert "tracks_resample_spans" in open(src).read()
    exe = str(tmp_path / "tracks_layout_host_check")
    subprocess.check_call(["c++", "-O1", "-std=c++17", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().endswith("tracks_layout_host_check: 0 failure(s)")
