"""The mastering report on the GPU: the meter kernels against the numpy definition
(tests/test_meter.py: ref_meter) at the sizes where they can go wrong (the workgroup
span of mm_meter_span and its seams, the 11-frame tail, ties, the int32 worst case),
the f32-buffer variant, the off-grid operator, and the report through every chain
entry point.  All peak fields are integers and are compared for equality."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from test_meter import TAPS, meter_fields, ref_meter, worst_case

pytestmark = pytest.mark.gpu

SMOKE = {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0,
         "saturation": 30, "width": 1.3, "multiband": True, "lufs": -14.0}


@pytest.fixture(scope="module")
def span():
    from mastering_amd import native
    return native.load().mm_meter_span()


def dev_meter(pcm, f32=False, loud=None):
    """mm_meter_device on a device copy of int16 `pcm` (or of pcm / 32768 as f32)."""
    import torch
    from mastering_amd import native
    x = np.ascontiguousarray(pcm, np.int16)
    host = x.astype(np.float32) / np.float32(32768) if f32 else x
    d = torch.from_numpy(host).cuda()
    torch.cuda.current_stream().synchronize()  # the copy is on torch's stream, the library uses its own
    ctx = native.context(0)
    m = native.MMMeter()
    ctx.check(ctx.lib.mm_meter_device(ctx.ptr, ctypes.c_void_p(d.data_ptr()),
                                      native.MM_OUT_F32 if f32 else native.MM_OUT_I16, x.shape[0],
                                      1 if x.ndim == 1 else x.shape[1],
                                      ctypes.byref(loud.job) if loud is not None else None, ctypes.byref(m)),
              "mm_meter_device")
    assert m.frames == x.shape[0]
    return m


def check(pcm, **kw):
    m = dev_meter(pcm, **kw)
    got, ref = meter_fields(m), ref_meter(pcm)
    assert got == ref
    return m


def sizes(span):
    return {"1": 1, "12": 12, "S-1": span - 1, "S": span, "S+1": span + 1, "3S+5": 3 * span + 5}


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("size", ["1", "12", "S-1", "S", "S+1", "3S+5"])
def test_random_at_the_seams(span, size, ch):
    n = sizes(span)[size]
    rng = np.random.default_rng(n * 2 + ch)
    pcm = rng.integers(-32768, 32768, (n, ch) if ch == 2 else (n,)).astype(np.int16)
    m = check(pcm)
    assert math.isnan(m.loudness)  # not requested
    check(pcm, f32=True)  # the MM_OUT_F32 buffer gives the identical mm_meter


@pytest.mark.parametrize("sign", [-32768, 32767])
@pytest.mark.parametrize("chan", [0, 1])
def test_impulses(span, chan, sign):
    """A full-scale impulse on one channel: at the first frame, on both sides of a
    workgroup seam, and at the last frame, where the peak lies in the tail."""
    n = span + 40
    for at in (0, span - 1, span, n - 1):
        pcm = np.zeros((n, 2), np.int16)
        pcm[at, chan] = sign
        m = check(pcm)
        assert m.true_peak_q28[chan] == 7964 * abs(sign) and m.true_peak_frame[chan] == at + 5
        assert m.true_peak_q28[1 - chan] == 0 and m.true_peak_frame[1 - chan] == 0
        assert m.sample_peak[chan] == abs(sign) and m.clipped[chan] == 1 and m.overs[chan] == 0
    assert m.true_peak_frame[chan] >= n  # the last one: past the last input frame


def test_tie_takes_the_smaller_frame(span):
    """Equal peaks in different waves and in different workgroups."""
    for a, b in ((5, 700), (300, span + 7), (span - 3, 2 * span + 1)):
        pcm = np.zeros(2 * span + 50, np.int16)
        pcm[a] = pcm[b] = 20000
        m = check(pcm)
        assert m.true_peak_frame[0] == a + 5


def test_more_spans_than_workgroups(span):
    """A launch is capped at 4 workgroups per compute unit (1024 on an MI355X); beyond
    that a workgroup walks several spans and carries its maxima across them.  Two equal
    peaks 1024 spans apart meet in one thread's registers: the smaller frame stays."""
    n = 1100 * span + 5
    pcm = np.random.default_rng(5).integers(-2000, 2001, n).astype(np.int16)
    a = span + 3
    for at in (a, a + 1024 * span):
        pcm[at - 12:at + 13] = 0
        pcm[at] = 32767
    m = check(pcm)
    assert m.true_peak_q28[0] == 7964 * 32767 and m.true_peak_frame[0] == a + 5 and m.clipped[0] == 2
    check(pcm, f32=True)


def test_silence(span):
    m = check(np.zeros((span + 3, 2), np.int16))
    assert list(m.true_peak_q28) == [0, 0] and list(m.true_peak_frame) == [0, 0] and list(m.sample_peak) == [0, 0]
    m = dev_meter(np.zeros((0, 2), np.int16))
    assert m.frames == 0 and list(m.true_peak_q28) == [0, 0]


@pytest.mark.parametrize("ch", [1, 2])
def test_worst_case_across_a_seam(span, ch):
    """The largest value an int16 sequence can reach (no int32 overflow), with the
    twelve frames that make it on both sides of a workgroup seam."""
    for at in (span + 5, span, span + 11, 2 * span - 1):
        s = worst_case(2 * span + 64, at)
        pcm = s if ch == 1 else np.stack([np.zeros_like(s), s], axis=1)
        m = check(pcm)
        assert m.true_peak_q28[ch - 1] == 542994228 and m.true_peak_frame[ch - 1] == at and m.overs[ch - 1] >= 1
    check(pcm, f32=True)


def float_true_peak(x):
    """The f64 definition: y = sum_k H[p][k] x[m-k], accumulated for k = 0..11 in order."""
    H = TAPS / 8192.0
    v = np.asarray(x, np.float64).reshape(len(x), -1)
    out = []
    for s in v.T:
        z = np.concatenate([np.zeros(11), s, np.zeros(11)])
        y = H[:, 0, None] * z[None, 11:11 + len(s) + 11]
        for k in range(1, 12):
            y = y + H[:, k, None] * z[None, 11 - k:11 - k + len(s) + 11]
        out.append(np.abs(y).max())
    return np.array(out)


def test_true_peak_operator_on_grid(span):
    from mastering_amd import ops
    pcm = np.random.default_rng(3).integers(-32768, 32768, (span + 77, 2)).astype(np.int16)
    want = np.array(ref_meter(pcm)["true_peak_q28"]) / 2.0 ** 28
    assert np.array_equal(ops.true_peak(pcm.astype(np.float32) / np.float32(32768)), want)
    assert np.array_equal(ops.true_peak(pcm[:, 0] / 32768.0), want[:1])
    imp = np.zeros(100, np.float32)
    imp[99] = -1.0
    assert ops.true_peak(imp)[0] == 7964 / 8192  # in the tail


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_true_peak_operator_off_grid(dtype):
    """Within twice the 12-term dot-product rounding bound of the f64 definition
    (the two sides may round differently): 24 * 2^-53 * sum|H[1]| * max|x|."""
    from mastering_amd import ops
    rng = np.random.default_rng(11)
    for shape in ((1,), (13,), (3001, 2)):
        x = (0.5 * rng.standard_normal(shape)).astype(dtype)
        got, want = ops.true_peak(x), float_true_peak(x)
        tol = 24 * 2.0 ** -53 * 2.0228271484375 * float(np.max(np.abs(x)))
        print(f"true_peak {np.dtype(dtype).name} {shape}: max |got - want| = {np.max(np.abs(got - want)):.3e}, "
              f"bound {tol:.3e}")
        assert got.shape == want.shape and np.all(np.abs(got - want) <= tol)


# ------------------------------------------------------------------ the chain
@pytest.fixture(scope="module")
def smoke_runs():
    """The smoke input mastered without and with the report (shared, read-only)."""
    from mastering_amd import master_pcm, native
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcm = pink_noise_pcm16(3 * rate, rate, 2, track=0)
    ctx = native.context(0)
    ctx.timing(True)
    plain, info0 = master_pcm(pcm, rate, SMOKE)
    stats0 = ctx.kernel_stats()
    ctx.timing(False)
    ctx.timing(True)
    out, info = master_pcm(pcm, rate, dict(SMOKE, report=True))
    stats = ctx.kernel_stats()
    ctx.timing(False)
    return {"rate": rate, "plain": plain, "info0": info0, "stats0": stats0, "out": out, "info": info, "stats": stats}


def check_report(rep, out):
    ref = ref_meter(out)
    for f in ("sample_peak", "true_peak_q28", "true_peak_frame", "clipped", "overs"):
        assert rep[f] == ref[f], f
    assert rep["true_peak_dbtp"] == [20 * math.log10(v / 2 ** 28) if v else -math.inf for v in ref["true_peak_q28"]]
    assert rep["sample_peak_dbfs"] == [20 * math.log10(v / 32768) if v else -math.inf for v in ref["sample_peak"]]
    assert rep["max_true_peak_dbtp"] == max(rep["true_peak_dbtp"])
    assert rep["frames"] == len(out)


def test_chain_report_leaves_the_audio_alone(smoke_runs):
    r = smoke_runs
    assert np.array_equal(r["out"], r["plain"])
    assert "report" not in r["info0"]
    assert set(r["info"]) - {"report"} == set(r["info0"])
    assert r["info"]["loudness"] == r["info0"]["loudness"] and r["info"]["gain_linear"] == r["info0"]["gain_linear"]
    assert not [k for k in r["stats0"] if "meter" in k], r["stats0"].keys()
    assert "meter_i16" in r["stats"]


def test_chain_report_peaks(smoke_runs):
    check_report(smoke_runs["info"]["report"], smoke_runs["out"])


def test_chain_report_loudness(smoke_runs, oracle):
    r = smoke_runs
    rep = r["info"]["report"]
    mono = (r["out"].astype(np.float32) / np.float32(32768)).mean(axis=1)
    L = oracle.integrated_loudness(mono, r["rate"])
    print(f"output loudness {rep['output_loudness']:.6f} LUFS, oracle {L:.6f}, target {SMOKE['lufs']}")
    assert abs(rep["output_loudness"] - L) <= 4e-4
    assert rep["loudness_error"] == rep["output_loudness"] - SMOKE["lufs"]


def test_meter_pcm_matches_the_chain(smoke_runs):
    from mastering_amd import engine
    r = smoke_runs
    rep = engine.meter_pcm(r["out"], r["rate"])
    want = {k: v for k, v in r["info"]["report"].items() if k not in ("loudness_error", "output_loudness")}
    assert {k: rep[k] for k in want} == want
    assert abs(rep["output_loudness"] - r["info"]["report"]["output_loudness"]) <= 4e-4  # other K-weighting tile
    assert engine.meter_pcm(r["out"], r["rate"], loudness=False)["output_loudness"] is None
    assert engine.meter_pcm(r["out"].astype(np.float32) / np.float32(32768), r["rate"], loudness=False) == \
        engine.meter_pcm(r["out"], r["rate"], loudness=False)


def test_last_meters_needs_a_metering_call(smoke_runs):
    from mastering_amd import engine, master_pcm, native
    ctx = native.context(0)
    master_pcm(smoke_runs["out"][:22050], 44100, {"multiband": False, "report": True})
    assert len(engine.meters(ctx)) == 1
    master_pcm(smoke_runs["out"][:22050], 44100, {"multiband": False})
    with pytest.raises(RuntimeError):
        engine.meters(ctx)


def test_process_report_on_the_written_file(tmp_path):
    from conftest import GOLDEN
    from mastering_amd import process, wavio
    d = np.load(os.path.join(GOLDEN, "mono_hot_2s.npz"))
    settings = json.loads(str(d["settings"]))
    src, dst, dst0 = str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(tmp_path / "out0.wav")
    wavio.write_wav(src, d["pcm"], int(d["rate"]))
    info = process(src, dst, dict(settings, report=True))
    info0 = process(src, dst0, settings)
    got, _ = wavio.read_wav(dst)
    assert np.array_equal(got, wavio.read_wav(dst0)[0]) and "report" not in info0
    check_report(info["report"], got)
    assert info["report"]["channels"] == 1 and len(info["report"]["true_peak_q28"]) == 1


def test_batch_reports_each_track():
    import torch
    from mastering_amd import Job, engine, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcms = [pink_noise_pcm16(30000, rate, 2, track=1), pink_noise_pcm16(41000, rate, 2, track=2, level_dbfs=-6.0)]
    params = [{"multiband": True, "lufs": -14.0}, {"saturation": 50, "lufs": -9.0}]
    jobs = [Job(len(p), rate, 2, q, report=True) for p, q in zip(pcms, params)]
    for j in jobs:
        j.job.in_kind = native.MM_IN_I16
    xs = [torch.from_numpy(p).cuda() for p in pcms]
    outs = [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]
    torch.cuda.current_stream().synchronize()
    ctx = native.context(0)
    master_batch(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs])
    ms = engine.meters(ctx)
    assert len(ms) == 2
    for m, o, q in zip(ms, outs, params):
        out = o.cpu().numpy()
        assert meter_fields(m) == ref_meter(out)
        check_report(engine.report_dict(m, q["lufs"]), out)
        assert not math.isnan(m.loudness)
    assert meter_fields(ms[0]) != meter_fields(ms[1])


def test_short_signal_has_peaks_but_no_loudness():
    from mastering_amd import master_pcm
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(9000, 44100, 2, track=3)  # 0.2 s: shorter than one loudness block
    out, info = master_pcm(pcm, 44100, {"saturation": 20, "width": 1.2, "report": True})
    check_report(info["report"], out)
    assert info["report"]["output_loudness"] is None and "loudness_error" not in info["report"]


def test_worker_writes_the_report(tmp_path):
    from conftest import GOLDEN
    from mastering_amd import wavio
    from mastering_amd.worker import process_audio_from_gcs
    d = np.load(os.path.join(GOLDEN, "mono_hot_2s.npz"))
    settings = json.loads(str(d["settings"]))
    (tmp_path / "bkt" / "up").mkdir(parents=True)
    wavio.write_wav(str(tmp_path / "bkt" / "up" / "t.wav"), d["pcm"], int(d["rate"]))
    done = tmp_path / "bkt" / "processed" / "mastered_t.wav"
    process_audio_from_gcs("gs://bkt/up/t.wav", settings, root=str(tmp_path))
    assert done.exists() and not os.path.exists(str(done) + ".report.json")
    process_audio_from_gcs("gs://bkt/up/t.wav", dict(settings, report=True), root=str(tmp_path))
    rep = json.loads(open(str(done) + ".report.json").read())
    ref = ref_meter(wavio.read_wav(str(done))[0])
    assert rep["true_peak_q28"] == ref["true_peak_q28"] and rep["true_peak_frame"] == ref["true_peak_frame"]
    assert os.path.exists(str(done) + ".complete")
