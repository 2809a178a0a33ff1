"""The true-peak ceiling on the GPU: the three kernels against the numpy definition
(tests/test_ceiling.py: ref_ceiling), samples and statistics, at the sizes where they can
go wrong (the workgroup span of mm_ceiling_span and its seams, windows that reach over
several spans, the 11-frame tail, ties), on the int16 and the f32 buffer, through the
three branches, and through every chain entry point.  All comparisons are equalities
on integers.  Both new kernels launch one workgroup per span, so there is no case of
more spans than workgroups (the meter pass has its own in tests/test_gpu_meter.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_ceiling import ONE, ceiling_stats, q28, ref_ceiling
from test_gpu_meter import SMOKE, check_report
from test_meter import ref_meter

pytestmark = pytest.mark.gpu

RATE = 44100


@pytest.fixture(scope="module")
def span():
    from mastering_amd import native
    return native.load().mm_ceiling_span()


def dev_ceiling(pcm, C, W, f32=False):
    """mm_ceiling_device on a device copy of int16 `pcm` (or of pcm / 32768 as f32):
    (the buffer afterwards as int16, its raw host copy, the statistics)."""
    import torch
    from mastering_amd import native
    x = np.ascontiguousarray(pcm, np.int16)
    host = x.astype(np.float32) / np.float32(32768) if f32 else x
    d = torch.from_numpy(host).cuda()
    torch.cuda.current_stream().synchronize()  # the copy is on torch's stream, the library uses its own
    ctx = native.context(0)
    m = native.MMCeiling()
    ctx.check(ctx.lib.mm_ceiling_device(ctx.ptr, ctypes.c_void_p(d.data_ptr()),
                                        native.MM_OUT_F32 if f32 else native.MM_OUT_I16, x.shape[0],
                                        1 if x.ndim == 1 else x.shape[1], C, W, ctypes.byref(m)),
              "mm_ceiling_device")
    raw = d.cpu().numpy()
    if f32:
        k = raw * np.float32(32768)
        assert np.array_equal(k, np.rint(k)) and np.abs(k).max(initial=0) <= 32768  # still on the int16 grid
        return k.astype(np.int16), raw, ceiling_stats(m)
    return raw, raw, ceiling_stats(m)


def check(pcm, C, W, both=True):
    want, st = ref_ceiling(pcm, C, W)
    for f32 in ((False, True) if both else (False,)):
        got, _, gst = dev_ceiling(pcm, C, W, f32)
        assert gst == st, ("f32" if f32 else "i16", gst, st)
        assert np.array_equal(got, want), "f32" if f32 else "i16"
    return want, st


def sizes(span):
    return {"1": 1, "12": 12, "S-1": span - 1, "S": span, "S+1": span + 1, "3S+5": 3 * span + 5}


@pytest.mark.parametrize("W", [1, 220, 1024])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("size", ["1", "12", "S-1", "S", "S+1", "3S+5"])
def test_seams(span, size, ch, W):
    """A -30 dBFS bed with full-scale peaks at the first frame, inside the first ramp, on
    both sides of a seam, one window past it and at the last frame (its peak lies in the
    tail); in stereo on one channel only, and the other must come down with it."""
    n = sizes(span)[size]
    rng = np.random.default_rng(100 * n + 10 * ch + W)
    pcm = rng.integers(-1036, 1037, (n, ch)).astype(np.int16)
    for at in (0, W - 1, span - 1, span, span + W, n - 1):
        if at < n:
            pcm[at, 0] = 32767 if at % 2 else -32768
    C = q28(-1.0)
    want, st = check(pcm if ch == 2 else pcm[:, 0], C, W)
    assert st["tp_in_q28"] > C >= st["tp_out_q28"] and st["limited_frames"] > 0
    if ch == 2 and n > 1:
        assert np.any(want[:, 1] != pcm[:, 1])


@pytest.mark.parametrize("W", [16, 220])
def test_ties_across_a_seam(span, W):
    """A plateau of equal over-ceiling peaks on both sides of a seam: equal needs, one hold."""
    pcm = np.zeros(2 * span + 7, np.int16)
    pcm[span - 48:span + 49:16] = 32000
    want, st = check(pcm, q28(-3.0), W)
    assert st["limited_frames"] >= 96 + 12 + 4 * W and len(set(want[span - 48:span + 49:16].tolist())) == 1


def test_arguments(span):
    from mastering_amd import engine
    pcm = np.zeros((64, 2), np.int16)
    for C, W in ((2 ** 24 - 1, 16), (2 ** 28 + 1, 16), (2 ** 27, 0), (2 ** 27, 1025)):
        with pytest.raises(ValueError):
            dev_ceiling(pcm, C, W)
    got, _, st = dev_ceiling(np.zeros((0, 2), np.int16), 2 ** 27, 16)
    assert st["frames"] == 0 and st["tp_out_q28"] == 0 and got.shape == (0, 2)
    out, d = engine.ceiling_pcm(np.full(500, 30000, np.int16), RATE, -6.0)
    want, wst = ref_ceiling(np.full(500, 30000, np.int16), q28(-6.0), 220)
    assert np.array_equal(out, want) and {k: d[k] for k in wst} == wst and d["window"] == 220


# ------------------------------------------------------------------ the three branches
@pytest.fixture(scope="module")
def branches():
    from mastering_amd.synth import pink_noise_pcm16
    return {"under": pink_noise_pcm16(20000, RATE, 2, track=3, level_dbfs=-18.0),
            "limited": pink_noise_pcm16(20000, RATE, 2, track=2, level_dbfs=-12.0),
            "trimmed": pink_noise_pcm16(20000, RATE, 2, track=1, level_dbfs=-6.0)}


def timed(fn):
    from mastering_amd import native
    ctx = native.context(0)
    ctx.timing(True)
    try:
        res = fn()
        return res, ctx.kernel_stats()
    finally:
        ctx.timing(False)


def test_branch_under_the_ceiling_writes_nothing(branches):
    pcm = branches["under"]
    for f32 in (False, True):
        before = pcm.astype(np.float32) / np.float32(32768) if f32 else pcm
        (got, raw, st), stats = timed(lambda: dev_ceiling(pcm, q28(-1.0), 220, f32))
        assert raw.tobytes() == before.tobytes()
        assert st == ref_ceiling(pcm, q28(-1.0), 220)[1]
        assert st["limited_frames"] == 0 and st["trim_q16"] == ONE and st["tp_out_q28"] == st["tp_in_q28"]
        # one call: need, apply and the peak pass (which skips the untouched track) once each
        assert stats["ceil_tracks_need"][1] == stats["ceil_tracks_apply"][1] == stats["ceil_tracks_peak"][1] == 1
        assert "ceil_tracks_trim" not in stats and "meter_i16" not in stats


@pytest.mark.parametrize("W", [1, 16, 220, 1024])
def test_branch_limited_without_a_trim(branches, W):
    (want, st), stats = timed(lambda: check(branches["limited"], q28(-1.0), W))
    assert st["trim_q16"] == ONE and st["limited_frames"] > 0 and "ceil_tracks_trim" not in stats
    # two calls (int16 and f32), each one need, one apply and one peak pass
    assert stats["ceil_tracks_need"][1] == stats["ceil_tracks_apply"][1] == stats["ceil_tracks_peak"][1] == 2
    assert "meter_i16" not in stats


@pytest.mark.parametrize("W", [1, 16, 220])
def test_branch_trimmed(branches, W):
    (want, st), stats = timed(lambda: check(branches["trimmed"], q28(-1.0), W))
    assert (st["trim_q16"] != ONE) == (W != 220) == ("ceil_tracks_trim" in stats)
    # two calls (int16 and f32): the peak pass twice a call only with a trim
    assert stats["ceil_tracks_need"][1] == stats["ceil_tracks_apply"][1] == 2 and "meter_i16" not in stats
    assert stats["ceil_tracks_peak"][1] == (4 if W != 220 else 2) and stats.get("ceil_tracks_trim", (0, 0))[1] == (2 if W != 220 else 0)
    assert st["tp_out_q28"] <= q28(-1.0) < st["tp_in_q28"]


# ------------------------------------------------------------------ the chain
@pytest.fixture(scope="module")
def smoke_runs():
    """The smoke input mastered plainly, with a ceiling, and with a ceiling and the report."""
    from mastering_amd import master_pcm, native
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(3 * RATE, RATE, 2, track=0)
    ctx = native.context(0)
    runs = {"pcm": pcm}
    for name, extra in (("plain", {}), ("ceil", {"ceiling_dbtp": -1.0}), ("deep", {"ceiling_dbtp": -9.0}),
                        ("both", {"ceiling_dbtp": -1.0, "report": True})):
        ctx.timing(True)
        out, info = master_pcm(pcm, RATE, dict(SMOKE, **extra))
        runs[name] = (out, info, ctx.kernel_stats())
        ctx.timing(False)
    return runs


def test_chain_without_the_key_queues_nothing_new(smoke_runs, oracle):
    out, info, stats = smoke_runs["plain"]
    assert "ceiling" not in info and not [k for k in stats if "ceil" in k or "meter" in k], stats.keys()
    ref = oracle.master(smoke_runs["pcm"], RATE, SMOKE)  # the unceilinged chain: smoke()'s own check
    assert np.sqrt(np.mean(((out.astype(np.float64) - ref) / 32768.0) ** 2)) <= 1e-5


def test_last_ceilings_needs_a_ceiling(smoke_runs):
    from mastering_amd import engine, master_pcm, native
    ctx = native.context(0)
    pcm = smoke_runs["pcm"][:22050]
    master_pcm(pcm, RATE, {"multiband": False, "ceiling_dbtp": -12.0})
    assert len(engine.ceilings(ctx)) == 1
    master_pcm(pcm, RATE, {"multiband": False})
    with pytest.raises(RuntimeError):
        engine.ceilings(ctx)


@pytest.mark.parametrize("name,db", [("ceil", -1.0), ("deep", -9.0), ("both", -1.0)])
def test_chain_ceiling_is_the_reference_on_the_plain_output(smoke_runs, name, db):
    from mastering_amd import design
    plain, info0, _ = smoke_runs["plain"]
    out, info, stats = smoke_runs[name]
    want, st = ref_ceiling(plain, q28(db), design.ceiling_window(RATE))
    print(f"{name}: tp_in {info['ceiling']['tp_in_dbtp']:+.3f} dBTP -> {info['ceiling']['tp_out_dbtp']:+.3f}, "
          f"limited {st['limited_frames']} frames, trim {st['trim_q16']}")
    assert np.array_equal(out, want)
    assert {k: info["ceiling"][k] for k in st} == st and info["ceiling"]["window"] == 220
    assert info["ceiling"]["ceiling_dbtp"] == 20 * np.log10(q28(db) / 2 ** 28)
    assert info["ceiling"]["trimmed"] == (st["trim_q16"] != ONE)
    assert info["loudness"] == info0["loudness"] and info["gain_linear"] == info0["gain_linear"]
    assert stats["ceil_tracks_need"][1] == stats["ceil_tracks_apply"][1] == 1
    assert ("meter_i16" in stats) == (name == "both")  # the meter's kernel runs for the report alone
    assert set(info) - {"ceiling", "report"} == set(info0)
    if name == "deep":  # whatever the smoke output's own peak, this one is limited
        assert st["limited_frames"] > 0 and st["tp_in_q28"] > q28(db) >= st["tp_out_q28"]


def test_chain_report_measures_the_delivered_samples(smoke_runs):
    out, info, _ = smoke_runs["both"]
    check_report(info["report"], out)
    assert max(info["report"]["true_peak_q28"]) == info["ceiling"]["tp_out_q28"] <= q28(-1.0)
    assert np.array_equal(out, smoke_runs["ceil"][0])


def test_process_ceiling_on_the_written_file(tmp_path):
    from conftest import GOLDEN
    from mastering_amd import design, process, wavio
    d = np.load(os.path.join(GOLDEN, "mono_hot_2s.npz"))
    settings = json.loads(str(d["settings"]))
    rate = int(d["rate"])
    src, dst, dst0 = str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(tmp_path / "out0.wav")
    wavio.write_wav(src, d["pcm"], rate)
    info0 = process(src, dst0, settings)
    info = process(src, dst, dict(settings, ceiling_dbtp=-2.0, report=True))
    plain, got = wavio.read_wav(dst0)[0], wavio.read_wav(dst)[0]
    want, st = ref_ceiling(plain, q28(-2.0), design.ceiling_window(rate))
    assert "ceiling" not in info0 and np.array_equal(got, want)
    assert {k: info["ceiling"][k] for k in st} == st and info["ceiling"]["channels"] == 1
    assert st["tp_in_q28"] > q28(-2.0) >= st["tp_out_q28"]  # a hot input: the ceiling had work to do
    check_report(info["report"], got)


def test_batch_ceilings_in_job_order():
    import torch
    from mastering_amd import Job, design, engine, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16
    pcms = [pink_noise_pcm16(30000, RATE, 2, track=1), pink_noise_pcm16(41000, RATE, 2, track=2, level_dbfs=-6.0),
            pink_noise_pcm16(30000, RATE, 2, track=1)]
    params = {"multiband": True, "lufs": -9.0}
    dbs = [-3.0, -6.0, None]

    def run(ceilings):
        jobs = [Job(len(p), RATE, 2, params, ceiling_dbtp=db) for p, db in zip(pcms, ceilings)]
        for j in jobs:
            j.job.in_kind = native.MM_IN_I16
        xs = [torch.from_numpy(p).cuda() for p in pcms]
        outs = [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]
        torch.cuda.current_stream().synchronize()
        ctx = native.context(0)
        master_batch(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs])
        return [o.cpu().numpy() for o in outs], ctx

    plain, ctx = run([None] * 3)
    with pytest.raises(RuntimeError):
        engine.ceilings(ctx)
    outs, ctx = run(dbs)
    cs = engine.ceilings(ctx)
    assert len(cs) == 3 and cs[2].frames == 0 and np.array_equal(outs[2], plain[2])
    for i in (0, 1):
        want, st = ref_ceiling(plain[i], q28(dbs[i]), design.ceiling_window(RATE))
        assert np.array_equal(outs[i], want) and ceiling_stats(cs[i]) == st
        assert st["tp_in_q28"] > st["ceiling_q28"] >= st["tp_out_q28"]
    assert cs[0].ceiling_q28 != cs[1].ceiling_q28
