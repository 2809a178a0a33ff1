"""The EBU R 128 report on the GPU: the K-weighting pass's hop energies (mm_op_r128_hops)
against the sequential host restatement (mm_r128_host) at the sizes where the pass can go
wrong (tiles that straddle hops, partial last tile and hop, one lane, one workgroup, more
than one look-back window), the figures of mm_r128_pcm, and the report through the chain's
entry points."""
import ctypes
import math

import numpy as np
import pytest

from test_r128 import (EBU_3342, FIGURES, design_rate, gate_margin, host_r128, ref_hops, ref_r128, same, sine,
                       stepped_noise)

pytestmark = pytest.mark.gpu

# Largest relative deviation of a hop energy of the pass from mm_r128_host's over the cases
# of test_hop_energies below, measured on an MI355X: 3.983e-12, on the long-carry case (the
# others: 1.0e-14 to 6.2e-13).  It is rounding-order noise of the tile scan against the
# sequential filter; anything above 1e-7 (4.3e-7 LU) would be a defect, not a tolerance.
# The tests allow 8 x the measured value, to cover other signals: 3.19e-11 (1.4e-10 LU).
MEASURED = 3.983e-12
TOL = 8 * MEASURED
assert MEASURED < 1e-7

P_FULL = {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0,
          "saturation": 30, "width": 1.3, "multiband": True, "lufs": -14.0}


@pytest.fixture(scope="module")
def span():
    from mastering_amd import native
    return native.load().mm_r128_span()


def gpu_hops(pcm, rate, f32=False):
    """The pass's hop energies for int16 `pcm` (or for pcm / 32768 as an MM_OUT_F32 buffer)."""
    from mastering_amd import engine, native
    x = np.ascontiguousarray(pcm, np.int16)
    host = x.astype(np.float32) / np.float32(32768) if f32 else x
    H = 10 * x.shape[0] // rate
    e = np.full(H + 1, -1.0)
    ctx = native.context(0)
    n = ctx.check(ctx.lib.mm_op_r128_hops(ctx.ptr, host.ctypes.data_as(ctypes.c_void_p),
                                          native.MM_OUT_F32 if f32 else native.MM_OUT_I16, x.shape[0],
                                          1 if x.ndim == 1 else x.shape[1], rate, engine.kweight_sos(design_rate(rate)),
                                          e.ctypes.data_as(native.c_double_p), H), "mm_op_r128_hops")
    assert n == H and e[H] == -1.0
    return e[:H]


def gpu_r128(pcm, rate):
    from mastering_amd import engine, native
    x = np.ascontiguousarray(pcm, np.int16)
    ctx = native.context(0)
    m = native.MMR128()
    ctx.check(ctx.lib.mm_r128_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), native.MM_OUT_I16, x.shape[0],
                                  1 if x.ndim == 1 else x.shape[1], rate, engine.kweight_sos(design_rate(rate)),
                                  ctypes.byref(m)), "mm_r128_pcm")
    return m


def long_carry(n, rate):
    """0.4 FS DC + a 30 Hz sine + noise, stereo: the high-pass state is far from zero at
    every workgroup boundary, so a wrong carry shows."""
    t = np.arange(n) / rate
    rng = np.random.default_rng(3)
    cols = [32768.0 * (0.4 + 0.3 * np.sin(2 * np.pi * 30.0 * t + ph)) + rng.normal(0.0, 800.0, n) for ph in (0.0, 1.0)]
    return np.ascontiguousarray(np.stack([np.clip(np.round(c), -32768, 32767).astype(np.int16) for c in cols], axis=1))


def hop_cases(span):
    tile = span // 256
    return {"straddle-stereo": (44100, 321987, 2), "straddle-mono": (44100, 321987, 1), "one-frame": (44100, 1, 2),
            "tile-1": (2000, tile - 1, 2), "one-span": (44100, span, 2), "floor-rate": (2000, 6001, 2),
            "192k": (192000, 250003, 2), "long-carry": (44100, 65 * span + 17, 2)}


def case_signal(span, name):
    rate, n, ch = hop_cases(span)[name]
    return (long_carry(n, rate) if name == "long-carry" else stepped_noise(n, rate, ch)), rate


def deviation(e, ref):
    assert len(e) == len(ref)
    return float(np.max(np.abs(e - ref) / ref)) if len(e) else 0.0


@pytest.mark.parametrize("name", ["straddle-stereo", "straddle-mono", "one-frame", "tile-1", "one-span", "floor-rate",
                                  "192k", "long-carry"])
def test_hop_energies(span, name):
    pcm, rate = case_signal(span, name)
    ref, _ = host_r128(pcm, rate)
    e = gpu_hops(pcm, rate)
    dev = deviation(e, ref)
    print(f"r128 hop energies {name}: {len(e)} hops, largest relative deviation {dev:.3e}")
    assert np.all(np.isfinite(e)) and np.all(ref > 0)
    assert dev <= TOL
    assert np.array_equal(gpu_hops(pcm, rate), e)  # two runs are bit-identical (no atomics)
    if name != "long-carry":  # the decoded doubles of the f32 buffer are equal
        assert np.array_equal(gpu_hops(pcm, rate, f32=True), e)


@pytest.mark.parametrize("name", ["3342-1", "noise"])
def test_figures(name):
    rate = 44100
    pcm = sine(EBU_3342["3342-1"][0], rate) if name == "3342-1" else stepped_noise(321987, rate, 2)
    # the inputs keep every block level clear of the gates, so the hop energies' rounding
    # noise cannot move a block across one (stated from the numpy restatement)
    r = ref_r128(ref_hops(pcm, rate), rate)
    assert gate_margin(r) >= 1e-3
    _, h = host_r128(pcm, rate)
    m = gpu_r128(pcm, rate)
    assert (m.frames, m.channels, m.rate, m.hops) == (len(pcm), 2, rate, h.hops)
    assert (m.momentary_blocks, m.short_term_blocks, m.lra_blocks) == (h.momentary_blocks, h.short_term_blocks,
                                                                       h.lra_blocks)
    for f in FIGURES:
        assert math.isfinite(getattr(h, f)) and abs(getattr(m, f) - getattr(h, f)) <= 1e-6, f
    if name == "3342-1":
        assert abs(m.lra - 10.0) <= 1.0


@pytest.fixture(scope="module")
def chain_runs():
    from mastering_amd import master_pcm
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcm = pink_noise_pcm16(2 * rate, rate, 2, track=0)
    plain = master_pcm(pcm, rate, dict(P_FULL, report=True))
    with_r128 = master_pcm(pcm, rate, dict(P_FULL, report=True, r128=True))
    return pcm, rate, plain, with_r128


def test_chain_report_leaves_everything_else_alone(chain_runs):
    from mastering_amd import r128_pcm
    _, rate, (out0, info0), (out1, info1) = chain_runs
    assert np.array_equal(out0, out1)
    assert "r128" not in info0 and {k: v for k, v in info1.items() if k != "r128"} == info0
    r = info1["r128"]
    assert r == r128_pcm(out1, rate)
    assert r["hops"] == 20 and r["short_term_max_lufs"] is None and r["lra_lu"] is None
    # the reference's channel-mean measure reads at least 10 log10 2 lower than a BS.1770
    # meter does (|L + R|^2 / 4 <= (L^2 + R^2) / 2: 3.01 LU for centred content, 6.02 for
    # uncorrelated channels)
    assert 2.9 < r["integrated_lufs"] - info1["report"]["output_loudness"] < 6.2


def test_chain_alone_and_on_f32_output(chain_runs):
    from mastering_amd import master_pcm, native
    pcm, rate, (out0, _), (_, info1) = chain_runs
    out, info = master_pcm(pcm, rate, dict(P_FULL, r128=True), out_kind=native.MM_OUT_F32)
    assert "report" not in info and info["r128"] == info1["r128"]
    assert np.array_equal(out, out0.astype(np.float32) / np.float32(32768))


def test_delivery_reports_the_delivered_samples(chain_runs):
    from mastering_amd import master_pcm, r128_pcm
    pcm, rate, _, _ = chain_runs
    params = dict(P_FULL, output_rate=48000, ceiling_dbtp=-1.0)
    out0, info0 = master_pcm(pcm, rate, params)
    out, info = master_pcm(pcm, rate, dict(params, r128=True))
    assert np.array_equal(out, out0) and {k: v for k, v in info.items() if k != "r128"} == info0
    assert info["rate"] == 48000 and info["r128"] == r128_pcm(out, 48000)
    assert info["r128"]["hops"] == 10 * len(out) // 48000


def test_process_reports_the_written_file(tmp_path):
    """The file path (mm_master_wav) on a mono golden input: the same report as r128_pcm
    of the written samples, and the same file as without the key."""
    import json
    import os
    from conftest import GOLDEN
    from mastering_amd import process, r128_pcm, wavio
    d = np.load(os.path.join(GOLDEN, "mono_hot_2s.npz"))
    settings = json.loads(str(d["settings"]))
    src, dst, dst0 = str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(tmp_path / "out0.wav")
    wavio.write_wav(src, d["pcm"], int(d["rate"]))
    info = process(src, dst, dict(settings, r128=True))
    info0 = process(src, dst0, settings)
    got, rate = wavio.read_wav(dst)
    assert np.array_equal(got, wavio.read_wav(dst0)[0]) and "r128" not in info0 and "report" not in info
    assert got.ndim == 1 and info["r128"] == r128_pcm(got, rate) and info["r128"]["integrated_lufs"] is not None


def test_short_inputs():
    from mastering_amd import master_pcm
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    _, info = master_pcm(pink_noise_pcm16(rate // 5, rate, 2, track=3), rate, {"saturation": 20, "r128": True})
    r = info["r128"]
    assert r["hops"] == 2 and r["lra_blocks"] == 0 and all(v is None for k, v in r.items() if k not in ("hops", "lra_blocks"))
    _, info = master_pcm(pink_noise_pcm16(rate, rate, 2, track=3), rate, {"saturation": 20, "r128": True})
    r = info["r128"]
    assert r["hops"] == 10 and r["integrated_lufs"] is not None and r["momentary_max_lufs"] is not None
    assert r["short_term_max_lufs"] is None and r["lra_lu"] is None and r["lra_low_lufs"] is None


def test_batch_reports_the_jobs_that_asked():
    import torch
    from mastering_amd import Job, engine, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcms = [pink_noise_pcm16(30000, rate, 2, track=1), pink_noise_pcm16(41000, rate, 2, track=2, level_dbfs=-6.0)]
    jobs = [Job(len(pcms[0]), rate, 2, {"multiband": True, "lufs": -14.0}, r128=True),
            Job(len(pcms[1]), rate, 2, {"saturation": 50, "lufs": -9.0})]
    for j in jobs:
        j.job.in_kind = native.MM_IN_I16
    xs = [torch.from_numpy(p).cuda() for p in pcms]
    outs = [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]
    torch.cuda.current_stream().synchronize()
    ctx = native.context(0)
    master_batch(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs])
    rs = engine.r128s(ctx)
    assert len(rs) == 2
    assert engine.r128_dict(rs[0]) == engine.r128_pcm(outs[0].cpu().numpy(), rate) and rs[0].frames == jobs[0].frames_proc
    assert rs[1].frames == 0 and rs[1].hops == 0 and all(math.isnan(getattr(rs[1], f)) for f in FIGURES)
    with pytest.raises(RuntimeError, match="did not meter"):
        engine.meters(ctx)
    # a master call that asks for none leaves none
    master_batch(ctx, jobs[1:], [xs[1].data_ptr()], [outs[1].data_ptr()])
    with pytest.raises(RuntimeError, match="no R 128 report"):
        engine.r128s(ctx)


def test_refusals_leave_the_context_usable():
    from mastering_amd import engine, native
    ctx = native.context(0)
    x = np.zeros((1000, 2), np.int16)
    p, sos, m = x.ctypes.data_as(ctypes.c_void_p), engine.kweight_sos(48000), native.MMR128()
    I16 = native.MM_OUT_I16
    for args, words in (((p, I16, 1000, 3, 48000, sos, ctypes.byref(m)), "channels must be 1 or 2"),
                        ((p, 7, 1000, 2, 48000, sos, ctypes.byref(m)), "kind 7"),
                        ((p, I16, 1000, 2, 1999, sos, ctypes.byref(m)), "rate below 2000"),
                        ((p, I16, 2 ** 31, 2, 48000, sos, ctypes.byref(m)), "frames out of range"),
                        ((None, I16, 1000, 2, 48000, sos, ctypes.byref(m)), "bad arguments"),
                        ((p, I16, 1000, 2, 48000, None, ctypes.byref(m)), "bad arguments"),
                        ((p, I16, 1000, 2, 48000, sos, None), "bad arguments")):
        with pytest.raises(ValueError, match=words):
            ctx.check(ctx.lib.mm_r128_pcm(ctx.ptr, *args), "mm_r128_pcm")
    ctx.check(ctx.lib.mm_r128_pcm(ctx.ptr, None, I16, 0, 2, 48000, sos, ctypes.byref(m)), "mm_r128_pcm")
    assert m.frames == 0 and m.channels == 2 and m.hops == 0 and all(math.isnan(getattr(m, f)) for f in FIGURES)
    pcm = sine([(-23.0, 1)], 48000)
    assert same(gpu_r128(pcm, 48000).integrated, host_r128(pcm, 48000)[1].integrated, 1e-6)
