"""The delivery QC report on the GPU (csrc/qc.hip): the span kernel, its
records and the fold against the sequential host restatement mm_qc_host, every field of mm_qc
and the whole hop table, at the places where the run operator and the hop pieces can go wrong
(runs that end on, start on, cross and cover spans; silence at either end and across seams;
11 hop pieces in a span, a hop of nine spans), for both buffer kinds, mono and stereo; the
batch entry on tracks that lie side by side in one allocation; and the report through the
master call and deliver_batch."""
import ctypes

import numpy as np
import pytest

from test_qc import host_qc, qc_fields, same_qc

pytestmark = pytest.mark.gpu

RATE = 44100
P = {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0,
     "saturation": 30, "width": 1.3, "multiband": True, "lufs": -9.0}
INFO_KEYS = {"loudness", "gain_db", "gain_linear", "frames", "comp_iters", "comp_walked", "comp_jumped", "comp_active",
             "chunks", "tile"}


@pytest.fixture(scope="module")
def S():
    from mastering_amd import native
    s = native.load().mm_qc_span()
    assert s == 2048
    return s


def as_kind(x, f32):
    return x.astype(np.float32) / np.float32(32768) if f32 else x


def gpu_qc(pcm, rate, q=1, r=3, f32=False):
    """(fields, hop table) of mm_qc_pcm on int16 `pcm` (or on pcm / 32768 as an MM_OUT_F32 buffer)."""
    from mastering_amd import native
    x = np.ascontiguousarray(pcm, np.int16)
    host = np.ascontiguousarray(as_kind(x, f32))
    table = np.full((10 * x.shape[0] // rate + 1, 3), -7, np.int64)
    ctx = native.context(0)
    m = native.MMQc()
    ctx.check(ctx.lib.mm_qc_pcm(ctx.ptr, host.ctypes.data_as(ctypes.c_void_p), native.MM_OUT_F32 if f32 else native.MM_OUT_I16,
                                x.shape[0], 1 if x.ndim == 1 else x.shape[1], rate, q, r, ctypes.byref(m),
                                table.ctypes.data_as(native.c_int64_p)), "mm_qc_pcm")
    assert (table[-1] == -7).all()  # nothing past H rows
    return qc_fields(m), table[:-1]


def check(pcm, rate=RATE, q=1, r=3, kinds=(False, True)):
    """The device equals the host restatement, field by field and hop by hop; returns the fields."""
    want, want_table = host_qc(pcm, rate, q, r)
    for f32 in kinds:
        got, table = gpu_qc(pcm, rate, q, r, f32)
        assert same_qc(got, want) == [], (f32, same_qc(got, want), got, want)
        assert np.array_equal(table, want_table), f32
    return want


def noise(n, ch=2, seed=1, amp=12000):
    x = np.random.default_rng(seed).integers(-amp, amp, (n, ch) if ch == 2 else (n,)).astype(np.int16)
    x[np.abs(x) <= 1] = 2  # (no frame of the bed is silent at q = 1)
    return x


@pytest.mark.parametrize("ch", [1, 2])
def test_lengths(S, ch):
    """One frame, a partial span, whole spans, a last span without a frame (the grid counts
    frames + 11) and several spans, on hard-clipped noise: runs of both rails everywhere."""
    rng = np.random.default_rng(2)
    for n in (1, S - 11, S - 10, S - 1, S, S + 1, 2 * S, 3 * S + 5):
        x = np.clip(rng.normal(0.0, 40000.0, (n, ch) if ch == 2 else (n,)), -32768, 32767).astype(np.int16)
        got = check(x, 2000 if n == S + 1 else RATE)
        assert got["frames"] == n and (n < 100 or got["clip_runs"][0] > 0)


def test_rail_runs_at_the_seams(S):
    n = 3 * S + 5
    for name, runs, want in (
            ("ends on a span's last frame", [(S - 5, S, 32767)], (1, 5, S - 5)),
            ("starts on a span's first frame", [(S, S + 4, -32768)], (1, 4, S)),
            ("crosses a seam", [(2 * S - 2, 2 * S + 3, 32767)], (1, 5, 2 * S - 2)),
            ("covers a span and touches both neighbours", [(S - 1, 2 * S + 1, -32767)], (1, S + 2, S - 1)),
            ("r - 1 and r across seams", [(S - 1, S + 1, 32767), (2 * S - 1, 2 * S + 2, 32767)], (1, 3, 2 * S - 1)),
            ("two equal longest runs: the first wins", [(100, 110, 32767), (S + 100, S + 110, -32768)], (2, 10, 100)),
            ("opposite rails side by side across a seam", [(S - 4, S, 32767), (S, S + 4, -32768)], (2, 4, S - 4)),
            ("at both ends of the signal", [(0, 3, 32767), (n - 7, n, 32767)], (2, 7, n - 7))):
        x = noise(n)
        for a, b, v in runs:
            x[a:b, 0] = v
            x[a:b, 1] = -v if v != -32768 else 32767  # the other channel: the same runs at the other rail
        got = check(x)
        for c in range(2):
            assert (got["clip_runs"][c], got["clip_longest"][c], got["clip_longest_at"][c]) == want, (name, c)
        check(np.ascontiguousarray(x[:, 0]))  # and as a mono signal


def test_rail_everywhere(S):
    n = 3 * S + 5
    for v in (32767, -32768):
        got = check(np.full((n, 2), v, np.int16))
        assert got["clip_runs"] == [1, 1] and got["clip_longest"] == [n, n] and got["clip_longest_at"] == [0, 0]
    x = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)  # runs of length 1
    got = check(np.stack([x, np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int16)], axis=1))
    assert got["clip_runs"] == [0, 0] and got["clip_samples"] == [n, n] and got["clip_longest"] == [1, 1]
    assert check(x, r=1)["clip_runs"][0] == n


def test_silence(S):
    n = 2 * S + 3
    z = np.zeros((n, 2), np.int16)
    z[::3, 0], z[1::3, 1] = 1, -1  # an undithered LSB toggle counts as silence at q = 1
    got = check(z)
    assert (got["lead_silence"], got["trail_silence"], got["silent_frames"]) == (n, n, n)
    assert (got["silence_longest"], got["silence_longest_at"]) == (n, 0)
    got = check(z, q=0)  # ... and not at q = 0
    assert got["silent_frames"] == n - len(z[::3]) - len(z[1::3]) and got["silence_longest"] == 1 and got["lead_silence"] == 0
    for at in (0, n - 1, S - 1, S):
        x = z.copy()
        x[at, 1] = -300
        got = check(x)
        assert (got["lead_silence"], got["trail_silence"], got["silent_frames"]) == (at, n - 1 - at, n - 1)
        assert got["silence_longest"] == max(at, n - 1 - at)
        check(np.ascontiguousarray(x[:, 1]))
    x = noise(3 * S + 5)
    x[S - 7:2 * S + 9] = 0  # a dropout across two seams
    x[100:130] = 1
    got = check(x)
    assert (got["silence_longest"], got["silence_longest_at"]) == (S + 16, S - 7) and got["lead_silence"] == 0
    assert got["silent_frames"] == S + 16 + 30


def test_hops(S):
    """Rate 2000: 11 hop pieces in a span and every wave astride a hop; 11025: uneven hops; a
    length just short of 4 hops: no window; 192000: a hop longer than nine spans, and with
    -32768 on both channels the largest window sums."""
    rng = np.random.default_rng(4)
    n = 3 * S + 5
    x = np.clip(rng.normal(0.0, 20000.0, (n, 2)), -32768, 32767).astype(np.int16)
    x[:, 1] = (0.5 * x[:, 1] - 0.5 * x[:, 0]).astype(np.int16)
    got = check(x, 2000)
    assert got["hops"] == 30 and got["corr_windows"] == 27 and got["corr_negative"] > 0
    check(np.ascontiguousarray(x[:, 0]), 2000)
    assert check(x, 11025)["hops"] == 5
    got = check(noise(4 * 4410 - 1, seed=8, amp=30000), RATE)
    assert got["hops"] == 3 and got["corr_windows"] == 0 and got["corr_min_hop"] == -1
    n = 4 * 19200 + 7
    got = check(np.full((n, 2), -32768, np.int16), 192000)
    assert got["hops"] == 4 and got["corr_windows"] == 1 and got["corr_min"] == 1.0
    assert got["sq"] == [n << 30, n << 30] and got["cross"] == n << 30


def batch_tracks(S):
    """Six tracks of lengths {0, 1, S, S + 1, 3S + 5, 2} cut from ONE array: neighbours end and
    begin at the same rail, and in silence, so a run that joined across two tracks would show."""
    lens = [0, 1, S, S + 1, 3 * S + 5, 2]
    x = noise(sum(lens), seed=6)
    off = np.concatenate([[0], np.cumsum(lens)])
    x[off[1]:off[2] + 4] = 32767          # track 1 (one frame) at the rail, and track 2 begins there too
    x[off[3] - 5:off[3] + 6] = 0          # track 2 ends and track 3 begins in silence
    x[off[4] - 3:off[4] + 2] = -32768     # track 3 ends and track 4 begins at the other rail
    x[off[5] - 2:] = 32767                # track 4 ends, and all of track 5 lies, at the rail
    return x, lens, off


@pytest.mark.parametrize("f32", [False, True], ids=["i16", "f32"])
def test_batch_side_by_side(S, f32):
    import torch
    from mastering_amd import engine, native
    x, lens, off = batch_tracks(S)
    ctx = native.context(0)
    d = torch.from_numpy(np.ascontiguousarray(as_kind(x, f32))).cuda()
    torch.cuda.current_stream().synchronize()
    step = d.element_size() * 2
    n = len(lens)
    out = (native.MMQc * n)()
    ctx.check(ctx.lib.mm_batch_qc_device(ctx.ptr, engine._pointers([d.data_ptr() + int(o) * step for o in off[:-1]]),
                                         native.MM_OUT_F32 if f32 else native.MM_OUT_I16, (ctypes.c_int64 * n)(*lens), n, 2,
                                         2000, 1, 3, out), "mm_batch_qc_device")
    last = engine.qcs(ctx, n)
    for t in range(n):
        track = x[off[t]:off[t + 1]]
        want, _ = host_qc(track, 2000)
        assert same_qc(qc_fields(out[t]), want) == [], (t, same_qc(qc_fields(out[t]), want))
        alone, _ = gpu_qc(track, 2000, f32=f32)
        assert same_qc(qc_fields(out[t]), alone) == [], t
        assert same_qc(qc_fields(last[t]), want) == [], t
    assert out[2].clip_longest[0] == 4 and out[1].clip_longest[0] == 1 and out[5].clip_longest[0] == 2
    assert out[2].trail_silence == 5 and out[3].lead_silence == 6 and out[4].clip_longest_at[0] == 0


def test_batch_python_entry(S):
    from mastering_amd import qc_batch_pcm, qc_pcm
    x, lens, off = batch_tracks(S)
    tracks = [np.ascontiguousarray(x[off[t]:off[t + 1]]) for t in range(len(lens))]
    for f32 in (False, True):
        got = qc_batch_pcm([as_kind(t, f32) for t in tracks], 11025, silence_lsb=2, min_run=2)
        assert got == [qc_pcm(as_kind(t, f32), 11025, silence_lsb=2, min_run=2) for t in tracks]
        assert got[4]["min_run"] == 2 and got[4]["silence_lsb"] == 2 and got[4]["frames"] == lens[4]
    one = qc_batch_pcm([tracks[4]], RATE)  # n = 1 is the single-track entry
    assert one == [qc_pcm(tracks[4], RATE)]
    d, table = qc_pcm(tracks[4], 2000, curve=True)
    assert table.shape == (d["hops"], 3) and np.array_equal(table, host_qc(tracks[4], 2000)[1])
    with pytest.raises(ValueError, match="one channel count"):
        qc_batch_pcm([tracks[2], tracks[2][:, 0]], RATE)
    with pytest.raises(ValueError, match="min_run"):
        qc_pcm(tracks[2], RATE, min_run=0)
    with pytest.raises(ValueError, match="track 0: rate below 2000"):
        qc_batch_pcm(tracks[:3], 1999)


@pytest.fixture(scope="module")
def hot():
    from mastering_amd.synth import pink_noise_pcm16
    return pink_noise_pcm16(int(1.5 * RATE), RATE, 2, track=31, level_dbfs=-6.0)


def test_master_call_reports_what_it_delivered(hot):
    from mastering_amd import engine, master_pcm, native, qc_pcm
    plain, info_plain = master_pcm(hot, RATE, P)
    assert set(info_plain) == INFO_KEYS  # without the key: the call of before
    out, info = master_pcm(hot, RATE, dict(P, qc=True, report=True))
    assert np.array_equal(out, plain) and set(info) == INFO_KEYS | {"qc", "report"}
    assert info["qc"] == qc_pcm(out, RATE)
    assert info["qc"]["clip_samples"] == info["report"]["clipped"]
    assert info["qc"]["frames"] == len(out) and info["qc"]["rate"] == RATE and info["qc"]["corr_windows"] > 0
    assert same_qc(qc_fields(engine.qcs(native.context(0), 1)[0]), host_qc(out, RATE)[0]) == []
    out, info = master_pcm(hot, RATE, dict(P, qc=True))  # alone: no other report is made
    assert np.array_equal(out, plain) and set(info) == INFO_KEYS | {"qc"} and info["qc"] == qc_pcm(out, RATE)
    with pytest.raises(RuntimeError):
        engine.meters(native.context(0), 1)
    out, info = master_pcm(hot, RATE, dict(P, qc=True, report=True, output_rate=48000, ceiling_dbtp=-1.0))
    assert info["rate"] == 48000 and info["qc"] == qc_pcm(out, 48000)  # of what was delivered
    assert info["qc"]["clip_samples"] == info["report"]["clipped"] and info["qc"]["frames"] == len(out)
    ref, info_ref = master_pcm(hot, RATE, dict(P, report=True, output_rate=48000, ceiling_dbtp=-1.0))
    assert np.array_equal(out, ref) and {k: v for k, v in info.items() if k != "qc"} == info_ref
    mono, info = master_pcm(np.ascontiguousarray(hot[:, 0]), RATE, dict(P, qc=True), out_kind=native.MM_OUT_F32)
    assert info["qc"] == qc_pcm(mono, RATE) and info["qc"]["channels"] == 1 and info["qc"]["corr_min"] is None


def test_deliver_batch_with_qc():
    import torch
    from mastering_amd import Job, deliver_batch, native, qc_pcm
    from mastering_amd.synth import pink_noise_pcm16
    pcms = [pink_noise_pcm16(int(1.2 * RATE) + 100 * i, RATE, 2, track=40 + i, level_dbfs=-10.0) for i in range(3)]
    ctx = native.context(0)

    def run(**kw):
        jobs = [Job(len(p), RATE, 2, P) for p in pcms]
        for j in jobs:
            j.job.in_kind = native.MM_IN_I16
        xs = [torch.from_numpy(p).cuda() for p in pcms]
        outs = [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]
        torch.cuda.current_stream().synchronize()
        lv = deliver_batch(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs], (-14.0, -16.0, -11.0), -1.0,
                           **kw)[1]
        return [o.cpu().numpy() for o in outs], lv

    plain, lv_plain = run()
    outs, lv = run(qc=True)
    for a, b, d, e in zip(outs, plain, lv, lv_plain):
        assert np.array_equal(a, b) and "qc" not in e
        assert {k: v for k, v in d.items() if k != "qc"} == e  # the level dicts are otherwise what they were
        assert d["qc"] == qc_pcm(a, RATE)
