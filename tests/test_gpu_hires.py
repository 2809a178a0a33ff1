"""24- and 32-bit integer PCM on the GPU.  The decode kernel against the numpy
definition (bit patterns) at the sizes where it can go wrong: every byte phase of the
input pointer, every 16-byte phase of the output, the ends of a workgroup span
(mm_pcm_decode_span) and more spans than workgroups; and every way into the chain
(master_device, master_pcm, process on files, the worker, the GUI batch entry,
master_batch fused and on streams) against the same call on the float32 array or file of
the decoded values.  Everything here is an equality: the chain runs as MM_IN_F32 on the
decoded floats, so the delivered bytes and every statistic must be the same."""
import base64
import ctypes
import json
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMOKE = {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0,
         "saturation": 30, "width": 1.3, "multiband": True, "lufs": -14.0}
EQ_ONLY = {"bass_boost": 4.0, "treble_boost": 3.0}
I24_EDGES = [0x7FFFFF, -0x800000, -1, 1, 0]
I32_EDGES = [2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, 2 ** 24 + 3, 0, 1, -1]
MAX_GRID = 2048  # workgroups of the decode launch (csrc/decode.hip: DEC_MAX_GRID)


# ------------------------------------------------------------------ helpers
def pack24(s):
    """sign-extended 24-bit values (any shape, C order) -> packed little-endian uint8"""
    u = (np.asarray(s, dtype=np.int64).reshape(-1) & 0xFFFFFF).astype(np.uint32)
    return np.ascontiguousarray(np.stack([u & 0xFF, (u >> 8) & 0xFF, u >> 16], axis=1).astype(np.uint8)).reshape(-1)


def f32_of_24(s):
    return (np.asarray(s, dtype=np.float64) / 2 ** 23).astype(np.float32)


def f32_of_32(s):
    return (np.asarray(s, dtype=np.float64) / 2 ** 31).astype(np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def wide_pink(frames, rate, ch, track, low_bits, level_dbfs=-6.0):
    """Pink noise as sign-extended samples of 16 + low_bits bits: the int16 programme
    with `low_bits` random bits below it (0: on the int16 grid)."""
    from mastering_amd.synth import pink_noise_pcm16
    p = pink_noise_pcm16(frames, rate, ch, track=track, level_dbfs=level_dbfs).astype(np.int64) << low_bits
    if low_bits:
        p |= np.random.default_rng(track).integers(0, 1 << low_bits, p.shape)
    return p


def dev_bytes(raw_u8, phase):
    """A device copy of `raw_u8` whose pointer has byte phase `phase` (torch allocations
    are aligned far beyond 4 bytes).  Returns (the slice, keep-alive)."""
    import torch
    buf = torch.empty(raw_u8.size + 8, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[phase:phase + raw_u8.size]
    view.copy_(torch.from_numpy(raw_u8))
    assert view.data_ptr() % 4 == phase % 4
    return view, buf


def sync():
    import torch
    torch.cuda.current_stream().synchronize()  # copies are on torch's stream, the library uses its own


@pytest.fixture(scope="module")
def span():
    from mastering_amd import native
    return native.load().mm_pcm_decode_span()


@pytest.fixture(scope="module")
def pool(span):
    """Random samples (the edge values first), shared by the kernel tests."""
    n = (MAX_GRID + 1) * span + 5
    rng = np.random.default_rng(24)
    s24 = rng.integers(-2 ** 23, 2 ** 23, n)
    s24[:len(I24_EDGES)] = I24_EDGES
    s32 = rng.integers(-2 ** 31, 2 ** 31, n)
    s32[:len(I32_EDGES)] = I32_EDGES
    s32[7:107] = 2 ** 24 + np.arange(100)  # ties and near-ties of the int -> f32 conversion
    return {"raw24": pack24(s24), "want24": f32_of_24(s24), "raw32": s32.astype(np.int32).view(np.uint8),
            "want32": f32_of_32(s32)}


def decode_device(kind, raw_view, n, hs):
    """mm_pcm_decode_device into a float tensor at 16-byte phase `hs` (in floats) with NaN
    sentinels around it: (rc, the n floats, True if every sentinel is still NaN)."""
    import torch
    from mastering_amd import native
    out = torch.full((hs + n + 64,), float("nan"), dtype=torch.float32, device="cuda")
    assert out.data_ptr() % 16 == 0
    sync()
    ctx = native.context(0)
    rc = ctx.lib.mm_pcm_decode_device(ctx.ptr, kind, ctypes.c_void_p(raw_view.data_ptr()), n,
                                      ctypes.c_void_p(out.data_ptr() + 4 * hs))
    host = out.cpu().numpy()
    return rc, host[hs:hs + n], bool(np.isnan(host[:hs]).all() and np.isnan(host[hs + n:]).all())


def sizes(span):
    return [0, 1, 2, 3, 4, 5, 15, 16, 17, 64 * 16 - 1, 64 * 16, 64 * 16 + 1, span - 1, span, span + 1, 2 * span + 3]


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_decode_i24_every_phase_and_size(span, pool, phase):
    from mastering_amd import native
    view, _keep = dev_bytes(pool["raw24"][:3 * (2 * span + 3)], phase)
    for k, n in enumerate(sizes(span)):
        for hs in {0, (k + phase) % 4}:
            rc, got, clean = decode_device(native.MM_IN_I24, view, n, hs)
            assert rc == 0, (n, hs)
            assert np.array_equal(bits(got), bits(pool["want24"][:n])), (n, hs)
            assert clean, (n, hs)


def test_decode_i32_every_size(span, pool):
    from mastering_amd import native
    view, _keep = dev_bytes(pool["raw32"][:4 * (2 * span + 3)], 0)
    for k, n in enumerate(sizes(span)):
        for hs in {0, 1 + k % 3}:
            rc, got, clean = decode_device(native.MM_IN_I32, view, n, hs)
            assert rc == 0, (n, hs)
            assert np.array_equal(bits(got), bits(pool["want32"][:n])), (n, hs)
            assert clean, (n, hs)
    assert pool["want32"][0] == 1.0 and pool["want32"][1] == -1.0  # INT32_MAX, INT32_MIN


def test_decode_starts_inside_the_input(span, pool):
    """A pointer into the middle of packed data (a track inside a timeline): sample
    offsets 1, 2, 3 give byte phases 3, 2, 1 of the same allocation."""
    from mastering_amd import native
    view, _keep = dev_bytes(pool["raw24"][:3 * (span + 40)], 0)
    for skip in (1, 2, 3, 5):
        n = span + 40 - skip - 1
        rc, got, clean = decode_device(native.MM_IN_I24, view[3 * skip:], n, skip % 4)
        assert rc == 0 and clean
        assert np.array_equal(bits(got), bits(pool["want24"][skip:skip + n])), skip


@pytest.mark.parametrize("kind_name,phase,hs", [("I24", 1, 3), ("I32", 0, 1)])
def test_decode_more_spans_than_workgroups(span, pool, kind_name, phase, hs):
    """(MAX_GRID + 1) spans and a few samples: workgroups take a second span."""
    from mastering_amd import native
    n = (MAX_GRID + 1) * span + 5
    kind, raw, want = ((native.MM_IN_I24, pool["raw24"], pool["want24"]) if kind_name == "I24"
                       else (native.MM_IN_I32, pool["raw32"], pool["want32"]))
    view, _keep = dev_bytes(raw, phase)
    rc, got, clean = decode_device(kind, view, n, hs)
    assert rc == 0 and clean
    assert np.array_equal(bits(got), bits(want[:n]))


def test_decode_refuses_bad_arguments(pool):
    from mastering_amd import native
    view, _keep = dev_bytes(pool["raw32"][:4 * 64], 2)
    rc, _, clean = decode_device(native.MM_IN_I32, view, 32, 0)  # an int32 pointer at byte phase 2
    assert rc == native.MM_ERR_ARG and clean
    view0, _keep0 = dev_bytes(pool["raw32"][:4 * 64], 0)
    for kind in (native.MM_IN_F32, native.MM_IN_I16, 4):
        rc, _, clean = decode_device(kind, view0, 32, 0)
        assert rc == native.MM_ERR_ARG and clean
    rc, _, clean = decode_device(native.MM_IN_I24, view0, -1, 0)
    assert rc == native.MM_ERR_ARG and clean


def test_decode_pcm_operator(pool):
    from mastering_amd import ops
    n = 5000
    assert np.array_equal(bits(ops.decode_pcm(pool["raw24"][:3 * n], 24)), bits(pool["want24"][:n]))
    s32 = pool["raw32"][:4 * n].view(np.int32).reshape(-1, 2)
    got = ops.decode_pcm(s32, 32)
    assert got.shape == s32.shape and np.array_equal(bits(got).reshape(-1), bits(pool["want32"][:n]))
    assert ops.decode_pcm(np.empty(0, np.uint8), 24).shape == (0,)
    with pytest.raises(TypeError):
        ops.decode_pcm(pool["raw24"][:10], 24)
    with pytest.raises(TypeError):
        ops.decode_pcm(s32.astype(np.int16), 32)
    with pytest.raises(ValueError):
        ops.decode_pcm(s32, 16)


# ------------------------------------------------------------------ 2. master_device
def run_device(ptr, kind, frames, rate, ch, params, out_kind, report=False, ceiling=None):
    """master_device on a device input: everything it delivers and reports, as bytes."""
    import torch
    from mastering_amd import Job, engine, master_device, native
    job = Job(frames, rate, ch, params, out_kind, report=report, ceiling_dbtp=ceiling)
    job.job.in_kind = kind
    out = torch.zeros(job.frames_proc * ch, dtype=torch.int16 if out_kind == native.MM_OUT_I16 else torch.float32,
                      device="cuda")
    sync()
    ctx = native.context(0)
    res = native.MMResult()
    master_device(ctx, job, ptr, out.data_ptr(), res)
    got = {"out": out.cpu().numpy().tobytes(), "res": result_tuple(res), "frames": job.frames_proc}
    if report:
        got["meter"] = bytes(engine.meters(ctx, 1)[0])
    if ceiling is not None:
        got["ceiling"] = bytes(engine.ceilings(ctx, 1)[0])
    return got


def result_tuple(r):
    return (repr(r.loudness), repr(r.gain_linear), r.frames_out, r.comp_iters, r.comp_active, r.comp_walked,
            r.comp_jumped)


DEVICE_CASES = {
    # name: (frames, rate, channels, low bits, byte phase, report, ceiling)
    "stereo_3s": (3 * 44100, 44100, 2, 8, 1, True, -1.0),
    "mono_odd_48k": (48001, 48000, 1, 8, 3, False, None),
    "stereo_3s_on_grid": (3 * 44100, 44100, 2, 0, 2, True, -1.0),
}


@pytest.mark.parametrize("f32_out", [False, True], ids=["i16_out", "f32_out"])
@pytest.mark.parametrize("case", list(DEVICE_CASES))
def test_master_device_i24_equals_f32(case, f32_out):
    import torch
    from mastering_amd import native
    frames, rate, ch, low, phase, report, ceiling = DEVICE_CASES[case]
    s = wide_pink(frames, rate, ch, 3, low) << (8 - low)  # 24-bit samples
    if low:
        assert np.any(s & 0xFF)  # off the int16 grid: the exciter's tanhf path
    else:
        assert not np.any(s & 0xFF) and np.any(s)  # on it: the table path
    x = f32_of_24(s)
    view, _keep = dev_bytes(pack24(s), phase)
    xf = torch.from_numpy(x).cuda()
    kind = native.MM_OUT_F32 if f32_out else native.MM_OUT_I16
    a = run_device(view.data_ptr(), native.MM_IN_I24, frames, rate, ch, SMOKE, kind, report, ceiling)
    b = run_device(xf.data_ptr(), native.MM_IN_F32, frames, rate, ch, SMOKE, kind, report, ceiling)
    assert a["res"] == b["res"]
    assert a["out"] == b["out"]
    assert a.get("meter") == b.get("meter") and a.get("ceiling") == b.get("ceiling")
    # (pydub's millisecond slicing: 48 001 frames are processed as 48 000)
    assert a["frames"] == frames - frames % 2 and a["res"][2] == a["frames"]
    assert len(a["out"]) == a["frames"] * ch * (4 if f32_out else 2) and any(a["out"])
    assert a["res"][3] >= 1 and a["res"][4] > 0  # the compressor ran


# ------------------------------------------------------------------ 3. master_pcm
@pytest.mark.parametrize("low,ch,frames,rate", [(16, 2, 3 * 44100, 44100), (8, 1, 48001, 48000)],
                         ids=["stereo_32bit", "mono_24bit_left_justified"])
def test_master_pcm_int32_equals_f32(low, ch, frames, rate):
    from mastering_amd import master_pcm, native
    s = wide_pink(frames, rate, ch, 5, low)
    left = (s << (16 - low)).astype(np.int32)  # left-justified
    x = f32_of_32(left)
    if low == 8:
        assert np.array_equal(bits(x), bits(f32_of_24(s)))
    params = dict(SMOKE, report=True, ceiling_dbtp=-1.0)
    for kind in (native.MM_OUT_I16, native.MM_OUT_F32):
        out_a, info_a = master_pcm(left, rate, params, out_kind=kind)
        out_b, info_b = master_pcm(x, rate, params, out_kind=kind)
        assert out_a.dtype == out_b.dtype and out_a.shape == out_b.shape
        assert out_a.shape == (frames - frames % 2,) + left.shape[1:]  # (pydub's millisecond slicing)
        assert out_a.tobytes() == out_b.tobytes()
        assert json.dumps(info_a, sort_keys=True) == json.dumps(info_b, sort_keys=True)
        assert info_a["report"]["frames"] == info_a["frames"] == out_a.shape[0] and info_a["comp_iters"] >= 1


# ------------------------------------------------------------------ 4. files
GUID_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"


def write_wide_wav(path, s, rate, bits_, extensible=False):
    """`s`: sign-extended samples of `bits_` bits, [N] or [N, ch]."""
    ch = 1 if s.ndim == 1 else s.shape[1]
    payload = pack24(s).tobytes() if bits_ == 24 else np.ascontiguousarray(s).astype("<i4").tobytes()
    ba = ch * bits_ // 8
    if extensible:
        fmt = struct.pack("<HHIIHHHHIH", 0xFFFE, ch, rate, rate * ba, ba, bits_, 22, bits_, 3, 1) + GUID_TAIL
    else:
        fmt = struct.pack("<HHIIHH", 1, ch, rate, rate * ba, ba, bits_)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", 3) + b"abc\x00"
    body += b"data" + struct.pack("<I", len(payload)) + payload
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def same_info(a, b):
    a, b = dict(a), dict(b)
    a.pop("output_path"), b.pop("output_path")
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


@pytest.fixture(scope="module")
def file_track():
    """3 s stereo, 24 significant bits, and its float32 form."""
    s = wide_pink(3 * 44100, 44100, 2, 7, 8)
    return s, f32_of_24(s)


@pytest.mark.parametrize("form", ["i24", "i24_extensible", "i32"])
@pytest.mark.parametrize("fmt", ["pcm16", "f32"])
def test_process_wide_file_equals_f32_file(tmp_path, file_track, form, fmt):
    from mastering_amd import process, wavio
    s, x = file_track
    src, ref_src = str(tmp_path / "in.wav"), str(tmp_path / "ref.wav")
    if form == "i32":
        write_wide_wav(src, s << 8, 44100, 32)
    else:
        write_wide_wav(src, s, 44100, 24, extensible=form.endswith("extensible"))
    wavio.write_wav(ref_src, x, 44100)
    got, _ = wavio.read_wav(src)
    assert got.dtype == np.int32 and np.array_equal(got, (s << 8).astype(np.int32))
    params = dict(SMOKE, report=True, ceiling_dbtp=-1.0, output_format=fmt)
    info = process(src, str(tmp_path / "out.wav"), params)
    ref = process(ref_src, str(tmp_path / "ref_out.wav"), params)
    assert (tmp_path / "out.wav").read_bytes() == (tmp_path / "ref_out.wav").read_bytes()
    assert same_info(info, ref) and info["frames"] == 3 * 44100
    y, _ = wavio.read_wav(str(tmp_path / "out.wav"))
    assert y.dtype == (np.int16 if fmt == "pcm16" else np.float32) and y.shape == (3 * 44100, 2)  # 16-bit delivery


def test_process_i24_file_larger_than_a_staging_buffer(tmp_path):
    """33 s stereo at 44.1 kHz: 8.7 MB of packed samples, so the 8 MiB staging boundary
    (no multiple of 3) falls inside a sample, and the file spans two 30 s chunks."""
    from mastering_amd import process, wavio
    frames = 33 * 44100
    assert frames * 6 > (8 << 20) and (8 << 20) % 3
    s = wide_pink(frames, 44100, 2, 9, 8)
    src, ref_src = str(tmp_path / "in.wav"), str(tmp_path / "ref.wav")
    write_wide_wav(src, s, 44100, 24)
    wavio.write_wav(ref_src, f32_of_24(s), 44100)
    info = process(src, str(tmp_path / "out.wav"), EQ_ONLY)
    ref = process(ref_src, str(tmp_path / "ref_out.wav"), EQ_ONLY)
    assert (tmp_path / "out.wav").read_bytes() == (tmp_path / "ref_out.wav").read_bytes()
    assert same_info(info, ref) and info["frames"] == frames and info["chunks"] == 2
    y, _ = wavio.read_wav(str(tmp_path / "out.wav"))
    assert np.any(y[-1000:]) and np.any(y[(8 << 20) // 6 - 2:(8 << 20) // 6 + 2])


def test_worker_and_gui_batch_take_i24_files(tmp_path, file_track):
    from mastering_amd import gui_compat, process, wavio
    from mastering_amd.worker import handle_push
    s, x = file_track
    settings = dict(SMOKE)
    ref_src = str(tmp_path / "ref.wav")
    wavio.write_wav(ref_src, x, 44100)
    process(ref_src, str(tmp_path / "ref_out.wav"), settings)
    want = (tmp_path / "ref_out.wav").read_bytes()
    # the Pub/Sub push handler on an object
    (tmp_path / "bkt" / "uploads").mkdir(parents=True)
    write_wide_wav(str(tmp_path / "bkt" / "uploads" / "track.wav"), s, 44100, 24)
    job = {"gcs_uri": "gs://bkt/uploads/track.wav", "settings": settings}
    env = {"message": {"data": base64.b64encode(json.dumps(job).encode()).decode()}}
    assert handle_push(env, str(tmp_path)) == ("", 204)
    assert (tmp_path / "bkt" / "processed" / "mastered_track.wav").read_bytes() == want
    assert (tmp_path / "bkt" / "processed" / "mastered_track.wav.complete").exists()
    # the GUI's folder batch
    (tmp_path / "in").mkdir()
    write_wide_wav(str(tmp_path / "in" / "a.wav"), s, 44100, 24, extensible=True)
    write_wide_wav(str(tmp_path / "in" / "b.wav"), s << 8, 44100, 32)
    messages = []
    results = gui_compat.batch_process_audio(settings, str(tmp_path / "in"), str(tmp_path / "out"), messages.append)
    assert sorted(results) == ["a.wav", "b.wav"] and all(isinstance(v, dict) for v in results.values()), results
    assert (tmp_path / "out" / "a_mastered.wav").read_bytes() == want
    assert (tmp_path / "out" / "b_mastered.wav").read_bytes() == want
    assert "complete: 2 files" in messages[-1]


# ------------------------------------------------------------------ 5. batches
def run_batch(jobs_spec, ptrs, kind):
    """master_batch on device inputs: per track (output bytes, result)."""
    import torch
    from mastering_amd import Job, master_batch, native
    jobs = [Job(frames, rate, ch, params) for frames, rate, ch, params in jobs_spec]
    for j in jobs:
        j.job.in_kind = kind
    outs = [torch.full((j.frames_proc * j.channels,), 12345, dtype=torch.int16, device="cuda") for j in jobs]
    sync()
    res = master_batch(native.context(0), jobs, ptrs, [o.data_ptr() for o in outs])
    return [(o.cpu().numpy().tobytes(), result_tuple(r)) for o, r in zip(outs, res)]


def check_batch(tracks, spec, ptrs24, keep):
    """the I24 batch against the same batch on float32 tensors of the decoded values"""
    import torch
    from mastering_amd import native
    xs = [torch.from_numpy(f32_of_24(s)).cuda() for s in tracks]
    a = run_batch(spec, ptrs24, native.MM_IN_I24)
    b = run_batch(spec, [x.data_ptr() for x in xs], native.MM_IN_F32)
    for t, (ta, tb) in enumerate(zip(a, b)):
        assert ta[1] == tb[1], t
        assert ta[0] == tb[0], t
        assert any(ta[0]), t
    del keep
    return a


@pytest.mark.parametrize("rate,ch", [(44100, 2), (11025, 1)], ids=["stereo_44k", "mono_11k"])
def test_batch_i24_fused_and_streams(rate, ch):
    """(a) two same-settings tracks as separate tensors (one exactly a 30 s chunk, one 2 s
    with an odd frame count: the fused gather), (b) the same two back to back in one
    tensor (track 2 at 30 s * rate * channels * 3 bytes: 2 mod 4 at 11 025 Hz mono),
    (c) with a third track of other settings, which runs on a stream of its own."""
    from mastering_amd import design
    chunk = design.pydub_frame(design.CHUNK_MS, rate)
    assert chunk == 30 * rate
    n2 = 2 * rate + 1
    t1, t2, t3 = wide_pink(chunk, rate, ch, 11, 8), wide_pink(n2, rate, ch, 12, 8), wide_pink(rate + 7, rate, ch, 13, 8)
    spec = [(chunk, rate, ch, SMOKE), (n2, rate, ch, SMOKE)]
    # (a) separate tensors at different byte phases
    v1, k1 = dev_bytes(pack24(t1), 1)
    v2, k2 = dev_bytes(pack24(t2), 2)
    a = check_batch([t1, t2], spec, [v1.data_ptr(), v2.data_ptr()], (k1, k2))
    # (b) one tensor, back to back
    both, kb = dev_bytes(np.concatenate([pack24(t1), pack24(t2)]), 0)
    off2 = chunk * ch * 3
    if (rate, ch) == (11025, 1):
        assert off2 == 992250 and off2 % 4 == 2  # the misaligned start inside the timeline
    b = check_batch([t1, t2], spec, [both.data_ptr(), both.data_ptr() + off2], kb)
    assert [x[0] for x in a] == [x[0] for x in b]
    # (c) a third track with other settings
    v3, k3 = dev_bytes(pack24(t3), 3)
    spec3 = spec + [(rate + 7, rate, ch, dict(SMOKE, lufs=-9.0, saturation=10))]
    c = check_batch([t1, t2, t3], spec3, [v1.data_ptr(), v2.data_ptr(), v3.data_ptr()], (k1, k2, k3))
    assert [x[0] for x in c[:2]] == [x[0] for x in a]


def test_batch_i24_in_place_timeline():
    """Two tracks of whole chunks back to back in one tensor: the fused timeline is
    decoded where it lies, here from a pointer at byte phase 1 (11 025 Hz mono: the
    second track starts 992 250 bytes on, at phase 3)."""
    rate, ch = 11025, 1
    chunk = 30 * rate
    t1, t2 = wide_pink(chunk, rate, ch, 21, 8), wide_pink(chunk, rate, ch, 22, 8)
    both, kb = dev_bytes(np.concatenate([pack24(t1), pack24(t2)]), 1)
    spec = [(chunk, rate, ch, SMOKE), (chunk, rate, ch, SMOKE)]
    assert (both.data_ptr() + chunk * 3) % 4 == 3
    check_batch([t1, t2], spec, [both.data_ptr(), both.data_ptr() + chunk * 3], kb)


def test_stage_chunks_takes_i24():
    """The staged entry (time-sharded ranks) gets the decode from the same hook: the
    staged pre-gain mix of an I24 range equals that of its float32 form."""
    import torch
    from mastering_amd import Job, native
    frames, rate = 48001, 48000
    s = wide_pink(frames, rate, 2, 31, 8)
    view, _keep = dev_bytes(pack24(s), 3)
    xf = torch.from_numpy(f32_of_24(s)).cuda()
    sync()
    ctx = native.context(0)
    mixes = []
    for kind, ptr in ((native.MM_IN_I24, view.data_ptr()), (native.MM_IN_F32, xf.data_ptr())):
        job = Job(frames, rate, 2, dict(SMOKE, lufs=None))
        job.job.in_kind = kind
        ctx.check(ctx.lib.mm_stage_chunks(ctx.ptr, ctypes.byref(job.job), ctypes.c_void_p(ptr)), "mm_stage_chunks")
        mix = np.zeros((job.frames_proc, 2), np.int16)
        ctx.check(ctx.lib.mm_read_mix(ctx.ptr, mix.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))), "mm_read_mix")
        mixes.append(mix)
    assert np.array_equal(mixes[0], mixes[1]) and np.any(mixes[0])
