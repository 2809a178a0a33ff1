"""The sample-rate converter on the GPU: the kernel against the numpy definition
(tests/test_resample.py: ref_resample), samples and statistics, at the sizes where it can
go wrong (the workgroup span of mm_resample_span and its seams, a halo that reaches over a
seam, spans cut into several staged pieces, the first and last frames), on the int16 and
the f32 buffer, and the delivery path through every entry point against the composition
of its parts.  All comparisons are equalities on integers.  The kernel launches one
workgroup per span, so there is no case of more spans than workgroups."""
import ctypes
import os

import numpy as np
import pytest

from test_ceiling import ceiling_stats, q28, ref_ceiling
from test_gpu_meter import SMOKE, check_report
from test_resample import ONE, ref_resample, resample_stats, resampler

pytestmark = pytest.mark.gpu

PAIRS = [(96000, 44100), (44100, 48000), (96000, 48000), (192000, 44100)]


@pytest.fixture(scope="module")
def span():
    from mastering_amd import native
    return native.load().mm_resample_span()


def planned(rate_in, rate_out):
    """(mm_resampler with its content key, (L, M, K, c)) of a designed pair."""
    from mastering_amd import design
    L, M, K, c = design.resample_taps(rate_in, rate_out)
    return resampler(rate_in, rate_out, L, M, K, c, design.resample_key(rate_in, rate_out)), (L, M, K, c)


def dev_resample(pcm, rs, f32=False, kind=None, ch=None):
    """mm_resample_device on a device copy of int16 `pcm` (or of pcm / 32768 as f32):
    (the output as int16, the statistics)."""
    import torch
    from mastering_amd import native
    x = np.ascontiguousarray(pcm, np.int16)
    host = x.astype(np.float32) / np.float32(32768) if f32 else x
    n_out = -(-x.shape[0] * rs.L // rs.M)
    d = torch.from_numpy(host).cuda()
    o = torch.full((n_out,) + x.shape[1:], 77, dtype=d.dtype, device="cuda")
    torch.cuda.current_stream().synchronize()  # the copies are on torch's stream, the library uses its own
    ctx = native.context(0)
    m = native.MMResample()
    ctx.check(ctx.lib.mm_resample_device(ctx.ptr, ctypes.c_void_p(d.data_ptr()),
                                         (native.MM_OUT_F32 if f32 else native.MM_OUT_I16) if kind is None else kind,
                                         x.shape[0], (1 if x.ndim == 1 else x.shape[1]) if ch is None else ch,
                                         ctypes.byref(rs), ctypes.c_void_p(o.data_ptr()), ctypes.byref(m)),
              "mm_resample_device")
    assert (m.rate_in, m.rate_out) == (rs.rate_in, rs.rate_out)
    raw = o.cpu().numpy()
    if f32:
        k = raw * np.float32(32768)
        assert np.array_equal(k, np.rint(k)) and np.abs(k).max(initial=0) <= 32768  # on the int16 grid
        return k.astype(np.int16), resample_stats(m)
    return raw, resample_stats(m)


def check(pcm, rs, table, both=True):
    want, st = ref_resample(pcm, *table)
    for f32 in ((False, True) if both else (False,)):
        got, gst = dev_resample(pcm, rs, f32)
        assert gst == st, ("f32" if f32 else "i16", gst, st)
        assert np.array_equal(got, want), "f32" if f32 else "i16"
    return want, st


def smallest_input(frames_out, L, M):
    """The smallest N that gives at least frames_out output frames, and what it gives (exactly
    frames_out when the rate goes down; going up, a length between two inputs is not reachable)."""
    n = (frames_out - 1) * M // L + 1
    got = -(-n * L // M)
    assert -(-(n - 1) * L // M) < frames_out <= got < frames_out + L / M
    assert got == frames_out or L > M
    return n, got


def seam_signal(n, ch, span, L, M, seed):
    """A -30 dBFS bed with full-scale samples at the first frame, on both sides of the input
    position of every seam and at the last frame."""
    rng = np.random.default_rng(seed)
    pcm = rng.integers(-1036, 1037, (n, ch)).astype(np.int16)
    marks = [0, n - 1]
    for s in range(1, -(-n * L // M) // span + 1):
        b = s * span * M // L
        marks += [b - 1, b]
    for i, at in enumerate(marks):
        if 0 <= at < n:
            pcm[at, i % ch] = 32767 if i % 2 else -32768
    return pcm if ch == 2 else pcm[:, 0]


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("size", ["1", "K", "S-1", "S", "S+1", "3S+5"])
@pytest.mark.parametrize("pair", PAIRS)
def test_seams(span, pair, size, ch):
    rs, table = planned(*pair)
    L, M, K, _ = table
    frames_out = {"1": 1, "K": K, "S-1": span - 1, "S": span, "S+1": span + 1, "3S+5": 3 * span + 5}[size]
    n, frames_out = smallest_input(frames_out, L, M)
    want, st = check(seam_signal(n, ch, span, L, M, 1000 * frames_out + 10 * ch + L), rs, table)
    assert st["frames_out"] == frames_out == len(want) and max(st["peak"]) > 1036


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("L,M,K", [(1, 16, 4), (3, 40, 6), (1, 640, 2)])
def test_spans_staged_in_pieces(span, L, M, K, ch):
    """Ratios steeper than 8: the input of a span does not fit the LDS lines, and the
    workgroup stages it in several pieces (seams inside a span)."""
    rng = np.random.default_rng(L * M + K)
    c = rng.integers(-(1 << 20), 1 << 20, (L, K))
    c[:, 0] += ONE - c.sum(axis=1)
    rs = resampler(1000 * M, 1000 * L, L, M, K, c)
    n, _ = smallest_input(2 * span + 3, L, M)
    pcm = rng.integers(-32768, 32768, (n, ch)).astype(np.int16)
    check(pcm if ch == 2 else pcm[:, 0], rs, (L, M, K, c))


@pytest.mark.parametrize("pair", [(96000, 44100), (44100, 48000)])
def test_clipping(span, pair):
    """A full-scale square wave overshoots the int16 range; one channel of the stereo case is silent."""
    rs, table = planned(*pair)
    n = 3 * span
    sq = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    want, st = check(sq, rs, table)
    assert st["clipped"][0] > 0 and st["peak"] == [32768]
    want, st = check(np.stack([np.zeros(n, np.int16), sq], axis=1), rs, table)
    assert st["clipped"][0] == 0 and st["clipped"][1] > 0 and st["peak"] == [0, 32768]
    assert not want[:, 0].any()


def test_edge_cases_and_arguments(span):
    from mastering_amd import engine, native
    rs, table = planned(96000, 44100)
    for shape in ((0,), (0, 2)):
        got, st = dev_resample(np.zeros(shape, np.int16), rs)
        assert got.shape == shape and st["frames_out"] == 0 and st["clipped"] == st["peak"] == [0] * len(st["peak"])
    pcm = np.zeros((64, 2), np.int16)
    with pytest.raises(ValueError):
        dev_resample(pcm, rs, kind=7)
    with pytest.raises(ValueError):
        dev_resample(pcm, rs, ch=3)
    L, M, K, c = table
    for bad in (resampler(96000, 44100, L, M, K - 1, c), resampler(96000, 96000, L, L, K, c),
                resampler(96000, 48000, L, M, K, c), resampler(96000, 44100, L, M, K, c.astype(np.int64) * 8)):
        with pytest.raises(ValueError):
            dev_resample(pcm, bad)
    for a, b in ((44100, 44100), (96000, 44101), (44100, 5000)):
        with pytest.raises(ValueError):
            engine.resample_pcm(pcm, a, b)
    with pytest.raises(TypeError):
        engine.resample_pcm(pcm.astype(np.int32), 96000, 44100)
    ctx = native.context(0)
    with pytest.raises(RuntimeError):  # no delivery ran on this context yet, or the last call was none
        engine.master_pcm(pcm, 44100, {"multiband": False})
        ctx.check(ctx.lib.mm_last_resample(ctx.ptr, ctypes.byref(native.MMResample())), "mm_last_resample")


@pytest.mark.parametrize("ch", [1, 2])
def test_resample_pcm_is_the_reference(ch):
    from mastering_amd import design, engine
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(5000, 48000, ch, track=4, level_dbfs=-9.0)
    for a, b in ((48000, 44100), (44100, 96000)):
        L, M, K, c = design.resample_taps(a, b)
        want, st = ref_resample(pcm, L, M, K, c)
        out, d = engine.resample_pcm(pcm, a, b)
        assert out.dtype == np.int16 and np.array_equal(out, want)
        assert {k: d[k] for k in st} == st and (d["rate_in"], d["rate_out"]) == (a, b)
        outf, df = engine.resample_pcm(pcm.astype(np.float32) / np.float32(32768), a, b)
        assert outf.dtype == np.float32 and np.array_equal(outf * np.float32(32768), want) and df == d


def test_taps_cache_is_keyed():
    """A second call with the same key equals the first; another pair on the same context is
    right, and so is the first pair after it; a table without a key is uploaded every time."""
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(4000, 96000, 2, track=5, level_dbfs=-12.0)
    a, ta = planned(96000, 44100)
    b, tb = planned(96000, 48000)
    first = dev_resample(pcm, a)
    again = dev_resample(pcm, a)
    assert np.array_equal(first[0], again[0]) and first[1] == again[1]
    assert np.array_equal(first[0], ref_resample(pcm, *ta)[0])
    check(pcm, b, tb, both=False)
    check(pcm, a, ta, both=False)
    L, M, K, c = tb
    flipped = np.ascontiguousarray(c[:, ::-1])  # another table of the same geometry, no key
    check(pcm, resampler(96000, 48000, L, M, K, flipped), (L, M, K, flipped), both=False)
    check(pcm, b, tb, both=False)


# ------------------------------------------------------------------ the delivery path
RATE = 96000
HOT = dict(SMOKE, lufs=-6.0)  # pushed into the limiter: the converted output exceeds -1 dBTP


@pytest.fixture(scope="module")
def chain():
    """1.5 s of pink noise at 96 kHz mastered plainly, and the composition of the parts on it."""
    from mastering_amd import design, master_pcm, native
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(144000, RATE, 2, track=6, level_dbfs=-12.0)
    ctx = native.context(0)
    ctx.timing(True)
    plain, info0 = master_pcm(pcm, RATE, HOT)
    stats0 = ctx.kernel_stats()
    ctx.timing(False)
    L, M, K, c = design.resample_taps(RATE, 44100)
    conv, rst = ref_resample(plain, L, M, K, c)
    C, W = q28(-1.0), design.ceiling_window(44100)
    want, cst = ref_ceiling(conv, C, W)
    return dict(pcm=pcm, plain=plain, info0=info0, stats0=stats0, conv=conv, rst=rst, want=want, cst=cst, C=C, W=W)


@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_chain_is_the_composition(chain, kind):
    from mastering_amd import engine, master_pcm, native
    ctx = native.context(0)
    ctx.timing(True)
    out, info = master_pcm(chain["pcm"], RATE, dict(HOT, output_rate=44100, ceiling_dbtp=-1.0, report=True),
                           native.MM_OUT_F32 if kind == "f32" else native.MM_OUT_I16)
    stats = ctx.kernel_stats()
    ctx.timing(False)
    if kind == "f32":
        assert out.dtype == np.float32
        out = (out * np.float32(32768)).astype(np.int16)
    rst, cst = chain["rst"], chain["cst"]
    print(f"{kind}: resample clipped {rst['clipped']} peak {rst['peak']}, ceiling tp_in {cst['tp_in_q28'] / 2 ** 28:.4f} "
          f"-> {cst['tp_out_q28'] / 2 ** 28:.4f}, limited {cst['limited_frames']}")
    assert cst["tp_in_q28"] > chain["C"]  # hot enough: the ceiling has work to do after the converter
    assert np.array_equal(out, chain["want"])
    assert {k: info["resample"][k] for k in rst} == rst
    assert (info["resample"]["rate_in"], info["resample"]["rate_out"]) == (RATE, 44100)
    assert {k: info["ceiling"][k] for k in cst} == cst and info["ceiling"]["window"] == chain["W"] == 220
    assert info["ceiling"]["tp_out_q28"] <= chain["C"]
    check_report(info["report"], chain["want"])
    assert max(info["report"]["true_peak_q28"]) == cst["tp_out_q28"]
    assert info["report"]["output_loudness"] == engine.meter_pcm(chain["want"], 44100)["output_loudness"]
    assert info["report"]["loudness_error"] == info["report"]["output_loudness"] - HOT["lufs"]
    assert info["rate"] == 44100 and info["frames"] == len(chain["want"]) == rst["frames_out"]
    assert set(info) - {"resample", "rate", "ceiling", "report"} == set(chain["info0"])
    assert info["loudness"] == chain["info0"]["loudness"] and info["gain_linear"] == chain["info0"]["gain_linear"]
    assert stats["resample_tracks"][1] == 1 and "resample_tracks" not in chain["stats0"]


def test_chain_without_a_ceiling_or_report(chain):
    from mastering_amd import engine, master_pcm, native
    out, info = master_pcm(chain["pcm"], RATE, dict(HOT, output_rate=44100))
    assert np.array_equal(out, chain["conv"]) and "ceiling" not in info and "report" not in info
    assert {k: info["resample"][k] for k in chain["rst"]} == chain["rst"]
    ctx = native.context(0)
    for what in (engine.meters, engine.ceilings):
        with pytest.raises(RuntimeError):
            what(ctx)


def test_process_delivers_the_file(chain, tmp_path):
    from mastering_amd import process, wavio
    from test_wav_hires import _pack24, _wav
    src, dst = str(tmp_path / "in24.wav"), str(tmp_path / "out.wav")
    _wav(src, _pack24(chain["pcm"].astype(np.int64) << 8), 1, 2, RATE, 24)
    info = process(src, dst, dict(HOT, output_rate=44100, ceiling_dbtp=-1.0, report=True))
    got, rate = wavio.read_wav(dst)
    assert rate == 44100 and got.shape == chain["want"].shape and np.array_equal(got, chain["want"])
    assert os.path.getsize(dst) == 44 + chain["want"].nbytes
    assert info["rate"] == 44100 and info["frames"] == len(got) and info["output_path"] == os.path.abspath(dst)
    assert {k: info["ceiling"][k] for k in chain["cst"]} == chain["cst"]
    assert {k: info["resample"][k] for k in chain["rst"]} == chain["rst"]
    check_report(info["report"], got)


def test_without_output_rate_nothing_changes(chain, tmp_path):
    from mastering_amd import master_pcm, process, wavio
    params = dict(HOT, ceiling_dbtp=-1.0, report=True)
    base, info0 = master_pcm(chain["pcm"], RATE, params)
    same, info = master_pcm(chain["pcm"], RATE, dict(params, output_rate=RATE))
    assert same.tobytes() == base.tobytes() and info == info0 and "resample" not in info and "rate" not in info
    assert np.array_equal(master_pcm(chain["pcm"], RATE, HOT)[0], chain["plain"])
    src = str(tmp_path / "in.wav")
    wavio.write_wav(src, chain["pcm"], RATE)
    outs = []
    for name, extra in (("a.wav", {}), ("b.wav", {"output_rate": RATE})):
        inf = process(src, str(tmp_path / name), dict(params, **extra))
        inf.pop("output_path")
        outs.append((open(tmp_path / name, "rb").read(), inf))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1] == info0
    assert wavio.read_wav(str(tmp_path / "a.wav"))[1] == RATE
    assert np.array_equal(wavio.read_wav(str(tmp_path / "a.wav"))[0], base)


def test_delivery_refuses_a_job_that_acts_at_the_source_rate(chain):
    import torch
    from mastering_amd import Job, native
    pcm = chain["pcm"][:9600]
    x = torch.from_numpy(pcm).cuda()
    ctx = native.context(0)

    def deliver(job):
        job.job.in_kind = native.MM_IN_I16
        o = torch.zeros((job.frames_out, 2), dtype=torch.int16, device="cuda")
        torch.cuda.current_stream().synchronize()
        ctx.check(ctx.lib.mm_deliver_device(ctx.ptr, ctypes.byref(job.job), ctypes.byref(job.delivery),
                                            ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(o.data_ptr()), None),
                  "mm_deliver_device")
        return o.cpu().numpy()

    params = {"multiband": False}
    job = Job(len(pcm), RATE, 2, params, output_rate=44100, ceiling_dbtp=-1.0, report=True)
    job.job.ceiling_q28 = job.delivery.ceiling_q28
    with pytest.raises(ValueError, match="source rate"):
        deliver(job)
    job = Job(len(pcm), RATE, 2, params, output_rate=44100, report=True)
    job.job.meter_on = 1
    with pytest.raises(ValueError, match="source rate"):
        deliver(job)
    job = Job(len(pcm), RATE, 2, params, output_rate=44100)
    job.resampler.rs.rate_in = 48000  # not the job's rate
    with pytest.raises(ValueError):
        deliver(job)
    job = Job(len(pcm), RATE, 2, params, output_rate=44100)
    from mastering_amd import design, master_pcm
    want = ref_resample(master_pcm(pcm, RATE, params)[0], *design.resample_taps(RATE, 44100))[0]
    assert np.array_equal(deliver(job), want)
