"""The linear-phase FIR and the reference match on the GPU: fir_pcm against the numpy restatement
of the definition (test_fir.ref_fir) across the kernel's span seams, the keyed cache of the taps,
match_pcm against the same composition in numpy, and params['match'] in a master call against
the composition of the public parts.  Every comparison is an equality."""
import numpy as np
import pytest

from test_fir import fir_stats, random_taps, ref_fir, tilt
from test_gpu_meter import SMOKE

pytestmark = pytest.mark.gpu


def limit_taps(K, seed):
    """random_taps with the centre tap raised until sum |c| = 2^24 - 1: just under the limit."""
    c = random_taps(K, seed).astype(np.int64)
    H = (K - 1) // 2
    c[H] = abs(c[H]) + (1 << 24) - 1 - np.abs(c).sum()
    assert np.abs(c).sum() == (1 << 24) - 1 and np.array_equal(c, c[::-1])
    return c.astype(np.int32)


def gpu_signals(N, ch, seed):
    rng = np.random.default_rng(seed)
    shape = (N,) if ch == 1 else (N, ch)
    return {"noise": np.clip(rng.standard_normal(shape) * 9000, -32768, 32767).astype(np.int16),
            "top rail": np.full(shape, 32767, np.int16), "bottom rail": np.full(shape, -32768, np.int16)}


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("K", [3, 129, 2047, 8191])
def test_fir_pcm_is_the_definition(K, ch):
    """Samples and statistics, int16 and float32 buffers, with a table just under sum |c| = 2^24
    (the rails and the noise clip), at lengths around the half length and the span S; at K = 8191
    and N = 3 S + 5 every span's halo reaches across its neighbours: the seam case that matters."""
    from mastering_amd import engine, native
    S = native.load().mm_fir_span()
    H = (K - 1) // 2
    taps = limit_taps(K, K + ch)
    clipped = 0
    for N in (1, H, K, S - 1, S, S + 1, 3 * S + 5):
        for name, x in gpu_signals(N, ch, 7 * K + N).items():
            want, st = ref_fir(x, taps)
            out, d = engine.fir_pcm(x, 48000, taps, key=0)
            assert out.dtype == np.int16 and np.array_equal(out, want), (N, name)
            assert fir_stats(d) == st and d["rate"] == 48000, (N, name)
            outf, df = engine.fir_pcm((x / 32768.0).astype(np.float32), 48000, taps)
            assert outf.dtype == np.float32 and np.array_equal(outf, (want / 32768.0).astype(np.float32)), (N, name)
            assert fir_stats(df) == st, (N, name)
            clipped += sum(st["clipped"])
    assert clipped > 0


def test_taps_cache_is_keyed():
    """The context keeps the device copy of the taps under the caller's key: a call with the same
    key and K does not read the table again, so ANOTHER table under that key gives the first
    table's output (the key is a content key: a caller that reuses one for other taps gets what
    it asked for); key 0 uploads on every call; another K under the same key is read."""
    from mastering_amd import engine
    x = gpu_signals(3000, 2, 1)["noise"]
    a, b, c = random_taps(129, 1, 0.3), random_taps(129, 2, 0.3), random_taps(131, 3, 0.3)
    want = {name: ref_fir(x, t)[0] for name, t in (("a", a), ("b", b), ("c", c))}
    assert not np.array_equal(want["a"], want["b"])
    assert np.array_equal(engine.fir_pcm(x, 44100, a, key=5)[0], want["a"])
    assert np.array_equal(engine.fir_pcm(x, 44100, b, key=5)[0], want["a"])  # not re-read
    assert np.array_equal(engine.fir_pcm(x, 44100, b, key=0)[0], want["b"])  # no key: uploaded
    assert np.array_equal(engine.fir_pcm(x, 44100, a, key=0)[0], want["a"])
    assert np.array_equal(engine.fir_pcm(x, 44100, b, key=5)[0], want["b"])  # (the keyless upload dropped the key)
    assert np.array_equal(engine.fir_pcm(x, 44100, c, key=5)[0], want["c"])  # another K: read
    assert np.array_equal(engine.fir_pcm(x, 44100, a)[0], want["a"])         # the content key of the engine
    assert np.array_equal(engine.fir_pcm(x, 44100, b)[0], want["b"])


def test_refusals_leave_the_context_usable():
    import ctypes
    from mastering_amd import engine, native
    x = gpu_signals(500, 2, 2)["noise"]
    good = random_taps(9, 1)
    off = good.copy()
    off[1] += 1
    full = np.zeros(5, np.int32)
    full[[0, 4]], full[2] = 1 << 22, 1 << 23
    for taps in (good[:8], np.array([1 << 22], np.int32), np.ones(8193, np.int32), off, full):
        with pytest.raises(ValueError, match="fir|K must"):
            engine.fir_pcm(x, 44100, taps, key=0)
    with pytest.raises(ValueError, match="channels"):
        engine.fir_pcm(np.zeros((10, 3), np.int16), 44100, good)
    assert np.array_equal(engine.fir_pcm(x, 44100, good)[0], ref_fir(x, good)[0])
    ctx = native.context(0)
    m = native.MMFirResult()
    ctx.check(ctx.lib.mm_last_fir(ctx.ptr, ctypes.byref(m)), "mm_last_fir")
    assert m.frames == 500 and m.K == 9 and m.channels == 2
    out, d = engine.fir_pcm(np.zeros((0, 2), np.int16), 44100, good)
    assert out.shape == (0, 2) and d["frames"] == 0 and d["peak"] == [0, 0]
    # out of place: ranges that overlap anywhere are refused, ranges that touch are not
    import torch
    buf = torch.from_numpy(np.concatenate([x, x])).cuda()
    torch.cuda.synchronize()
    f = engine.Fir(good, 44100)
    for shift, ok in ((0, False), (100, False), (499, False), (500, True)):
        rc = ctx.lib.mm_fir_device(ctx.ptr, ctypes.c_void_p(buf.data_ptr()), native.MM_OUT_I16, 500, 2, ctypes.byref(f.fir),
                                   ctypes.c_void_p(buf.data_ptr() + 4 * shift), ctypes.byref(m))
        assert (rc == 0) == ok, shift
        if not ok:
            with pytest.raises(ValueError, match="overlap"):
                ctx.check(rc, "mm_fir_device")
    assert np.array_equal(buf[500:].cpu().numpy(), ref_fir(x, good)[0]) and np.array_equal(buf[:500].cpu().numpy(), x)


# ------------------------------------------------------------------ the match
def filtered_copy(pcm, rate, curve_db):
    """`pcm` through a known curve (one gain a band), as a reference to match."""
    from mastering_amd import design, engine
    taps = design.match_taps(rate, curve_db, trim=0.5 * design.match_headroom(rate, curve_db))
    return engine.fir_pcm(pcm, rate, taps)[0]


@pytest.mark.parametrize("level_dbfs", [-10.0, -24.0])
def test_match_pcm_is_the_numpy_composition(level_dbfs):
    """match_pcm equals spectrum_pcm's figures -> match_gains -> match_taps -> ref_fir (twice when the
    first pass clips), samples and match_dict, on 1.5 s of pink noise (the hot one clips at its peaks)
    against a filtered copy of itself."""
    from mastering_amd import engine
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcm = pink_noise_pcm16(66150, rate, 2, track=3, level_dbfs=level_dbfs)
    centres, _ = tilt(rate)
    curve = 8.0 * np.sin(np.arange(centres.size) * (2 * np.pi / 24.0))
    reference = filtered_copy(pcm, rate, curve)
    out, d = engine.match_pcm(pcm, rate, (reference, rate))
    gains = engine.match_gains(engine.spectrum_pcm(pcm, rate), engine.spectrum_pcm(reference, rate))
    outs = []
    want = engine.match_apply(lambda taps: (outs.append(ref_fir(pcm, taps)), outs[-1][1])[1], gains, rate)
    print(f"match at {level_dbfs} dBFS: passes {d['passes']}, trim {d['trim_db']:.3f} dB, clipped {d['fir']['clipped']}")
    assert d["status"] == "matched" and d["passes"] == want["passes"] == len(outs) and d["fir"]["clipped"] == [0, 0]
    assert d["passes"] == (2 if level_dbfs == -10.0 else 1)  # (the hot one runs the trimmed second pass)
    assert np.array_equal(out, outs[-1][0])
    assert fir_stats(d["fir"]) == want["fir"]
    assert {k: v for k, v in d.items() if k != "fir"} == {k: v for k, v in want.items() if k != "fir"}
    # the same through a spectrum_dict, with less of it asked
    out2, d2 = engine.match_pcm(pcm, rate, engine.spectrum_pcm(reference, rate), amount=0.5, max_db=3.0)
    g2 = engine.match_gains(engine.spectrum_pcm(pcm, rate), engine.spectrum_pcm(reference, rate), 0.5, 3.0)
    assert d2["bands"][5]["gain_db"] == g2["gains_db"][5] and max(abs(g) for g in g2["gains_db"]) <= 1.5
    assert out2.shape == pcm.shape and d2["amount"] == 0.5 and d2["max_db"] == 3.0


def test_match_pcm_unmeasurable_returns_the_signal():
    from mastering_amd import engine
    x = gpu_signals(3000, 2, 5)["noise"]  # shorter than one 8192-sample frame: no spectrum
    out, d = engine.match_pcm(x, 44100, (x, 44100))
    assert np.array_equal(out, x) and d["status"] == "unmeasurable" and d["passes"] == 0 and d["fir"] is None


# ------------------------------------------------------------------ in a master call
RATE = 96000
END = dict(output_rate=44100, ceiling_dbtp=-1.0, deliver_lufs=-14.0, report=True, r128=True, qc=True, spectrum=True)


@pytest.fixture(scope="module")
def call():
    """1.5 s of pink noise at 96 kHz, a reference, the master call with the match and every end,
    and the composition of the public parts on the same input."""
    from mastering_amd import engine
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(144000, RATE, 2, track=6, level_dbfs=-12.0)
    ref_pcm = pink_noise_pcm16(66150, 44100, 2, track=9, level_dbfs=-20.0)
    centres, _ = tilt(44100)
    reference = engine.spectrum_pcm(filtered_copy(ref_pcm, 44100, np.linspace(-5.0, 5.0, centres.size)), 44100)
    match = {"reference": reference, "amount": 0.8, "max_db": 9.0}
    out, info = engine.master_pcm(pcm, RATE, dict(SMOKE, match=match, **END))
    head, head_info = engine.master_pcm(pcm, RATE, dict(SMOKE, output_rate=44100))
    matched, md = engine.match_pcm(head, 44100, reference, amount=0.8, max_db=9.0)
    levelled, lv = engine.level_pcm(matched, 44100, -14.0, ceiling_dbtp=-1.0)
    return dict(pcm=pcm, match=match, out=out, info=info, head_info=head_info, md=md, levelled=levelled, lv=lv)


def test_master_pcm_with_match_is_the_composition(call):
    from mastering_amd import engine
    out, info, want = call["out"], call["info"], call["levelled"]
    assert np.array_equal(out, want)
    assert {k: info[k] for k in call["head_info"]} == call["head_info"] and info["rate"] == 44100
    assert info["match"] == call["md"] and info["match"]["status"] == "matched" and info["match"]["rate"] == 44100
    assert info["level"] == call["lv"]
    report = engine.meter_pcm(want, 44100)
    report["loudness_error"] = report["output_loudness"] - SMOKE["lufs"]
    assert info["report"] == report
    assert info["r128"] == engine.r128_pcm(want, 44100)
    assert info["qc"] == engine.qc_pcm(want, 44100)
    assert info["spectrum"] == engine.spectrum_pcm(want, 44100)
    assert info["ceiling"]["tp_out_q28"] == max(report["true_peak_q28"]) <= info["ceiling"]["ceiling_q28"]
    assert set(info) == set(call["head_info"]) | {"match", "level", "ceiling", "report", "r128", "qc", "spectrum"}


def test_process_with_match_writes_the_same_samples(call, tmp_path):
    from mastering_amd import engine, wavio
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    wavio.write_wav(src, call["pcm"], RATE)
    info = engine.process(src, dst, dict(SMOKE, match=call["match"], **END))
    got, rate = wavio.read_wav(dst)
    assert rate == 44100 and np.array_equal(got, call["out"])
    assert info.pop("output_path") == dst and info == call["info"]
    # a reference given as a 16-bit PCM WAV is measured as the (pcm, rate) pair is
    ref = str(tmp_path / "ref.wav")
    wavio.write_wav(ref, call["out"], 44100)
    a, ia = engine.master_pcm(call["pcm"][:48000], RATE, {"match": {"reference": ref}})
    b, ib = engine.master_pcm(call["pcm"][:48000], RATE, {"match": {"reference": (call["out"], 44100)}})
    assert np.array_equal(a, b) and ia == ib and ia["match"]["status"] == "matched"


def test_without_match_nothing_changes(call, tmp_path):
    """Without the key, or with None, both functions are the calls they were: the same bytes, the
    same info keys, and no fir launch."""
    from mastering_amd import engine, native, wavio
    ctx = native.context(0)
    params = dict(SMOKE, **END)
    ctx.timing(True)
    try:
        before = ctx.kernel_stats().get("fir", (0.0, 0))[1]
        a, ia = engine.master_pcm(call["pcm"], RATE, params)
        b, ib = engine.master_pcm(call["pcm"], RATE, dict(params, match=None))
        assert a.tobytes() == b.tobytes() and ia == ib and "match" not in ia
        src = str(tmp_path / "in.wav")
        wavio.write_wav(src, call["pcm"], RATE)
        files = []
        for name, extra in (("a.wav", {}), ("b.wav", {"match": None})):
            inf = engine.process(src, str(tmp_path / name), dict(params, **extra))
            inf.pop("output_path")
            files.append((open(tmp_path / name, "rb").read(), inf))
        assert files[0] == files[1] and files[0][1] == ia
        assert np.array_equal(wavio.read_wav(str(tmp_path / "a.wav"))[0], a)
        assert ctx.kernel_stats().get("fir", (0.0, 0))[1] == before
        engine.master_pcm(call["pcm"][:48000], RATE, dict(SMOKE, match=call["match"]))
        assert ctx.kernel_stats().get("fir", (0.0, 0))[1] > before
    finally:
        ctx.timing(False)
