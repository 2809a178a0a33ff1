"""A batch and an album delivered at another rate on the GPU: deliver_batch / master_album /
process_batch with `output_rate` against the composition of their parts on the batch's OWN
mastered mids (read back from `d_mids`): resample_pcm per track, then level_pcm per track (the
album: album_level_pcm of the converted mids).  The composition starts from the batch's mids,
not from master_pcm: batch and single-track chains may differ in rare samples.  All
comparisons are equalities: bytes, and dicts of integers and of doubles computed from the
same integers."""
import ctypes

import numpy as np
import pytest

from test_ceiling import q28
from test_gpu_resample import HOT

pytestmark = pytest.mark.gpu

RATE, OUT_RATE = 96000, 44100
TARGETS = (-7.0, -14.0, -5.5)  # the first and last push pink noise into the ceiling at the new rate
CEILING = -1.0


@pytest.fixture(scope="module")
def pcms():
    """Three tracks of 1.5 s hot 96 kHz pink noise at different levels."""
    from mastering_amd.synth import pink_noise_pcm16
    return [pink_noise_pcm16(144000, RATE, 2, track=30 + i, level_dbfs=lv) for i, lv in enumerate((-12.0, -18.0, -9.0))]


def run(pcms, call, output_rate=None):
    """`call(ctx, jobs, d_ins, d_outs, output_rate, d_mids)` on fresh device buffers:
    (its return value, the mids read back or None, the outputs read back)."""
    import torch
    from mastering_amd import Job, engine, native
    ctx = native.context(0)
    jobs = [Job(len(p), RATE, 2, HOT) for p in pcms]
    for j in jobs:
        j.job.in_kind = native.MM_IN_I16
    xs = [torch.from_numpy(p).cuda() for p in pcms]
    procs = [torch.full((j.frames_proc, 2), 77, dtype=torch.int16, device="cuda") for j in jobs]
    if output_rate is None:
        mids, outs = None, procs
    else:
        rs = engine.Resampler(RATE, output_rate)
        mids, outs = procs, [torch.full((rs.frames_out(j.frames_proc), 2), 77, dtype=torch.int16, device="cuda") for j in jobs]
    torch.cuda.current_stream().synchronize()
    got = call(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs], output_rate,
               None if mids is None else [m.data_ptr() for m in mids])
    return got, None if mids is None else [m.cpu().numpy() for m in mids], [o.cpu().numpy() for o in outs]


def level_alone(pcm, rate, target, ceiling_dbtp):
    """mm_level_pcm on one track: (samples, level_dict, ceiling_dict, r128_dict of the samples)."""
    from mastering_amd import design, engine, native
    x = pcm.copy()
    ctx = native.context(0)
    m, ce = native.MMLevel(), native.MMCeiling()
    ctx.check(ctx.lib.mm_level_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), native.MM_OUT_I16, x.shape[0], 2, rate,
                                   engine.kweight_sos(rate), design.level_clu(target), design.ceiling_q28(ceiling_dbtp),
                                   design.ceiling_window(rate), ctypes.byref(m), ctypes.byref(ce)), "mm_level_pcm")
    return x, engine.level_dict(m), engine.ceiling_dict(ce), engine.r128_pcm(x, rate)


@pytest.fixture(scope="module")
def delivered(pcms):
    from mastering_amd import deliver_batch
    (res, lvs), mids, outs = run(pcms, lambda ctx, jobs, i, o, r, m: deliver_batch(ctx, jobs, i, o, TARGETS, CEILING, r, m),
                                 OUT_RATE)
    return res, lvs, mids, outs


def test_deliver_batch_at_another_rate_is_the_composition(pcms, delivered):
    from mastering_amd import engine, level_pcm, resample_pcm
    res, lvs, mids, outs = delivered
    assert len(res) == len(lvs) == 3
    hot = 0
    for t in range(3):
        assert mids[t].shape == (144000, 2) and not np.all(mids[t] == 77)
        conv, rd = resample_pcm(mids[t], RATE, OUT_RATE)
        want, ld, cd, r128 = level_alone(conv, OUT_RATE, TARGETS[t], CEILING)
        again, ld2 = level_pcm(conv, OUT_RATE, TARGETS[t], CEILING)
        assert again.tobytes() == want.tobytes() and ld2 == ld
        d = dict(lvs[t])
        assert outs[t].shape == want.shape == (engine.Resampler(RATE, OUT_RATE).frames_out(144000), 2)
        assert outs[t].tobytes() == want.tobytes(), t
        assert d.pop("resample") == rd and (rd["rate_in"], rd["rate_out"], rd["frames_out"]) == (RATE, OUT_RATE, len(want))
        assert d.pop("ceiling") == cd and d.pop("r128") == r128
        assert d == ld and d["rate"] == OUT_RATE and d["window"] == 220 and d["target_lufs"] == TARGETS[t]
        assert cd["tp_out_q28"] <= q28(CEILING)
        print(f"track {t}: status {d['status']} loudness {d['loudness']} limited {d['limited_frames']} "
              f"resample peak {rd['peak']} clipped {rd['clipped']}")
        hot += d["limited_frames"] > 0
    assert hot  # hot enough: a ceiling had work to do at the new rate


def test_master_album_at_another_rate_is_the_composition(pcms):
    from mastering_amd import album_level_pcm, master_album, resample_pcm
    (res, album), mids, outs = run(pcms, lambda ctx, jobs, i, o, r, m: master_album(ctx, jobs, i, o, -14.0, CEILING, r, m),
                                   OUT_RATE)
    convs, rds = zip(*[resample_pcm(m, RATE, OUT_RATE) for m in mids])
    convs, rds = list(convs), list(rds)
    want, wd = album_level_pcm(convs, OUT_RATE, -14.0, CEILING)
    d = dict(album)
    assert d.pop("resample") == rds and len(rds) == 3
    assert d == wd and d["rate"] == OUT_RATE
    for t in range(3):
        assert outs[t].tobytes() == want[t].tobytes(), t
        assert d["tracks"][t]["ceiling"]["tp_out_q28"] <= q28(CEILING)


def test_process_batch_writes_the_delivered_rate(pcms, delivered, tmp_path):
    from mastering_amd import process_batch, wavio
    res, lvs, mids, outs = delivered
    ins = [str(tmp_path / f"in{i}.wav") for i in range(3)]
    dst = [str(tmp_path / f"out{i}.wav") for i in range(3)]
    for p, x in zip(ins, pcms):
        wavio.write_wav(p, x, RATE)
    infos = process_batch(ins, dst, dict(HOT, deliver_lufs=list(TARGETS), ceiling_dbtp=CEILING), output_rate=OUT_RATE)
    for p, y, info, d in zip(dst, outs, infos, lvs):
        got, rate = wavio.read_wav(p)
        assert rate == OUT_RATE and got.shape == y.shape and np.array_equal(got, y)
        assert info["level"] == d and info["resample"] == d["resample"]
        assert info["rate"] == OUT_RATE and info["frames"] == len(y)


def test_process_album_writes_the_delivered_rate(pcms, tmp_path):
    from mastering_amd import process_album, wavio
    ins = [str(tmp_path / f"in{i}.wav") for i in range(3)]
    dst = [str(tmp_path / f"out{i}.wav") for i in range(3)]
    for p, x in zip(ins, pcms):
        wavio.write_wav(p, x, RATE)
    infos, album = process_album(ins, dst, dict(HOT, deliver_lufs=-14.0, ceiling_dbtp=CEILING), output_rate=OUT_RATE)
    assert album["rate"] == OUT_RATE and len(album["resample"]) == 3
    for p, info, rd in zip(dst, infos, album["resample"]):
        got, rate = wavio.read_wav(p)
        assert rate == OUT_RATE and len(got) == rd["frames_out"] == info["frames"] and info["rate"] == OUT_RATE
        assert info["resample"] == rd


def test_without_output_rate_nothing_changes(pcms):
    """deliver_batch without output_rate, with None and with the jobs' own rate: byte-equal to
    master_batch + level_batch_pcm, the dicts without "resample", and d_mids is not touched."""
    from mastering_amd import deliver_batch, level_batch_pcm, master_batch
    _, _, plain = run(pcms, lambda ctx, jobs, i, o, r, m: master_batch(ctx, jobs, i, o))
    want, ds = level_batch_pcm(plain, RATE, TARGETS, CEILING)
    for call in (lambda ctx, jobs, i, o, r, m: deliver_batch(ctx, jobs, i, o, TARGETS, CEILING),
                 lambda ctx, jobs, i, o, r, m: deliver_batch(ctx, jobs, i, o, TARGETS, CEILING, None, None),
                 lambda ctx, jobs, i, o, r, m: deliver_batch(ctx, jobs, i, o, TARGETS, CEILING, RATE, [0, 0, 0])):
        (res, lvs), _, outs = run(pcms, call)
        for y, w, d, e in zip(outs, want, lvs, ds):
            assert y.tobytes() == w.tobytes() and d == e and "resample" not in d
