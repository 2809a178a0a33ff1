"""The release-jump records on the device after the base rule changed
(csrc/compressor.hip rec_base): comp_rms_t writes the record of every tile whose
largest M reaches the band's fixed base, comp_describe copies it to the tile's
compact index and walks only the tiles below that base.

One-chunk tracks of 2-4 s: the smallest shapes with a partial last tile (2 s at
48 kHz: 426.67 tiles), a partly filled column block (392 / 427 / 588 / 784 tiles
against blocks of 256), a chunk start, and both record branches inside one column
block (the P_FULL high band; the staircase, where most tiles lie below the base).
  * wrong records show up as wrong output: the goldens (also with the release jumps
    off, which must change nothing), a mono, a 48 kHz and the staircase case,
    bit-identical;
  * needlessly uncovered records show up only in the records themselves:
    mm_solve_records against the CPU restatement (tests/test_record_base.py), bit for
    bit, NaNs included."""
import ctypes
import json
import os

import numpy as np
import pytest

import signals as S
from conftest import GOLDEN
from test_gpu_signals import HOT_BANDS, _compress_bands, _oracle_bands
from test_record_base import RATE, band_records, bands_of, e0fix_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["full_4s", "hot_4s"])
def test_goldens_with_and_without_jumps(name, monkeypatch):
    from mastering_amd import master_pcm
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    st = json.loads(str(d["settings"]))
    out, info = master_pcm(d["pcm"], int(d["rate"]), st)
    assert np.array_equal(out, d["out"]), np.mean(out == d["out"])
    monkeypatch.setenv("MM_COMP_NOJUMP", "1")
    ref, info_nj = master_pcm(d["pcm"], int(d["rate"]), st)
    monkeypatch.delenv("MM_COMP_NOJUMP")
    print(f"{name}: jumped {info['comp_jumped']} walked {info['comp_walked']} iters {info['comp_iters']}; "
          f"jumps off: walked {info_nj['comp_walked']} iters {info_nj['comp_iters']}")
    assert info_nj["comp_jumped"] == 0
    assert np.array_equal(out, ref), np.mean(out == ref)


@pytest.mark.parametrize("seconds,rate,channels", [(3, 44100, 1), (2, 48000, 2)], ids=["mono_3s", "48k_2s"])
def test_multiband_vs_oracle(seconds, rate, channels):
    from mastering_amd import ops
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(seconds * rate, rate, channels, track=3)
    got = ops.apply_multiband_compressor(pcm, *HOT_BANDS, frame_rate=rate)
    ref = S.oracle.apply_multiband_compressor(pcm, rate, HOT_BANDS[0::2], HOT_BANDS[1::2])
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), np.mean(got == ref)


def test_staircase_vs_oracle():
    bands = S.staircase_bands(1)
    got, ref = _compress_bands(bands, RATE), _oracle_bands(bands, RATE)
    assert np.array_equal(got, ref), np.mean(got == ref)


def _device_records(ctx, band, cap):
    tiles = np.empty(cap, np.int32)
    mmax = np.empty(cap, np.float64)
    rec = np.empty((cap, 16), np.float64)
    n = ctypes.c_int64()
    D = ctypes.POINTER(ctypes.c_double)
    ctx.check(ctx.lib.mm_solve_records(ctx.ptr, band, cap, tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                       mmax.ctypes.data_as(D), rec.ctypes.data_as(D), ctypes.byref(n)),
              "mm_solve_records")
    assert 0 <= n.value <= cap
    return tiles[:n.value], mmax[:n.value], rec[:n.value].view(np.uint64)


@pytest.mark.parametrize("shift", [1, -1])
def test_r0_must_be_the_first_nonzero_row(shift):
    """comp_rms_t writes a record for a tile with a nonzero M, comp_describe copies one
    for a tile with an rms >= r0: a job whose r0 is not the table's first nonzero row
    is refused (MM_ERR_ARG) before anything is queued."""
    import torch

    from mastering_amd import Job, native
    job = Job(RATE, RATE, 2, S.P_HOT)
    job.job.band[1].r0 += shift
    ctx = native.context(0)
    d_in = torch.zeros((RATE, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="first nonzero row"):
        ctx.check(ctx.lib.mm_stage_chunks(ctx.ptr, ctypes.byref(job.job), ctypes.c_void_p(d_in.data_ptr())), "stage")


@pytest.mark.parametrize("source", ["full", "hot"])
def test_records_equal_the_restatement(source):
    import torch

    from mastering_amd import Job, native
    from mastering_amd.synth import pink_noise_pcm16
    params = {"full": S.P_FULL, "hot": S.P_HOT}[source]
    pcm = pink_noise_pcm16(2 * RATE, RATE, 2, track=0)  # the input of bands_of(source)
    job = Job(pcm.shape[0], RATE, 2, params)
    ctx = native.context(0)
    d_in = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.float32) / 32768)).cuda()
    ctx.check(ctx.lib.mm_stage_chunks(ctx.ptr, ctypes.byref(job.job), ctypes.c_void_p(d_in.data_ptr())), "stage")
    ntiles = -(-job.frames_proc // job.tile)
    both = 0
    for b, (M, _, R, table) in enumerate(bands_of(source)):
        assert len(M) == job.frames_proc
        e0fix = e0fix_of(table)
        live, mx, base, q = band_records(M, R, e0fix, job.tile)
        tiles, mmax, rec = _device_records(ctx, b, ntiles)
        print(f"{source} band {b}: {len(live)} active tiles, {int(np.count_nonzero(base != e0fix))} below the base")
        assert np.array_equal(tiles, live)
        assert np.array_equal(mmax.view(np.uint64), mx.view(np.uint64))
        assert np.array_equal(rec, q), np.flatnonzero((rec != q).any(axis=1))[:8]
        both += int((base != e0fix).any() and (base == e0fix).any())
    if source == "full":
        assert both >= 1  # a band with both record branches
