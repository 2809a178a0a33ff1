"""The compressor and the loudness gate on structured signals (tests/signals.py): the
device against the CPU oracle where the *structure* of the input selects the branch.
Pink noise (every other GPU comparison) keeps each band always or never above its
threshold and loses no loudness block to a gate; these inputs have sparse and partial
tiles, bands without any active frame, the tables' first and last rows, states many
binades above M, and blocks cut by the absolute and by the relative gate.
tests/test_signals.py asserts from the oracle that each input has that structure.

Integer work and the exact envelope solve are compared with np.array_equal; the
whole chain through test_gpu_parity._check (its MIN_EXACT floor: a K-weighting carry
can move L by ~1e-9 LU, and the 4e-4 LU bound).  mm_result.comp_active is compared
with the oracle's active-frame count (rms >= r0, summed over bands and chunks).
The solve statistics (sweeps, re-walked and jumped tiles) are printed, not asserted:
nothing here can derive them (DESIGN.md §4 records them)."""
import ctypes
import functools

import numpy as np
import pytest

import signals as S
from conftest import record_exact
from test_gpu_parity import _batch_on_fresh_context, _check, _oracle_mix, _staged_mix

pytestmark = pytest.mark.gpu

RATE = S.RATE
DEFAULT_BANDS = (-25.0, 6.0, -20.0, 3.0, -15.0, 4.0)  # AME:67-72
HOT_BANDS = (-16.0, 6.0, -21.0, 3.0, -27.0, 4.0)      # P_HOT's thresholds
CHAIN = [n for n in S.CATALOGUE if n != "sub_gate"]


@functools.lru_cache(maxsize=None)
def _signal(name, channels=2):
    pcm = S.chunk_seam(channels=channels) if name == "chunk_seam" else S.CATALOGUE[name](channels=channels)
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def _reference(name, channels=2):
    """(oracle output, oracle loudness, oracle active band-frames) at P_HOT, computed once."""
    pcm = _signal(name, channels)
    ref, L = S.oracle.master(pcm, RATE, S.P_HOT, return_loudness=True)
    ref.setflags(write=False)
    return ref, L, S.structure(pcm, RATE, S.P_HOT)["active"]


def _print_solve(what, iters, walked, jumped, active):
    print(f"solve {what}: comp_iters={iters} comp_walked={walked} comp_jumped={jumped} comp_active={active}")


# ----------------------------------------------------------------- band level
def _compress_bands(bands, rate, params=None):
    """Three int16 band arrays through mm_op_compress_bands (no crossover in front),
    the job built as legacy.apply_multiband_compressor builds its own."""
    from mastering_amd import Job, native, ops
    bands = [np.ascontiguousarray(b) for b in bands]
    ch = 1 if bands[0].ndim == 1 else bands[0].shape[1]
    job = Job(bands[0].shape[0], rate, ch, dict(params or {}, multiband=True), single_chunk=True)
    mix = np.full_like(bands[0], 12345)
    ctx = native.context(0)
    ctx.check(ctx.lib.mm_op_compress_bands(ctx.ptr, ctypes.byref(job.job), ops._ptr(bands[0]), ops._ptr(bands[1]),
                                           ops._ptr(bands[2]), ops._ptr(mix)), "mm_op_compress_bands")
    return mix


def _oracle_bands(bands, rate, params=None):
    o = S.oracle
    c = [o.compress_band(b, rate, t, r, at, rel) for b, (t, r, at, rel) in zip(bands, S.band_settings(params))]
    return o.overlay_add(o.overlay_add(c[0], c[1]), c[2])


@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("name", ["const_fs", "staircase"])
def test_band_level(name, channels, rate):
    """const_fs gathers the tables' last row (window rms 32 768); staircase walks the
    first nonzero row from both sides with the state ~15 binades above M, where no
    jump record covers it: the fix-up has to step and e_fold_tile takes its uncovered
    branch."""
    bands = S.const_fs_bands(channels) if name == "const_fs" else S.staircase_bands(channels)
    got, ref = _compress_bands(bands, rate), _oracle_bands(bands, rate)
    record_exact(np.mean(got == ref), "i16")
    assert np.array_equal(got, ref), np.mean(got == ref)


# ----------------------------------------------------------------- stage level
@pytest.mark.parametrize("bands", [HOT_BANDS, DEFAULT_BANDS], ids=["hot", "default"])
@pytest.mark.parametrize("name", CHAIN)
def test_multiband_stage(name, bands):
    """ops.apply_multiband_compressor (crossover, three compressors, overlay) on the
    raw signal, as test_ops.py::test_multiband compares the reference's vectors."""
    from mastering_amd import ops
    pcm = _signal(name)
    got = ops.apply_multiband_compressor(pcm, *bands, frame_rate=RATE)
    ref = S.oracle.apply_multiband_compressor(pcm, RATE, bands[0::2], bands[1::2])
    assert got.shape == ref.shape
    record_exact(np.mean(got == ref), "i16")
    assert np.array_equal(got, ref), np.mean(got == ref)


# ----------------------------------------------------------------- pre-gain mix
@pytest.mark.parametrize("saturation", [30, 0], ids=["hot", "hot_sat0"])
@pytest.mark.parametrize("name", ["bursts", "square_fs", "step_down"])
def test_pre_gain_mix(name, saturation):
    params = dict(S.P_HOT, saturation=saturation)
    pcm = _signal(name)
    mix, ref = _staged_mix(pcm, params), _oracle_mix(S.oracle, pcm, params)
    record_exact(np.mean(mix == ref), "mix")
    assert np.array_equal(mix, ref), np.mean(mix == ref)


# ----------------------------------------------------------------- whole chain
def _master_and_check(name, channels, as_int16):
    from mastering_amd import master_pcm
    pcm = _signal(name, channels)
    out, info = master_pcm(pcm if as_int16 else pcm.astype(np.float32) / 32768, RATE, S.P_HOT)
    ref, L, active = _reference(name, channels)
    _print_solve(f"{name}[{channels}ch]", info["comp_iters"], info["comp_walked"], info["comp_jumped"],
                 info["comp_active"])
    _, exact = _check(out, info, ref, L)
    print(f"solve {name}[{channels}ch]: identical samples {exact:.7f}")
    if np.isfinite(L):
        assert np.isfinite(info["loudness"])
    else:
        assert info["loudness"] == -np.inf, info["loudness"]
    assert info["comp_active"] == active, (info["comp_active"], active)


@pytest.mark.parametrize("name", list(S.CATALOGUE))
def test_whole_chain(name):
    """master_pcm at P_HOT against oracle.master.  sub_gate: every block lies under
    -70 LUFS, so L = -inf and the gain is inf; inf and NaN products become 0 in the
    int16 output, as the reference's own silence_1s.npz fixes for NaN."""
    _master_and_check(name, 2, False)


@pytest.mark.parametrize("name", ["bursts", "fade_in_cut"])
def test_whole_chain_mono_int16(name):
    _master_and_check(name, 1, True)


def test_chunk_seam():
    """A burst and the loud part of a level step across frame 30 s x rate: each chunk
    restarts the window and the attenuation."""
    _master_and_check("chunk_seam", 2, False)


# ----------------------------------------------------------------- fused unit
def test_fused_unit():
    """The six catalogue signals and a 0.7 s clip as one mm_master_batch: in the fused
    timeline the compact ranking of active tiles runs across tracks of very different
    activity (none at all on sub_gate), and the gate sees -inf next to finite tracks."""
    from mastering_amd.synth import pink_noise_pcm16
    names = list(S.CATALOGUE)
    clip = pink_noise_pcm16(int(0.7 * RATE), RATE, 2, 46)
    pcms = [_signal(n) for n in names] + [clip]
    outs, res, _ = _batch_on_fresh_context(pcms, RATE, S.P_HOT)
    refs = [_reference(n) for n in names]
    ref, L = S.oracle.master(clip, RATE, S.P_HOT, return_loudness=True)
    refs.append((ref, L, S.structure(clip, RATE, S.P_HOT)["active"]))
    for t, (ref, L, active) in enumerate(refs):
        what = (names + ["clip_0.7s"])[t]
        _print_solve(f"fused {what}", res[t].comp_iters, res[t].comp_walked, res[t].comp_jumped, res[t].comp_active)
        _check(outs[t], {"loudness": res[t].loudness}, ref, L)
        if not np.isfinite(L):
            assert res[t].loudness == -np.inf, (what, res[t].loudness)
        assert res[t].comp_active == active, (what, res[t].comp_active, active)
