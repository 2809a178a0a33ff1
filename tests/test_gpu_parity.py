"""GPU parity: the HIP chain (through the C-ABI) against the CPU oracle and the
reference-generated golden fixtures.  Tolerances from BASELINE.json north_star:
PCM RMS diff <= 1e-5 (decoded /32768) and |dLUFS| <= 0.1 LU."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, record_exact

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5
LU_TOL = 0.1

P_FULL = {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0,
          "saturation": 30, "width": 1.3, "multiband": True, "lufs": -14.0}
P_HOT = dict(P_FULL, low_thresh=-16.0, mid_thresh=-21.0, high_thresh=-27.0)


def rms_diff(a, b):
    return float(np.sqrt(np.mean(((a.astype(np.float64) - b.astype(np.float64)) / 32768.0) ** 2)))


# Identical int16 output samples (round 6, profiles/r06_gpu_pytest.log).  The
# exciter reads numpy's own float32 values on the int16 grid (design.saturation_table)
# and the loudness block energies follow numpy's float32 reduction order
# (kw_blocks_kernel), so every reference golden and every oracle comparison of the
# single-track path is bit-identical: GOLDEN_EXACT.  The one remaining source of
# differences is the K-weighting carry: the look-back composes tile maps, so a
# tile's carry-in can differ from lfilter's sequential state in its last bits and,
# rarely, flip an f32 filter output next to a rounding boundary; that moves a block
# energy by one f32 step and L by ~1e-9 LU, and the gain then moves a few f32
# products across an int16 boundary (measured: >= 0.99993 on the cases it touches:
# the fused batches, 44056 Hz).  The time-sharded path (C4) keeps f64 segment
# energies (an all-reduce of segments; its block sums are not numpy's): tolerance.
GOLDEN_EXACT = 1.0
MIN_EXACT = 0.9998
def _check(out, info, ref, L, min_exact=MIN_EXACT):
    """North-star tolerances, plus the identical-sample floor; records the
    fraction (printed at the end of the run)."""
    assert out.shape == ref.shape
    r = rms_diff(out, ref)
    exact = float(np.mean(out == ref))
    record_exact(exact)
    if min_exact is not None:
        assert exact >= min_exact, f"identical-sample fraction {exact:.7f} < {min_exact}"
    assert r <= RMS_TOL, f"rms diff {r:.3e} (exact frac {exact:.6f})"
    if L is not None and np.isfinite(L):
        assert abs(info["loudness"] - L) <= LU_TOL
        assert abs(info["loudness"] - L) <= 4e-4  # internal target
    return r, exact


GOLDEN_CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if not p.endswith("primitives.npz") and not os.path.basename(p).startswith("legacy"))


@pytest.mark.parametrize("path", GOLDEN_CASES, ids=[os.path.basename(p)[:-4] for p in GOLDEN_CASES])
def test_golden(path):
    """Every reference golden through master_pcm (per-stage vectors: test_ops.py)."""
    from mastering_amd import master_pcm
    d = np.load(path)
    st = json.loads(str(d["settings"]))
    out, info = master_pcm(d["pcm"], int(d["rate"]), st)
    L = float(d["loudness"])
    _check(out, info, d["out"], None if np.isnan(L) else L, GOLDEN_EXACT)


@pytest.mark.parametrize("seconds,params,track", [(35, P_FULL, 1), (12, P_HOT, 2)])
def test_vs_oracle(oracle, seconds, params, track):
    from mastering_amd import master_pcm
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(seconds * 44100, 44100, 2, track)
    out, info = master_pcm(pcm, 44100, params)
    ref, L = oracle.master(pcm, 44100, params, return_loudness=True)
    _check(out, info, ref, L, GOLDEN_EXACT)  # (measured bit-identical)


@pytest.mark.parametrize("saturation", [10, 55.5, 100])
def test_exciter_every_grid_input(saturation):
    """apply_saturation's operator on every int16-grid input equals numpy's value
    (design.saturation_table) for all 65 536 inputs.  (The chain's EQ kernel instead
    corrects its tanhf with 2-bit codes built from that table by sat_corr_kernel;
    test_mix_with_exciter and the goldens check that path end to end.)"""
    from mastering_amd import design, ops
    tab, _ = design.saturation_table(saturation)
    x = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16).astype(np.float32) / 32768
    y = ops.apply_saturation(x, saturation)
    assert np.array_equal(y, tab)


def _staged_mix(pcm, params):
    import ctypes

    import torch

    from mastering_amd import Job, native
    job = Job(pcm.shape[0], 44100, 2, params)
    ctx = native.context(0)
    d_in = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.float32) / 32768)).cuda()
    ctx.check(ctx.lib.mm_stage_chunks(ctx.ptr, ctypes.byref(job.job), ctypes.c_void_p(d_in.data_ptr())), "stage")
    mix = np.empty((job.frames_proc, 2), np.int16)
    ctx.check(ctx.lib.mm_read_mix(ctx.ptr, mix.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))), "read_mix")
    return mix


def _oracle_mix(oracle, pcm, params):
    thr, rat = oracle.multiband_params(params)
    ref = []
    for s, e in oracle.chunk_ranges(pcm.shape[0], 44100):
        x = oracle.saturation(oracle.pcm_to_float(pcm[s:e]), params.get("saturation", 0))
        y = oracle.quantize(oracle.stereo_width(oracle.equalize(x, 44100, params), params.get("width", 1.0)))
        ref.append(oracle.multiband(y, 44100, thr, rat))
    return np.concatenate(ref)


def test_mix_bit_exact_without_tanh(oracle):
    """Pre-gain mix (chunks + EQ + width + multiband + overlay, AME:48-80) with the
    exciter off: the quantised IIR passes run scipy's own operation order (iir.hip
    df2t<true>), the rest is integer work and the exact envelope solve, so the int16
    mix is identical to the oracle's (measured 100 %; only a tile-scan carry that
    differs from scipy's serial state in its last bit next to an int16 boundary could
    move a sample)."""
    from mastering_amd.synth import pink_noise_pcm16
    params = dict(P_HOT, saturation=0)
    pcm = pink_noise_pcm16(31 * 44100, 44100, 2, 5)
    mix, ref = _staged_mix(pcm, params), _oracle_mix(oracle, pcm, params)
    record_exact(np.mean(mix == ref), "mix")
    assert np.array_equal(mix, ref), np.mean(mix == ref)


def test_mix_with_exciter(oracle):
    """With the exciter on: numpy's float32 tanh is not correctly rounded, so the device
    corrects its tanhf by a 2-bit code per int16-grid input onto numpy's own values
    (design.saturation_table, sat_corr_kernel): the pre-gain mix is bit-identical."""
    from mastering_amd.synth import pink_noise_pcm16
    pcm = pink_noise_pcm16(31 * 44100, 44100, 2, 5)
    mix, ref = _staged_mix(pcm, P_HOT), _oracle_mix(oracle, pcm, P_HOT)
    record_exact(np.mean(mix == ref), "mix")
    assert np.array_equal(mix, ref), np.mean(mix == ref)


class _ThreadCollectives:
    """Ranks as threads of one process (one mm_ctx each) on the single GPU."""

    def __init__(self, world):
        import threading
        self.world = world
        self.bar = threading.Barrier(world)
        self.slots = [None] * world

    def bind(self, rank):
        outer = self

        class C:
            def all_gather(self, vec):
                outer.slots[rank] = np.asarray(vec, np.float64)
                outer.bar.wait()
                out = np.stack(outer.slots)
                outer.bar.wait()
                return out

            def all_reduce_sum(self, vec):
                return self.all_gather(vec).sum(axis=0)

        return C()


def test_time_sharded_on_one_gpu(oracle):
    """The C4 orchestration (distributed.master_time_sharded) over the C-ABI with
    two ranks on one GPU: stitched output == oracle; same loudness on both ranks."""
    import threading

    import torch

    from mastering_amd import distributed as D
    from mastering_amd import native
    from mastering_amd.synth import pink_noise_pcm16
    rate, world = 44100, 2
    pcm = pink_noise_pcm16(65 * rate, rate, 2, 9)
    ref, Lref = oracle.master(pcm, rate, P_FULL, return_loudness=True)
    coll = _ThreadCollectives(world)
    outs, infos, errs = [None] * world, [None] * world, []

    def rank_main(r):
        try:
            plan = D.plan_time_shards(pcm.shape[0], rate, 2, world, r)
            be = D.GpuBackend(native.Context(0))
            x = torch.from_numpy(pcm[plan.in_lo:plan.in_hi].astype(np.float32) / 32768).cuda()
            out = torch.empty((plan.frames, 2), dtype=torch.int16, device="cuda")
            infos[r] = D.master_time_sharded(be, plan, P_FULL, x.data_ptr(), out.data_ptr(), coll.bind(r))
            be.ctx.sync()
            outs[r] = out.cpu().numpy()
            be.ctx.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
            coll.bar.abort()

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=100)
    assert not errs, errs
    assert infos[0]["loudness"] == infos[1]["loudness"]
    _check(np.concatenate(outs), infos[0], ref, Lref)


def test_staged_job_owns_its_loudness_geometry():
    """mm_stage_chunks keeps its own copy of the job's loudness arrays (seg_bounds,
    block_lo, block_hi): zeroing the caller's arrays after staging changes neither the
    range's end state nor its segment energies, bit for bit.  1 s of mono 44.1 kHz is
    the smallest input the staged path accepts (the 0.4 s block must fit)."""
    import torch

    from mastering_amd import distributed as D
    from mastering_amd import native
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcm = pink_noise_pcm16(rate, rate, 1, 5)
    plan = D.plan_time_shards(pcm.shape[0], rate, 1, 1, 0)
    x = torch.from_numpy(pcm[plan.in_lo:plan.in_hi].astype(np.float32) / 32768).cuda()

    def run(overwrite):
        be = D.GpuBackend(native.Context(0))
        job = be.make_job(plan, {"lufs": -14.0}, native.MM_OUT_I16)
        be.stage(job, x.data_ptr())
        if overwrite:
            assert job._segb.any() and job._hi.any()  # (the overwrite changes them)
            for a in (job._segb, job._lo, job._hi):
                a[...] = 0
        z = be.kweight_range_end()
        e = be.hop_energies(np.zeros(4))
        be.ctx.close()
        return z, e

    z0, e0 = run(False)
    z1, e1 = run(True)
    assert e0.size == len(plan.local_bounds) - 1 and np.any(e0 > 0) and np.any(z0 != 0)
    assert z1.tobytes() == z0.tobytes()
    assert e1.tobytes() == e0.tobytes()


@pytest.mark.parametrize("warmup", [0, 1])
def test_compressor_resume_path(oracle, monkeypatch, warmup):
    """With little or no speculative warm-up and ONE queued fix-up sweep, the
    sweeps do not converge before the chain's sync, so the host resumes (more
    sweeps, back end again): the result must still be exact against the oracle."""
    from mastering_amd import engine, master_pcm
    from mastering_amd.synth import pink_noise_pcm16
    monkeypatch.setattr(engine, "COMP_WARMUP", warmup)
    monkeypatch.setenv("MM_COMP_SWEEPS", "1")
    pcm = pink_noise_pcm16(40 * 44100, 44100, 2, 11)
    out, info = master_pcm(pcm, 44100, P_HOT)
    assert info["comp_iters"] >= 1, info["comp_iters"]  # the one queued sweep changed ends
    ref, L = oracle.master(pcm, 44100, P_HOT, return_loudness=True)
    _check(out, info, ref, L)
    # the control block is zeroed by each pass's finalize: the resumed chain still
    # reports the first pass's active band-frames (kept on the host)
    monkeypatch.delenv("MM_COMP_SWEEPS")
    _, info2 = master_pcm(pcm, 44100, P_HOT)
    assert info["comp_active"] == info2["comp_active"] > 0, (info["comp_active"], info2["comp_active"])


def _batch_on_fresh_context(pcms, rate, params, timing=False):
    """Same-settings stereo f32 tracks through mm_master_batch on a fresh context:
    (outputs, results, per-kernel launch counts when `timing`)."""
    import torch

    from mastering_amd import Job, master_batch, native
    jobs = [Job(p.shape[0], rate, 2, params) for p in pcms]
    xs = [torch.from_numpy(p.astype(np.float32) / 32768).cuda() for p in pcms]
    outs = [torch.full((j.frames_proc, 2), 12345, dtype=torch.int16, device="cuda") for j in jobs]
    torch.cuda.synchronize()
    ctx = native.Context(0)
    ctx.timing(timing)
    res = master_batch(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs])
    launches = {name: n for name, (_, n) in ctx.kernel_stats().items()} if timing else None
    ctx.close()
    return [o.cpu().numpy() for o in outs], res, launches


def test_fused_unit_resume_path(oracle, monkeypatch):
    """The resume loop on a fused unit: with ONE queued fix-up sweep the 40 s track
    (the input test_compressor_resume_path resumes on) and a 3.2 s track, fused into
    one timeline, need more sweeps after the unit's sync; both stay exact against the
    oracle, and the active band-frames kept on the host over the resume (rb_keep /
    rb_finish) land on the right track.  (A run of two tracks is always cut into two
    units of one, so a third 31 s track follows: the scheduler then fuses the first
    two and runs the third as the second unit; two `eq` launches show that split.)"""
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    pcms = [pink_noise_pcm16(40 * rate, rate, 2, 11), pink_noise_pcm16(int(3.2 * rate), rate, 2, 12),
            pink_noise_pcm16(31 * rate, rate, 2, 13)]
    monkeypatch.setenv("MM_COMP_SWEEPS", "1")
    outs, res, launches = _batch_on_fresh_context(pcms, rate, P_HOT, timing=True)
    assert launches["eq"] == 2, launches  # units {40 s, 3.2 s} and {31 s}
    assert res[0].comp_iters == res[1].comp_iters >= 1, (res[0].comp_iters, res[1].comp_iters)
    for t in range(3):
        ref, L = oracle.master(pcms[t], rate, P_HOT, return_loudness=True)
        _check(outs[t], {"loudness": res[t].loudness}, ref, L)
    monkeypatch.delenv("MM_COMP_SWEEPS")
    _, res2, _ = _batch_on_fresh_context(pcms, rate, P_HOT)
    for t in (0, 1):
        assert res[t].comp_active == res2[t].comp_active > 0, (t, res[t].comp_active, res2[t].comp_active)


@pytest.mark.parametrize("channels,params,in_i16,seconds",
                         [(2, P_HOT, False, 0.7), (2, P_HOT, False, 30.0), (2, P_HOT, False, 31.7),
                          (1, P_FULL, True, 31.7), (2, dict(P_HOT, lufs=None), False, 31.7)],
                         ids=["stereo_hot_0.7s", "stereo_hot_30s", "stereo_hot_31.7s", "mono_full_i16_31.7s",
                              "stereo_hot_nolufs_31.7s"])
def test_unit_of_one_equals_direct_call(oracle, channels, params, in_i16, seconds):
    """A single track is a unit of one: mm_master_device and mm_master_batch with
    n = 1, each on a fresh context, give the same bytes and the same result fields
    (sub-chunk, one whole chunk, a ragged last chunk: where a padded timeline and the
    track's own geometry would differ), and both are right against the oracle."""
    import torch

    from mastering_amd import Job, master_batch, master_device, native
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    n = int(round(seconds * rate))
    pcm = pink_noise_pcm16(n, rate, channels, 950)
    x = torch.from_numpy(pcm.copy() if in_i16 else pcm.astype(np.float32) / 32768).cuda()

    def run(batch):
        job = Job(n, rate, channels, params)
        job.job.in_kind = native.MM_IN_I16 if in_i16 else native.MM_IN_F32
        out = torch.full((job.frames_proc, channels), 12345, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ctx = native.Context(0)
        if batch:
            res = master_batch(ctx, [job], [x.data_ptr()], [out.data_ptr()])[0]
        else:
            res = master_device(ctx, job, x.data_ptr(), out.data_ptr(), native.MMResult())
        ctx.close()
        return out.cpu().numpy(), res

    (a, ra), (b, rb) = run(False), run(True)
    assert a.tobytes() == b.tobytes()
    fields = ("loudness", "gain_linear", "comp_iters", "comp_active", "comp_walked", "comp_jumped")
    np.testing.assert_array_equal([getattr(ra, f) for f in fields], [getattr(rb, f) for f in fields])  # (NaN == NaN)
    ref, L = oracle.master(pcm, rate, params, return_loudness=True)
    for out, r in ((a, ra), (b, rb)):
        _check(out.reshape(ref.shape), {"loudness": r.loudness}, ref, L)


def test_fused_unit_without_multiband_after_one_with(oracle):
    """A fused unit with the compressor off reports no active band-frames: the
    readback block then holds no per-chunk counts, and what an earlier multiband
    unit on the same contexts left there (or what lies past it: 20 chunks per unit
    here) is not read.  Every track against the oracle."""
    import torch

    from mastering_amd import Job, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    plain = dict(P_FULL, multiband=False)
    pcms = [pink_noise_pcm16(int(s * rate), rate, 2, 960 + t) for t, s in enumerate((3.2, 31.7, 0.7, 30.0))]
    xs = [torch.from_numpy(p.astype(np.float32) / 32768).cuda() for p in pcms]
    ctx = native.Context(0)

    def run(params):
        # the plain batch repeats the tracks: two units of 20 chunks, more than their readback block spans
        k = 1 if params["multiband"] else 8
        jobs = [Job(p.shape[0], rate, 2, params) for p in pcms] * k
        outs = [torch.full((j.frames_proc, 2), 12345, dtype=torch.int16, device="cuda") for j in jobs]
        torch.cuda.synchronize()
        res = master_batch(ctx, jobs, [x.data_ptr() for x in xs] * k, [o.data_ptr() for o in outs])
        return [o.cpu().numpy() for o in outs], res

    _, res = run(P_FULL)
    assert sum(r.comp_active for r in res) > 0  # (the contexts now hold a multiband unit's counts)
    outs, res = run(plain)
    assert [r.comp_active for r in res] == [0] * len(res), [r.comp_active for r in res]
    assert [(r.comp_walked, r.comp_jumped) for r in res] == [(0, 0)] * len(res)
    for t, pcm in enumerate(pcms):
        ref, L = oracle.master(pcm, rate, plain, return_loudness=True)
        for rep in range(8):
            _check(outs[rep * len(pcms) + t], {"loudness": res[rep * len(pcms) + t].loudness}, ref, L)
    ctx.close()


def test_fused_unit_kweight_sub_tiles(oracle, monkeypatch):
    """MM_KW_SUB=3 (three K-weighting lanes per 225-frame tile) on a fused unit: the
    K-weighting stage then has more look-back blocks than the stereo chunk stages, and
    the control block's regions are sized for them (the unit tells stage_front its
    K-weighting block count).  Ragged stereo tracks against the oracle."""
    from mastering_amd import design
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    monkeypatch.setenv("MM_KW_SUB", "3")
    assert design.kweight_sub(design.choose_tile(30 * rate)) == 3
    pcms = [pink_noise_pcm16(int(s * rate), rate, 2, 900 + t) for t, s in enumerate((3.2, 31.7, 0.7))]
    outs, res, _ = _batch_on_fresh_context(pcms, rate, P_FULL)
    for t, pcm in enumerate(pcms):
        ref, L = oracle.master(pcm, rate, P_FULL, return_loudness=True)
        _check(outs[t], {"loudness": res[t].loudness}, ref, L)


@pytest.mark.parametrize("channels,params,in_i16,rate", [(2, P_FULL, False, 44100), (1, P_HOT, True, 44100),
                                                          (2, dict(P_FULL, lufs=None), False, 44100),
                                                          (2, P_HOT, True, 48000)],
                         ids=["stereo_full", "mono_hot_i16", "stereo_nolufs", "stereo_hot_48k"])
def test_fused_batch_ragged(oracle, monkeypatch, channels, params, in_i16, rate):
    """mm_master_batch fuses same-settings tracks into one timeline (whole chunks
    per track, the last one zero-padded): ragged lengths (sub-chunk, chunk + a
    fraction, exactly one chunk, a sub-second clip) each against the oracle, and
    the stream path (MM_BATCH_STREAMS_ONLY) gives the same loudness."""
    import torch

    from mastering_amd import Job, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16
    lens = [int(3.2 * rate), int(31.7 * rate), 30 * rate, int(0.7 * rate), int(62.05 * rate)]
    pcms = [pink_noise_pcm16(n, rate, channels, 900 + t) for t, n in enumerate(lens)]
    kind = native.MM_IN_I16 if in_i16 else native.MM_IN_F32
    xs = [torch.from_numpy(p.copy() if in_i16 else p.astype(np.float32) / 32768).cuda() for p in pcms]
    jobs = [Job(n, rate, channels, params) for n in lens]
    for j in jobs:
        j.job.in_kind = kind
    ctx = native.context(0)

    def run():
        outs = [torch.full((j.frames_proc, channels), 12345, dtype=torch.int16, device="cuda") for j in jobs]
        res = master_batch(ctx, jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs])
        return [o.cpu().numpy() for o in outs], res

    outs, res = run()
    for t, pcm in enumerate(pcms):
        ref, L = oracle.master(pcm, rate, params, return_loudness=True)
        _check(outs[t].reshape(ref.shape), {"loudness": res[t].loudness}, ref, L)
    monkeypatch.setenv("MM_BATCH_STREAMS_ONLY", "1")
    outs2, res2 = run()
    for t in range(len(pcms)):
        if params.get("lufs") is not None:
            assert abs(res[t].loudness - res2[t].loudness) <= 1e-9
        assert rms_diff(outs[t], outs2[t]) <= RMS_TOL and np.mean(outs[t] == outs2[t]) >= 0.9999


def test_batch_mixed_settings_units(oracle):
    """A batch whose settings change along it: same-settings runs become fused units
    (split in two), a lone track stays a single chain, and every result lands in its
    own slot (each track against the oracle with its own settings)."""
    import torch

    from mastering_amd import Job, master_batch, native
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100
    plan = [(P_FULL, 4.1), (P_FULL, 31.0), (P_FULL, 2.2), (P_HOT, 3.3), (P_HOT, 5.0), (P_FULL, 1.5),
            (dict(P_FULL, lufs=None), 2.0)]
    pcms = [pink_noise_pcm16(int(s * rate), rate, 2, 700 + t) for t, (_, s) in enumerate(plan)]
    jobs = [Job(p.shape[0], rate, 2, st) for p, (st, _) in zip(pcms, plan)]
    xs = [torch.from_numpy(p.astype(np.float32) / 32768).cuda() for p in pcms]
    outs = [torch.empty((j.frames_proc, 2), dtype=torch.int16, device="cuda") for j in jobs]
    res = master_batch(native.context(0), jobs, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs])
    for t, (pcm, (st, _)) in enumerate(zip(pcms, plan)):
        ref, L = oracle.master(pcm, rate, st, return_loudness=True)
        assert res[t].frames_out == jobs[t].frames_proc
        _check(outs[t].cpu().numpy(), {"loudness": res[t].loudness}, ref, L)


def test_multiband_at_rate_without_25_frame_tiles(oracle):
    """44056 Hz: no tile length in [64, 512] that divides the 30 s chunk is a
    multiple of the walkers' 25-row load blocks (choose_tile picks 240): the
    M plane pads each tile to whole blocks with identity rows (round 3 refused
    this rate with multiband on)."""
    from mastering_amd import design, master_pcm
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44056
    assert design.choose_tile(30 * rate) % 25 != 0
    pcm = pink_noise_pcm16(40 * rate, rate, 2, 21)
    out, info = master_pcm(pcm, rate, P_HOT)
    ref, L = oracle.master(pcm, rate, P_HOT, return_loudness=True)
    _check(out, info, ref, L)


def test_sweep_queue_across_settings_on_one_context():
    """One context, jobs whose settings alternate (P_FULL, P_HOT, P_FULL) and a
    longer track: the sweep count a context learns from its last solve is reset
    when the compressor settings or the geometry change (comp_signature), and the
    output never depends on the context's history (the solve is exact for any
    number of queued sweeps): every job equals the same job on a fresh context.
    The jobs also exercise the control block's hand-over (round 6): each chain's last
    finalize block zeroes the block for the next one, whose fill is then skipped when
    it needs no more bytes (the 40 s jobs after the 70 s one), and the readback it
    hands over (loudness, active and re-walked counts) matches a fresh context's."""
    import ctypes

    from mastering_amd import Job, native
    from mastering_amd.engine import _device_input
    from mastering_amd.synth import pink_noise_pcm16
    rate = 44100

    def run(ctx, pcm, st):
        job = Job(pcm.shape[0], rate, 2, st)
        x, job.job.in_kind = _device_input(pcm)
        out = np.empty((job.frames_proc, 2), np.int16)
        res = native.MMResult()
        ctx.check(ctx.lib.mm_master(ctx.ptr, ctypes.byref(job.job), x.ctypes.data_as(ctypes.c_void_p),
                                    out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(res)), "mm_master")
        return out, res

    a = pink_noise_pcm16(40 * rate, rate, 2, 31)
    b = pink_noise_pcm16(70 * rate, rate, 2, 32)
    plan = [(a, P_FULL), (a, P_HOT), (a, P_FULL), (b, P_HOT), (a, P_HOT)]
    shared = native.Context(0)
    for pcm, st in plan:
        out, res = run(shared, pcm, st)
        fresh = native.Context(0)
        ref, rres = run(fresh, pcm, st)
        fresh.close()
        assert np.array_equal(out, ref)
        assert res.loudness == rres.loudness
        assert res.comp_iters == rres.comp_iters
        assert (res.comp_active, res.comp_walked, res.comp_jumped) == (rres.comp_active, rres.comp_walked,
                                                                      rres.comp_jumped)
    shared.close()


@pytest.mark.parametrize("name", ["full_4s.npz", "loud_sat100.npz", "mono_hot_2s.npz"])
def test_exciter_table_prepass(name, monkeypatch):
    """The exciter's other exact path: when the correction codes are incomplete (an
    entry more than one f32 step from numpy's value; MM_SAT_GATHER forces it) the
    full table is applied by a pointwise pre-pass (sat_pre_kernel) and the EQ runs
    with the exciter off: still bit-identical to the reference."""
    from mastering_amd import master_pcm
    monkeypatch.setenv("MM_SAT_GATHER", "1")
    d = np.load(os.path.join(GOLDEN, name))
    st = json.loads(str(d["settings"]))
    out, info = master_pcm(d["pcm"], int(d["rate"]), st)
    L = float(d["loudness"])
    _check(out, info, d["out"], None if np.isnan(L) else L, GOLDEN_EXACT)
