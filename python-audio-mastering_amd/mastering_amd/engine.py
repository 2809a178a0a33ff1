"""MI355X mastering engine — the drop-in for the reference's hot path.

Reference boundary: `process_audio_from_gcs(gcs_uri, settings)`
(worker/audio_mastering_engine.py:24, "AME"), whose DSP is AME:43-98.  Here the
same chain runs behind `process(input_path, output_path, params)` with local WAV
IO instead of GCS; `params` uses the worker's settings keys and defaults
(AME:58-86).  All per-sample work runs in hand-written HIP kernels
(libmastering_amd.so, include/mastering.h) — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os

import numpy as np

from . import design, native

# AME:15-20, verbatim values and descriptions.
EQ_PRESETS = {
    "techno": {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0,
               "description": "Boosted sub-bass and highs, scooped mids for a powerful club sound."},
    "dubstep": {"bass_boost": 5.0, "mid_cut": 4.0, "presence_boost": 2.0, "treble_boost": 3.5,
                "description": "Aggressive low-end and crisp highs, with a significant mid-cut."},
    "pop": {"bass_boost": 2.0, "mid_cut": 0.0, "presence_boost": 3.5, "treble_boost": 2.5,
            "description": "Focused on vocal clarity with a solid low-end and bright highs."},
    "rock": {"bass_boost": 1.5, "mid_cut": -2.0, "presence_boost": 2.5, "treble_boost": 1.0,
             "description": "Warm low-mids for guitars and punchy presence for snare/vocals."},
}

COMP_WARMUP = 0  # super-tiles of speculative warm-up walk before each one (none: the sweeps' jumps repair starts)
COMP_MAX_ITERS = 100000
# envelope solve unit: super-tiles of 4 tiles (900 frames at the default tile) at
# EVERY rate, the tile count the super-tile release records assume (SJ_TPS in
# csrc/compressor.hip).  Not scaled with the rate (comp_rms maps a wave to one tile
# position of 64 super-tiles, so its M stores are 512-byte runs at any length).
COMP_SUPER_FRAMES = 900


def comp_super_frames(rate: int, tile: int = design.DEFAULT_TILE) -> int:
    """Super-tile length in frames: COMP_SUPER_FRAMES / DEFAULT_TILE (4) whole tiles of
    the track's tile at every rate."""
    del rate  # (see COMP_SUPER_FRAMES)
    return max(1, int(round(COMP_SUPER_FRAMES / design.DEFAULT_TILE))) * tile


class Resampler:
    """The mm_resampler POD of a rate pair plus the taps it points to (design.resample_taps;
    ValueError for a pair outside the converter's limits)."""

    def __init__(self, rate_in: int, rate_out: int):
        self.L, self.M, self.K, self.taps = design.resample_taps(rate_in, rate_out)
        rs = native.MMResampler()
        rs.rate_in, rs.rate_out, rs.L, rs.M, rs.K = int(rate_in), int(rate_out), self.L, self.M, self.K
        rs.taps = self.taps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        rs.taps_key = design.resample_key(rate_in, rate_out)
        self.rs = rs

    def frames_out(self, frames: int) -> int:
        return design.resample_frames(frames, self.L, self.M)


# (master_pcm and process take the key off before they plan)
MATCH_REFUSAL = ("the reference match (params['match']) works on one whole delivered track, in master_pcm and process: "
                 "not available for a batch, an album, a time-sharded range or a staged job")


class Job:
    """A planned mastering job: the mm_job POD plus the host arrays it points to."""

    def __init__(self, frames_in: int, rate: int, channels: int, params: dict, out_kind: int = native.MM_OUT_I16,
                 seg_bounds=None, check_length: bool = True, single_chunk: bool = False,
                 crossover=(design.LOW_CROSSOVER, design.HIGH_CROSSOVER), report: bool = False,
                 ceiling_dbtp: float | None = None, output_rate: int | None = None, r128: bool = False,
                 deliver_lufs: float | None = None, qc: bool = False, spectrum: bool = False):
        """`seg_bounds` (time-sharded ranks, distributed.py): this range's loudness
        segment bounds relative to its first frame; the whole-track gating then
        happens on the host after the all-reduce.  `check_length=False` skips
        pyloudnorm's minimum-length check (it applies to the whole track).
        `single_chunk`: the whole input is ONE line (the per-stage operators of
        ops.py, which the reference calls on one chunk) instead of AME:48's 30 s
        chunks; `crossover`: apply_multiband_compressor's (low, high) Hz.  `report`:
        meter the delivered output at the end of the chain (mm_job.meter_on); its
        loudness is measured too whenever the track spans one 0.4 s block, with or
        without a LUFS target.  `ceiling_dbtp` (in [-24, 0]): hold the delivered output
        under this true-peak ceiling (mm_job.ceiling_q28, design.ceiling_q28) after the
        chain and before the report; not on a time-sharded range, whose rank does not
        hold its neighbours' frames.  `output_rate` (other than `rate`): plan a delivery
        at that rate (mm_delivery, self.delivery; run it with mm_deliver*): the chain
        runs at `rate`, its output is converted (design.resample_taps), and the ceiling
        (window design.ceiling_window(output_rate)) and the report act on the converted
        signal, so mm_job.ceiling_q28 and meter_on stay 0; None or `rate` itself plans
        exactly the job planned without it.  ValueError for a rate pair outside the
        converter's limits.  `r128`: the EBU R 128 report of the delivered output (bit 1 of
        meter_on, mm_last_r128; independent of `report`): kweight.sos is then filled whatever
        else is planned; with `output_rate` the bit moves to the delivery, as `report` does;
        not on a time-sharded range, whose rank does not hold the whole track.
        `deliver_lufs` (in [-40, -5]): level the delivered output to that EBU R 128 integrated
        loudness under the ceiling (mm_delivery.level_clu, design.level_clu; mm_level): it plans
        a delivery, with `output_rate` or without (then without a converter: self.resampler and
        self.output_rate stay None), to which the ceiling and the reports move, and the `loud`
        job with the sections of the delivered rate; not on a time-sharded range or a per-stage
        operator.  `qc`: the delivery QC report of the delivered output (bit 2 of meter_on,
        mm_last_qc; independent of `report` and `r128`); with a delivery the bit moves to it, as
        `r128` does; not on a time-sharded range, whose rank does not hold the whole track.
        `spectrum`: the spectrum report of the delivered output (bit 3 of meter_on, mm_last_spectrum;
        independent of the other three), placed and refused exactly as `qc`."""
        if deliver_lufs is not None and (seg_bounds is not None or single_chunk):
            raise ValueError("a loudness target (deliver_lufs) needs the whole chain: not available on a "
                             "time-sharded range or a per-stage operator")
        level = 0 if deliver_lufs is None else design.level_clu(deliver_lufs)
        self.deliver_lufs = None if deliver_lufs is None else level / 100.0
        if ceiling_dbtp is not None and seg_bounds is not None:
            raise ValueError("the true-peak ceiling needs the whole track: not available on a time-sharded range")
        if r128 and seg_bounds is not None:
            raise ValueError("the R 128 report needs the whole track: not available on a time-sharded range")
        if qc and seg_bounds is not None:
            raise ValueError("the QC report needs the whole track: not available on a time-sharded range")
        if spectrum and seg_bounds is not None:
            raise ValueError("the spectrum report needs the whole track: not available on a time-sharded range")
        if output_rate is not None and int(output_rate) == int(rate):
            output_rate = None
        if output_rate is not None and (seg_bounds is not None or single_chunk):
            raise ValueError("delivery at another rate needs the whole chain: not available on a time-sharded "
                             "range or a per-stage operator")
        self.output_rate = None if output_rate is None else int(output_rate)
        self.resampler = Resampler(rate, output_rate) if output_rate is not None else None
        delivers = output_rate is not None or level != 0
        plan_report, report = report, bool(report) and not delivers  # (a delivery's report is planned below)
        plan_r128, r128 = bool(r128), bool(r128) and not delivers
        plan_qc, qc = bool(qc), bool(qc) and not delivers
        plan_spectrum, spectrum = bool(spectrum), bool(spectrum) and not delivers
        if channels not in (1, 2):
            raise ValueError("only mono and stereo are supported (AME:119,137,152)")
        params = dict(params or {})
        if params.get("match") is not None:
            raise ValueError(MATCH_REFUSAL)
        self.params = params
        self.rate, self.channels, self.frames_in = int(rate), int(channels), int(frames_in)
        multiband = bool(params.get("multiband"))
        if single_chunk:
            bounds = [(0, self.frames_in)] if self.frames_in else []
            self.tile = design.OPS_TILE
            self.tiles_per_chunk = max(1, -(-self.frames_in // self.tile))
        else:
            bounds = design.chunk_bounds(self.frames_in, self.rate)
            nominal = design.pydub_frame(design.CHUNK_MS, self.rate)
            design.check_chunk_geometry(bounds, nominal, self.rate, multiband)
            # without the compressor the chain is the IIR stages alone, which want the
            # lanes of shorter tiles on a short track (C1: 0.139 ms at 125 against 0.188 at 225)
            self.tile = design.choose_tile(nominal, None if multiband else design.NOCOMP_TILE)
            self.tiles_per_chunk = nominal // self.tile
        self.chunks = bounds
        self.frames_proc = bounds[-1][1] if bounds else 0
        lufs = params.get("lufs")
        if check_length and lufs is not None and self.frames_proc < 0.4 * self.rate:
            # pyloudnorm util.valid_audio (AME:218)
            raise ValueError("Audio must have length greater than the block size.")

        j = native.MMJob()
        j.frames_in, j.frames_proc = self.frames_in, self.frames_proc
        j.channels, j.rate, j.tile, j.tiles_per_chunk = self.channels, self.rate, self.tile, self.tiles_per_chunk
        on, keep, mix, drive = design.saturation_consts(params.get("saturation", 0))
        j.sat_on, j.sat_keep, j.sat_mix, j.sat_drive = on, keep, mix, drive
        if on:  # the exciter on the int16 grid: numpy's own float32 values (design.saturation_table)
            self._sat_tab, j.sat_key = design.saturation_table(params.get("saturation", 0))
            j.sat_table = self._sat_tab.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        w = params.get("width", 1.0)
        j.width_on = int(w != 1.0 and self.channels == 2)
        j.width = float(w) if w is not None else 1.0
        j.multiband_on = int(multiband)
        j.lufs_on = int(lufs is not None)
        j.lufs_target = float(lufs) if lufs is not None else 0.0
        j.out_kind = out_kind
        G = -(-self.frames_proc // self.tile) if self.frames_proc else 0
        self.G = G
        tpb = design.LB_THREADS // self.channels  # stereo stages run lane pairs
        # --- EQ (1 branch)
        eq = design.eq_sections(self.rate, params)
        self._fill_iir(j.eq, eq, [len(eq)], self.tile, tpb)
        # --- crossover (2 branches of 2)
        if multiband:
            self._fill_iir(j.xover, design.crossover_sections(self.rate, *crossover), [2, 2], self.tile, tpb)
            self._tables = []
            for b in range(3):
                tk, td, rk, rd = design.BAND_DEFAULTS[b]
                at, rel = design.BAND_TIMES[b]
                bc = design.band_constants(self.rate, params.get(tk, td), params.get(rk, rd), at, rel)
                tab = np.ascontiguousarray(bc["lut"])
                self._tables.append(tab)
                jb = j.band[b]
                jb.thresh_rms, jb.attack_frames, jb.release_frames = bc["thresh_rms"], bc["attack_frames"], \
                    bc["release_frames"]
                jb.look = bc["look"]
                nz = np.flatnonzero(tab[:, 0])
                jb.r0 = int(nz[0]) if nz.size else 32769
                jb.lut = tab.ctypes.data_as(native.c_double_p)
                jb.lut_key = bc["lut_key"]
        j.comp_warmup = COMP_WARMUP
        j.comp_max_iters = COMP_MAX_ITERS
        j.comp_super = comp_super_frames(self.rate, self.tile)
        j.meter_on = ((native.REPORT_METER if report else 0) | (native.REPORT_R128 if r128 else 0)
                      | (native.REPORT_QC if qc else 0) | (native.REPORT_SPECTRUM if spectrum else 0))
        self.ceiling_dbtp = None if ceiling_dbtp is None else float(ceiling_dbtp)
        j.ceiling_q28 = 0 if ceiling_dbtp is None else design.ceiling_q28(ceiling_dbtp)
        # --- loudness (with `report` alone: the geometry only, for the meter; with `r128`
        # alone: the K-weighting sections only, for its own pass)
        loud_geometry = lufs is not None or (report and self.frames_proc >= 0.4 * self.rate)
        if loud_geometry or r128:
            self._fill_iir(j.kweight, design.kweight_sections(self.rate), [2],
                           self.tile // design.kweight_sub(self.tile), design.LB_THREADS)
        if loud_geometry:
            if seg_bounds is None:
                nb, lo, hi, segb, scale = design.loudness_blocks(self.frames_proc, self.rate)
            else:  # rank-local segments; blocks are gated over the whole track elsewhere
                segb = np.asarray(seg_bounds, dtype=np.int64)
                nb, lo, hi, scale = 1, np.zeros(1, np.int64), segb[-1:].copy(), 1.0 / (0.4 * self.rate)
            self._lo, self._hi, self._segb = (np.ascontiguousarray(lo), np.ascontiguousarray(hi),
                                              np.ascontiguousarray(segb))
            j.n_blocks = nb
            j.block_lo = self._lo.ctypes.data_as(native.c_int64_p)
            j.block_hi = self._hi.ctypes.data_as(native.c_int64_p)
            j.n_segs = len(segb) - 1
            j.seg_bounds = self._segb.ctypes.data_as(native.c_int64_p)
            j.block_scale = scale
        self.job = j
        self.frames_out, self.delivery = self.frames_proc, None
        if delivers:  # the ceiling and the report move behind the converter and the level
            d = native.MMDelivery()
            out_rate = self.rate
            if self.resampler is not None:
                self.frames_out = self.resampler.frames_out(self.frames_proc)
                d.rs = ctypes.pointer(self.resampler.rs)
                out_rate = self.output_rate
            d.ceiling_q28, j.ceiling_q28 = j.ceiling_q28, 0
            d.window = design.ceiling_window(out_rate)
            d.meter_on = ((native.REPORT_METER if plan_report else 0) | (native.REPORT_R128 if plan_r128 else 0)
                          | (native.REPORT_QC if plan_qc else 0) | (native.REPORT_SPECTRUM if plan_spectrum else 0))
            d.level_clu = level
            # the output's loudness, as meter_pcm plans it, and the sections of the output's rate for the
            # R 128 report and the level; the QC and spectrum reports read its rate alone
            if (plan_report and self.frames_out >= 0.4 * out_rate) or plan_r128 or level or plan_qc or plan_spectrum:
                self._loud = Job(self.frames_out, out_rate, self.channels, {}, single_chunk=True,
                                 report=bool(plan_report), r128=plan_r128 or bool(level))
                d.loud = ctypes.pointer(self._loud.job)
            self.delivery = d

    @staticmethod
    @functools.lru_cache(maxsize=32)
    def _tables(sections, branches, tile, tpb):
        A = design.transition_matrix(list(sections), list(branches))
        t = design.lookback_tables(A, tile, tpb)
        return (np.ascontiguousarray(t["tile_pow"].reshape(design.TILE_POW, -1)),
                np.ascontiguousarray(t["blk_pow"].reshape(design.BLK_POW, -1)))

    @classmethod
    def _fill_iir(cls, dst, sections, branches, tile, tpb):
        dst.nsec = len(sections)
        dst.nsec_branch0 = branches[0]
        dst.dim = 2 * len(sections)
        dst.tpb = tpb
        dst.tile = int(tile)
        for s, sec in enumerate(sections):
            for k in range(5):
                dst.sos[s][k] = float(sec[k])
        if not sections:
            return
        key = tuple(tuple(float(v) for v in sec) for sec in sections)
        tp, bp = cls._tables(key, tuple(branches), int(tile), int(tpb))
        ctypes.memmove(dst.phi_tile_pow, tp.ctypes.data, tp.nbytes)
        ctypes.memmove(dst.phi_blk_pow, bp.ctypes.data, bp.nbytes)


def _device_input(pcm: np.ndarray, wide: bool = False):
    """PCM as the library takes it: int16 stays int16 (decoded /32768 on the GPU,
    AME:117-121; half the PCIe bytes), float32 is taken as decoded PCM.  `wide` (the
    mastering chain only; the meter and the ceiling are defined on the int16 grid):
    int32 is 24- or 32-bit PCM left-justified, as wavio.read_wav returns it, decoded
    on the GPU as x = RN_f32(s) * 2^-31 (MM_IN_I32)."""
    if pcm.dtype == np.int16:
        return np.ascontiguousarray(pcm), native.MM_IN_I16
    if pcm.dtype == np.float32:
        return np.ascontiguousarray(pcm), native.MM_IN_F32
    if wide and pcm.dtype == np.int32:
        return np.ascontiguousarray(pcm), native.MM_IN_I32
    raise TypeError("PCM must be int16, float32 or (left-justified 24/32-bit) int32" if wide
                    else "PCM must be int16 or float32")


def _info(job: "Job", res: native.MMResult) -> dict:
    return {"loudness": res.loudness if job.job.lufs_on else None,
            "gain_db": (float(job.job.lufs_target) - res.loudness) if job.job.lufs_on else None,
            "gain_linear": res.gain_linear, "frames": job.frames_proc, "comp_iters": res.comp_iters,
            "comp_walked": res.comp_walked, "comp_jumped": res.comp_jumped, "comp_active": res.comp_active,
            "chunks": len(job.chunks), "tile": job.tile}


def _db(x: float) -> float:
    return 20.0 * math.log10(x) if x > 0 else -math.inf


def report_dict(m: native.MMMeter, lufs_target=None) -> dict:
    """An mm_meter as the report of `info["report"]`: per-channel lists of the sample
    peak (dBFS), the BS.1770-4 true peak (dBTP) and its frame, clipped samples and
    inter-sample overs, the raw integers they come from, and the loudness of the
    delivered output (None when it was not measured or the track is shorter than one
    0.4 s block).  No reference counterpart: the reference never measures its output."""
    ch = int(m.channels)
    sp = [int(m.sample_peak[c]) for c in range(ch)]
    tp = [int(m.true_peak_q28[c]) for c in range(ch)]
    loud = None if math.isnan(m.loudness) else float(m.loudness)
    rep = {"frames": int(m.frames), "channels": ch,
           "sample_peak": sp, "true_peak_q28": tp,
           "sample_peak_dbfs": [_db(v / 32768.0) for v in sp],
           "true_peak_dbtp": [_db(v / 2.0 ** 28) for v in tp],
           "true_peak_frame": [int(m.true_peak_frame[c]) for c in range(ch)],
           "clipped": [int(m.clipped[c]) for c in range(ch)],
           "overs": [int(m.overs[c]) for c in range(ch)],
           "max_true_peak_dbtp": _db(max(tp, default=0) / 2.0 ** 28),
           "output_loudness": loud}
    if lufs_target is not None and loud is not None:
        rep["loudness_error"] = loud - float(lufs_target)
    return rep


def _last(ctx: native.Context, fn_name: str, struct, cap: int) -> list:
    """The per-track structs of the context's last master call (mm_last_meters / mm_last_ceilings)."""
    arr = (struct * max(cap, 1))()
    n = ctx.check(getattr(ctx.lib, fn_name)(ctx.ptr, cap, arr), fn_name)
    return _last(ctx, fn_name, struct, n) if n > cap else list(arr[:n])


def meters(ctx: native.Context, cap: int = native.BATCH_STREAMS) -> list:
    """The mm_meter of every track of the context's last master call (mm_last_meters):
    one for master_device, one per job for master_batch.  RuntimeError if that call did
    not meter (no job had `report`)."""
    return _last(ctx, "mm_last_meters", native.MMMeter, cap)


def r128_dict(m: native.MMR128) -> dict:
    """An mm_r128 as `info["r128"]`: the EBU R 128 figures of the delivered output (None
    where the struct holds NaN: the signal is shorter than the 0.4 s or 3 s the figure
    needs).  `integrated_lufs` is what an ITU-R BS.1770 meter reads (every channel
    K-weighted, energies summed); report_dict's `output_loudness` is the reference's
    channel-mean measure, up to 3.01 LU lower.  No reference counterpart."""
    def val(x):
        return None if math.isnan(x) else float(x)
    return {"integrated_lufs": val(m.integrated), "momentary_max_lufs": val(m.momentary_max),
            "short_term_max_lufs": val(m.short_term_max), "lra_lu": val(m.lra), "lra_low_lufs": val(m.lra_low),
            "lra_high_lufs": val(m.lra_high), "relative_gate_lufs": val(m.relative_gate), "hops": int(m.hops),
            "lra_blocks": int(m.lra_blocks)}


def r128s(ctx: native.Context, cap: int = native.BATCH_STREAMS) -> list:
    """The mm_r128 of every track of the context's last master call (mm_last_r128): one for
    master_device, one per job for master_batch, in job order (frames 0 and NaN figures:
    that job did not ask).  RuntimeError if no job of that call had `r128`."""
    return _last(ctx, "mm_last_r128", native.MMR128, cap)


def kweight_sos(rate: int):
    """design.kweight_sections(rate) as the C-ABI's `const double sos[2][5]`."""
    sos = ((ctypes.c_double * 5) * 2)()
    for s, sec in enumerate(design.kweight_sections(rate)):
        for k in range(5):
            sos[s][k] = float(sec[k])
    return sos


def r128_pcm(pcm: np.ndarray, rate: int, device: int = 0) -> dict:
    """The EBU R 128 report (r128_dict) of an int16 (or float32 = int16 / 32768) array [N]
    or [N, ch] without mastering it (mm_r128_pcm)."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    ctx = native.context(device)
    m = native.MMR128()
    ctx.check(ctx.lib.mm_r128_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, x.shape[0], ch, int(rate),
                                  kweight_sos(rate), ctypes.byref(m)), "mm_r128_pcm")
    return r128_dict(m)


def _ratio_db(num: int, den: int) -> float | None:
    """10 log10(num / den) of two non-negative integers (None for 0 / 0, -inf for 0 / den)."""
    if den == 0:
        return None
    return 10.0 * math.log10(num / den) if num > 0 else -math.inf


def qc_dict(m: native.MMQc) -> dict:
    """An mm_qc as `info["qc"]`: the struct's integers (per-channel figures as lists) and what
    derives from them.  `dc_offset` (of full scale); `correlation` (overall phase correlation,
    None for mono or a silent channel) and `corr_min` (the lowest of a gated 400 ms window, None
    without one) at `corr_min_seconds`; `mono_fold_db`, the level of (L + R) / 2 against the
    channel mean, and `side_mid_db`, side against mid (None for mono or silence);
    `dual_mono` (L == R everywhere); `effective_bits` (16 minus the zero low bits all samples
    share; 0 for digital zero); lead, trail and longest silence in seconds; `dropout` = (at,
    len) of the longest silent run if it touches neither end, else None.  No verdicts:
    thresholds are the caller's.  No reference counterpart."""
    ch, N, rate = int(m.channels), int(m.frames), int(m.rate)
    d = {f: int(getattr(m, f)) for f in ("frames", "channels", "rate", "hops", "silence_lsb", "min_run", "cross",
                                         "lead_silence", "trail_silence", "silent_frames", "silence_longest",
                                         "silence_longest_at", "corr_windows", "corr_negative", "corr_min_hop")}
    for f in ("sum", "sq", "smin", "smax", "or_bits", "clip_samples", "clip_runs", "clip_longest", "clip_longest_at"):
        d[f] = [int(getattr(m, f)[c]) for c in range(ch)]
    d["corr_min"] = None if math.isnan(m.corr_min) else float(m.corr_min)
    d["corr_min_seconds"] = None if d["corr_min_hop"] < 0 else (d["corr_min_hop"] * rate // 10) / rate
    d["dc_offset"] = [s / N / 32768.0 if N else 0.0 for s in d["sum"]]
    d["effective_bits"] = [16 - ((b & -b).bit_length() - 1) if b else 0 for b in d["or_bits"]]
    d["correlation"] = d["mono_fold_db"] = d["side_mid_db"] = None
    d["dual_mono"] = False
    if ch == 2:
        sq0, sq1, x = d["sq"][0], d["sq"][1], d["cross"]
        if sq0 and sq1:
            d["correlation"] = x / math.sqrt(sq0 * sq1)
        d["mono_fold_db"] = _ratio_db(sq0 + sq1 + 2 * x, 2 * (sq0 + sq1))
        d["side_mid_db"] = _ratio_db(sq0 + sq1 - 2 * x, sq0 + sq1 + 2 * x)
        d["dual_mono"] = sq0 + sq1 - 2 * x == 0
    sec = (lambda n: n / rate) if rate else (lambda n: 0.0)
    d["lead_silence_seconds"], d["trail_silence_seconds"] = sec(d["lead_silence"]), sec(d["trail_silence"])
    d["silence_longest_seconds"] = sec(d["silence_longest"])
    at, ln = d["silence_longest_at"], d["silence_longest"]
    d["dropout"] = (at, ln) if at > 0 and at + ln < N else None
    return d


def qcs(ctx: native.Context, cap: int = native.BATCH_STREAMS) -> list:
    """The mm_qc of every track of the context's last master call or QC batch (mm_last_qc), in
    job order (frames 0: that job did not ask).  RuntimeError if that call made none."""
    return _last(ctx, "mm_last_qc", native.MMQc, cap)


def qc_pcm(pcm: np.ndarray, rate: int, silence_lsb: int = 1, min_run: int = 3, curve: bool = False, device: int = 0):
    """The delivery QC report (qc_dict) of an int16 (or float32 = int16 / 32768) array [N] or
    [N, ch] without mastering it (mm_qc_pcm).  A frame is silent when every channel lies within
    `silence_lsb` of zero; a clip run counts from `min_run` consecutive full-scale samples.
    `curve=True` returns (qc_dict, the [H, 3] int64 hop table of sum L^2, sum R^2, sum L R a
    100 ms hop), from which the correlation over time can be plotted."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    ctx = native.context(device)
    m = native.MMQc()
    table = np.zeros((10 * x.shape[0] // int(rate) if int(rate) > 0 else 0, 3), np.int64) if curve else None
    ctx.check(ctx.lib.mm_qc_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, x.shape[0], ch, int(rate),
                                int(silence_lsb), int(min_run), ctypes.byref(m),
                                table.ctypes.data_as(native.c_int64_p) if curve else None), "mm_qc_pcm")
    return (qc_dict(m), table) if curve else qc_dict(m)


def qc_batch_pcm(tracks, rate: int, silence_lsb: int = 1, min_run: int = 3, device: int = 0) -> list:
    """The delivery QC reports ([qc_dict ...]) of the tracks of a batch (int16 or float32 = int16
    / 32768 arrays [N] or [N, ch], one rate, channel count and sample type) without mastering
    them (mm_batch_qc_pcm: one memset, two launches and one read-back whatever their number).
    Every track receives what qc_pcm gives on it alone."""
    xs, kind, ch, frames = _album_tracks(tracks, "a batch")
    n = len(xs)
    ctx = native.context(device)
    out = (native.MMQc * n)()
    ctx.check(ctx.lib.mm_batch_qc_pcm(ctx.ptr, _pointers([x.ctypes.data for x in xs]), kind, frames, n, ch, int(rate),
                                      int(silence_lsb), int(min_run), out), "mm_batch_qc_pcm")
    return [qc_dict(m) for m in out]


def _batch_qc(ctx: native.Context, d_outs, kind: int, frames, ch: int, rate: int) -> list:
    """The QC reports of the delivered buffers of a batch or album call, after its level (one
    mm_batch_qc_device call at the delivered rate, with a master call's parameters)."""
    n = len(d_outs)
    out = (native.MMQc * n)()
    ctx.check(ctx.lib.mm_batch_qc_device(ctx.ptr, _pointers(d_outs), kind, frames, n, ch, int(rate), 1, 3, out),
              "mm_batch_qc_device")
    return [qc_dict(m) for m in out]


def spectrum_bands(rate: int) -> np.ndarray:
    """The 1/3-octave bands of the spectrum report at `rate` (mm_spectrum_bands; no GPU): an
    [n_bands, 3] float64 array of lower edge, centre and upper edge in Hz, from the 20 Hz band to
    the band that rate / 2 clips."""
    lib = native.load()
    edges = np.zeros((native.SPECTRUM_MAX_BANDS, 3), np.float64)
    n = lib.mm_spectrum_bands(int(rate), native.SPECTRUM_MAX_BANDS, edges.ctypes.data_as(native.c_double_p))
    if n < 0:
        raise ValueError(f"mm_spectrum_bands failed ({n}): rate below 2000 Hz")
    return edges[:n].copy()


def occupied_hz(bins: np.ndarray, rate: int, threshold_db: float) -> float | None:
    """The frequency of the highest bin of a spectrum report's bin table whose level, 10 log10(16 S
    / N^2) with S summed over the channels (0 dB: a full-scale sine on that bin), reaches
    `threshold_db`; None if no bin does (or the table is NaN)."""
    N = native.SPECTRUM_N
    power = 16.0 * (bins[:, 0] + bins[:, 1]) / (N * N)
    with np.errstate(invalid="ignore"):
        hit = np.flatnonzero(power >= 10.0 ** (threshold_db / 10.0))
    return float(hit[-1]) * rate / N if hit.size else None


def spectrum_dict(m: native.MMSpectrum, bands: np.ndarray, bins: np.ndarray) -> dict:
    """An mm_spectrum, its band table [n_bands, 4] (ms L, ms R, ms C, bins_in_band) and its bin
    table [N/2 + 1, 3] as `info["spectrum"]`: the struct's integers, `total_dbfs` a channel, and
    under "bands" one dict a band with `centre_hz`, `lo_hz`, `hi_hz`, `bins_in_band`, `level_dbfs` (a
    list a channel: 10 log10(2 ms), 0 for a full-scale sine), and for stereo `correlation` (C_b /
    sqrt(L_b R_b), None where a channel is silent), `mid_dbfs` and `side_dbfs` (of (L + R ± 2 C) /
    4).  Overall: `rolloff_hz` (keys "95", "99", "99.9": the lowest bin frequency below and at which
    that share of the power of all channels lies) and `occupied_hz` (keys "-60", "-90":
    occupied_hz at those thresholds).  An unmeasurable signal (n_frames 0) has None throughout.
    Figures, not verdicts.  No reference counterpart."""
    ch, rate = int(m.channels), int(m.rate)
    d = {f: int(getattr(m, f)) for f in ("frames", "channels", "rate", "n_fft", "hop", "n_frames", "n_bands")}
    measured = d["n_frames"] > 0

    def db(ms):
        if not measured or math.isnan(ms):
            return None
        return 10.0 * math.log10(2.0 * ms) if ms > 0 else -math.inf

    d["total_ms"] = [float(m.total_ms[c]) if measured else None for c in range(ch)]
    d["total_dbfs"] = [db(float(m.total_ms[c])) for c in range(ch)]
    d["bands"] = []
    for (lo, centre, hi), (L, R, C, width) in zip(spectrum_bands(rate) if rate else (), bands):
        b = {"centre_hz": float(centre), "lo_hz": float(lo), "hi_hz": float(hi), "bins_in_band": float(width),
             "ms": [float(v) if measured else None for v in (L, R)[:ch]],
             "level_dbfs": [db(float(v)) for v in (L, R)[:ch]]}
        if ch == 2:
            b["cross_ms"] = float(C) if measured else None
            b["correlation"] = float(C / math.sqrt(L * R)) if measured and L > 0 and R > 0 else None
            b["mid_dbfs"] = db(max(0.0, float(L + R + 2 * C) / 4.0))
            b["side_dbfs"] = db(max(0.0, float(L + R - 2 * C) / 4.0))
        d["bands"].append(b)
    d["rolloff_hz"] = {"95": None, "99": None, "99.9": None}
    d["occupied_hz"] = {"-60": None, "-90": None}
    if measured:
        N = native.SPECTRUM_N
        weight = np.full(native.SPECTRUM_BINS, 2.0)
        weight[0] = weight[-1] = 1.0
        cum = np.cumsum(weight * (bins[:, 0] + bins[:, 1]))
        if cum[-1] > 0:
            for key in d["rolloff_hz"]:
                k = int(np.searchsorted(cum, float(key) / 100.0 * cum[-1], side="left"))
                d["rolloff_hz"][key] = min(k, N // 2) * rate / N
        for key in d["occupied_hz"]:
            d["occupied_hz"][key] = occupied_hz(bins, rate, float(key))
    return d


def _spectrum_of(m: native.MMSpectrum, bins: np.ndarray) -> dict:
    """spectrum_dict of a struct and its bin table, the bands by the tail the library ends in."""
    bands = np.zeros((native.SPECTRUM_MAX_BANDS, 4), np.float64)
    if m.rate:  # (a job of a batch that did not ask: a cleared struct)
        rc = native.load().mm_spectrum_from_bins(bins.ctypes.data_as(native.c_double_p), m.frames, m.channels, m.rate,
                                                 ctypes.byref(native.MMSpectrum()), bands.ctypes.data_as(native.c_double_p))
        if rc < 0:
            raise ValueError(f"mm_spectrum_from_bins failed ({rc})")
    return spectrum_dict(m, bands[:m.n_bands], bins)


def spectra(ctx: native.Context, cap: int = native.BATCH_STREAMS) -> list:
    """The mm_spectrum of every track of the context's last master call or spectrum batch
    (mm_last_spectrum), in job order (frames 0: that job did not ask).  RuntimeError if that call
    made none."""
    return _last(ctx, "mm_last_spectrum", native.MMSpectrum, cap)


def spectrum_bins(ctx: native.Context, track: int = 0) -> np.ndarray:
    """The bin table [N/2 + 1, 3] float64 (S_L, S_R, C) of track `track` of those reports
    (mm_last_spectrum_bins)."""
    bins = np.zeros((native.SPECTRUM_BINS, 3), np.float64)
    ctx.check(ctx.lib.mm_last_spectrum_bins(ctx.ptr, int(track), native.SPECTRUM_BINS, bins.ctypes.data_as(native.c_double_p)),
              "mm_last_spectrum_bins")
    return bins


def _last_spectra(ctx: native.Context, n: int, curve: bool = False) -> list:
    """[spectrum_dict ...] (with `curve`: [(spectrum_dict, bin table) ...]) of the context's last reports."""
    out = []
    for t, m in enumerate(spectra(ctx, n)):
        bins = spectrum_bins(ctx, t)
        out.append((_spectrum_of(m, bins), bins) if curve else _spectrum_of(m, bins))
    return out


def spectrum_pcm(pcm: np.ndarray, rate: int, curve: bool = False, device: int = 0):
    """The spectrum report (spectrum_dict) of an int16 (or float32 = int16 / 32768) array [N] or
    [N, ch] without mastering it (mm_spectrum_pcm).  `curve=True` returns (spectrum_dict, the
    [N/2 + 1, 3] float64 bin table of S_L, S_R and C)."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    ctx = native.context(device)
    m = native.MMSpectrum()
    bins = np.zeros((native.SPECTRUM_BINS, 3), np.float64)
    bands = np.zeros((native.SPECTRUM_MAX_BANDS, 4), np.float64)
    ctx.check(ctx.lib.mm_spectrum_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, x.shape[0], ch, int(rate),
                                      ctypes.byref(m), bands.ctypes.data_as(native.c_double_p),
                                      bins.ctypes.data_as(native.c_double_p)), "mm_spectrum_pcm")
    d = spectrum_dict(m, bands[:m.n_bands], bins)
    return (d, bins) if curve else d


def spectrum_batch_pcm(tracks, rate: int, curve: bool = False, device: int = 0) -> list:
    """The spectrum reports ([spectrum_dict ...]; with `curve` [(spectrum_dict, bin table) ...]) of
    the tracks of a batch (int16 or float32 = int16 / 32768 arrays [N] or [N, ch], one rate, channel
    count and sample type) without mastering them (mm_batch_spectrum_pcm: two launches and one
    read-back whatever their number).  Every track receives what spectrum_pcm gives on it alone,
    bit for bit."""
    xs, kind, ch, frames = _album_tracks(tracks, "a batch")
    n = len(xs)
    ctx = native.context(device)
    out = (native.MMSpectrum * n)()
    ctx.check(ctx.lib.mm_batch_spectrum_pcm(ctx.ptr, _pointers([x.ctypes.data for x in xs]), kind, frames, n, ch, int(rate),
                                            out), "mm_batch_spectrum_pcm")
    return _last_spectra(ctx, n, curve)


def _batch_spectrum(ctx: native.Context, d_outs, kind: int, frames, ch: int, rate: int, curve: bool = False) -> list:
    """The spectrum reports of the delivered buffers of a batch or album call, after its level (one
    mm_batch_spectrum_device call at the delivered rate)."""
    n = len(d_outs)
    out = (native.MMSpectrum * n)()
    ctx.check(ctx.lib.mm_batch_spectrum_device(ctx.ptr, _pointers(d_outs), kind, frames, n, ch, int(rate), out),
              "mm_batch_spectrum_device")
    return _last_spectra(ctx, n, curve)


def ceiling_dict(m: native.MMCeiling) -> dict:
    """An mm_ceiling as `info["ceiling"]`: the struct's integers, the ceiling and the linked
    true peak before and after in dBTP, the largest gain reduction in dB (limiter and
    trim together) and whether the static trim ran.  No reference counterpart."""
    d = {f: int(getattr(m, f)) for f, _ in native.MMCeiling._fields_}
    d["ceiling_dbtp"] = _db(d["ceiling_q28"] / 2.0 ** 28)
    d["tp_in_dbtp"] = _db(d["tp_in_q28"] / 2.0 ** 28)
    d["tp_out_dbtp"] = _db(d["tp_out_q28"] / 2.0 ** 28)
    d["max_reduction_db"] = -_db(d["min_gain_q16"] / 65536.0) - _db(d["trim_q16"] / 65536.0)
    d["trimmed"] = d["trim_q16"] != 65536
    return d


def ceilings(ctx: native.Context, cap: int = native.BATCH_STREAMS) -> list:
    """The mm_ceiling of every track of the context's last master call (mm_last_ceilings):
    one for master_device, one per job for master_batch, in job order (frames 0: that
    job set none).  RuntimeError if no job of that call had `ceiling_dbtp`."""
    return _last(ctx, "mm_last_ceilings", native.MMCeiling, cap)


def level_dict(m: native.MMLevel) -> dict:
    """An mm_level as `info["level"]`: the struct's integers, the status as a word
    (native.LEVEL_STATUS), the target, the source's and the delivered loudness in LUFS (None
    where the struct holds NaN or -inf: unmeasurable), the delivered gain and the limiter's
    largest reduction in dB, and the per-pass gains (dB) and loudness cut to `passes`.
    No reference counterpart."""
    def val(x):
        return float(x) if math.isfinite(x) else None
    n = int(m.passes)
    d = {f: int(getattr(m, f)) for f in ("frames", "channels", "rate", "target_clu", "ceiling_q28", "window", "passes",
                                         "gain_q16", "min_gain_q16", "clipped", "limited_frames")}
    d["status"] = native.LEVEL_STATUS[int(m.status)]
    d["target_lufs"] = d["target_clu"] / 100.0
    d["source_lufs"], d["loudness"] = val(m.source_lufs), val(m.loudness)
    d["gain_db"] = _db(d["gain_q16"] / 65536.0)
    d["max_reduction_db"] = -_db(d["min_gain_q16"] / 65536.0)
    d["pass_gain_q16"] = [int(m.pass_gain_q16[k]) for k in range(n)]
    d["pass_gain_db"] = [_db(g / 65536.0) for g in d["pass_gain_q16"]]
    d["pass_lufs"] = [val(m.pass_lufs[k]) for k in range(n)]
    return d


def levels(ctx: native.Context, cap: int = 1) -> list:
    """The mm_level of the context's last master call (mm_last_levels): one for a call planned
    with `deliver_lufs`.  RuntimeError if that call set no loudness target."""
    return _last(ctx, "mm_last_levels", native.MMLevel, cap)


def level_pcm(pcm: np.ndarray, rate: int, target_lufs: float, ceiling_dbtp: float | None = None,
              window: int | None = None, device: int = 0):
    """Level an int16 (or float32 = int16 / 32768) array [N] or [N, ch] to `target_lufs` (EBU
    R 128 integrated, in [-40, -5]) under the true-peak ceiling `ceiling_dbtp` (None: no
    ceiling, the gain is then capped where a sample would clip) without mastering it
    (mm_level_pcm): returns (a new array, level_dict).  `window`: the ceiling's look-ahead
    frames (default design.ceiling_window(rate))."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    x = x.copy()
    C = 0 if ceiling_dbtp is None else design.ceiling_q28(ceiling_dbtp)
    w = design.ceiling_window(rate) if window is None else int(window)
    ctx = native.context(device)
    m = native.MMLevel()
    ctx.check(ctx.lib.mm_level_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, x.shape[0], ch, int(rate),
                                   kweight_sos(rate), design.level_clu(target_lufs), C, w, ctypes.byref(m), None),
              "mm_level_pcm")
    return x, level_dict(m)


def _album_tracks(tracks, what: str = "an album"):
    """The tracks of an album (or of `what`) as the album entries take them: (arrays, kind,
    channels, frames as a c_int64 array).  ValueError for what is not an album: no track or
    more than native.ALBUM_TRACKS, or tracks that differ in channel count or sample type."""
    tracks = list(tracks)
    if not 1 <= len(tracks) <= native.ALBUM_TRACKS:
        raise ValueError(f"{what} has 1 to {native.ALBUM_TRACKS} tracks, not {len(tracks)}")
    xs, kinds, chs = [], set(), set()
    for t in tracks:
        x, kind = _out_kind(np.asarray(t))
        xs.append(x)
        kinds.add(kind)
        chs.add(1 if x.ndim == 1 else x.shape[1])
    if len(chs) != 1:
        raise ValueError(f"the tracks of {what} must have one channel count")
    if len(kinds) != 1:
        raise ValueError(f"the tracks of {what} must have one sample type (all int16 or all float32)")
    frames = (ctypes.c_int64 * len(xs))(*[x.shape[0] for x in xs])
    return xs, kinds.pop(), chs.pop(), frames


def _pointers(addresses):
    return (ctypes.c_void_p * len(addresses))(*[ctypes.c_void_p(int(a)) for a in addresses])


def _album_dict(ctx: native.Context, n: int, ceiling: bool) -> dict:
    """The result of the context's last album level (mm_last_album): level_dict's fields, the
    album's r128_dict under "r128" and, under "tracks", one dict a track with its own "r128"
    and, when a ceiling was set, "ceiling"."""
    lv, alb = native.MMLevel(), native.MMR128()
    ctx.check(ctx.lib.mm_last_album(ctx.ptr, ctypes.byref(lv), ctypes.byref(alb)), "mm_last_album")
    d = level_dict(lv)
    d["r128"] = r128_dict(alb)
    d["tracks"] = [{"r128": r128_dict(r)} for r in r128s(ctx, n)]
    if ceiling:
        for t, ce in zip(d["tracks"], ceilings(ctx, n)):
            t["ceiling"] = ceiling_dict(ce)
    return d


def album_r128_pcm(tracks, rate: int, device: int = 0) -> dict:
    """The album EBU R 128 report (r128_dict) of int16 (or float32 = int16 / 32768) arrays [N]
    or [N, ch], measured as one programme whose gating blocks never span two tracks
    (mm_album_r128_pcm: one K-weighting launch for all tracks).  `r128s(ctx)` then holds the
    per-track reports."""
    xs, kind, ch, frames = _album_tracks(tracks)
    ctx = native.context(device)
    m = native.MMR128()
    ctx.check(ctx.lib.mm_album_r128_pcm(ctx.ptr, _pointers([x.ctypes.data for x in xs]), kind, frames, len(xs), ch,
                                        int(rate), kweight_sos(rate), ctypes.byref(m)), "mm_album_r128_pcm")
    return r128_dict(m)


def album_level_pcm(tracks, rate: int, target_lufs: float, ceiling_dbtp: float | None = None,
                    window: int | None = None, device: int = 0):
    """Level the tracks of an album (int16 or float32 = int16 / 32768 arrays [N] or [N, ch], one
    rate, channel count and sample type) by ONE static gain, so that the album measured as one
    programme reads `target_lufs` with every track under `ceiling_dbtp` (None: no ceiling, the
    gain is capped where a sample of any track would clip): mm_album_level_pcm.  Returns (new
    arrays, album dict): level_dict's fields plus "r128" (the album's r128_dict) and "tracks"
    (per track "r128" and, with a ceiling, "ceiling")."""
    xs, kind, ch, frames = _album_tracks(tracks)
    xs = [x.copy() for x in xs]
    C = 0 if ceiling_dbtp is None else design.ceiling_q28(ceiling_dbtp)
    w = design.ceiling_window(rate) if window is None else int(window)
    clu = design.level_clu(target_lufs)
    ctx = native.context(device)
    ctx.check(ctx.lib.mm_album_level_pcm(ctx.ptr, _pointers([x.ctypes.data for x in xs]), kind, frames, len(xs), ch,
                                         int(rate), kweight_sos(rate), clu, C, w), "mm_album_level_pcm")
    return xs, _album_dict(ctx, len(xs), bool(C))


def _per_track(value, n: int, what: str) -> list:
    """A scalar, or one value per track, as a list of n.  ValueError for a sequence of another length."""
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != n:
            raise ValueError(f"{what}: {len(value)} values for {n} tracks")
        return list(value)
    return [value] * n


def _batch_targets(n: int, target_lufs, ceiling_dbtp, name: str = "target_lufs"):
    """Per-track targets and ceilings as the batch level takes them: (level_clu, ceiling_q28) as
    c_int32 arrays (a ceiling of None: 0, no ceiling for that track)."""
    clu = [design.level_clu(v) for v in _per_track(target_lufs, n, name)]
    C = [0 if v is None else design.ceiling_q28(v) for v in _per_track(ceiling_dbtp, n, "ceiling_dbtp")]
    return (ctypes.c_int32 * n)(*clu), (ctypes.c_int32 * n)(*C)


def _batch_dicts(ctx: native.Context, C) -> list:
    """The results of the context's last batch level: one level_dict a track with its "r128"
    (r128_dict of the delivered samples) and, where that track has a ceiling, "ceiling"."""
    n = len(C)
    out = [level_dict(m) for m in levels(ctx, n)]
    for d, r in zip(out, r128s(ctx, n)):
        d["r128"] = r128_dict(r)
    if any(C):
        for d, q, ce in zip(out, C, ceilings(ctx, n)):
            if q:
                d["ceiling"] = ceiling_dict(ce)
    return out


def ceiling_batch_pcm(tracks, rate: int, ceiling_dbtp, window: int | None = None, device: int = 0):
    """Hold the tracks of a batch (int16 or float32 = int16 / 32768 arrays [N] or [N, ch], one
    channel count and sample type) under their true-peak ceilings, `ceiling_dbtp` a scalar or one
    value per track, without mastering them (mm_batch_ceiling_pcm: the ceiling's launches each
    cover all tracks).  Every track receives what ceiling_pcm gives on it alone.  Returns (new
    arrays, [ceiling_dict ...])."""
    xs, kind, ch, frames = _album_tracks(tracks, "a batch")
    n = len(xs)
    C = (ctypes.c_int32 * n)(*[design.ceiling_q28(v) for v in _per_track(ceiling_dbtp, n, "ceiling_dbtp")])
    xs = [x.copy() for x in xs]
    w = design.ceiling_window(rate) if window is None else int(window)
    ctx = native.context(device)
    out = (native.MMCeiling * n)()
    ctx.check(ctx.lib.mm_batch_ceiling_pcm(ctx.ptr, _pointers([x.ctypes.data for x in xs]), kind, frames, n, ch, C, w, out),
              "mm_batch_ceiling_pcm")
    return xs, [ceiling_dict(m) for m in out]


def level_batch_pcm(tracks, rate: int, target_lufs, ceiling_dbtp=None, window: int | None = None, device: int = 0):
    """Level the tracks of a batch (int16 or float32 = int16 / 32768 arrays [N] or [N, ch], one
    rate, channel count and sample type), every track to its OWN `target_lufs` under its own
    `ceiling_dbtp` (each a scalar or one value per track; a ceiling of None: none for that track):
    mm_batch_level_pcm.  Every track receives what level_pcm gives on it alone, bit for bit; the
    passes of all tracks run in lockstep, every launch over all tracks.  Returns (new arrays,
    [level_dict ...]), each dict with "r128" (the delivered samples' r128_dict) and, where that
    track has a ceiling, "ceiling"."""
    xs, kind, ch, frames = _album_tracks(tracks, "a batch")
    n = len(xs)
    clu, C = _batch_targets(n, target_lufs, ceiling_dbtp)
    xs = [x.copy() for x in xs]
    w = design.ceiling_window(rate) if window is None else int(window)
    ctx = native.context(device)
    ctx.check(ctx.lib.mm_batch_level_pcm(ctx.ptr, _pointers([x.ctypes.data for x in xs]), kind, frames, n, ch, int(rate),
                                         kweight_sos(rate), clu, C, w), "mm_batch_level_pcm")
    return xs, _batch_dicts(ctx, list(C))


def resample_dict(m: native.MMResample) -> dict:
    """An mm_resample as `info["resample"]`: the struct's integers (clipped and peak as
    per-channel lists) and the largest delivered sample in dBFS.  No reference counterpart."""
    ch = int(m.channels)
    d = {f: int(getattr(m, f)) for f in ("frames_in", "frames_out", "channels", "rate_in", "rate_out", "L", "M", "K")}
    d["clipped"] = [int(m.clipped[c]) for c in range(ch)]
    d["peak"] = [int(m.peak[c]) for c in range(ch)]
    d["peak_dbfs"] = _db(max(d["peak"], default=0) / 32768.0)
    return d


def _finish_info(info: dict, job: "Job", ctx: native.Context) -> dict:
    """The chain's info with what the end of the master call added: the level, the ceiling
    and the report of the delivered signal and, for a delivery at another rate, the
    delivered frames and rate and the converter's statistics."""
    end = job.job if job.delivery is None else job.delivery  # who carries ceiling_q28 and meter_on
    if job.delivery is not None and job.delivery.level_clu:
        info["level"] = level_dict(levels(ctx, 1)[0])
    if job.resampler is not None:
        m = native.MMResample()
        ctx.check(ctx.lib.mm_last_resample(ctx.ptr, ctypes.byref(m)), "mm_last_resample")
        info["frames"], info["rate"], info["resample"] = job.frames_out, job.output_rate, resample_dict(m)
    if end.ceiling_q28:
        info["ceiling"] = ceiling_dict(ceilings(ctx, 1)[0])
    if end.meter_on & native.REPORT_METER:
        info["report"] = report_dict(meters(ctx, 1)[0], job.job.lufs_target if job.job.lufs_on else None)
    if end.meter_on & native.REPORT_R128:
        info["r128"] = r128_dict(r128s(ctx, 1)[0])
    if end.meter_on & native.REPORT_QC:
        info["qc"] = qc_dict(qcs(ctx, 1)[0])
    if end.meter_on & native.REPORT_SPECTRUM:
        info["spectrum"] = _last_spectra(ctx, 1)[0]
    return info


def _out_kind(pcm: np.ndarray):
    """An int16 or float32 array as the stages on the delivered signal take it: (array, kind)."""
    x, in_kind = _device_input(pcm)
    return x, native.MM_OUT_I16 if in_kind == native.MM_IN_I16 else native.MM_OUT_F32


def resample_pcm(pcm: np.ndarray, rate_in: int, rate_out: int, device: int = 0):
    """Convert an int16 (or float32 = int16 / 32768) array [N] or [N, ch] to another
    sample rate without mastering it (mm_resample_pcm): returns (a new array of
    ceil(N * L / M) frames, resample_dict).  ValueError for a rate pair outside the
    converter's limits (design.resample_geometry)."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    rs = Resampler(rate_in, rate_out)
    n_out = rs.frames_out(x.shape[0])
    out = np.empty((n_out,) if pcm.ndim == 1 else (n_out, ch), x.dtype)
    ctx = native.context(device)
    m = native.MMResample()
    ctx.check(ctx.lib.mm_resample_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, x.shape[0], ch,
                                      ctypes.byref(rs.rs), out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(m)),
              "mm_resample_pcm")
    return out, resample_dict(m)


def resample_batch_pcm(tracks, rate_in: int, rate_out: int, device: int = 0):
    """Convert the tracks of a batch (int16 or float32 = int16 / 32768 arrays [N] or [N, ch], one
    channel count and sample type) to another sample rate without mastering them
    (mm_batch_resample_pcm: ONE converter launch covers all tracks).  Every track receives what
    resample_pcm gives on it alone, samples and statistics; a track without frames is valid.
    Returns (new arrays, [resample_dict ...]).  ValueError for a rate pair outside the
    converter's limits (design.resample_geometry)."""
    xs, kind, ch, frames = _album_tracks(tracks, "a batch")
    n = len(xs)
    rs = Resampler(rate_in, rate_out)
    outs = [np.empty((rs.frames_out(x.shape[0]),) + x.shape[1:], x.dtype) for x in xs]
    ctx = native.context(device)
    ms = (native.MMResample * n)()
    ctx.check(ctx.lib.mm_batch_resample_pcm(ctx.ptr, _pointers([x.ctypes.data for x in xs]), kind, frames, n, ch,
                                            ctypes.byref(rs.rs), _pointers([o.ctypes.data for o in outs]), ms),
              "mm_batch_resample_pcm")
    return outs, [resample_dict(m) for m in ms]


class Fir:
    """The mm_fir POD of a table of taps plus the array it points to.  `key`: the content key the
    context caches the device copy under (default design.match_key(taps); 0: no key, the table
    is checked and uploaded on every call)."""

    def __init__(self, taps, rate: int, key: int | None = None):
        self.taps = np.ascontiguousarray(taps, dtype=np.int32)
        f = native.MMFir()
        f.rate, f.K = int(rate), int(self.taps.size)
        f.taps = self.taps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        f.taps_key = design.match_key(self.taps) if key is None else int(key)
        self.fir = f


def fir_dict(m: native.MMFirResult) -> dict:
    """An mm_fir_result as a dict: the struct's integers (clipped, peak and peak_unclipped as
    per-channel lists) and the largest delivered sample in dBFS.  No reference counterpart."""
    ch = int(m.channels)
    d = {f: int(getattr(m, f)) for f in ("frames", "channels", "rate", "K")}
    for f in ("clipped", "peak", "peak_unclipped"):
        d[f] = [int(getattr(m, f)[c]) for c in range(ch)]
    d["peak_dbfs"] = _db(max(d["peak"], default=0) / 32768.0)
    return d


def fir_pcm(pcm: np.ndarray, rate: int, taps, key: int | None = None, device: int = 0):
    """Filter an int16 (or float32 = int16 / 32768) array [N] or [N, ch] with the symmetric int32
    `taps` (multiples of 2^-22, as design.match_taps makes them) without mastering it
    (mm_fir_pcm): returns (a new array of the same shape, fir_dict).  Frame n stays at frame n.
    `key`: as Fir's.  ValueError for a table mm_fir refuses."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    f = Fir(taps, rate, key)
    out = np.empty_like(x)
    ctx = native.context(device)
    m = native.MMFirResult()
    ctx.check(ctx.lib.mm_fir_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, x.shape[0], ch, ctypes.byref(f.fir),
                                 out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(m)), "mm_fir_pcm")
    return out, fir_dict(m)


def fir_host(pcm: np.ndarray, rate: int, taps):
    """fir_pcm's definition restated in plain C++ on the host (mm_fir_host; int16 only, no GPU):
    (a new array, fir_dict).  ValueError for what the library refuses."""
    x = np.ascontiguousarray(pcm, dtype=np.int16)
    ch = 1 if x.ndim == 1 else x.shape[1]
    f = Fir(taps, rate, 0)
    out = np.zeros_like(x)
    m = native.MMFirResult()
    p16 = ctypes.POINTER(ctypes.c_int16)
    rc = native.load().mm_fir_host(x.ctypes.data_as(p16), x.shape[0], ch, ctypes.byref(f.fir), out.ctypes.data_as(p16),
                                   ctypes.byref(m))
    if rc < 0:
        raise ValueError(f"mm_fir_host failed ({rc}): a table or a signal mm_fir refuses")
    return out, fir_dict(m)


MATCH_FLOOR_DB = -90.0  # a band at or below this level is not compared
MATCH_MIN_BANDS = 3     # comparable bands a match needs


def _band_level(band: dict) -> float | None:
    """10 log10 of the mean over the channels of a band's `ms` (None: not measured; -inf: silent)."""
    ms = band["ms"]
    if any(v is None or math.isnan(v) for v in ms):
        return None
    mean = sum(ms) / len(ms)
    return 10.0 * math.log10(mean) if mean > 0 else -math.inf


def match_gains(source_spectrum: dict, reference_spectrum: dict, amount: float = 1.0, max_db: float = 12.0) -> dict:
    """The match rule on two spectrum_dicts (their rates may differ): one gain in dB per band of
    the source's table, for design.match_taps at the source's rate.  A band's level is 10 log10
    of the mean over the channels of its `ms` (one curve serves both channels).  A band is
    comparable when the reference has a band of the same `lo_hz` / `hi_hz` (the band Nyquist clips
    usually has none), both have `bins_in_band` >= 1 and both levels lie above -90 dB.  On those
    the gain is reference - source, less the unweighted mean of these differences (the loudness
    is deliver_lufs's business), clipped to +-`max_db` and multiplied by `amount` in [0, 1]; every
    other band takes the gain of the nearest comparable band, the lower one on a tie.  Fewer than
    three comparable bands, or a spectrum without a frame (n_frames 0): status "unmeasurable" and
    all gains 0.  Returns {"status" ("matched" | "unmeasurable"), "amount", "max_db", "comparable"
    (their count), "gains_db" (a list), "bands": one dict a band with `centre_hz`, `source_dbfs`,
    `reference_dbfs` (None: no such band, or not measured), `comparable`, `gain_db`}."""
    amount, max_db = float(amount), float(max_db)
    if not 0.0 <= amount <= 1.0:
        raise ValueError(f"match: amount must lie in [0, 1], not {amount}")
    if not max_db >= 0.0:
        raise ValueError(f"match: max_db must not be negative, not {max_db}")
    ref = {(b["lo_hz"], b["hi_hz"]): b for b in reference_spectrum["bands"]}
    measured = source_spectrum["n_frames"] > 0 and reference_spectrum["n_frames"] > 0
    bands, diff = [], {}
    for i, b in enumerate(source_spectrum["bands"]):
        r = ref.get((b["lo_hz"], b["hi_hz"]))
        src = _band_level(b) if measured else None
        rf = _band_level(r) if measured and r is not None else None
        ok = (src is not None and rf is not None and b["bins_in_band"] >= 1 and r["bins_in_band"] >= 1
              and src > MATCH_FLOOR_DB and rf > MATCH_FLOOR_DB)
        if ok:
            diff[i] = rf - src
        bands.append({"centre_hz": b["centre_hz"], "source_dbfs": src, "reference_dbfs": rf, "comparable": ok,
                      "gain_db": 0.0})
    out = {"status": "unmeasurable", "amount": amount, "max_db": max_db, "comparable": len(diff), "bands": bands}
    if len(diff) >= MATCH_MIN_BANDS:
        out["status"] = "matched"
        mean = sum(diff.values()) / len(diff)
        idx = sorted(diff)
        for i, b in enumerate(bands):
            near = min(idx, key=lambda k: (abs(k - i), k))  # (the lower one on a tie)
            b["gain_db"] = amount * min(max_db, max(-max_db, diff[near] - mean))
    out["gains_db"] = [b["gain_db"] for b in bands]
    return out


def _spectrum_device(ctx: native.Context, d_pcm: int, kind: int, frames: int, ch: int, rate: int) -> dict:
    """The spectrum report (spectrum_dict) of a device-resident signal (mm_spectrum_device)."""
    m = native.MMSpectrum()
    bins = np.zeros((native.SPECTRUM_BINS, 3), np.float64)
    bands = np.zeros((native.SPECTRUM_MAX_BANDS, 4), np.float64)
    ctx.check(ctx.lib.mm_spectrum_device(ctx.ptr, ctypes.c_void_p(d_pcm), kind, frames, ch, int(rate), ctypes.byref(m),
                                         bands.ctypes.data_as(native.c_double_p), bins.ctypes.data_as(native.c_double_p)),
              "mm_spectrum_device")
    return spectrum_dict(m, bands[:m.n_bands], bins)


def _match_reference(reference, device: int = 0) -> dict:
    """A match's reference as a spectrum_dict: a spectrum_dict itself, a (pcm, rate) pair measured
    with spectrum_pcm, or the path of a 16-bit PCM WAV read and measured (ValueError for another
    sample format: references wider than 16 bit are not taken)."""
    if isinstance(reference, dict):
        return reference
    if isinstance(reference, (str, os.PathLike)):
        from . import wavio
        pcm, rate = wavio.read_wav(os.fspath(reference))
        if pcm.dtype != np.int16:
            raise ValueError(f"params['match']: the reference {os.fspath(reference)!r} is not a 16-bit PCM WAV")
        return spectrum_pcm(pcm, rate, device=device)
    pcm, rate = reference
    return spectrum_pcm(np.asarray(pcm), int(rate), device=device)


def match_apply(first_pass, gains: dict, rate: int, K: int | None = None):
    """The match after its rule: the taps of `gains` (match_gains) at `rate`, under
    design.match_headroom's trim where their sum |c| would reach 2^24, one pass of
    `first_pass(taps)` -> fir_dict, and, if that pass clipped, the taps redesigned with the trim
    lowered by design.match_trim and applied once more from the untouched source, which cannot
    clip.  `first_pass` is called once or twice and each call filters the source anew.  Returns the
    match_dict of match_pcm; nothing runs for an unmeasurable match.  The composition is the same
    whatever applies the taps: fir_pcm, mm_fir_device on device buffers, or a host restatement."""
    K = design.match_length(rate) if K is None else int(K)
    d = {"status": gains["status"], "K": K, "rate": int(rate), "amount": gains["amount"], "max_db": gains["max_db"],
         "trim_db": 0.0, "passes": 0, "fir": None, "bands": [dict(b, realised_db=0.0) for b in gains["bands"]]}
    if gains["status"] != "matched":
        return d
    fit = design.match_headroom(rate, gains["gains_db"], K)  # (1.0 unless sum |c| would reach 2^24)
    taps = design.match_taps(rate, gains["gains_db"], K, fit)
    realised = design.fir_response_db(taps, rate, [b["centre_hz"] for b in d["bands"]])
    for b, r in zip(d["bands"], realised):
        b["realised_db"] = float(r) - 20.0 * math.log10(fit)
    fir = first_pass(taps)
    d["passes"], trim = 1, fit
    if any(fir["clipped"]):
        trim = fit * design.match_trim(K, max(fir["peak_unclipped"]))
        fir = first_pass(design.match_taps(rate, gains["gains_db"], K, trim))
        d["passes"] = 2
        assert not any(fir["clipped"]), "the trimmed match clipped"
    d["trim_db"] = 20.0 * math.log10(trim)
    d["fir"] = fir
    return d


def _match_device(ctx: native.Context, d_in: int, d_out: int, kind: int, frames: int, ch: int, rate: int,
                  reference: dict, amount: float, max_db: float, K: int | None = None) -> dict:
    """The match on device buffers: the spectrum of the signal at `d_in` (mm_spectrum_device), the
    gains against the `reference` spectrum_dict, the taps, and mm_fir_device from `d_in` into `d_out`
    (twice when the first pass clips).  Returns the match_dict; `d_out` holds the matched signal when
    its `passes` > 0, else nothing was written and `d_in` is what is delivered."""
    gains = match_gains(_spectrum_device(ctx, d_in, kind, frames, ch, rate), reference, amount, max_db)

    def run(taps):
        f = Fir(taps, rate)
        m = native.MMFirResult()
        ctx.check(ctx.lib.mm_fir_device(ctx.ptr, ctypes.c_void_p(d_in), kind, frames, ch, ctypes.byref(f.fir),
                                        ctypes.c_void_p(d_out), ctypes.byref(m)), "mm_fir_device")
        return fir_dict(m)

    return match_apply(run, gains, rate, K)


def _device_pair(x: np.ndarray, device: int):
    """A host signal on the device and a second buffer of its shape (torch: plumbing only)."""
    import torch
    dev = torch.device("cuda", device)
    d_in = torch.from_numpy(x).to(dev)
    d_out = torch.empty_like(d_in)
    torch.cuda.synchronize(dev)
    return d_in, d_out


def match_pcm(pcm: np.ndarray, rate: int, reference, amount: float = 1.0, max_db: float = 12.0, taps: int | None = None,
              device: int = 0):
    """Match the tonal balance of an int16 (or float32 = int16 / 32768) array [N] or [N, ch] to a
    reference without mastering it: returns (a new array, match_dict).  `reference`: a
    spectrum_dict, or a (pcm, rate) pair measured with spectrum_pcm; its rate may differ.  On the
    device: the signal's spectrum (mm_spectrum_device), match_gains, design.match_taps (`taps`:
    their number, default design.match_length(rate)), and one mm_fir_device pass into a second
    buffer; if that pass clips, the taps are redesigned with design.match_trim and applied once
    more from the untouched source, and that pass cannot clip.  The curve is tonal (its mean over
    the comparable bands is 0 dB) and linked (one curve for both channels).
    match_dict: `status` ("matched", or "unmeasurable": the signal is returned unchanged), `K`,
    `rate`, `amount`, `max_db`, `trim_db` (<= 0; 0 when the table fit and one pass sufficed), `passes`, per band
    `centre_hz`, `source_dbfs`, `reference_dbfs`, `comparable`, `gain_db` (asked) and `realised_db`
    (the integer taps' response at the centre, trim excluded: the lowest bands are
    resolution-limited), and `fir`, the last pass's fir_dict.  Figures, not verdicts."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    amount, max_db = float(amount), float(max_db)
    ref = _match_reference(reference, device)
    ctx = native.context(device)
    d_in, d_out = _device_pair(x, device)
    d = _match_device(ctx, d_in.data_ptr(), d_out.data_ptr(), kind, x.shape[0], ch, rate, ref, amount, max_db, taps)
    return (d_out if d["passes"] else d_in).cpu().numpy(), d


def _batch_resampler(jobs, output_rate, d_mids, what: str):
    """The converter of a batch or album call (`what`) whose jobs share one rate: None when
    `output_rate` is None or that rate (the call is then exactly the call without it, and
    `d_mids` is not looked at), else the Resampler.  ValueError, before any device work, for an
    `output_rate` without one `d_mids` buffer per job or a rate pair outside the converter's
    limits (design.resample_geometry)."""
    if output_rate is None or int(output_rate) == jobs[0].rate:
        return None
    if d_mids is None:
        raise ValueError(f"{what} at another rate (output_rate) is mastered into d_mids: one caller-owned buffer of "
                         "frames_proc frames per job")
    if len(d_mids) != len(jobs):
        raise ValueError(f"d_mids: {len(d_mids)} buffers for {len(jobs)} jobs")
    return Resampler(jobs[0].rate, int(output_rate))


def _batch_convert(ctx: native.Context, jobs, rs: Resampler, d_mids, d_outs, kind: int, ch: int):
    """All mastered tracks from `d_mids` into `d_outs` at the converter's rate_out in one
    mm_batch_resample_device call: (the delivered frames as a c_int64 array, [resample_dict ...])."""
    n = len(jobs)
    frames = (ctypes.c_int64 * n)(*[j.frames_proc for j in jobs])
    ms = (native.MMResample * n)()
    ctx.check(ctx.lib.mm_batch_resample_device(ctx.ptr, _pointers(d_mids), kind, frames, n, ch, ctypes.byref(rs.rs),
                                               _pointers(d_outs), ms), "mm_batch_resample_device")
    return (ctypes.c_int64 * n)(*[int(m.frames_out) for m in ms]), [resample_dict(m) for m in ms]


def _delivery_jobs(jobs, noun: str, call: str):
    """Refuses (ValueError) jobs that `call` ("the album call" / "the batch call") cannot master and
    level as the tracks of `noun` ("an album" / "a batch to deliver"): their count, a plan of their
    own for what the call does, or more than one rate, channel count or output kind.  Returns the
    shared (rate, channels, output kind)."""
    if not 1 <= len(jobs) <= native.ALBUM_TRACKS:
        raise ValueError(f"{noun} has 1 to {native.ALBUM_TRACKS} tracks, not {len(jobs)}")
    if any(j.delivery is not None for j in jobs):
        raise ValueError(f"the jobs of {noun} are planned without a delivery (output_rate, deliver_lufs): "
                         f"{call} levels them")
    if any(j.job.ceiling_q28 for j in jobs):
        raise ValueError(f"the jobs of {noun} are planned without ceiling_dbtp: {call} holds the ceiling")
    if any(j.job.meter_on for j in jobs):
        raise ValueError(f"the jobs of {noun} are planned without report or r128: they would describe the tracks "
                         f"before the level, and {call}'s own per-track reports replace them")
    if len({j.rate for j in jobs}) != 1:
        raise ValueError(f"the tracks of {noun} must have one sample rate")
    if len({j.channels for j in jobs}) != 1:
        raise ValueError(f"the tracks of {noun} must have one channel count")
    if len({int(j.job.out_kind) for j in jobs}) != 1:
        raise ValueError(f"the tracks of {noun} must have one output kind")
    return jobs[0].rate, jobs[0].channels, int(jobs[0].job.out_kind)


def _master_converted(ctx: native.Context, jobs, d_ins, d_outs, output_rate, d_mids, noun: str, kind: int, ch: int):
    """Master the checked jobs of `noun` as a batch into `d_outs`, or with an `output_rate` other
    than theirs into `d_mids` and from there, converted, into `d_outs`: (the batch's results, the
    frames in `d_outs` as a c_int64 array, their rate, [resample_dict ...] or None without a
    converter).  _batch_resampler's refusals come before any device work."""
    rs = _batch_resampler(jobs, output_rate, d_mids, noun)
    res = master_batch(ctx, jobs, d_ins, d_outs if rs is None else d_mids)
    if rs is None:
        return res, (ctypes.c_int64 * len(jobs))(*[j.frames_proc for j in jobs]), jobs[0].rate, None
    frames, converted = _batch_convert(ctx, jobs, rs, d_mids, d_outs, kind, ch)
    return res, frames, int(output_rate), converted


def ceiling_pcm(pcm: np.ndarray, rate: int, ceiling_dbtp: float, window: int | None = None, device: int = 0):
    """Hold an int16 (or float32 = int16 / 32768) array [N] or [N, ch] under a true-peak
    ceiling without mastering it (mm_ceiling_pcm): returns (a new array, ceiling_dict).
    `window`: look-ahead frames (default design.ceiling_window(rate))."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    x = x.copy()
    w = design.ceiling_window(rate) if window is None else int(window)
    ctx = native.context(device)
    m = native.MMCeiling()
    ctx.check(ctx.lib.mm_ceiling_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, x.shape[0], ch,
                                     design.ceiling_q28(ceiling_dbtp), w, ctypes.byref(m)), "mm_ceiling_pcm")
    return x, ceiling_dict(m)


def meter_pcm(pcm: np.ndarray, rate: int, loudness: bool = True, device: int = 0) -> dict:
    """Meter an int16 (or float32 = int16 / 32768) array [N] or [N, ch] without
    mastering it: the report of `report_dict` (mm_meter_pcm)."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    x, kind = _out_kind(pcm)
    job = Job(x.shape[0], rate, ch, {}, single_chunk=True, report=True) if loudness else None
    ctx = native.context(device)
    m = native.MMMeter()
    ctx.check(ctx.lib.mm_meter_pcm(ctx.ptr, x.ctypes.data_as(ctypes.c_void_p), kind, x.shape[0], ch,
                                   ctypes.byref(job.job) if job is not None else None, ctypes.byref(m)),
              "mm_meter_pcm")
    return report_dict(m)


def master_pcm(pcm: np.ndarray, rate: int, params: dict, out_kind: int = native.MM_OUT_I16, device: int = 0):
    """Run the whole chain (AME:48-89) on a PCM array [N] or [N, ch] on the GPU.
    Returns (out_pcm, info) with out_pcm int16 (or f32 = int16/32768).  The input is
    int16, float32, or int32 holding 24- or 32-bit PCM left-justified (what
    wavio.read_wav returns for such files): that is decoded on the GPU and mastered
    exactly as the float32 array of the same values; the output stays 16-bit.
    params['report'] (truthy) adds info['report'] (report_dict) on the output;
    params['ceiling_dbtp'] holds the output under that true-peak ceiling first and adds
    info['ceiling'] (ceiling_dict).  params['output_rate'] other than `rate` delivers at
    that rate (mm_deliver): the chain's output is converted on the GPU, the ceiling and
    the report then act on the converted signal, out_pcm has info['frames'] frames at
    info['rate'] and info['resample'] (resample_dict) is added; absent or equal to `rate`,
    the call is exactly the call without it.  params['r128'] (truthy; independent of
    'report') adds info['r128'] (r128_dict): the EBU R 128 figures of the delivered output.
    params['deliver_lufs'] (in [-40, -5]) levels the delivered output, at either rate, to
    that R 128 integrated loudness with the ceiling held and adds info['level']
    (level_dict); absent or None, the call is exactly the call without it.  params['qc']
    (truthy; independent of the other reports) adds info['qc'] (qc_dict): the delivery QC report
    of the delivered output, with silence_lsb 1 and min_run 3.  params['spectrum'] (truthy;
    independent too) adds info['spectrum'] (spectrum_dict): the spectrum report of the delivered output.
    params['match'] = {"reference": a spectrum_dict, a (pcm, rate) pair or the path of a 16-bit PCM
    WAV, "amount": 1.0, "max_db": 12.0} brings the output's tonal balance to the reference's
    (match_pcm) after the chain and the converter, at the delivered rate, and before the level, the
    ceiling and the reports, and adds info['match'] (match_dict); deliver_lufs makes up what its
    trim took.  Absent or None, the call is exactly the call without it."""
    ch = 1 if pcm.ndim == 1 else pcm.shape[1]
    params = dict(params or {})
    report = bool(params.pop("report", False))
    ceiling = params.pop("ceiling_dbtp", None)
    output_rate = params.pop("output_rate", None)
    r128 = bool(params.pop("r128", False))
    deliver_lufs = params.pop("deliver_lufs", None)
    qc = bool(params.pop("qc", False))
    spectrum = bool(params.pop("spectrum", False))
    match = params.pop("match", None)
    if match is not None:
        return _master_matched(pcm, rate, ch, params, out_kind, device, _match_params(match, device),
                               dict(report=report, ceiling_dbtp=ceiling, output_rate=output_rate, r128=r128,
                                    deliver_lufs=deliver_lufs, qc=qc, spectrum=spectrum))
    job = Job(pcm.shape[0], rate, ch, params, out_kind, report=report, ceiling_dbtp=ceiling, output_rate=output_rate,
              r128=r128, deliver_lufs=deliver_lufs, qc=qc, spectrum=spectrum)
    x, job.job.in_kind = _device_input(pcm, wide=True)
    shape = (job.frames_out,) if ch == 1 else (job.frames_out, ch)
    out = np.empty(shape, np.int16 if out_kind == native.MM_OUT_I16 else np.float32)
    ctx = native.context(device)
    res = native.MMResult()
    if job.delivery is not None:
        ctx.check(ctx.lib.mm_deliver(ctx.ptr, ctypes.byref(job.job), ctypes.byref(job.delivery),
                                     x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.byref(res)), "mm_deliver")
    else:
        ctx.check(ctx.lib.mm_master(ctx.ptr, ctypes.byref(job.job), x.ctypes.data_as(ctypes.c_void_p),
                                    out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(res)), "mm_master")
    return out, _finish_info(_info(job, res), job, ctx)


def _match_params(match, device: int = 0) -> dict:
    """params['match'] checked, before any device work on the track: {"reference": a spectrum_dict
    (a (pcm, rate) pair or the path of a 16-bit PCM WAV is measured here), "amount", "max_db"}."""
    if not isinstance(match, dict) or match.get("reference") is None:
        raise ValueError("params['match'] is a dict with a 'reference': a spectrum_dict, a (pcm, rate) pair or the path "
                         "of a 16-bit PCM WAV")
    extra = set(match) - {"reference", "amount", "max_db"}
    if extra:
        raise ValueError(f"params['match'] has no key {sorted(extra)[0]!r} (reference, amount, max_db)")
    amount, max_db = float(match.get("amount", 1.0)), float(match.get("max_db", 12.0))
    if not 0.0 <= amount <= 1.0 or not max_db >= 0.0:
        raise ValueError(f"params['match']: amount in [0, 1] and max_db >= 0, not {amount} and {max_db}")
    return {"reference": _match_reference(match["reference"], device), "amount": amount, "max_db": max_db}


def _deliver_end(ctx: native.Context, job: "Job", d: int, kind: int, frames: int, ch: int, rate: int, info: dict) -> dict:
    """The end of a master call, as `job` plans it, on a delivered device buffer, by the device
    entries of the stages: the level or the ceiling in place (mm_level_device / mm_ceiling_device),
    then the reports (mm_meter_device, mm_r128_device, mm_qc_device, mm_spectrum_device), into
    `info` under _finish_info's keys."""
    end = job.job if job.delivery is None else job.delivery  # who carries ceiling_q28 and meter_on
    level = 0 if job.delivery is None else int(job.delivery.level_clu)
    C, on, w = int(end.ceiling_q28), int(end.meter_on), design.ceiling_window(rate)
    p = ctypes.c_void_p(d)
    ce = native.MMCeiling()
    if level:
        lv = native.MMLevel()
        ctx.check(ctx.lib.mm_level_device(ctx.ptr, p, kind, frames, ch, rate, kweight_sos(rate), level, C, w, ctypes.byref(lv),
                                          ctypes.byref(ce) if C else None), "mm_level_device")
        info["level"] = level_dict(lv)
    elif C:
        ctx.check(ctx.lib.mm_ceiling_device(ctx.ptr, p, kind, frames, ch, C, w, ctypes.byref(ce)), "mm_ceiling_device")
    if C:
        info["ceiling"] = ceiling_dict(ce)
    if on & native.REPORT_METER:
        m = native.MMMeter()
        loud = ctypes.byref(job.job) if job.delivery is None else job.delivery.loud
        ctx.check(ctx.lib.mm_meter_device(ctx.ptr, p, kind, frames, ch, loud, ctypes.byref(m)), "mm_meter_device")
        info["report"] = report_dict(m, job.job.lufs_target if job.job.lufs_on else None)
    if on & native.REPORT_R128:
        m = native.MMR128()
        ctx.check(ctx.lib.mm_r128_device(ctx.ptr, p, kind, frames, ch, rate, kweight_sos(rate), ctypes.byref(m)),
                  "mm_r128_device")
        info["r128"] = r128_dict(m)
    if on & native.REPORT_QC:
        m = native.MMQc()
        ctx.check(ctx.lib.mm_qc_device(ctx.ptr, p, kind, frames, ch, rate, 1, 3, ctypes.byref(m), None), "mm_qc_device")
        info["qc"] = qc_dict(m)
    if on & native.REPORT_SPECTRUM:
        info["spectrum"] = _spectrum_device(ctx, d, kind, frames, ch, rate)
    return info


def _master_matched(pcm: np.ndarray, rate: int, ch: int, params: dict, out_kind: int, device: int, match: dict, end: dict):
    """master_pcm with params['match'], composed over device buffers as deliver_batch composes: the
    master or deliver call without its end (the chain and, with `output_rate`, the converter), the
    match at the delivered rate (_match_device), then the end the call asked for (_deliver_end):
    the level, the ceiling and the reports, which so stay statements about the delivered samples.
    `end`: Job's keywords of the call.  Nothing is queued before both plans stand."""
    import torch
    full = Job(pcm.shape[0], rate, ch, params, out_kind, **end)  # what the call asks for: its refusals, its end
    head = Job(pcm.shape[0], rate, ch, params, out_kind, output_rate=end["output_rate"])
    x, head.job.in_kind = _device_input(pcm, wide=True)
    ctx = native.context(device)
    dev = torch.device("cuda", device)
    d_in = torch.from_numpy(x).to(dev)
    dtype = torch.int16 if out_kind == native.MM_OUT_I16 else torch.float32
    d_mid = torch.empty((head.frames_out, ch), dtype=dtype, device=dev)
    d_out = torch.empty_like(d_mid)
    torch.cuda.synchronize(dev)
    res = native.MMResult()
    master_device(ctx, head, d_in.data_ptr(), d_mid.data_ptr(), res)
    info = _finish_info(_info(head, res), head, ctx)
    out_rate = head.rate if head.output_rate is None else head.output_rate
    info["match"] = _match_device(ctx, d_mid.data_ptr(), d_out.data_ptr(), out_kind, head.frames_out, ch, out_rate,
                                  match["reference"], match["amount"], match["max_db"])
    d = d_out if info["match"]["passes"] else d_mid
    _deliver_end(ctx, full, d.data_ptr(), out_kind, head.frames_out, ch, out_rate, info)
    out = d.cpu().numpy()
    return (out[:, 0] if pcm.ndim == 1 else out), info


def wav_info(path: str, device: int = 0) -> native.MMWavInfo:
    """RIFF/WAVE header of `path` (PCM of 16, 24 or 32 bits, or float32), parsed by the library."""
    ctx = native.context(device)
    info = native.MMWavInfo()
    ctx.check(ctx.lib.mm_wav_probe(ctx.ptr, os.fsencode(path), ctypes.byref(info)), "mm_wav_probe")
    return info


def master_device(ctx: native.Context, job: Job, d_in: int, d_out: int, res: native.MMResult | None = None):
    """Device-resident variant (pointers from e.g. torch tensors).  With `res`
    the loudness, gain and compressor statistics are returned in it.  A job planned
    with `report=True` is metered: `meters(ctx)[0]` (see report_dict); one planned with
    `ceiling_dbtp` is held under it first: `ceilings(ctx)[0]` (see ceiling_dict).  One planned
    with `output_rate` is delivered at that rate (mm_deliver_device): `d_out` then holds
    `job.frames_out` frames.  One planned with `r128=True`: `r128s(ctx)[0]` (see r128_dict).
    One planned with `deliver_lufs` is delivered too, levelled: `levels(ctx)[0]` (see level_dict)."""
    if job.delivery is not None:
        ctx.check(ctx.lib.mm_deliver_device(ctx.ptr, ctypes.byref(job.job), ctypes.byref(job.delivery),
                                            ctypes.c_void_p(d_in), ctypes.c_void_p(d_out),
                                            ctypes.byref(res) if res is not None else None), "mm_deliver_device")
        return res
    ctx.check(ctx.lib.mm_master_device(ctx.ptr, ctypes.byref(job.job), ctypes.c_void_p(d_in),
                                       ctypes.c_void_p(d_out), ctypes.byref(res) if res is not None else None),
              "mm_master_device")
    return res


def master_batch(ctx: native.Context, jobs, d_ins, d_outs, with_results: bool = True):
    """A batch of independent tracks with device-resident inputs/outputs
    (mm_master_batch).  Tracks with the same settings run as ONE timeline (each on
    whole chunks, every stage launched once for the batch); otherwise up to
    native.BATCH_STREAMS of them are in flight at once, each on its own stream.
    Returns one MMResult per job (or None).  Jobs planned with `report=True` are
    metered: `meters(ctx, len(jobs))` holds one mm_meter per job, in job order; jobs
    planned with `ceiling_dbtp` are held under it: `ceilings(ctx, len(jobs))`; jobs planned
    with `r128=True` get their R 128 report: `r128s(ctx, len(jobs))`.  A job planned with
    `output_rate` or `deliver_lufs` is refused here: a batch is delivered at another rate by
    deliver_batch / master_album (their `output_rate` keyword, not a job's plan), which master
    with this call and convert all tracks afterwards."""
    n = len(jobs)
    if any(j.delivery is not None and j.delivery.level_clu for j in jobs):
        raise ValueError("a loudness target (deliver_lufs) re-measures one delivered track pass by pass: "
                         "not available for a batch")
    if any(j.delivery is not None for j in jobs):
        raise ValueError("delivery at another rate (output_rate) is not available for a batch")
    arr = (native.MMJob * n)(*[j.job for j in jobs])
    ins = (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(p)) for p in d_ins])
    outs = (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(p)) for p in d_outs])
    res = (native.MMResult * n)() if with_results else None
    ctx.check(ctx.lib.mm_master_batch(ctx.ptr, n, arr, ins, outs, res), "mm_master_batch")
    return list(res) if with_results else None


def master_album(ctx: native.Context, jobs, d_ins, d_outs, deliver_lufs: float, ceiling_dbtp: float | None = None,
                 output_rate: int | None = None, d_mids=None, qc: bool = False, spectrum: bool = False):
    """Master the tracks of an album as a batch (master_batch) and level the album in place on
    `d_outs` (mm_album_level_device): one static gain for all tracks to `deliver_lufs` (the
    album's EBU R 128 integrated loudness), every track under `ceiling_dbtp`.  The jobs are
    planned without ceiling, delivery, level, report or r128 (the album call resets the
    context's per-call results, so a batch's meters would be lost without a word) and share
    one rate, channel count and output kind: anything else is a ValueError before anything runs.  Returns (the batch's results,
    album dict as album_level_pcm's); `r128s(ctx)` / `ceilings(ctx)` then hold the per-track
    reports of the levelled tracks, as after a batch.
    `output_rate` other than the jobs' rate delivers the album at that rate: the batch is
    mastered into `d_mids` (caller-owned device buffers, one per job, of frames_proc frames), all
    tracks are converted in ONE mm_batch_resample_device call into `d_outs`
    (Resampler.frames_out(frames_proc) frames each), and the album level runs on `d_outs` with the
    K-weighting and the ceiling window of `output_rate`; the album dict gains "resample", one
    resample_dict per track.  It is a keyword of this call on purpose: jobs planned with
    `output_rate` and params['output_rate'] stay refused, here and by master_batch.  None or the
    jobs' rate: the call is exactly the call without it.  An `output_rate` without `d_mids` (or
    with another count of them), or a rate pair design.resample_geometry refuses, is a
    ValueError before any device work.  `qc=True`: after the level one mm_batch_qc_device call
    runs over the delivered buffers at the delivered rate, and every entry of the album dict's
    "tracks" gains "qc" (qc_dict).  `spectrum=True`: likewise one mm_batch_spectrum_device call,
    and every entry gains "spectrum" (spectrum_dict)."""
    jobs = list(jobs)
    _, ch, kind = _delivery_jobs(jobs, "an album", "the album call")
    clu = design.level_clu(deliver_lufs)
    C = 0 if ceiling_dbtp is None else design.ceiling_q28(ceiling_dbtp)
    res, frames, rate, converted = _master_converted(ctx, jobs, d_ins, d_outs, output_rate, d_mids, "an album", kind, ch)
    ctx.check(ctx.lib.mm_album_level_device(ctx.ptr, _pointers(d_outs), kind, frames, len(jobs), ch, rate,
                                            kweight_sos(rate), clu, C, design.ceiling_window(rate)),
              "mm_album_level_device")
    album = _album_dict(ctx, len(jobs), bool(C))
    if converted is not None:
        album["resample"] = converted
    if qc:
        for t, q in zip(album["tracks"], _batch_qc(ctx, d_outs, kind, frames, ch, rate)):
            t["qc"] = q
    if spectrum:
        for t, q in zip(album["tracks"], _batch_spectrum(ctx, d_outs, kind, frames, ch, rate)):
            t["spectrum"] = q
    return res, album


def _batch_buffers(jobs, xs, kind: int, device: int, rs: "Resampler | None"):
    """The device buffers of a batch of files (torch: plumbing only): (inputs, mids or None,
    outputs).  With a converter the mids hold frames_proc frames and the outputs
    rs.frames_out(frames_proc); without one there are no mids."""
    import torch
    dev = torch.device("cuda", device)
    dtype = torch.int16 if kind == native.MM_OUT_I16 else torch.float32
    d_ins = [torch.from_numpy(x).to(dev) for x in xs]
    d_procs = [torch.empty((j.frames_proc, j.channels), dtype=dtype, device=dev) for j in jobs]
    d_outs = d_procs if rs is None else [torch.empty((rs.frames_out(j.frames_proc), j.channels), dtype=dtype, device=dev)
                                         for j in jobs]
    torch.cuda.synchronize(dev)
    return d_ins, None if rs is None else d_procs, d_outs


def _pointers_of(tensors):
    return None if tensors is None else [t.data_ptr() for t in tensors]


def _process_files(name: str, noun: str, words, per_file: bool, deliver, input_paths, output_paths, params: dict,
                   device: int, output_rate, qc: bool = False, spectrum: bool = False):
    """The files of process_album / process_batch (`name`; their tracks are those of `noun`): the
    params keys and their refusals (`words`: what the target is, which dict carries the reports,
    what the files then are, where the two calls' sentences differ), the files read and planned,
    everything that can be refused before the device is touched, the buffers, `deliver`
    (master_album's arguments in; the batch's results, the call's result, one dict a file for
    its info and [resample_dict ...] or None out), the files written.  `per_file`: deliver_lufs
    and ceiling_dbtp may name one value per file, checked before a file is read.  Returns (one
    info dict a file, the call's result)."""
    from . import wavio
    target, carrier, done = words
    params = dict(params or {})
    if params.get("deliver_lufs") is None:
        raise ValueError(f"{name} needs params['deliver_lufs']: {target}")
    deliver_lufs = params.pop("deliver_lufs")
    ceiling = params.pop("ceiling_dbtp", None)
    if params.pop("output_rate", None) is not None:
        raise ValueError("delivery at another rate (output_rate) is not available for a batch")
    fmt = params.pop("output_format", "pcm16")
    for key in ("report", "r128"):
        if params.get(key):
            raise ValueError(f"{name} takes no params['{key}']: the {carrier} carries the R 128 report and "
                             f"the ceiling of every {done} file (meter one with meter_pcm)")
        params.pop(key, None)
    if params.pop("qc", None):
        raise ValueError(f"{name} takes no params['qc']: the keyword qc=True puts every {done} file's QC report "
                         f"into the {carrier}")
    if params.pop("spectrum", None):
        raise ValueError(f"{name} takes no params['spectrum']: the keyword spectrum=True puts every {done} file's "
                         f"spectrum report into the {carrier}")
    if params.get("match") is not None:
        raise ValueError(f"{name} takes no params['match']: {MATCH_REFUSAL}")
    input_paths, output_paths = list(input_paths), list(output_paths)
    if len(input_paths) != len(output_paths):
        raise ValueError(f"{name} needs one output path for every input path")
    if per_file:
        _batch_targets(len(input_paths), deliver_lufs, ceiling, "deliver_lufs")  # (refused before a file is read)
    kind = native.MM_OUT_F32 if fmt == "f32" else native.MM_OUT_I16
    pcms, rates = zip(*[wavio.read_wav(p) for p in input_paths]) if input_paths else ((), ())
    if len(set(rates)) > 1:
        raise ValueError(f"the tracks of {noun} must have one sample rate")
    jobs, xs = [], []
    for pcm in pcms:
        job = Job(pcm.shape[0], rates[0], 1 if pcm.ndim == 1 else pcm.shape[1], params, kind)
        x, job.job.in_kind = _device_input(pcm, wide=True)
        jobs.append(job)
        xs.append(x)
    if len({j.channels for j in jobs}) > 1:
        raise ValueError(f"the tracks of {noun} must have one channel count")
    if not 1 <= len(jobs) <= native.ALBUM_TRACKS:
        raise ValueError(f"{noun} has 1 to {native.ALBUM_TRACKS} tracks, not {len(jobs)}")
    rs = Resampler(rates[0], int(output_rate)) if output_rate is not None and int(output_rate) != rates[0] else None
    ctx = native.context(device)
    d_ins, d_mids, d_outs = _batch_buffers(jobs, xs, kind, device, rs)
    res, result, extras, converted = deliver(ctx, jobs, _pointers_of(d_ins), _pointers_of(d_outs), deliver_lufs, ceiling,
                                             None if rs is None else int(output_rate), _pointers_of(d_mids), bool(qc),
                                             bool(spectrum))
    infos = []
    for t, (job, r, out, path) in enumerate(zip(jobs, res, d_outs, output_paths)):
        y = out.cpu().numpy()
        wavio.write_wav(path, y[:, 0] if job.channels == 1 else y, job.rate if rs is None else int(output_rate))
        info = dict(_info(job, r), **extras[t], output_path=os.path.abspath(path))
        if rs is not None:
            info["frames"], info["rate"], info["resample"] = y.shape[0], int(output_rate), converted[t]
        infos.append(info)
    return infos, result


def process_album(input_paths, output_paths, params: dict, device: int = 0, output_rate: int | None = None,
                  qc: bool = False, spectrum: bool = False):
    """Master the WAV files of an album with the same `params` and level them as one album
    (master_album): params['deliver_lufs'] (required) is the album's target, params['ceiling_dbtp']
    (optional) the true-peak ceiling of every track; params['output_format']='f32' writes
    float.  The files share one rate and channel count.  Returns (one info dict a file, album
    dict).  params['output_rate'] is refused: delivery at another rate is not available for a
    batch through the params; params['report'] and params['r128'] are refused too: the album
    dict carries every levelled file's R 128 report and ceiling.
    The keyword `output_rate` (not a params key, on purpose: the params key stays refused)
    other than the files' rate delivers the album at that rate (master_album's `output_rate`):
    the files are written with that rate in their headers and every info dict gains "frames",
    "rate" and "resample" as process's does; None or the files' rate: exactly the call without
    it.  ValueError for a rate pair design.resample_geometry refuses, before any device work.
    `qc=True`: master_album's keyword; every entry of the album dict's "tracks" gains "qc";
    `spectrum=True` likewise ("spectrum")."""
    def deliver(*call):
        res, album = master_album(*call)
        return res, album, [{}] * len(res), album.get("resample")

    return _process_files("process_album", "an album", ("the album's loudness target", "album dict", "levelled"), False,
                          deliver, input_paths, output_paths, params, device, output_rate, qc, spectrum)


def deliver_batch(ctx: native.Context, jobs, d_ins, d_outs, deliver_lufs, ceiling_dbtp=None,
                  output_rate: int | None = None, d_mids=None, qc: bool = False, spectrum: bool = False):
    """Master the tracks of a batch (master_batch) and level every track in place on `d_outs` to
    its own target (mm_batch_level_device): `deliver_lufs` and `ceiling_dbtp` are each a scalar
    or one value per job (a ceiling of None: none for that job).  The jobs are planned without
    ceiling, delivery, level, report or r128 (the batch level resets the context's per-call
    results, so a batch's meters would be lost without a word) and share one rate, channel count
    and output kind: anything else is a ValueError before anything runs.  Returns (the batch's
    results, [level_dict ...] as level_batch_pcm's); `levels(ctx)` / `r128s(ctx)` / `ceilings(ctx)`
    then hold the per-track results of the levelled tracks, as after a batch.
    `output_rate` other than the jobs' rate delivers the batch at that rate: the batch is
    mastered into `d_mids` (caller-owned device buffers, one per job, of frames_proc frames), all
    tracks are converted in ONE mm_batch_resample_device call into `d_outs`
    (Resampler.frames_out(frames_proc) frames each), and the batch level runs on `d_outs` with the
    K-weighting and the ceiling window of `output_rate`; every level dict gains "resample"
    (resample_dict).  It is a keyword of this call on purpose: jobs planned with `output_rate`
    and params['output_rate'] stay refused, here and by master_batch.  None or the jobs' rate:
    the call is exactly the call without it.  An `output_rate` without `d_mids` (or with another
    count of them), or a rate pair design.resample_geometry refuses, is a ValueError before any
    device work.  `qc=True`: after the level one mm_batch_qc_device call runs over the delivered
    buffers at the delivered rate, and every level dict gains "qc" (qc_dict).  `spectrum=True`:
    likewise one mm_batch_spectrum_device call, and every level dict gains "spectrum" (spectrum_dict)."""
    jobs = list(jobs)
    _, ch, kind = _delivery_jobs(jobs, "a batch to deliver", "the batch call")
    n = len(jobs)
    clu, C = _batch_targets(n, deliver_lufs, ceiling_dbtp, "deliver_lufs")
    res, frames, rate, converted = _master_converted(ctx, jobs, d_ins, d_outs, output_rate, d_mids, "a batch to deliver",
                                                     kind, ch)
    ctx.check(ctx.lib.mm_batch_level_device(ctx.ptr, _pointers(d_outs), kind, frames, n, ch, rate, kweight_sos(rate), clu, C,
                                            design.ceiling_window(rate)), "mm_batch_level_device")
    lvs = _batch_dicts(ctx, list(C))
    if converted is not None:
        for d, r in zip(lvs, converted):
            d["resample"] = r
    if qc:
        for d, q in zip(lvs, _batch_qc(ctx, d_outs, kind, frames, ch, rate)):
            d["qc"] = q
    if spectrum:
        for d, q in zip(lvs, _batch_spectrum(ctx, d_outs, kind, frames, ch, rate)):
            d["spectrum"] = q
    return res, lvs


def process_batch(input_paths, output_paths, params: dict, device: int = 0, output_rate: int | None = None,
                  qc: bool = False, spectrum: bool = False):
    """Master the WAV files of a batch with the same `params` and deliver every file to its own
    loudness target (deliver_batch): params['deliver_lufs'] (required) is a scalar or one value
    per file, params['ceiling_dbtp'] (optional) likewise; params['output_format']='f32' writes
    float.  The files share one rate and channel count.  Returns one info dict a file, with the
    file's level_dict under "level" (and in it "r128" and, with a ceiling, "ceiling").
    params['output_rate'] is refused: delivery at another rate is not available for a batch
    through the params; params['report'] and params['r128'] are refused too: the level dict
    carries every delivered file's R 128 report and ceiling.
    The keyword `output_rate` (not a params key, on purpose: the params key stays refused)
    other than the files' rate delivers every file at that rate (deliver_batch's `output_rate`):
    the files are written with that rate in their headers and every info dict gains "frames",
    "rate" and "resample" as process's does; None or the files' rate: exactly the call without
    it.  ValueError for a rate pair design.resample_geometry refuses, before any device work.
    `qc=True`: deliver_batch's keyword; every file's level dict gains "qc"; `spectrum=True` likewise
    ("spectrum")."""
    def deliver(*call):
        res, lvs = deliver_batch(*call)
        return res, lvs, [{"level": lv} for lv in lvs], [lv.get("resample") for lv in lvs]

    return _process_files("process_batch", "a batch to deliver", ("the loudness target of every file", "level dict", "delivered"),
                          True, deliver, input_paths, output_paths, params, device, output_rate, qc, spectrum)[0]


def process(input_path: str, output_path: str, params: dict, device: int = 0, verbose: bool = False) -> dict:
    """Master `input_path` (16-, 24- or 32-bit PCM or 32-bit float WAV) into `output_path`
    (16-bit PCM WAV, as AME:98 exports, whatever the input's width;
    params['output_format']='f32' writes float).
    The file streams through pinned staging into HBM and back (mm_master_wav); 24- and
    32-bit PCM cross PCIe as they lie in the file and are decoded on the GPU, and give
    exactly what the float32 file of the same values gives.
    params['report'] (truthy) adds info['report'] (report_dict) on the written samples;
    params['ceiling_dbtp'] holds them under that true-peak ceiling (info['ceiling']).
    params['output_rate'] other than the file's rate delivers at that rate (mm_deliver_wav):
    the header carries it and info['frames'] / info['rate'] / info['resample'] describe the
    written file; the ceiling and the report act on the converted samples.
    params['r128'] (truthy) adds info['r128'] (r128_dict), the EBU R 128 figures of the written samples.
    params['deliver_lufs'] levels the written samples to that R 128 integrated loudness under the
    ceiling (info['level'], level_dict).
    params['qc'] (truthy) adds info['qc'] (qc_dict), the delivery QC report of the written samples.
    params['spectrum'] (truthy) adds info['spectrum'] (spectrum_dict), their spectrum report.
    params['match'] (master_pcm's) matches the written samples' tonal balance to a reference
    (info['match']); the file is then read whole (wavio.read_wav), mastered as master_pcm masters
    it and written with wavio.write_wav.
    Raises ValueError for unreadable/unsupported input and RuntimeError for device
    failures, like the reference (AME:110-113)."""
    params = dict(params or {})
    fmt = params.pop("output_format", "pcm16")
    report = bool(params.pop("report", False))
    ceiling = params.pop("ceiling_dbtp", None)
    output_rate = params.pop("output_rate", None)
    r128 = bool(params.pop("r128", False))
    deliver_lufs = params.pop("deliver_lufs", None)
    qc = bool(params.pop("qc", False))
    spectrum = bool(params.pop("spectrum", False))
    kind = native.MM_OUT_F32 if fmt == "f32" else native.MM_OUT_I16
    if params.get("match") is not None:  # the file is read whole and mastered as master_pcm masters it
        from . import wavio
        match = _match_params(params.pop("match"), device)
        pcm, rate = wavio.read_wav(input_path)
        if verbose:
            print(f"Loaded {input_path}: {pcm.shape[0]} frames @ {rate} Hz")
        out, info = _master_matched(pcm, rate, 1 if pcm.ndim == 1 else pcm.shape[1], params, kind, device, match,
                                    dict(report=report, ceiling_dbtp=ceiling, output_rate=output_rate, r128=r128,
                                         deliver_lufs=deliver_lufs, qc=qc, spectrum=spectrum))
        wavio.write_wav(output_path, out, info.get("rate", rate))
        info["output_path"] = os.path.abspath(output_path)
        return info
    params.pop("match", None)
    wi = wav_info(input_path, device)
    if verbose:
        print(f"Loaded {input_path}: {wi.frames} frames @ {wi.rate} Hz")
    job = Job(wi.frames, wi.rate, wi.channels, params, kind, report=report, ceiling_dbtp=ceiling,
              output_rate=output_rate, r128=r128, deliver_lufs=deliver_lufs, qc=qc, spectrum=spectrum)
    ctx = native.context(device)
    res = native.MMResult()
    if job.delivery is not None:
        ctx.check(ctx.lib.mm_deliver_wav(ctx.ptr, ctypes.byref(job.job), ctypes.byref(job.delivery),
                                         os.fsencode(input_path), os.fsencode(output_path), ctypes.byref(res)),
                  "mm_deliver_wav")
    else:
        ctx.check(ctx.lib.mm_master_wav(ctx.ptr, ctypes.byref(job.job), os.fsencode(input_path),
                                        os.fsencode(output_path), ctypes.byref(res)), "mm_master_wav")
    info = _finish_info(_info(job, res), job, ctx)
    if verbose and info["loudness"] is not None:
        print(f"Current loudness: {info['loudness']:.2f} LUFS. Applying {info['gain_db']:.2f} dB gain...")
    info["output_path"] = os.path.abspath(output_path)
    return info
