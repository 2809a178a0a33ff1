"""ctypes binding of libmastering_amd.so (C-ABI declared in include/mastering.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU is
visible, every compute entry point raises.  Struct layouts mirror mastering.h
field for field (natural C alignment on x86-64).
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# MM_LIB: an alternative build of the same library (tools/ablation experiments only)
LIB_PATH = os.environ.get("MM_LIB") or os.path.join(_HERE, "libmastering_amd.so")

MM_OUT_I16, MM_OUT_F32 = 0, 1
MM_IN_F32, MM_IN_I16 = 0, 1
MM_IN_I24, MM_IN_I32 = 2, 3  # packed 24-bit / int32 PCM, decoded on the GPU (mm_pcm_decode_device)
MM_F32, MM_F64 = 0, 1  # per-stage operator sample dtypes
MM_ERR_ARG = -1
BATCH_STREAMS = 8  # MM_BATCH_STREAMS
MAX_DIM, TILE_POW, BLK_POW = 8, 8, 65

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_int32_p = ctypes.POINTER(ctypes.c_int32)


class MMIir(ctypes.Structure):
    _fields_ = [("nsec", ctypes.c_int32), ("nsec_branch0", ctypes.c_int32), ("dim", ctypes.c_int32),
                ("tpb", ctypes.c_int32), ("tile", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("sos", (ctypes.c_double * 5) * 4),
                ("phi_tile_pow", (ctypes.c_double * (MAX_DIM * MAX_DIM)) * TILE_POW),
                ("phi_blk_pow", (ctypes.c_double * (MAX_DIM * MAX_DIM)) * BLK_POW)]


class MMBand(ctypes.Structure):
    _fields_ = [("thresh_rms", ctypes.c_double), ("attack_frames", ctypes.c_double),
                ("release_frames", ctypes.c_double), ("look", ctypes.c_int32), ("r0", ctypes.c_int32),
                ("lut", c_double_p), ("lut_key", ctypes.c_uint64)]


class MMJob(ctypes.Structure):
    _fields_ = [("frames_in", ctypes.c_int64), ("frames_proc", ctypes.c_int64),
                ("channels", ctypes.c_int32), ("rate", ctypes.c_int32), ("tile", ctypes.c_int32),
                ("tiles_per_chunk", ctypes.c_int32),
                ("sat_keep", ctypes.c_float), ("sat_mix", ctypes.c_float), ("sat_drive", ctypes.c_float),
                ("sat_on", ctypes.c_int32), ("width", ctypes.c_double), ("width_on", ctypes.c_int32),
                ("multiband_on", ctypes.c_int32), ("lufs_on", ctypes.c_int32), ("out_kind", ctypes.c_int32),
                ("lufs_target", ctypes.c_double), ("eq", MMIir), ("xover", MMIir), ("kweight", MMIir),
                ("band", MMBand * 3), ("comp_warmup", ctypes.c_int32), ("comp_max_iters", ctypes.c_int32),
                ("comp_super", ctypes.c_int32), ("in_kind", ctypes.c_int32),
                ("n_blocks", ctypes.c_int64), ("block_lo", c_int64_p), ("block_hi", c_int64_p),
                ("n_segs", ctypes.c_int64), ("seg_bounds", c_int64_p), ("block_scale", ctypes.c_double),
                ("sat_table", ctypes.POINTER(ctypes.c_float)), ("sat_key", ctypes.c_uint64),
                ("meter_on", ctypes.c_int32), ("ceiling_q28", ctypes.c_int32)]


class MMResult(ctypes.Structure):
    _fields_ = [("loudness", ctypes.c_double), ("gain_linear", ctypes.c_double), ("frames_out", ctypes.c_int64),
                ("comp_iters", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("comp_active", ctypes.c_int64), ("comp_walked", ctypes.c_int64),
                ("comp_jumped", ctypes.c_int64)]


class MMSolveGeom(ctypes.Structure):
    _fields_ = [("tps", ctypes.c_int32), ("tile_rows", ctypes.c_int32), ("rows", ctypes.c_int32),
                ("walk_block", ctypes.c_int32), ("cols_per_chunk", ctypes.c_int64), ("chunks", ctypes.c_int64),
                ("chunk_plane_bytes", ctypes.c_int64), ("plane_bytes", ctypes.c_int64),
                ("col_block", ctypes.c_int32), ("rms_group_tiles", ctypes.c_int32)]


class MMMeter(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("channels", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("sample_peak", ctypes.c_int32 * 2), ("true_peak_q28", ctypes.c_int32 * 2),
                ("true_peak_frame", ctypes.c_int64 * 2), ("clipped", ctypes.c_int64 * 2),
                ("overs", ctypes.c_int64 * 2), ("loudness", ctypes.c_double)]


class MMR128(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("channels", ctypes.c_int32), ("rate", ctypes.c_int32),
                ("hops", ctypes.c_int64), ("momentary_blocks", ctypes.c_int64),
                ("short_term_blocks", ctypes.c_int64), ("lra_blocks", ctypes.c_int64),
                ("integrated", ctypes.c_double), ("relative_gate", ctypes.c_double),
                ("momentary_max", ctypes.c_double), ("short_term_max", ctypes.c_double),
                ("lra", ctypes.c_double), ("lra_low", ctypes.c_double), ("lra_high", ctypes.c_double)]


class MMQc(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("channels", ctypes.c_int32), ("rate", ctypes.c_int32),
                ("hops", ctypes.c_int64), ("silence_lsb", ctypes.c_int32), ("min_run", ctypes.c_int32),
                ("sum", ctypes.c_int64 * 2), ("sq", ctypes.c_int64 * 2), ("cross", ctypes.c_int64),
                ("smin", ctypes.c_int32 * 2), ("smax", ctypes.c_int32 * 2), ("or_bits", ctypes.c_uint32 * 2),
                ("lead_silence", ctypes.c_int64), ("trail_silence", ctypes.c_int64), ("silent_frames", ctypes.c_int64),
                ("silence_longest", ctypes.c_int64), ("silence_longest_at", ctypes.c_int64),
                ("clip_samples", ctypes.c_int64 * 2), ("clip_runs", ctypes.c_int64 * 2),
                ("clip_longest", ctypes.c_int64 * 2), ("clip_longest_at", ctypes.c_int64 * 2),
                ("corr_windows", ctypes.c_int64), ("corr_negative", ctypes.c_int64), ("corr_min_hop", ctypes.c_int64),
                ("corr_min", ctypes.c_double)]


class MMSpectrum(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("channels", ctypes.c_int32), ("rate", ctypes.c_int32),
                ("n_fft", ctypes.c_int32), ("hop", ctypes.c_int32), ("n_frames", ctypes.c_int64),
                ("n_bands", ctypes.c_int32), ("_pad", ctypes.c_int32), ("total_ms", ctypes.c_double * 2)]


SPECTRUM_N, SPECTRUM_HOP = 8192, 4096  # mm_spectrum's frame length and hop
SPECTRUM_BINS = SPECTRUM_N // 2 + 1    # rows of a bin table
SPECTRUM_MAX_BANDS = 80                # MM_SPECTRUM_MAX_BANDS

REPORT_METER, REPORT_R128, REPORT_QC, REPORT_SPECTRUM = 1, 2, 4, 8  # bits of mm_job.meter_on / mm_delivery.meter_on
c_sos_p = ctypes.POINTER(ctypes.c_double * 5)  # const double sos[2][5]


class MMCeiling(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("channels", ctypes.c_int32), ("window", ctypes.c_int32),
                ("ceiling_q28", ctypes.c_int32), ("tp_in_q28", ctypes.c_int32), ("tp_limited_q28", ctypes.c_int32),
                ("tp_out_q28", ctypes.c_int32), ("min_gain_q16", ctypes.c_int32), ("trim_q16", ctypes.c_int32),
                ("limited_frames", ctypes.c_int64)]


class MMResampler(ctypes.Structure):
    _fields_ = [("rate_in", ctypes.c_int32), ("rate_out", ctypes.c_int32), ("L", ctypes.c_int32),
                ("M", ctypes.c_int32), ("K", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("taps", ctypes.POINTER(ctypes.c_int32)), ("taps_key", ctypes.c_uint64)]


class MMResample(ctypes.Structure):
    _fields_ = [("frames_in", ctypes.c_int64), ("frames_out", ctypes.c_int64), ("channels", ctypes.c_int32),
                ("rate_in", ctypes.c_int32), ("rate_out", ctypes.c_int32), ("L", ctypes.c_int32),
                ("M", ctypes.c_int32), ("K", ctypes.c_int32), ("clipped", ctypes.c_int64 * 2),
                ("peak", ctypes.c_int32 * 2)]


class MMFir(ctypes.Structure):
    _fields_ = [("rate", ctypes.c_int32), ("K", ctypes.c_int32), ("taps", ctypes.POINTER(ctypes.c_int32)),
                ("taps_key", ctypes.c_uint64)]


class MMFirResult(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("channels", ctypes.c_int32), ("rate", ctypes.c_int32),
                ("K", ctypes.c_int32), ("_pad", ctypes.c_int32), ("clipped", ctypes.c_int64 * 2),
                ("peak", ctypes.c_int32 * 2), ("peak_unclipped", ctypes.c_int32 * 2)]


class MMDelivery(ctypes.Structure):
    _fields_ = [("rs", ctypes.POINTER(MMResampler)), ("ceiling_q28", ctypes.c_int32), ("window", ctypes.c_int32),
                ("meter_on", ctypes.c_int32), ("level_clu", ctypes.c_int32), ("loud", ctypes.POINTER(MMJob))]


LEVEL_PASSES = 5  # MM_LEVEL_PASSES
LEVEL_STATUS = ("off", "reached", "capped", "saturated", "passes", "unmeasurable")  # MM_LEVEL_* by value


class MMLevel(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("channels", ctypes.c_int32), ("rate", ctypes.c_int32),
                ("target_clu", ctypes.c_int32), ("ceiling_q28", ctypes.c_int32), ("window", ctypes.c_int32),
                ("status", ctypes.c_int32), ("passes", ctypes.c_int32), ("gain_q16", ctypes.c_int32),
                ("pass_gain_q16", ctypes.c_int32 * LEVEL_PASSES), ("min_gain_q16", ctypes.c_int32),
                ("source_lufs", ctypes.c_double), ("pass_lufs", ctypes.c_double * LEVEL_PASSES),
                ("loudness", ctypes.c_double), ("clipped", ctypes.c_int64), ("limited_frames", ctypes.c_int64)]


ABI_VERSION = 5  # MM_ABI_VERSION of include/mastering.h
ALBUM_TRACKS = 256  # MM_ALBUM_TRACKS


class MMWavInfo(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("data_offset", ctypes.c_int64), ("rate", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("format", ctypes.c_int32), ("bits", ctypes.c_int32)]


# every symbol include/mastering.h declares (checked by tests/test_abi.py)
EXPORTS = ("mm_create", "mm_destroy", "mm_last_error", "mm_sync", "mm_version", "mm_source_sha", "mm_master",
           "mm_master_device",
           "mm_stage_chunks", "mm_kweight_range_end", "mm_hop_energies", "mm_shard_loudness_device",
           "mm_shard_energies_device", "mm_gate_finalize_device", "mm_allreduce_sum_f64_device",
           "mm_allgather_f64_device",
           "mm_gate_loudness", "mm_finalize",
           "mm_read_mix", "mm_timing", "mm_kernel_stats", "mm_comm_unique_id", "mm_comm_init", "mm_comm_destroy",
           "mm_allreduce_sum_f64", "mm_allgather_f64", "mm_wav_probe", "mm_master_wav",
           "mm_op_pcm_to_float", "mm_op_saturation", "mm_op_saturation_table", "mm_op_stereo_width", "mm_op_quantize", "mm_op_soft_limiter",
           "mm_op_gain", "mm_op_sosfilt", "mm_op_loudness", "mm_op_multiband", "mm_master_batch",
           "mm_op_saturation_legacy", "mm_op_soft_limiter_legacy", "mm_op_sosfilt_mix", "mm_op_compress_bands",
           "mm_solve_geometry", "mm_solve_records", "mm_np_sum_f32", "mm_check_compressor_math",
           "mm_meter_device", "mm_meter_pcm", "mm_last_meters", "mm_op_true_peak", "mm_true_peak_host",
           "mm_meter_span",
           "mm_r128_from_hops", "mm_r128_host", "mm_r128_device", "mm_r128_pcm", "mm_op_r128_hops", "mm_r128_span",
           "mm_last_r128",
           "mm_qc_from_hops", "mm_qc_host", "mm_qc_device", "mm_qc_pcm", "mm_batch_qc_device", "mm_batch_qc_pcm",
           "mm_qc_span", "mm_last_qc",
           "mm_spectrum_bands", "mm_spectrum_from_bins", "mm_spectrum_host", "mm_spectrum_device", "mm_spectrum_pcm",
           "mm_batch_spectrum_device", "mm_batch_spectrum_pcm", "mm_last_spectrum", "mm_last_spectrum_bins",
           "mm_ceiling_device", "mm_ceiling_pcm", "mm_ceiling_host", "mm_last_ceilings", "mm_ceiling_span",
           "mm_ceiling_max_window",
           "mm_pcm_decode_device", "mm_op_pcm_decode", "mm_pcm_decode_host", "mm_pcm_decode_span",
           "mm_resample_device", "mm_resample_pcm", "mm_resample_host", "mm_resample_frames", "mm_resample_span",
           "mm_last_resample", "mm_deliver_device", "mm_deliver", "mm_deliver_wav",
           "mm_level_device", "mm_level_pcm", "mm_level_host", "mm_op_level_gain", "mm_last_levels", "mm_level_span",
           "mm_r128_album_from_hops", "mm_album_level_host", "mm_album_r128_device", "mm_album_r128_pcm",
           "mm_op_r128_album_hops", "mm_album_level_device", "mm_album_level_pcm", "mm_last_album",
           "mm_batch_ceiling_device", "mm_batch_ceiling_pcm", "mm_batch_level_device", "mm_batch_level_pcm",
           "mm_batch_resample_device", "mm_batch_resample_pcm",
           "mm_fir_device", "mm_fir_pcm", "mm_fir_host", "mm_fir_span", "mm_last_fir")

_lib = None
_lock = threading.Lock()


def load():
    """Load the HIP library; raise loudly if it was not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        try:  # share ONE HIP runtime with PyTorch when it is present (same soname)
            import torch  # noqa: F401
        except Exception:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"HIP extension not built: {LIB_PATH} missing (run __graft_entry__.build())")
        lib = ctypes.CDLL(LIB_PATH)
        vp = ctypes.c_void_p
        P = ctypes.POINTER
        sig = {
            "mm_create": ([ctypes.c_int, P(vp)], ctypes.c_int),
            "mm_destroy": ([vp], ctypes.c_int),
            "mm_last_error": ([vp], ctypes.c_char_p),
            "mm_sync": ([vp], ctypes.c_int),
            "mm_version": ([], ctypes.c_int),
            "mm_source_sha": ([], ctypes.c_char_p),
            "mm_master": ([vp, P(MMJob), vp, vp, P(MMResult)], ctypes.c_int),
            "mm_master_device": ([vp, P(MMJob), vp, vp, P(MMResult)], ctypes.c_int),
            "mm_master_batch": ([vp, ctypes.c_int, P(MMJob), P(vp), P(vp), P(MMResult)], ctypes.c_int),
            "mm_stage_chunks": ([vp, P(MMJob), vp], ctypes.c_int),
            "mm_wav_probe": ([vp, ctypes.c_char_p, P(MMWavInfo)], ctypes.c_int),
            "mm_master_wav": ([vp, P(MMJob), ctypes.c_char_p, ctypes.c_char_p, P(MMResult)], ctypes.c_int),
            "mm_kweight_range_end": ([vp, c_double_p], ctypes.c_int),
            "mm_hop_energies": ([vp, c_double_p, c_double_p], ctypes.c_int),
            "mm_shard_energies_device": ([vp, c_double_p, ctypes.c_int64, ctypes.c_int64, vp], ctypes.c_int),
            "mm_gate_finalize_device": ([vp, vp, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_int32), ctypes.c_double, ctypes.c_double, vp,
                                         c_double_p], ctypes.c_int),
            "mm_shard_loudness_device": ([vp, c_double_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                          ctypes.c_double, ctypes.c_double, ctypes.c_int32, vp, c_double_p],
                                         ctypes.c_int),
            "mm_gate_loudness": ([P(MMJob), c_double_p, c_double_p], ctypes.c_int),
            "mm_finalize": ([vp, ctypes.c_double, ctypes.c_int, vp], ctypes.c_int),
            "mm_read_mix": ([vp, P(ctypes.c_int16)], ctypes.c_int),
            "mm_timing": ([vp, ctypes.c_int], ctypes.c_int),
            "mm_kernel_stats": ([vp, ctypes.c_char_p, ctypes.c_int, c_double_p, c_int64_p, ctypes.c_int],
                                ctypes.c_int),
            "mm_comm_unique_id": ([ctypes.c_char_p], ctypes.c_int),
            "mm_comm_init": ([vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p], ctypes.c_int),
            "mm_comm_destroy": ([vp], ctypes.c_int),
            "mm_allreduce_sum_f64": ([vp, c_double_p, ctypes.c_int64], ctypes.c_int),
            "mm_allgather_f64": ([vp, c_double_p, c_double_p, ctypes.c_int64], ctypes.c_int),
            "mm_allreduce_sum_f64_device": ([vp, vp, ctypes.c_int64], ctypes.c_int),
            "mm_allgather_f64_device": ([vp, vp, vp, ctypes.c_int64], ctypes.c_int),
            "mm_op_pcm_to_float": ([vp, vp, ctypes.c_int64, vp], ctypes.c_int),
            "mm_op_saturation": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_double, vp], ctypes.c_int),
            "mm_op_saturation_table": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_double,
                                        ctypes.POINTER(ctypes.c_float), vp], ctypes.c_int),
            "mm_op_stereo_width": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_double, vp], ctypes.c_int),
            "mm_op_quantize": ([vp, ctypes.c_int, vp, ctypes.c_int64, vp], ctypes.c_int),
            "mm_op_soft_limiter": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_double], ctypes.c_int),
            "mm_op_gain": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_double, vp], ctypes.c_int),
            "mm_op_sosfilt": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_int, P(MMIir), ctypes.c_int, vp],
                              ctypes.c_int),
            "mm_op_loudness": ([vp, P(MMJob), ctypes.c_int, vp, c_double_p], ctypes.c_int),
            "mm_op_multiband": ([vp, P(MMJob), vp, vp], ctypes.c_int),
            "mm_op_saturation_legacy": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_double, vp], ctypes.c_int),
            "mm_op_soft_limiter_legacy": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_double], ctypes.c_int),
            "mm_op_sosfilt_mix": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_int, P(MMIir), ctypes.c_double,
                                   ctypes.c_double, vp], ctypes.c_int),
            "mm_op_compress_bands": ([vp, P(MMJob), vp, vp, vp, vp], ctypes.c_int),
            "mm_solve_geometry": ([P(MMJob), P(MMSolveGeom)], ctypes.c_int),
            "mm_solve_records": ([vp, ctypes.c_int, ctypes.c_int64, P(ctypes.c_int32), c_double_p, c_double_p,
                                  c_int64_p], ctypes.c_int),
            "mm_np_sum_f32": ([P(ctypes.c_float), ctypes.c_int64, P(ctypes.c_float)], ctypes.c_int),
            "mm_check_compressor_math": ([vp, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int64, c_double_p],
                                         ctypes.c_int),
            "mm_meter_device": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, P(MMJob), P(MMMeter)],
                                ctypes.c_int),
            "mm_meter_pcm": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, P(MMJob), P(MMMeter)],
                             ctypes.c_int),
            "mm_last_meters": ([vp, ctypes.c_int, P(MMMeter)], ctypes.c_int),
            "mm_op_true_peak": ([vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_int, c_double_p], ctypes.c_int),
            "mm_true_peak_host": ([P(ctypes.c_int16), ctypes.c_int64, ctypes.c_int, P(MMMeter)], ctypes.c_int),
            "mm_meter_span": ([], ctypes.c_int),
            "mm_r128_from_hops": ([c_double_p, ctypes.c_int64, ctypes.c_int32, P(MMR128)], ctypes.c_int),
            "mm_r128_host": ([P(ctypes.c_int16), ctypes.c_int64, ctypes.c_int, ctypes.c_int32, c_sos_p, c_double_p,
                              ctypes.c_int64, P(MMR128)], ctypes.c_int),
            "mm_r128_device": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, c_sos_p,
                                P(MMR128)], ctypes.c_int),
            "mm_r128_pcm": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, c_sos_p,
                             P(MMR128)], ctypes.c_int),
            "mm_op_r128_hops": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, c_sos_p,
                                 c_double_p, ctypes.c_int64], ctypes.c_int),
            "mm_r128_span": ([], ctypes.c_int),
            "mm_last_r128": ([vp, ctypes.c_int, P(MMR128)], ctypes.c_int),
            "mm_qc_from_hops": ([c_int64_p, ctypes.c_int64, ctypes.c_int32, P(MMQc)], ctypes.c_int),
            "mm_qc_host": ([P(ctypes.c_int16), ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                            P(MMQc), c_int64_p], ctypes.c_int),
            "mm_qc_device": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                              ctypes.c_int32, P(MMQc), c_int64_p], ctypes.c_int),
            "mm_qc_pcm": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                           ctypes.c_int32, P(MMQc), c_int64_p], ctypes.c_int),
            "mm_batch_qc_device": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                    ctypes.c_int32, ctypes.c_int32, P(MMQc)], ctypes.c_int),
            "mm_batch_qc_pcm": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                 ctypes.c_int32, ctypes.c_int32, P(MMQc)], ctypes.c_int),
            "mm_qc_span": ([], ctypes.c_int),
            "mm_last_qc": ([vp, ctypes.c_int, P(MMQc)], ctypes.c_int),
            "mm_spectrum_bands": ([ctypes.c_int32, ctypes.c_int, c_double_p], ctypes.c_int),
            "mm_spectrum_from_bins": ([c_double_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, P(MMSpectrum), c_double_p],
                                      ctypes.c_int),
            "mm_spectrum_host": ([P(ctypes.c_int16), ctypes.c_int64, ctypes.c_int, ctypes.c_int32, P(MMSpectrum), c_double_p,
                                  c_double_p], ctypes.c_int),
            "mm_spectrum_device": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, P(MMSpectrum),
                                    c_double_p, c_double_p], ctypes.c_int),
            "mm_spectrum_pcm": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, P(MMSpectrum),
                                 c_double_p, c_double_p], ctypes.c_int),
            "mm_batch_spectrum_device": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                          P(MMSpectrum)], ctypes.c_int),
            "mm_batch_spectrum_pcm": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                       P(MMSpectrum)], ctypes.c_int),
            "mm_last_spectrum": ([vp, ctypes.c_int, P(MMSpectrum)], ctypes.c_int),
            "mm_last_spectrum_bins": ([vp, ctypes.c_int, ctypes.c_int, c_double_p], ctypes.c_int),
            "mm_ceiling_device": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                   P(MMCeiling)], ctypes.c_int),
            "mm_ceiling_pcm": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                P(MMCeiling)], ctypes.c_int),
            "mm_ceiling_host": ([P(ctypes.c_int16), ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                 P(MMCeiling)], ctypes.c_int),
            "mm_last_ceilings": ([vp, ctypes.c_int, P(MMCeiling)], ctypes.c_int),
            "mm_ceiling_span": ([], ctypes.c_int),
            "mm_ceiling_max_window": ([], ctypes.c_int),
            "mm_pcm_decode_device": ([vp, ctypes.c_int, vp, ctypes.c_int64, vp], ctypes.c_int),
            "mm_op_pcm_decode": ([vp, ctypes.c_int, vp, ctypes.c_int64, vp], ctypes.c_int),
            "mm_pcm_decode_host": ([ctypes.c_int, vp, ctypes.c_int64, vp], ctypes.c_int),
            "mm_pcm_decode_span": ([], ctypes.c_int),
            "mm_resample_device": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, P(MMResampler), vp,
                                    P(MMResample)], ctypes.c_int),
            "mm_resample_pcm": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, P(MMResampler), vp,
                                 P(MMResample)], ctypes.c_int),
            "mm_resample_host": ([P(ctypes.c_int16), ctypes.c_int64, ctypes.c_int, P(MMResampler), P(ctypes.c_int16),
                                  P(MMResample)], ctypes.c_int),
            "mm_resample_frames": ([ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_int64_p], ctypes.c_int),
            "mm_resample_span": ([], ctypes.c_int),
            "mm_last_resample": ([vp, P(MMResample)], ctypes.c_int),
            "mm_deliver_device": ([vp, P(MMJob), P(MMDelivery), vp, vp, P(MMResult)], ctypes.c_int),
            "mm_deliver": ([vp, P(MMJob), P(MMDelivery), vp, vp, P(MMResult)], ctypes.c_int),
            "mm_deliver_wav": ([vp, P(MMJob), P(MMDelivery), ctypes.c_char_p, ctypes.c_char_p, P(MMResult)],
                               ctypes.c_int),
            "mm_level_device": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, c_sos_p,
                                 ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P(MMLevel), P(MMCeiling)], ctypes.c_int),
            "mm_level_pcm": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, c_sos_p,
                              ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P(MMLevel), P(MMCeiling)], ctypes.c_int),
            "mm_level_host": ([P(ctypes.c_int16), ctypes.c_int64, ctypes.c_int, ctypes.c_int32, c_sos_p,
                               ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P(MMLevel), P(MMCeiling)], ctypes.c_int),
            "mm_op_level_gain": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int32, vp,
                                  c_int64_p, P(ctypes.c_int32)], ctypes.c_int),
            "mm_last_levels": ([vp, ctypes.c_int, P(MMLevel)], ctypes.c_int),
            "mm_level_span": ([], ctypes.c_int),
            "mm_r128_album_from_hops": ([c_double_p, c_int64_p, ctypes.c_int, ctypes.c_int32, P(MMR128)], ctypes.c_int),
            "mm_album_level_host": ([P(P(ctypes.c_int16)), c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32, c_sos_p,
                                     ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P(MMLevel), P(MMR128), P(MMR128),
                                     P(MMCeiling)], ctypes.c_int),
            "mm_album_r128_device": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                      c_sos_p, P(MMR128)], ctypes.c_int),
            "mm_album_r128_pcm": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                   c_sos_p, P(MMR128)], ctypes.c_int),
            "mm_op_r128_album_hops": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                       c_sos_p, c_double_p, ctypes.c_int64], ctypes.c_int),
            "mm_album_level_device": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                       c_sos_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32], ctypes.c_int),
            "mm_album_level_pcm": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                    c_sos_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32], ctypes.c_int),
            "mm_last_album": ([vp, P(MMLevel), P(MMR128)], ctypes.c_int),
            "mm_batch_ceiling_device": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, c_int32_p,
                                         ctypes.c_int32, P(MMCeiling)], ctypes.c_int),
            "mm_batch_ceiling_pcm": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, c_int32_p,
                                      ctypes.c_int32, P(MMCeiling)], ctypes.c_int),
            "mm_batch_level_device": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                       c_sos_p, c_int32_p, c_int32_p, ctypes.c_int32], ctypes.c_int),
            "mm_batch_level_pcm": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                    c_sos_p, c_int32_p, c_int32_p, ctypes.c_int32], ctypes.c_int),
            "mm_batch_resample_device": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, P(MMResampler),
                                          P(vp), P(MMResample)], ctypes.c_int),
            "mm_batch_resample_pcm": ([vp, P(vp), ctypes.c_int, c_int64_p, ctypes.c_int, ctypes.c_int, P(MMResampler),
                                       P(vp), P(MMResample)], ctypes.c_int),
            "mm_fir_device": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, P(MMFir), vp, P(MMFirResult)],
                              ctypes.c_int),
            "mm_fir_pcm": ([vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, P(MMFir), vp, P(MMFirResult)],
                           ctypes.c_int),
            "mm_fir_host": ([P(ctypes.c_int16), ctypes.c_int64, ctypes.c_int, P(MMFir), P(ctypes.c_int16),
                             P(MMFirResult)], ctypes.c_int),
            "mm_fir_span": ([], ctypes.c_int),
            "mm_last_fir": ([vp, P(MMFirResult)], ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = res
        if lib.mm_version() != ABI_VERSION:  # the structs above mirror one header version
            raise RuntimeError(f"{LIB_PATH}: ABI version {lib.mm_version()}, this binding expects {ABI_VERSION}")
        _lib = lib
        return lib


class Context:
    """One HIP stream + device work buffers (mm_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        self.ptr = ctypes.c_void_p()
        rc = self.lib.mm_create(device, ctypes.byref(self.ptr))
        if rc != 0:
            raise RuntimeError(f"mm_create(device={device}) failed ({rc}): no usable MI355X/HIP device")
        self.device = device

    def check(self, rc: int, what: str):
        """Raise on a negative status: ValueError for bad arguments or input files
        (MM_ERR_ARG, like the reference's decode errors), RuntimeError otherwise."""
        if rc < 0:
            msg = self.lib.mm_last_error(self.ptr)
            text = f"{what} failed ({rc}): {msg.decode(errors='replace') if msg else ''}"
            raise ValueError(text) if rc == MM_ERR_ARG else RuntimeError(text)
        return rc

    def close(self):
        if self.ptr:
            self.lib.mm_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # timing ---------------------------------------------------------------
    def timing(self, enable: bool):
        self.check(self.lib.mm_timing(self.ptr, int(enable)), "mm_timing")

    def kernel_stats(self):
        cap = 64
        names = ctypes.create_string_buffer(8192)
        ms = (ctypes.c_double * cap)()
        n = (ctypes.c_int64 * cap)()
        k = self.check(self.lib.mm_kernel_stats(self.ptr, names, 8192, ms, n, cap), "mm_kernel_stats")
        labels = names.value.decode().split("\n") if k else []
        return {labels[i]: (ms[i], n[i]) for i in range(k)}

    def sync(self):
        self.check(self.lib.mm_sync(self.ptr), "mm_sync")


_tls = threading.local()


def context(device: int = 0) -> Context:
    """Per-thread context (the reference's GUI calls from a worker thread)."""
    ctxs = getattr(_tls, "ctxs", None)
    if ctxs is None:
        ctxs = _tls.ctxs = {}
    if device not in ctxs:
        ctxs[device] = Context(device)
    return ctxs[device]


def library_sha() -> str:
    """Source hash embedded in the loaded library (srcsha.library_sha at build time)."""
    return load().mm_source_sha().decode()
