"""mastering_amd — MI355X-native drop-in for the reference's mastering hot path.

Public surface (mirrors worker/audio_mastering_engine.py):
  EQ_PRESETS                   AME:15-20
  process(in, out, params)     AME:24-113 with local WAV IO instead of GCS
  master_pcm(pcm, rate, params)  the chain on an in-memory PCM array
  process_audio(settings, cb), batch_process_audio(settings, in_dir, out_dir, cb)
                               the desktop GUI's engine API (mastering_gui.py:204,220)
  apply_saturation, apply_eq_to_samples, apply_shelf_filter, apply_peak_filter,
  apply_stereo_width, apply_multiband_compressor, normalize_to_lufs, soft_limiter,
  audio_segment_to_float_array, float_array_to_audio_segment, integrated_loudness
                               the per-stage DSP helpers (AME:117-227), one HIP operator each
  worker.handle_push / worker.wsgi_app / worker.process_audio_from_gcs
                               the job worker (worker/main.py:15-50, AME:24-113) on a
                               local object tree
  params["report"], meter_pcm(pcm, rate), meters(ctx), true_peak(samples)
                               the mastering report (no reference counterpart): sample peak,
                               BS.1770-4 true peak and the loudness of the delivered output
  params["r128"], r128_pcm(pcm, rate), r128s(ctx)
                               the EBU R 128 report (no reference counterpart): integrated
                               loudness as a BS.1770 meter reads it, maximum momentary and
                               short-term loudness and the loudness range of the delivered output
  params["qc"], qc_pcm(pcm, rate), qc_batch_pcm(tracks, rate), qcs(ctx), deliver_batch / master_album /
  process_batch / process_album(..., qc=True)
                               the delivery QC report (no reference counterpart): phase
                               correlation overall and in 400 ms windows, DC offset, runs of
                               full-scale samples, digital silence at the ends and inside, bit
                               use and dual mono of the delivered output, as exact integers
  params["spectrum"], spectrum_pcm(pcm, rate), spectrum_batch_pcm(tracks, rate), spectra(ctx),
  spectrum_bands(rate), occupied_hz(bins, rate, db), deliver_batch / master_album / process_batch /
  process_album(..., spectrum=True)
                               the spectrum report (no reference counterpart): Welch's long-term
                               spectrum of the delivered output on 8192-sample frames, its 1/3-octave
                               bands with level, mid / side and phase correlation a band, roll-off
                               and occupied bandwidth
  params["ceiling_dbtp"], ceiling_pcm(pcm, rate, db), ceilings(ctx)
                               the true-peak ceiling (no reference counterpart): an exact
                               look-ahead limiter on the delivered output
  params["output_rate"], resample_pcm(pcm, rate_in, rate_out)
                               delivery at another sample rate (no reference counterpart): an
                               exact polyphase converter before the ceiling and the report
  params["deliver_lufs"], level_pcm(pcm, rate, lufs, ceiling_dbtp), levels(ctx)
                               delivery to an R 128 loudness target under the true-peak ceiling
                               (no reference counterpart): the static gain that makes the
                               delivered file read the target, re-measured after every limiter pass
  album_level_pcm(tracks, rate, lufs, ceiling_dbtp), album_r128_pcm(tracks, rate),
  master_album(ctx, jobs, d_ins, d_outs, lufs, ceiling_dbtp), process_album(ins, outs, params)
                               an album levelled as one programme (no reference counterpart):
                               one static gain for all tracks to an R 128 album target, every
                               track under the ceiling, the balance between the tracks kept
  level_batch_pcm(tracks, rate, lufs, ceiling_dbtp), ceiling_batch_pcm(tracks, rate, db),
  deliver_batch(ctx, jobs, d_ins, d_outs, lufs, ceiling_dbtp), process_batch(ins, outs, params)
                               a batch delivered track by track (no reference counterpart):
                               every track to its own R 128 target under its own ceiling, as
                               level_pcm gives it, with every launch of a pass over all tracks
  resample_batch_pcm(tracks, rate_in, rate_out), deliver_batch(..., output_rate=, d_mids=),
  master_album(..., output_rate=, d_mids=), process_batch / process_album(..., output_rate=)
                               a batch or an album delivered at another rate (no reference
                               counterpart): every track as resample_pcm gives it, all tracks
                               in one converter launch, then levelled at the new rate
  params["match"], match_pcm(pcm, rate, reference), match_gains(source, reference), fir_pcm(pcm, rate, taps)
                               the reference match (no reference counterpart): the delivered
                               output's 1/3-octave balance brought to a reference's by an exact
                               linear-phase FIR of up to 8191 taps, before the level and the ceiling
  legacy.master_pcm / legacy.process and main.py's helpers
                               the older monolithic engine (root main.py:46-192) as an
                               alternate DSP profile on the same HIP operators
"""
from .engine import (EQ_PRESETS, Job, album_level_pcm, album_r128_pcm, ceiling_batch_pcm, ceiling_pcm, ceilings,  # noqa: F401
                     deliver_batch, fir_pcm, level_batch_pcm, level_pcm, levels, master_album, master_batch, master_device,
                     master_pcm, match_gains, match_pcm, meter_pcm, meters, process, process_album, process_batch, qc_batch_pcm, qc_dict, qc_pcm, qcs,
                     r128_pcm, r128s, resample_batch_pcm, resample_pcm, occupied_hz, spectra, spectrum_bands, spectrum_batch_pcm,
                     spectrum_dict, spectrum_pcm)
from . import legacy  # noqa: F401
from .gui_compat import batch_process_audio, process_audio  # noqa: F401
from .ops import (apply_eq_to_samples, apply_multiband_compressor, apply_peak_filter, apply_saturation,  # noqa: F401
                  apply_shelf_filter, apply_stereo_width, audio_segment_to_float_array,
                  float_array_to_audio_segment, integrated_loudness, normalize_to_lufs, soft_limiter, true_peak)

__all__ = ["legacy", "EQ_PRESETS", "Job", "master_pcm", "master_device", "master_batch", "process", "process_audio", "batch_process_audio",
           "apply_saturation", "apply_eq_to_samples", "apply_shelf_filter", "apply_peak_filter", "apply_stereo_width",
           "apply_multiband_compressor", "normalize_to_lufs", "soft_limiter", "audio_segment_to_float_array",
           "float_array_to_audio_segment", "integrated_loudness", "true_peak", "meter_pcm", "meters", "ceiling_pcm",
           "ceilings", "resample_pcm", "r128_pcm", "r128s", "level_pcm", "levels", "album_level_pcm", "album_r128_pcm",
           "master_album", "process_album", "ceiling_batch_pcm", "level_batch_pcm", "deliver_batch", "process_batch",
           "resample_batch_pcm", "qc_pcm", "qc_batch_pcm", "qc_dict", "qcs",
           "spectrum_pcm", "spectrum_batch_pcm", "spectrum_dict", "spectra", "spectrum_bands", "occupied_hz",
           "match_pcm", "match_gains", "fir_pcm"]
