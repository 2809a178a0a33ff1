"""Host-side design of one mastering job (f64, the reference's own expressions).

Everything here is small, per-job and exact: filter coefficients, the compressor's
max-attenuation tables, chunk/tile geometry, IIR state-transition powers for the
tile scan and pyloudnorm's block geometry.  The per-sample work runs in the HIP
library; nothing here touches audio samples.

Reference anchors (worker/audio_mastering_engine.py = "AME"):
  chunking            AME:48-54 via pydub ms slicing (`len`, `__getitem__`)
  saturation consts   AME:131-134
  shelf / peak EQ     AME:170-194 (note: w0 = 4*pi*f/fs and gain = 10^(dB/20),
                      exactly as written; we reproduce, not "fix", the formula)
  crossover           AME:197-198 scipy.signal.butter(4, ..., output='sos')
  compressor consts   pydub compress_dynamic_range via AME:207-209
  K-weighting         pyloudnorm Meter(rate) filters via AME:213
  loudness blocks     pyloudnorm integrated_loudness via AME:218
"""
from __future__ import annotations

import functools
import hashlib
import math
import os

import numpy as np
import scipy.signal

MAX_DIM = 8
CHUNK_MS = 30 * 1000  # AME:48
DEFAULT_TILE = 225     # divides 30 s chunks at 11.025/22.05/44.1/48/88.2/96/192 kHz (round 4: T 75-250 swept,
                       # 225 fastest on C2, P_HOT, C3 and C5)
NOCOMP_TILE = 125      # tile of jobs without the multiband compressor (EQ / K-weighting lanes)
OPS_TILE = 125         # tile of the per-stage operators' look-back tables (== OPS_TILE in csrc/ops.hip)
WALK_BLOCK = 25        # rows per walk load block of the compressor's M plane (MM_WALK_B; the library reports
                       # it as mm_solve_geom.walk_block, checked in tests/test_abi.py)

EQ_KEYS = ("bass_boost", "mid_cut", "presence_boost", "treble_boost")
BAND_TIMES = ((10.0, 200.0), (5.0, 150.0), (1.0, 50.0))  # (attack, release) ms, AME:207-209
BAND_DEFAULTS = (("low_thresh", -25.0, "low_ratio", 6.0),
                 ("mid_thresh", -20.0, "mid_ratio", 3.0),
                 ("high_thresh", -15.0, "high_ratio", 4.0))  # AME:67-72


# ----------------------------------------------------------------- chunking
def pydub_len_ms(frames: int, rate: int) -> int:
    """pydub AudioSegment.__len__: round(1000 * frames / rate)."""
    return round(1000 * (float(frames) / rate))


def pydub_frame(ms, rate: int) -> int:
    """pydub _parse_position: int(ms * (rate / 1000.0))."""
    return int(ms * (rate / 1000.0))


def chunk_bounds(frames: int, rate: int):
    """Frame ranges of AME's `for start_ms in range(0, len(audio), 30000)` slices.
    The stop of the last slice may exceed `frames` (pydub pads <= 2 ms of silence)
    or fall short of it (frames past the last whole ms are dropped)."""
    n_ms = pydub_len_ms(frames, rate)
    out = []
    for s in range(0, n_ms, CHUNK_MS):
        e = min(s + CHUNK_MS, n_ms)
        a, b = pydub_frame(s, rate), pydub_frame(e, rate)
        if b - min(b, frames) > (2 * (rate / 1000.0)):
            raise ValueError("TooManyMissingFrames")
        out.append((a, b))
    return out


def check_chunk_geometry(bounds, nominal: int, rate: int, multiband: bool):
    """The tile-major timeline needs every 30 s chunk but the last to hold exactly
    `nominal` frames, and (with the multiband stage) pydub's overlay to keep each
    chunk's length (AME:210 re-slices the low band by ms: `seg[0:len(seg)]`).

    Both hold at every rate above 2 kHz: a chunk starts and ends at
    int(ms * (rate / 1000.0)) for whole ms (AME:54), the same expression that the
    overlay's re-slice evaluates after `len()` rounds the length back to the same
    ms (the rounding error 1000 / rate < 0.5 ms), and the checked rates 8-192 kHz
    give uniform chunks up to the 2^31-frame limit (tests/test_oracle.py).  Below
    2 kHz the reference's slicing can drop or pad frames per chunk; the engine
    refuses such input instead of mis-slicing it."""
    for a, b in bounds[:-1]:
        if b - a != nominal:
            raise NotImplementedError(f"non-uniform 30 s chunk lengths at {rate} Hz")
    if multiband:
        for a, b in bounds:
            f = b - a
            if pydub_frame(pydub_len_ms(f, rate), rate) != f:
                raise NotImplementedError(f"pydub overlay re-slicing changes a chunk's length at {rate} Hz")


def kweight_sub(tile: int) -> int:
    """K-weighting lanes per tile (the library takes any divisor of the tile as the
    K-weighting tables' sub-tile).  1: the mono filter keeps one lane per tile — 3
    sub-tiles of 75 frames (3x the lanes, 3x the look-back blocks) measured 0.083
    against 0.066 ms on C2 (round 5; 25-frame sub-tiles 2x slower in round 2).
    MM_KW_SUB sets it for A/B runs."""
    env = os.environ.get("MM_KW_SUB")
    if env:
        sub = int(env)
        if sub >= 1 and tile % sub == 0:
            return sub
    return 1


def choose_tile(chunk_frames: int, preferred: int | None = None) -> int:
    """The tile length of a chunk: `preferred` (DEFAULT_TILE) when it divides the chunk,
    else the divisor in [64, 512] nearest to it, counting the walk-block padding of the
    compressor's plane rows (tiles are padded to whole WALK_BLOCK-row blocks) as distance."""
    preferred = preferred or DEFAULT_TILE
    if chunk_frames % preferred == 0:
        return preferred
    best, best_cost = 0, None
    for t in range(64, 513):
        if chunk_frames % t == 0:
            cost = abs(t - preferred) / preferred + ((t + WALK_BLOCK - 1) // WALK_BLOCK * WALK_BLOCK - t) / t
            if best_cost is None or cost < best_cost:
                best, best_cost = t, cost
    if not best:
        raise NotImplementedError(
            f"no tile length in [64, 512] divides the {chunk_frames}-frame chunk; rate unsupported")
    return best


# --------------------------------------------------------------- EQ (AME:146-194)
def shelf_section(rate, cutoff_hz, gain_db, kind, q=0.707):
    """apply_shelf_filter coefficients (AME:170-182) -> (b0, b1, b2, a1, a2)."""
    nyq = 0.5 * rate
    wn = cutoff_hz / nyq
    g = 10.0 ** (gain_db / 20.0)
    cw = np.cos(wn * 2 * np.pi)
    alpha = np.sin(wn * 2 * np.pi) / (2.0 * q)
    sq = np.sqrt(g)
    if kind == "low":
        b0 = g * ((g + 1) - (g - 1) * cw + 2 * sq * alpha)
        b1 = 2 * g * ((g - 1) - (g + 1) * cw)
        b2 = g * ((g + 1) - (g - 1) * cw - 2 * sq * alpha)
        a0 = (g + 1) + (g - 1) * cw + 2 * sq * alpha
        a1 = -2 * ((g - 1) + (g + 1) * cw)
        a2 = (g + 1) + (g - 1) * cw - 2 * sq * alpha
    else:
        b0 = g * ((g + 1) + (g - 1) * cw + 2 * sq * alpha)
        b1 = -2 * g * ((g - 1) + (g + 1) * cw)
        b2 = g * ((g + 1) + (g - 1) * cw - 2 * sq * alpha)
        a0 = (g + 1) - (g - 1) * cw + 2 * sq * alpha
        a1 = 2 * ((g - 1) - (g + 1) * cw)
        a2 = (g + 1) - (g - 1) * cw - 2 * sq * alpha
    return (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)


def peak_section(rate, center_hz, gain_db, q=1.0):
    """apply_peak_filter coefficients (AME:185-193)."""
    nyq = 0.5 * rate
    wn = center_hz / nyq
    g = 10.0 ** (gain_db / 20.0)
    alpha = np.sin(wn * 2 * np.pi) / (2.0 * q)
    b0, b1, b2 = 1 + alpha * g, -2 * np.cos(wn * 2 * np.pi), 1 - alpha * g
    a0, a1, a2 = 1 + alpha / g, -2 * np.cos(wn * 2 * np.pi), 1 - alpha / g
    return (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)


def eq_sections(rate, params):
    """Active EQ sections in AME order (AME:154-161); 0 dB stages are skipped
    (AME:171,186 `if gain_db == 0: return samples`)."""
    bass, mid, pres, treb = (params.get(k, 0.0) for k in EQ_KEYS)
    secs = []
    if bass != 0:
        secs.append(shelf_section(rate, 250, bass, "low"))
    if -mid != 0:
        secs.append(peak_section(rate, 1000, -mid))
    if pres != 0:
        secs.append(peak_section(rate, 4000, pres))
    if treb != 0:
        secs.append(shelf_section(rate, 8000, treb, "high"))
    return secs


LOW_CROSSOVER, HIGH_CROSSOVER = 250, 4000  # apply_multiband_compressor defaults (AME:196)

# ITU-R BS.1770-4 Annex 2 true-peak interpolator: order 48, 4 phases x 12 taps, every
# tap a multiple of 2^-13 (written here as the integers H * 8192; phases 2 and 3 are
# phases 1 and 0 reversed).  The -12 dB attenuate / restore pair of the standard is
# fixed-point headroom and is omitted.  csrc/meter.hip carries the same integers.
_TRUE_PEAK_C = ((14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68),
                (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155))
TRUE_PEAK_TAPS = np.array([_TRUE_PEAK_C[0], _TRUE_PEAK_C[1], _TRUE_PEAK_C[1][::-1], _TRUE_PEAK_C[0][::-1]],
                          dtype=np.float64) / 8192.0
TRUE_PEAK_TAPS.setflags(write=False)

# The true-peak ceiling (include/mastering.h: mm_ceiling).  The library works on the
# integer ceiling alone and never evaluates a power.
CEILING_MAX_WINDOW = 1024  # mm_ceiling_max_window()


def ceiling_q28(db: float) -> int:
    """A ceiling in dBTP as mm_job.ceiling_q28: floor(10**(db/20) * 2**28), for db in [-24, 0]."""
    db = float(db)
    if not -24.0 <= db <= 0.0:  # (NaN fails both comparisons)
        raise ValueError(f"true-peak ceiling {db!r} dBTP outside [-24, 0]")
    return int(math.floor(10.0 ** (db / 20.0) * 2.0 ** 28))


def ceiling_window(rate: int) -> int:
    """The chain's look-ahead window in frames: 5 ms, round-half-even(rate / 200) computed
    in integers (220 at 44.1 kHz), within [1, CEILING_MAX_WINDOW]."""
    q, rem = divmod(int(rate), 200)
    if rem > 100 or (rem == 100 and q % 2 == 1):
        q += 1
    return min(CEILING_MAX_WINDOW, max(1, q))


def level_clu(lufs: float) -> int:
    """A delivery's loudness target in LUFS as mm_delivery.level_clu: round(100 * lufs)
    centi-LU, for lufs in [-40, -5] (include/mastering.h: mm_level; 0 means off there)."""
    lufs = float(lufs)
    if not -40.0 <= lufs <= -5.0:  # (NaN fails both comparisons)
        raise ValueError(f"loudness target {lufs!r} LUFS outside [-40, -5]")
    return int(round(100.0 * lufs))


# The sample-rate converter (include/mastering.h: mm_resampler).  The library convolves
# integers with the integer taps designed here and never evaluates a window.
RESAMPLE_MAX_PHASES = 640   # L and M
RESAMPLE_MAX_TAPS = 1024    # K
RESAMPLE_CROSSINGS = 64     # zero crossings a side
RESAMPLE_CUTOFF = 0.475     # of the lower sample rate
RESAMPLE_BETA = 10.0        # Kaiser window
RESAMPLE_ONE = 1 << 22      # DC gain of every phase


def resample_geometry(rate_in: int, rate_out: int):
    """(L, M, K) of the polyphase converter rate_in -> rate_out: L = rate_out / g and
    M = rate_in / g with g their gcd, K = 2 * ceil(64 * max(L, M) / L) taps a phase (64
    zero crossings a side, stretched by the decimation ratio).  ValueError outside the
    library's limits (L, M <= 640, K <= 1024, L != M)."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError(f"sample rates must be positive (got {rate_in} -> {rate_out})")
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    if L == M:
        raise ValueError(f"resampling {rate_in} -> {rate_out} Hz: the rates are equal")
    K = 2 * ((RESAMPLE_CROSSINGS * max(L, M) + L - 1) // L)
    if L > RESAMPLE_MAX_PHASES or M > RESAMPLE_MAX_PHASES or K > RESAMPLE_MAX_TAPS:
        raise ValueError(f"resampling {rate_in} -> {rate_out} Hz needs L = {L}, M = {M}, K = {K}: outside the "
                         f"converter's limits (L, M <= {RESAMPLE_MAX_PHASES}, K <= {RESAMPLE_MAX_TAPS})")
    return L, M, K


@functools.lru_cache(maxsize=16)
def _resample_table(rate_in: int, rate_out: int):
    L, M, K = resample_geometry(rate_in, rate_out)
    half = K // 2
    p = np.arange(L, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    d = p + (k - half) * L                    # distance in ticks of the L-times-oversampled grid
    t = d / L
    u = t / half
    fc = RESAMPLE_CUTOFF * min(1.0, L / M)
    w = np.where(np.abs(u) <= 1.0,
                 np.i0(RESAMPLE_BETA * np.sqrt(np.maximum(1.0 - u * u, 0.0))) / np.i0(RESAMPLE_BETA), 0.0)
    h = 2.0 * fc * np.sinc(2.0 * fc * t) * w
    h = h / h.sum(axis=1, keepdims=True)
    c = np.rint(h * RESAMPLE_ONE).astype(np.int64)
    for row in c:  # DC gain exactly 2^22: the residue goes to the first tap of largest magnitude
        row[int(np.argmax(np.abs(row)))] += RESAMPLE_ONE - int(row.sum())
    c = np.ascontiguousarray(c, dtype=np.int32)
    assert c.shape == (L, K) and int(np.abs(c.astype(np.int64)).sum(axis=1).max()) < 1 << 24
    c.setflags(write=False)
    head = np.array([L, M, K], np.int64).tobytes()
    key = int.from_bytes(hashlib.blake2b(head + c.tobytes(), digest_size=8).digest(), "little") or 1
    return L, M, K, c, key


def resample_taps(rate_in: int, rate_out: int):
    """The converter's taps (L, M, K, c): c int32 [L][K] (read-only), a Kaiser-windowed
    sinc (beta 10, cutoff 0.475 of the lower rate) sampled at d = p + (k - K/2) * L ticks
    of the oversampled grid for phase p and tap k, every row normalised to unit sum in
    f64, rounded to multiples of 2^-22 and corrected on its largest tap so that each
    phase has DC gain exactly 2^22.  ValueError for a pair outside the limits."""
    return _resample_table(int(rate_in), int(rate_out))[:4]


def resample_key(rate_in: int, rate_out: int) -> int:
    """Content key (nonzero 64-bit) of resample_taps' table: the context caches its device
    copy by this key (mm_resampler.taps_key)."""
    return _resample_table(int(rate_in), int(rate_out))[4]


def resample_frames(frames: int, L: int, M: int) -> int:
    """Output frames of the converter: ceil(frames * L / M) (mm_resample_frames)."""
    return -(-int(frames) * int(L) // int(M))


# The reference match's linear-phase FIR (include/mastering.h: mm_fir).  The library convolves
# integers with the integer taps designed here and never evaluates a window or a response.
MATCH_MAX_TAPS = 8191       # K (mm_fir's limit)
MATCH_FFT = 1 << 17         # points of the inverse real FFT the impulse response comes from
MATCH_BETA = 6.0            # Kaiser window
MATCH_ONE = 1 << 22         # a tap of 1.0
MATCH_SUM_LIMIT = 1 << 24   # sum |c| below this


def match_length(rate: int) -> int:
    """Taps of the match filter at `rate`: min(8191, 2 * floor(rate * 1024 / 44100) - 1), about
    46 ms (2047 at 44.1 kHz, 2227 at 48 kHz, 4457 at 96 kHz, 8191 at 192 kHz)."""
    return min(MATCH_MAX_TAPS, 2 * (int(rate) * 1024 // 44100) - 1)


def _band_centres(rate: int) -> np.ndarray:
    """Centres in Hz of the spectrum report's 1/3-octave bands at `rate` (mm_spectrum_bands; no GPU)."""
    from . import native
    edges = np.zeros((native.SPECTRUM_MAX_BANDS, 3), np.float64)
    n = native.load().mm_spectrum_bands(int(rate), native.SPECTRUM_MAX_BANDS, edges.ctypes.data_as(native.c_double_p))
    if n < 0:
        raise ValueError(f"mm_spectrum_bands failed ({n}): rate below 2000 Hz")
    return edges[:n, 1].copy()


def _match_half(rate: int, gains_db, K: int | None):
    """(K, the first (K + 1) / 2 taps of the match filter in f64, in units of 2^-22, untrimmed)."""
    rate = int(rate)
    K = match_length(rate) if K is None else int(K)
    if K < 3 or K > MATCH_MAX_TAPS or K % 2 == 0:
        raise ValueError(f"the match filter has an odd number of taps in [3, {MATCH_MAX_TAPS}], not {K}")
    centres = _band_centres(rate)
    g = np.asarray(gains_db, dtype=np.float64)
    if g.shape != centres.shape:
        raise ValueError(f"gains_db: {g.size} values for the {centres.size} bands at {rate} Hz")
    H = (K - 1) // 2
    f = np.arange(MATCH_FFT // 2 + 1, dtype=np.float64) * (rate / MATCH_FFT)
    with np.errstate(divide="ignore"):
        db = np.interp(np.log2(f), np.log2(centres), g)  # (log2 0 = -inf: the first gain)
    h = np.fft.irfft(10.0 ** (db / 20.0), MATCH_FFT)  # zero phase: h[-n] = h[n]
    return K, h[:H + 1][::-1] * np.kaiser(K, MATCH_BETA)[:H + 1] * MATCH_ONE  # taps 0..H (tap H: h[0])


def match_taps(rate: int, gains_db, K: int | None = None, trim: float = 1.0) -> np.ndarray:
    """The match filter's taps c[K], int32 multiples of 2^-22, exactly symmetric, for one gain in
    dB per band of the spectrum report at `rate` (engine.spectrum_bands).  The response in dB is
    piecewise-linear over log2 f through (centre, gain), constant below the first centre and
    above the last; its zero-phase impulse response is the inverse real FFT of MATCH_FFT points;
    the centre K taps (default match_length(rate); odd, 3..8191) are taken under a Kaiser window
    (beta 6) and multiplied by `trim`; the first (K + 1) / 2 are rounded and mirrored.
    ValueError for a K mm_fir refuses, a gain count other than the bands', or sum |c| >= 2^24
    (match_headroom gives the trim under which the table fits)."""
    K, half = _match_half(rate, gains_db, K)
    H = (K - 1) // 2
    c = np.rint(half * float(trim)).astype(np.int64)
    c = np.concatenate([c, c[:H][::-1]])
    if int(np.abs(c).sum()) >= MATCH_SUM_LIMIT:
        raise ValueError("the match filter's taps have sum |c| >= 2^24: design them under match_headroom's trim")
    return np.ascontiguousarray(c, dtype=np.int32)


def match_headroom(rate: int, gains_db, K: int | None = None) -> float:
    """The largest trim <= 1 under which match_taps' table keeps sum |c| < 2^24, the bound the
    filter's exactness rests on: 1.0 when the untrimmed table does, else (2^24 - K) / sum |c| of
    the unrounded taps (rounding moves the sum by at most K / 2).  A curve whose boosts and cuts
    alternate has a sum far above its largest gain, so curves of a few dB already need it."""
    K, half = _match_half(rate, gains_db, K)
    total = 2.0 * float(np.abs(half[:-1]).sum()) + float(abs(half[-1]))
    return 1.0 if total + K < MATCH_SUM_LIMIT else (MATCH_SUM_LIMIT - K) / total


def match_trim(K: int, peak_unclipped: int) -> float:
    """The factor by which the trim of the taps is lowered after a pass whose largest |y| before
    the clip was `peak_unclipped` > 32767: (32767 - K / 128 - 1) / peak_unclipped, under which the
    second pass cannot clip."""
    return (32767.0 - K / 128.0 - 1.0) / float(peak_unclipped)


def fir_response_db(taps, rate: int, freqs) -> np.ndarray:
    """20 log10 |C(f)| of integer symmetric taps (c / 2^22) at `freqs` Hz: the response the
    library's filter realises, evaluated directly (c[H] + 2 sum_d c[H + d] cos(2 pi f d / rate))."""
    c = np.asarray(taps, dtype=np.float64)
    H = (c.size - 1) // 2
    w = 2.0 * np.pi * np.asarray(freqs, dtype=np.float64) / float(rate)
    d = np.arange(1, H + 1, dtype=np.float64)
    amp = (c[H] + 2.0 * (np.cos(np.outer(w, d)) @ c[H + 1:])) / MATCH_ONE
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.abs(amp))


def match_key(taps) -> int:
    """Content key (nonzero 64-bit) of a table of taps: the context caches its device copy by
    this key (mm_fir.taps_key)."""
    c = np.ascontiguousarray(taps, dtype=np.int32)
    head = np.array([c.size], np.int64).tobytes()
    return int.from_bytes(hashlib.blake2b(head + c.tobytes(), digest_size=8).digest(), "little") or 1


def crossover_sections(rate, low_hz=LOW_CROSSOVER, high_hz=HIGH_CROSSOVER):
    """AME:197-198: butter(4) LP and HP as 2 SOS sections each."""
    lp = scipy.signal.butter(4, low_hz, btype="lowpass", fs=rate, output="sos")
    hp = scipy.signal.butter(4, high_hz, btype="highpass", fs=rate, output="sos")
    secs = []
    for sos in (lp, hp):
        for row in sos:
            assert row[3] == 1.0
            secs.append((row[0], row[1], row[2], row[4], row[5]))
    return secs


def kweight_sections(rate):
    """pyloudnorm 0.1.1 K-weighting: high_shelf(G=4, Q=1/sqrt2, 1500 Hz) then
    high_pass(G=0, Q=0.5, 38 Hz), RBJ forms normalised by a0."""
    out = []
    for G, Q, fc, kind in ((4.0, 1 / np.sqrt(2), 1500.0, "high_shelf"), (0.0, 0.5, 38.0, "high_pass")):
        A = 10 ** (G / 40.0)
        w0 = 2.0 * np.pi * (fc / rate)
        alpha = np.sin(w0) / (2.0 * Q)
        if kind == "high_shelf":
            b = (A * ((A + 1) + (A - 1) * np.cos(w0) + 2 * np.sqrt(A) * alpha),
                 -2 * A * ((A - 1) + (A + 1) * np.cos(w0)),
                 A * ((A + 1) + (A - 1) * np.cos(w0) - 2 * np.sqrt(A) * alpha))
            a = ((A + 1) - (A - 1) * np.cos(w0) + 2 * np.sqrt(A) * alpha,
                 2 * ((A - 1) - (A + 1) * np.cos(w0)),
                 (A + 1) - (A - 1) * np.cos(w0) - 2 * np.sqrt(A) * alpha)
        else:
            b = ((1 + np.cos(w0)) / 2, -(1 + np.cos(w0)), (1 + np.cos(w0)) / 2)
            a = (1 + alpha, -2 * np.cos(w0), 1 - alpha)
        bn = np.array(b) / a[0]
        an = np.array(a) / a[0]
        out.append((bn[0], bn[1], bn[2], an[1], an[2]))
    return out


# ------------------------------------------------------- tile-scan matrices
def transition_matrix(sections, branches):
    """One zero-input step of cascaded DF2T sections.  `branches` lists the number
    of sections per branch; every branch is fed by the same input.  State per
    section (z0, z1) in section order, padded to MAX_DIM."""
    A = np.zeros((MAX_DIM, MAX_DIM))
    nsec = len(sections)
    for col in range(2 * nsec):
        z = np.zeros(2 * nsec)
        z[col] = 1.0
        new = z.copy()
        s = 0
        for nb in branches:
            x = 0.0
            for _ in range(nb):
                b0, b1, b2, a1, a2 = sections[s]
                z0, z1 = z[2 * s], z[2 * s + 1]
                y = b0 * x + z0
                new[2 * s] = b1 * x - a1 * y + z1
                new[2 * s + 1] = b2 * x - a2 * y
                x = y
                s += 1
        A[: 2 * nsec, col] = new
    return A


LB_THREADS = 256  # threads per block of the single-pass IIR kernels (csrc/lookback.h)



TILE_POW, BLK_POW = 8, 65


def lookback_tables(A, tile, tpb):
    """Transition powers for the in-kernel tile carry (csrc/lookback.h):
    tile_pow[k] = Phi_T^(2^k) with Phi_T = A^tile (block-local Kogge-Stone and
    the per-tile carry application), blk_pow[e] = Phi_B^e with Phi_B = Phi_T^tpb
    (decoupled look-back over up to 64 predecessor blocks per window)."""
    phi = np.linalg.matrix_power(A, tile)
    tp = [phi]
    for _ in range(TILE_POW - 1):
        tp.append(tp[-1] @ tp[-1])
    pb = np.linalg.matrix_power(phi, tpb)
    bp = [np.eye(A.shape[0])]
    for _ in range(BLK_POW - 1):
        bp.append(bp[-1] @ pb)
    return {"tile_pow": np.stack(tp), "blk_pow": np.stack(bp)}


# ------------------------------------------------ compressor (pydub constants)
def _ratio_to_db(ratio):
    return 20 * math.log(float(ratio), 10)


@functools.lru_cache(maxsize=64)
def max_att_table(threshold, ratio):
    """pydub compress_dynamic_range's max_attenuation as a function of the
    integer audioop.rms value r in [0, 32768] (exact Python float expressions)."""
    thresh_rms = (float(1 << 16) / 2) * (10 ** (float(threshold) / 20))
    out = np.empty(32769, np.float64)
    k = 1 - (1.0 / ratio)
    for r in range(32769):
        if r == 0:
            dbo = 0.0
        else:
            dbo = max(_ratio_to_db(r / thresh_rms), 0)
        out[r] = k * dbo
    out.setflags(write=False)
    return out, thresh_rms


@functools.lru_cache(maxsize=64)
def step_table(threshold, ratio, attack_frames, release_frames):
    """Per integer rms r: {M, M/attack_frames, M/release_frames, 0} — the three
    numbers pydub's loop derives from rms_at(i) (max_attenuation,
    attenuation_inc, attenuation_dec), each a correctly rounded Python float."""
    M, _ = max_att_table(threshold, ratio)
    out = np.zeros((32769, 4), np.float64)
    out[:, 0] = M
    out[:, 1] = M / attack_frames   # numpy float64 division: IEEE, correctly rounded
    out[:, 2] = M / release_frames
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=64)
def table_key(threshold, ratio):
    """Content key of max_att_table(threshold, ratio) (nonzero 64-bit): the device
    caches a band's table by this key, not by the host pointer, whose memory an
    evicted table may hand to a different one."""
    M, _ = max_att_table(threshold, ratio)
    return int.from_bytes(hashlib.blake2b(M.tobytes(), digest_size=8).digest(), "little") | 1


def band_constants(rate, threshold, ratio, attack, release):
    table, thr = max_att_table(float(threshold), float(ratio))
    af = attack * (rate / 1000.0)
    rf = release * (rate / 1000.0)
    return {"table": table, "thresh_rms": thr, "attack_frames": af, "release_frames": rf, "look": int(af),
            "lut": step_table(float(threshold), float(ratio), af, rf),
            "lut_key": table_key(float(threshold), float(ratio))}


# ---------------------------------------------------- loudness block geometry
def loudness_blocks(frames: int, rate: int, block_size: float = 0.4):
    """pyloudnorm integrated_loudness block bounds (clamped to the data)."""
    T = frames / rate
    step = 1.0 - 0.75
    nblocks = int(np.round(((T - block_size) / (block_size * step)))) + 1
    j = np.arange(0, nblocks)
    lo = np.array([int(block_size * (jj * step) * rate) for jj in j], dtype=np.int64)
    hi = np.array([int(block_size * (jj * step + 1) * rate) for jj in j], dtype=np.int64)
    lo = np.minimum(lo, frames)
    hi = np.minimum(hi, frames)
    bounds = np.unique(np.concatenate([[0], lo, hi, [frames]]))
    return nblocks, lo, hi, bounds.astype(np.int64), 1.0 / (block_size * rate)


@functools.lru_cache(maxsize=16)
def saturation_table(percent):
    """apply_saturation (AME:128-134) on the int16 grid: entry k + 32768 is the
    reference's expression evaluated by numpy on the decoded sample k / 32768
    (AME:117-121: int16 -> float32 / 2**15), k = -32768..32767.  numpy's float32
    tanh is a SIMD polynomial that is not correctly rounded, so the device cannot
    recompute it bit for bit; it gathers these values instead (the per-sample work
    stays on the GPU; this is host-side design, like max_att_table).  numpy's result
    is a function of the element's value only (checked in tests/test_ops.py against
    2-D and strided evaluations), so the table equals the reference's output on
    every decoded PCM16 sample.  Returns (table float32[65536], content key)."""
    k = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    samples = k.astype(np.float32) / (2 ** 15)
    mix = (percent / 100.0) ** 2
    clean_signal = samples
    distorted_signal = np.tanh(samples * (1 + mix * 4))
    tab = np.ascontiguousarray((1 - mix) * clean_signal + mix * distorted_signal, dtype=np.float32)
    assert tab.dtype == np.float32 and tab.shape == (65536,)
    tab.setflags(write=False)
    key = int.from_bytes(hashlib.blake2b(tab.tobytes(), digest_size=8).digest(), "little") or 1
    return tab, key


def saturation_consts(percent):
    if percent == 0:
        return 0, 1.0, 0.0, 1.0
    mix = (percent / 100.0) ** 2
    return 1, float(np.float32(1 - mix)), float(np.float32(mix)), float(np.float32(1 + mix * 4))
