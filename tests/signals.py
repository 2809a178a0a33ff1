"""A catalogue of structured test signals, and the oracle's view of their structure.

The GPU comparisons otherwise feed stationary pink noise, on which every compressor
band is either always or never above its threshold and the loudness gates cut no
block.  The builders here are deterministic int16 signals whose *structure* selects
the other branches of the envelope solve (csrc/compressor.hip) and of the loudness
gate (csrc/gate.hip): sparse active tiles, partial tiles, the table's last row,
states many binades above the current M, blocks cut by either gate.

`structure(pcm, rate, params)` states, from the oracle alone, what a signal does to
the chain; tests/test_signals.py pins the property each signal exists for, and
tests/test_gpu_signals.py compares the device with the oracle on them.

The default length is 3.0 s at 44.1 kHz: 588 tiles of 225 frames, 2.3 column blocks
of 256 tiles, the shortest track that crosses two column-block seams.
"""
import numpy as np

from mastering_amd import design
from mastering_amd.synth import pink_noise_pcm16
from oracle import mastering_oracle as oracle
from oracle import thirdparty_restated as tp

RATE, SECONDS = 44100, 3.0
# band-level inputs: more than one column block of 256 operator tiles (125 frames), ragged last tile
BAND_FRAMES, HOLD = 33007, 4501

# the chain settings of the GPU comparisons (== tests/test_gpu_parity.py): the full chain
# at the reference's default thresholds, and at thresholds every band crosses
P_FULL = {"bass_boost": 4.0, "mid_cut": 3.0, "presence_boost": 1.0, "treble_boost": 3.0,
          "saturation": 30, "width": 1.3, "multiband": True, "lufs": -14.0}
P_HOT = dict(P_FULL, low_thresh=-16.0, mid_thresh=-21.0, high_thresh=-27.0)


def _layout(cols, channels):
    """[N] (mono: the first column) or [N, 2] int16 from per-channel float columns."""
    q = [np.clip(np.round(c), -32768, 32767).astype(np.int16) for c in cols]
    return q[0].copy() if channels == 1 else np.ascontiguousarray(np.stack(q[:2], axis=1))


def _pink(n, rate, seed, level_dbfs):
    """Stereo pink noise as float columns (the mono form of a signal is its left column)."""
    p = pink_noise_pcm16(n, rate, 2, track=seed, level_dbfs=level_dbfs).astype(np.float64)
    return [p[:, 0], p[:, 1]]


def bursts(seconds=SECONDS, rate=RATE, channels=2, period=0.3, on=0.06):
    """`on`-second bursts of 100 Hz + 1 kHz + 8 kHz sines (0.25 each) every `period`
    seconds, digital silence between: every band has sparse all-active tiles, so the
    compact ranking skips most tiles and super-tiles of four active tiles span gaps."""
    n = int(round(seconds * rate))
    t = np.arange(n) / rate
    x = 0.25 * (np.sin(2 * np.pi * 100 * t) + np.sin(2 * np.pi * 1000 * t) + np.sin(2 * np.pi * 8000 * t))
    gate = (np.arange(n) % int(round(period * rate))) < int(round(on * rate))
    left = x * gate * 32768
    return _layout([left, 0.9 * left], channels)


def square_fs(seconds=SECONDS, rate=RATE, channels=2, hz=60):
    """A full-scale square wave (+32767 / -32768), the right channel inverted in the
    second half: window rms at the top of the tables, a crossover that overshoots
    into the quantiser's clip, an overlay that saturates."""
    n = int(round(seconds * rate))
    hi = (np.arange(n) * 2 * hz // rate) % 2 == 0
    left = np.where(hi, 32767.0, -32768.0)
    right = left.copy()
    right[n // 2:] = np.where(hi[n // 2:], -32768.0, 32767.0)
    return _layout([left, right], channels)


def step_down(seconds=SECONDS, rate=RATE, channels=2, loud=0.4, drop_db=26.0):
    """Pink noise at -8 dBFS for `loud` seconds, then the same noise `drop_db` lower:
    deep attenuation, then a long hold and release over quiet tiles; most loudness
    blocks fall under the relative gate."""
    n = int(round(seconds * rate))
    cols = _pink(n, rate, 41, -8.0)
    k = int(round(loud * rate))
    for c in cols:
        c[k:] *= 10.0 ** (-drop_db / 20.0)
    return _layout(cols, channels)


def fade_in_cut(seconds=SECONDS, rate=RATE, channels=2, fade=2.44):
    """Pink noise faded in exponentially from -96 to -12 dBFS over `fade` seconds,
    then digital silence: blocks under the absolute gate, blocks under the relative
    gate, and a first active tile that lies late in the chunk.  Successive blocks
    lie ~3.4 LU apart; `fade` is chosen so that one of them passes the relative gate
    by less than 1 LU (a threshold 1 LU higher would cut it)."""
    n = int(round(seconds * rate))
    k = min(n, int(round(fade * rate)))
    env = np.zeros(n)
    env[:k] = 10.0 ** (-84.0 * (1.0 - np.arange(k) / (fade * rate)) / 20.0)
    return _layout([c * env for c in _pink(n, rate, 42, -12.0)], channels)


def clicks(seconds=SECONDS, rate=RATE, channels=2, every=0.11):
    """Full-scale single-sample clicks on alternating channels (alternating sign in
    mono) every `every` seconds over -60 dBFS noise: only the fastest band ever
    crosses its threshold, and the loudness gain drives the limiter."""
    n = int(round(seconds * rate))
    cols = _pink(n, rate, 43, -60.0)
    for k, i in enumerate(range(int(0.05 * rate), n, int(round(every * rate)))):
        if channels == 1:
            cols[0][i] = 32767.0 if k % 2 == 0 else -32768.0
        else:
            cols[k % 2][i] = 32767.0
    return _layout(cols, channels)


def sub_gate(seconds=SECONDS, rate=RATE, channels=2):
    """+-1 LSB noise with runs of zeros: not silent, yet every loudness block lies
    under -70 LUFS, so the loudness is -inf and the gain inf."""
    n = int(round(seconds * rate))
    rng = np.random.default_rng(44)
    x = rng.integers(-1, 2, size=(n, 2)).astype(np.float64)
    x[(np.arange(n) // 2000) % 3 == 1] = 0.0
    return _layout([x[:, 0], x[:, 1]], channels)


def chunk_seam(seconds=31.0, rate=RATE, channels=2, seam=30.0):
    """A track longer than one 30 s chunk in which a burst and the loud part of a
    step_down both straddle the chunk seam, where the window and the attenuation
    restart: quiet pink noise, -8 dBFS from 0.2 s before the seam to 0.2 s after it,
    and the bursts of `bursts` shifted so that one lies across the seam."""
    n = int(round(seconds * rate))
    cols = _pink(n, rate, 45, -8.0)
    a, b = int(round((seam - 0.2) * rate)), int(round((seam + 0.2) * rate))
    period, on = int(round(0.3 * rate)), int(round(0.06 * rate))
    shift = (int(round(seam * rate)) - on // 2) % period
    t = np.arange(n) / rate
    x = 0.25 * (np.sin(2 * np.pi * 100 * t) + np.sin(2 * np.pi * 1000 * t) + np.sin(2 * np.pi * 8000 * t))
    burst = x * (((np.arange(n) - shift) % period) < on) * 32768
    for k, c in enumerate(cols):
        c[:a] *= 10.0 ** (-26.0 / 20.0)
        c[b:] *= 10.0 ** (-26.0 / 20.0)
        c += burst * (1.0, 0.9)[k]
    return _layout(cols, channels)


CATALOGUE = {"bursts": bursts, "square_fs": square_fs, "step_down": step_down, "fade_in_cut": fade_in_cut,
             "clicks": clicks, "sub_gate": sub_gate}


# ----------------------------------------------------------------- band-level inputs
def band_r0(threshold, ratio):
    """The smallest integer rms with a nonzero max attenuation (mm_band.r0)."""
    nz = np.flatnonzero(design.max_att_table(float(threshold), float(ratio))[0])
    return int(nz[0]) if nz.size else 32769


def const_fs(frames=BAND_FRAMES, channels=1):
    """Every sample -32768: window rms 32 768, the last row of the table."""
    return np.full((frames,) if channels == 1 else (frames, channels), -32768, np.int16)


def staircase(r0, channels=1, hold=HOLD):
    """Constant levels held `hold` frames each around the table's first nonzero row
    `r0`.  A constant v (on every channel) has window rms exactly |v|, so after the
    loud first step the state sits some 15 binades above the tile's largest M."""
    levels = [20000, r0 + 1, r0, r0 - 1, r0, r0 + 2, 0, r0]
    x = np.repeat(np.array(levels, np.int16), hold)
    return x if channels == 1 else np.ascontiguousarray(np.repeat(x[:, None], channels, axis=1))


def band_settings(params=None):
    """[(threshold, ratio, attack ms, release ms)] of the three bands."""
    params = params or {}
    return [(float(params.get(tk, td)), float(params.get(rk, rd)), at, rel)
            for (tk, td, rk, rd), (at, rel) in zip(design.BAND_DEFAULTS, design.BAND_TIMES)]


def const_fs_bands(channels=1, frames=BAND_FRAMES):
    return [const_fs(frames, channels) for _ in range(3)]


def staircase_bands(channels=1, params=None, hold=HOLD):
    """(staircase at the low band's r0, staircase at the mid band's r0, zeros)."""
    (lt, lr, _, _), (mt, mr, _, _), _ = band_settings(params)
    lo, mid = staircase(band_r0(lt, lr), channels, hold), staircase(band_r0(mt, mr), channels, hold)
    return [lo, mid, np.zeros_like(lo)]


# ----------------------------------------------------------------- structure
def window_rms(band, look):
    """audioop.rms of the window [max(0, i - look), i) for every frame i, as pydub's
    compressor evaluates it (floor of the f64 sqrt of sum / samples; 0 when empty)."""
    b = band.astype(np.int64)
    ch = 1 if b.ndim == 1 else b.shape[1]
    e2 = b * b if b.ndim == 1 else (b * b).sum(axis=1)
    cs = np.concatenate([[0], np.cumsum(e2)])
    i = np.arange(b.shape[0])
    lo = np.maximum(i - look, 0)
    n = (i - lo) * ch
    S = cs[i] - cs[lo]
    rms = np.zeros(b.shape[0], np.int64)
    nz = n > 0
    rms[nz] = np.floor(np.sqrt(S[nz] / n[nz])).astype(np.int64)
    return rms


def _binade(x):
    return np.frexp(x)[1] - 1


def band_structure(band, rate, threshold, ratio, attack, release, tile):
    """One band of one chunk: active frames (rms >= r0), quiet / partial / all-active
    tiles of `tile` frames, the largest rms, the largest binade distance between the
    state entering an active frame and that frame's M, and the per-frame M."""
    bc = design.band_constants(rate, threshold, ratio, attack, release)
    r0 = band_r0(threshold, ratio)
    rms = window_rms(band, bc["look"])
    M = bc["table"][np.minimum(rms, 32768)]
    active = rms >= r0
    _, att = oracle.compress_band(band, rate, threshold, ratio, attack, release, return_att=True)
    prev = np.concatenate([[0.0], att[:-1]])
    k = active & (prev > 0.0) & (M > 0.0)
    dist = int(np.max(_binade(prev[k]) - _binade(M[k]))) if k.any() else 0
    ntiles = -(-band.shape[0] // tile)
    per_tile = np.add.reduceat(active.astype(np.int64), np.arange(0, band.shape[0], tile))
    size = np.minimum(tile, band.shape[0] - np.arange(ntiles) * tile)
    return {"frames": int(band.shape[0]), "active": int(active.sum()), "tiles": int(ntiles),
            "quiet": int((per_tile == 0).sum()), "full": int((per_tile == size).sum()),
            "partial": int(((per_tile > 0) & (per_tile < size)).sum()),
            "max_rms": int(rms.max()) if rms.size else 0, "binades": dist, "r0": r0, "M": M,
            "attack_frames": bc["attack_frames"], "release_frames": bc["release_frames"]}


def block_loudness(y, rate):
    """pyloudnorm's gating of the float mix `y` ([N] or [N, 2]), as the oracle's meter
    runs it: (block loudnesses, blocks under the absolute gate, blocks over it but
    not over the relative gate, relative threshold, integrated loudness)."""
    mono = y.mean(axis=1) if y.ndim == 2 else y
    x = mono.copy()
    meter = tp.Meter(rate)
    for f in meter._filters.values():
        x[:] = f.apply_filter(x)
    nblocks, lo, hi, _, scale = design.loudness_blocks(x.shape[0], rate)
    z = np.array([(1.0 / (0.4 * rate)) * np.sum(np.square(x[a:b])) for a, b in zip(lo, hi)], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lj = -0.691 + 10.0 * np.log10(z)
        J = lj >= -70.0
        gamma_r = (-0.691 + 10.0 * np.log10(np.mean(z[J])) - 10.0) if J.any() else np.nan
        keep = (lj > gamma_r) & (lj > -70.0)
    return {"blocks": lj, "abs_gated": int((~J).sum()), "rel_gated": int((J & ~keep).sum()),
            "gamma_r": float(gamma_r), "loudness": float(oracle.integrated_loudness(mono, rate))}


def structure(pcm, rate, params):
    """What the oracle's chain makes of `pcm`: per chunk and band a band_structure
    (without the M sequence unless asked for through band_structure itself), their
    active frames summed (what mm_result.comp_active reports), and the loudness
    blocks of the post-chain mix."""
    N = pcm.shape[0]
    thr, rat = oracle.multiband_params(params)
    tile = design.choose_tile(design.pydub_frame(design.CHUNK_MS, rate))
    chunks, mix = [], []
    for s, e in oracle.chunk_ranges(N, rate):
        c = pcm[s:min(e, N)]
        if e > N:
            c = np.concatenate([c, np.zeros((e - N,) + pcm.shape[1:], np.int16)])
        x = oracle.equalize(oracle.saturation(oracle.pcm_to_float(c), params.get("saturation", 0)), rate, params)
        if params.get("width", 1.0) != 1.0:
            x = oracle.stereo_width(x, params.get("width"))
        q = oracle.quantize(x)
        if params.get("multiband"):
            bands = oracle.band_split(q, rate)
            chunks.append([band_structure(b, rate, t, r, at, rel, tile)
                           for b, t, r, (at, rel) in zip(bands, thr, rat, oracle.BAND_TIMES)])
            q = oracle.multiband(q, rate, thr, rat)
        mix.append(q)
    out = {"tile": tile, "chunks": chunks, "active": sum(b["active"] for ch in chunks for b in ch)}
    y = oracle.pcm_to_float(np.concatenate(mix))
    if y.shape[0] >= 0.4 * rate:
        out["loudness"] = block_loudness(y, rate)
    return out


def gate_margin(loud):
    """The smallest distance of a finite block loudness from -70 LUFS or from the
    relative threshold (inf when there is none)."""
    lj = loud["blocks"][np.isfinite(loud["blocks"])]
    d = [np.abs(lj + 70.0)]
    if np.isfinite(loud["gamma_r"]):
        d.append(np.abs(lj - loud["gamma_r"]))
    d = np.concatenate(d)
    return float(d.min()) if d.size else float("inf")
