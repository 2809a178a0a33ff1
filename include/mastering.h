/*
 * mastering.h — C-ABI of the MI355X mastering engine (libmastering_amd.so).
 *
 * Drop-in boundary for the reference's hot path
 *   worker/audio_mastering_engine.py:24  process_audio_from_gcs(gcs_uri, settings)
 * whose per-chunk DSP is AME:48-77 (saturation AME:128, EQ AME:146, width AME:136,
 * int16 quantise AME:123, multiband AME:196) and whose whole-track tail is
 * AME:80-89 (concat, LUFS normalise AME:212, soft limiter AME:224, int16).
 * The Python host (python-audio-mastering_amd/mastering_amd/engine.py) mirrors the
 * reference's `process(...)`/`apply_*` surface and calls these entry points via
 * ctypes.  Plain pointers and sizes only; no torch types.
 *
 * Conventions: every function returns 0 on success and a negative code on error;
 * mm_last_error() then holds a message (per context, NUL terminated).  One context
 * per host thread; a context owns one hipStream_t and its device work buffers.
 * Host-side filter design (EQ/crossover/K-weighting coefficients, compressor
 * max-attenuation tables, state-transition powers, chunk and loudness-block
 * geometry) is done by the caller in f64 with the reference's exact expressions
 * and passed in mm_job, so coefficients are bit-identical to the reference's.
 */
#ifndef MASTERING_AMD_H
#define MASTERING_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_OK 0
#define MM_ERR_ARG (-1)
#define MM_ERR_HIP (-2)
#define MM_ERR_RCCL (-3)
#define MM_ERR_STATE (-4)

#define MM_MAX_DIM 8      /* max IIR state dimension per channel (4 biquads) */
#define MM_TILE_POW 8     /* Phi_T^(2^k), k < MM_TILE_POW (tiles per block <= 256) */
#define MM_BLK_POW 65     /* Phi_B^e, e = 0..64 (one look-back window of 64 blocks) */

#define MM_OUT_I16 0 /* interleaved int16 PCM (what AME:89/98 writes)            */
#define MM_OUT_F32 1 /* interleaved f32 = the same PCM / 32768 (decoded form)    */

#define MM_IN_F32 0  /* input: interleaved f32 (decoded PCM16 / 32768)           */
#define MM_IN_I16 1  /* input: interleaved int16 PCM, decoded (x / 32768) on the GPU */
/* Integer PCM above 16 bits (no reference counterpart), decoded on the GPU
 * (mm_pcm_decode_device) at the top of the chain, which then runs as MM_IN_F32 on
 * the decoded floats: every delivered byte and every field of mm_result, mm_meter
 * and mm_ceiling equals those of the same call on that f32 array.  With s the
 * sign-extended little-endian sample:
 *   MM_IN_I24  packed 3-byte samples at any byte address: x = float(s) * 2^-23 (exact)
 *   MM_IN_I32  4-byte aligned int32: x = RN_f32(s) * 2^-31 (one round-to-nearest-even
 *              conversion, then an exact scale; INT32_MAX decodes to 1.0); a 24-bit
 *              sample left-justified (s << 8) gives the MM_IN_I24 value */
#define MM_IN_I24 2
#define MM_IN_I32 3

typedef struct mm_ctx mm_ctx;

/* One IIR stage = 1..2 branches of cascaded DF2T biquads fed by the same input.
 * sos[s] = {b0, b1, b2, a1, a2} (a0 == 1), branches laid out branch-major.
 * State-transition matrices of the zero-input recurrence (row-major
 * MM_MAX_DIM x MM_MAX_DIM, only dim x dim used) for the in-kernel tile carry
 * (csrc/lookback.h):
 *   phi_tile_pow[k]  Phi_T^(2^k), Phi_T = A^tile (A: one frame)
 *   phi_blk_pow[e]   Phi_B^e, Phi_B = Phi_T^tpb (tpb = tiles per thread block:
 *                    128 for stereo stages, 256 for mono ones) */
typedef struct mm_iir {
    int32_t nsec;            /* total sections (0 = stage inactive)           */
    int32_t nsec_branch0;    /* sections in branch 0 (rest are branch 1)      */
    int32_t dim;             /* state dim per channel = 2 * nsec              */
    int32_t tpb;             /* tiles per block the block powers were made for */
    int32_t tile;            /* frames per tile the tile powers were made for (the
                                job's tile; K-weighting: a divisor of it, its
                                lanes then run tile/kweight.tile sub-tiles each) */
    int32_t _pad;
    double sos[4][5];
    double phi_tile_pow[MM_TILE_POW][MM_MAX_DIM * MM_MAX_DIM];
    double phi_blk_pow[MM_BLK_POW][MM_MAX_DIM * MM_MAX_DIM];
} mm_iir;

/* Per-band pydub compress_dynamic_range parameters (AME:207-209). */
typedef struct mm_band {
    double thresh_rms;       /* 32768 * 10**(thr/20)                          */
    double attack_frames;    /* attack_ms * (rate/1000.0)                      */
    double release_frames;   /* release_ms * (rate/1000.0)                     */
    int32_t look;            /* int(attack_frames)                             */
    int32_t r0;              /* smallest rms r with M[r] != 0 (32769: none)     */
    const double *lut;       /* host table [32769][4] per integer rms r:
                                {M, M/attack_frames, M/release_frames, 0} with
                                M = (1-1/ratio)*max(20*log(r/thr,10), 0) (0 if r
                                == 0), all in Python float arithmetic          */
    uint64_t lut_key;        /* content key of the M column of lut (nonzero; the
                                context uploads a table only when the key of its
                                cached copy differs).  0: no key, uploaded on
                                every call                                     */
} mm_band;

/* A mastering job for one track (geometry + settings, all host memory). */
typedef struct mm_job {
    int64_t frames_in;       /* decoded input frames N                         */
    int64_t frames_proc;     /* processed frames (pydub 30 s slicing, AME:48-54) */
    int32_t channels;        /* 1 or 2                                         */
    int32_t rate;
    int32_t tile;            /* frames per tile T (divides every full chunk)    */
    int32_t tiles_per_chunk; /* K = chunk_frames / T                            */
    /* settings (AME:58-86) */
    float sat_keep;          /* f32(1 - mix)      (AME:131-134), mix=(s/100)^2 */
    float sat_mix;           /* f32(mix)                                        */
    float sat_drive;         /* f32(1 + 4*mix)                                  */
    int32_t sat_on;          /* saturation != 0                                 */
    double width;            /* AME:60-61                                       */
    int32_t width_on;        /* width != 1.0 and stereo                         */
    int32_t multiband_on;    /* AME:65                                          */
    int32_t lufs_on;         /* settings["lufs"] is not None (AME:84)           */
    int32_t out_kind;        /* MM_OUT_I16 | MM_OUT_F32                         */
    double lufs_target;
    mm_iir eq;               /* AME:154-161, active stages only                */
    mm_iir xover;            /* butter(4) LP250 (branch 0) + HP4000 (branch 1)  */
    mm_iir kweight;          /* pyloudnorm high_shelf then high_pass            */
    mm_band band[3];         /* low / mid / high                                */
    int32_t comp_warmup;     /* super-tiles of speculative warm-up walk before each one */
    int32_t comp_max_iters;  /* cap on fix-up sweeps (exactness check)          */
    int32_t comp_super;      /* frames per super-tile of the envelope solve (rounded to whole tiles) */
    int32_t in_kind;         /* MM_IN_F32 (0), MM_IN_I16, MM_IN_I24 or MM_IN_I32 */
    /* loudness geometry (pyloudnorm integrated_loudness, block 0.4 s, step 0.1 s) */
    int64_t n_blocks;
    const int64_t *block_lo; /* host [n_blocks] first frame of each block        */
    const int64_t *block_hi; /* host [n_blocks] one-past-last frame (clamped)    */
    int64_t n_segs;          /* distinct boundaries - 1                         */
    const int64_t *seg_bounds; /* host [n_segs+1] sorted distinct block bounds   */
    double block_scale;      /* 1.0 / (0.4 * rate)                              */
    /* apply_saturation (AME:128-134) tabulated on the int16 grid (ABI 4): host
       [65536] f32, entry k + 32768 = the reference's expression evaluated by numpy
       on k / 32768 (AME:121's decoded samples), so the exciter is bit-identical to
       numpy's float32 tanh wherever the input is a decoded int16 (always on the
       reference's path); NULL: the device tanhf (within 2 ulp) everywhere.  Inputs
       off the grid (f32 WAV) always take tanhf. */
    const float *sat_table;
    uint64_t sat_key;        /* content key of sat_table (nonzero; cached per context) */
    /* mastering report (ABI 5): meter the delivered output at the end of the chain,
       before any copy-out (mm_last_meters).  The loudness of the output is included
       when the job carries loudness geometry (kweight, blocks, segments), whether or
       not lufs_on is set.  0: the chain queues exactly what it queued before.  Bit 1
       (MM_REPORT_R128; a new value of this field, the struct is unchanged) adds the R 128
       report of the delivered output (mm_last_r128), which needs kweight.sos and rate.  Bit 2
       (MM_REPORT_QC; again a new value only) adds its QC report (mm_last_qc), which needs rate.
       Bit 3 (MM_REPORT_SPECTRUM; a new value only) adds its spectrum report (mm_last_spectrum,
       mm_last_spectrum_bins), which needs rate. */
    int32_t meter_on;
    /* true-peak ceiling (ABI 5, the former trailing pad): 0 = off, the chain queues exactly
       what it queued before; else the ceiling C as linear * 2^28, 2^24 <= C <= 2^28
       (-24.08 .. 0 dBTP; design.ceiling_q28).  The delivered output of the track is then
       rewritten in place (mm_ceiling, window of 5 ms) after the chain and before the
       report, so that its true peak, measured as mm_meter measures it, is at most C. */
    int32_t ceiling_q28;
} mm_job;

typedef struct mm_result {
    double loudness;         /* integrated loudness of the pre-gain mix (LUFS)   */
    double gain_linear;      /* 10 ** ((target - L) / 20), 1.0 if lufs off       */
    int64_t frames_out;      /* == frames_proc                                   */
    int32_t comp_iters;      /* fix-up sweeps the compressor needed              */
    int32_t _pad;
    int64_t comp_active;     /* active (M != 0) frames over the three bands      */
    int64_t comp_walked;     /* frames re-walked by the fix-up sweeps            */
    int64_t comp_jumped;     /* frames the sweeps crossed by exact release jumps */
} mm_result;

/* What was delivered (no reference counterpart: the reference never measures its
 * output).  Peaks are exact integers: with C = H * 8192 the taps of ITU-R BS.1770-4
 * Annex 2 (order 48, 4 phases x 12 taps, all multiples of 2^-13; the -12 dB
 * attenuate / restore pair of the standard is fixed-point headroom and is omitted)
 * and s = 0 outside [0, frames), the oversampled signal of a channel is
 *   Y[m][p] = sum_{k<12} C[p][k] * s[m-k],  m in [0, frames + 11), p in 0..3
 * (the full convolution: the 11-frame tail belongs to it), exact in int32. */
typedef struct mm_meter {
    int64_t frames;
    int32_t channels;
    int32_t _pad;
    int32_t sample_peak[2];     /* max |s|, 0..32768                                */
    int32_t true_peak_q28[2];   /* max |Y|; linear true peak = this / 2^28          */
    int64_t true_peak_frame[2]; /* smallest m at which it occurs (may be >= frames) */
    int64_t clipped[2];         /* samples with |s| >= 32767                        */
    int64_t overs[2];           /* m with max_p |Y[m][p]| > 2^28 (above 0 dBFS)     */
    double loudness;            /* pyloudnorm integrated loudness of the channel mean of
                                   s / 32768 as f32 (AME:213-218 applied to the output);
                                   NaN when not requested or shorter than 0.4 s      */
} mm_meter;

/* The true-peak ceiling (no reference counterpart), all integers.  Notation of
 * mm_meter; ONE = 2^16; C = ceiling_q28; W = window (frames); C_t = C - 8286 (8286 >
 * 16571 / 2, the largest sum of |taps| of a phase: requantising a scaled signal moves a
 * sample by at most 1/2, hence |Y| by at most 8285.5).
 *   1. P[m] = max over channels and phases of |Y_c[m][p]|, TP0 = max P.  If TP0 <= C
 *      the signal is not touched (no byte is written).
 *   2. r[m] = ONE if P[m] <= C_t, else floor(C_t * 2^16 / P[m])      (in [1900, 65535])
 *   3. R[n] = min r[n .. n+11] for n in [0, frames) (the m that sample n feeds); ONE outside
 *   4. h[k] = min R[k-W .. k+W] for k in [-W, frames + W)
 *   5. g[n] = floor(sum h[n-W .. n+W] / (2W + 1))   (every window holds n: g[n] <= R[n])
 *   6. s'[c][n] = s[c][n] if g[n] == ONE, else (s[c][n] * g[n] + 2^15) >> 16 (arithmetic)
 *   7. TP1 = true peak of s'.  If TP1 <= C: done.
 *   8. Else every sample once more by g_t = floor(C_t * 2^16 / TP1), same rounding:
 *      |Y''| <= g_t * TP1 / 2^16 + 8285.5 <= C_t + 8285.5 < C.
 * Channels are linked: one gain per frame. */
typedef struct mm_ceiling {
    int64_t frames;          /* 0: this track had no ceiling (mm_last_ceilings)     */
    int32_t channels;
    int32_t window;          /* W                                                   */
    int32_t ceiling_q28;     /* C                                                   */
    int32_t tp_in_q28;       /* TP0: linked true peak of the input                  */
    int32_t tp_limited_q28;  /* TP1: after the limiter (== TP0 when not touched)    */
    int32_t tp_out_q28;      /* of the delivered samples; <= C whenever TP0 > C     */
    int32_t min_gain_q16;    /* min g (ONE when not touched)                        */
    int32_t trim_q16;        /* g_t, ONE when no trim was needed                    */
    int64_t limited_frames;  /* frames with g < ONE                                 */
} mm_ceiling;

/* Delivery to an R 128 loudness target under the true-peak ceiling (no reference counterpart):
 * the static gain that makes the DELIVERED signal read the target on a BS.1770-4 meter with
 * the ceiling held, found by re-measuring after every limiter pass.
 * Notation: s[c][n] the source on the int16 grid (1 or 2 channels, N frames, rate R); T the
 * target in LUFS, carried as centi-LU level_clu = round(100 T) (0: off); C, W the ceiling and
 * window of mm_ceiling (C = 0: no ceiling); ONE = 2^16; I(x) = mm_r128.integrated of x with
 * the caller's K-weighting sections; gain(x, g)[n] = clip(((int64)x[n] * g + 2^15) >> 16,
 * -32768, 32767) (arithmetic shift; `clipped` counts the samples the clip moved);
 * ceil(x, C, W) = mm_ceiling as it stands; q(G) = clamp(floor(G * 2^16 + 0.5), 2^8, 2^21).
 * Constants: MM_LEVEL_PASSES = 5, TOL = 0.05 LU, SMIN = 0.25.
 *   1. I_src = I(s).  Not finite (fewer than 4 hops, or silence): the result is ceil(s, C, W),
 *      or s itself when C = 0; status UNMEASURABLE, passes = 0.
 *   2. g_0 = q(10^((T - I_src) / 20)).
 *   3. Pass k forms y_k from the SOURCE, never from y_(k-1): rounding does not accumulate.
 *      C = 0:  g_peak = min(floor(32767 * 2^16 / max|s|), 2^21); g_k > g_peak: g_k = g_peak and
 *              the pass is capped.  y_k = gain(s, g_k): nothing can clip.
 *      C != 0, g_k <= ONE:  y_k = ceil(gain(s, g_k), C, W).
 *      C != 0, g_k > ONE (the limiter runs BEFORE the boost, so that the boost cannot clip
 *              first):  g_cap = ((C - 8286) * 2^16) >> 24; g_k > g_cap: g_k = g_cap and the pass
 *              is capped.  C' = floor((C - 8286) * 2^16 / g_k) (>= 2^24: a legal ceiling).
 *              y_k = ceil(gain(ceil(s, C', W), g_k), C, W).  Since |Y(gain(u, g))| <= g |Y(u)| /
 *              2^16 + 8285.5 < C, the last ceil is normally a meter pass that writes nothing:
 *              it is there so that the guarantee is mm_ceiling's own even if a sample clipped.
 *   4. I_k = I(y_k), d_k = 20 log10(g_k / 2^16).  y_k is delivered at the first of these that
 *      holds, in this order: |T - I_k| <= TOL: REACHED; the pass was capped: CAPPED; k >= 1,
 *      d_k != d_(k-1) and the measured slope m = (I_k - I_(k-1)) / (d_k - d_(k-1)) < SMIN:
 *      SATURATED (the limiter eats the gain: pushing on only squashes the signal);
 *      k = MM_LEVEL_PASSES - 1: PASSES_SPENT.
 *   5. Otherwise g_(k+1) = q((g_k / 2^16) * 10^((T - I_k) / (20 slope))), slope = min(m, 1)
 *      when m is defined (a secant step), 1 on pass 0.
 * Channels are linked: one gain for all of them. */
#define MM_LEVEL_PASSES 5
#define MM_LEVEL_OFF 0
#define MM_LEVEL_REACHED 1
#define MM_LEVEL_CAPPED 2
#define MM_LEVEL_SATURATED 3
#define MM_LEVEL_PASSES_SPENT 4
#define MM_LEVEL_UNMEASURABLE 5
typedef struct mm_level {
    int64_t frames;          /* 0: this track had no loudness target (mm_last_levels) */
    int32_t channels;
    int32_t rate;
    int32_t target_clu;      /* level_clu                                            */
    int32_t ceiling_q28;     /* C (0: none)                                          */
    int32_t window;          /* W                                                    */
    int32_t status;          /* MM_LEVEL_*                                           */
    int32_t passes;          /* passes run; the last one is delivered                */
    int32_t gain_q16;        /* g of the delivered pass (ONE if none)                */
    int32_t pass_gain_q16[MM_LEVEL_PASSES]; /* g_k, after any cap                    */
    int32_t min_gain_q16;    /* of the delivered pass's limiting ceil call: the one at C',
                                else the one at C (ONE: none, or nothing limited)     */
    double source_lufs;      /* I_src                                                */
    double pass_lufs[MM_LEVEL_PASSES]; /* I_k (NaN: pass not run)                    */
    double loudness;         /* I of the delivered signal; NaN if unmeasurable       */
    int64_t clipped;         /* samples the delivered pass's gain clipped            */
    int64_t limited_frames;  /* of the same ceil call as min_gain_q16                */
} mm_level;

/* The sample-rate converter (no reference counterpart), all integers.  With g =
 * gcd(rate_in, rate_out): L = rate_out / g, M = rate_in / g.  taps is the caller's table
 * c[L][K] (design.resample_taps: a Kaiser-windowed sinc of 64 zero crossings a side, every
 * phase with DC gain exactly 2^22).  For input s (int16, 0 outside [0, N)) the output has
 * frames_out = ceil(N * L / M) frames; frame n of a channel is
 *   q = n * M (int64), b = q / L, p = q % L
 *   acc = sum_{k<K} c[p][k] * s[b + K/2 - k]
 *   y = (acc + 2^21) >> 22 (arithmetic), delivered clipped to [-32768, 32767].
 * Output frame 0 lies at input time 0: no latency, no tail.  Channels are independent.
 * A table is refused (MM_ERR_ARG) unless K is even and 2 <= K <= 1024, 1 <= L, M <= 640,
 * gcd(L, M) = 1, L != M, rate_in * L == rate_out * M and every row has sum |c| < 2^24.
 * Then |acc| < 2^39: the sum is exact in int64 and in f64 FMAs in any order. */
typedef struct mm_resampler {
    int32_t rate_in, rate_out;
    int32_t L, M, K;
    int32_t _pad;
    const int32_t *taps;     /* host [L][K]                                          */
    uint64_t taps_key;       /* content key of taps (nonzero; the context keeps its
                                device copy while the key and L, M, K stay the same).
                                0: no key, checked and uploaded on every call          */
} mm_resampler;

typedef struct mm_resample {
    int64_t frames_in;
    int64_t frames_out;
    int32_t channels;
    int32_t rate_in, rate_out;
    int32_t L, M, K;
    int64_t clipped[2];      /* y outside the int16 range                            */
    int32_t peak[2];         /* max |delivered sample|, 0..32768                     */
} mm_resample;

/* The linear-phase FIR (no reference counterpart), all integers: the stage a reference match
 * applies its curve with (design.match_taps).  taps is the caller's table c[K], int32
 * multiples of 2^-22, K odd, H = (K - 1) / 2, symmetric: c[k] == c[K-1-k].  For input s
 * (int16, 0 outside [0, N)) the output has N frames; frame n of a channel is
 *   acc = sum_{k<K} c[k] * s[n + H - k]
 *   y = (acc + 2^21) >> 22 (arithmetic), delivered clipped to [-32768, 32767].
 * Frame n stays at frame n: no latency, no tail.  Channels are independent.
 * A table is refused (MM_ERR_ARG) unless K is odd and 3 <= K <= 8191, the taps are symmetric
 * and sum |c| < 2^24.  Then |acc| < 2^39: the sum is exact in int64 and in f64 FMAs in any
 * order, with the pairs of equal taps folded or not. */
typedef struct mm_fir {
    int32_t rate;            /* of the signal: carried into mm_fir_result, nothing else    */
    int32_t K;
    const int32_t *taps;     /* host [K]                                             */
    uint64_t taps_key;       /* content key of taps (nonzero; the context keeps its
                                device copy while the key and K stay the same).
                                0: no key, checked and uploaded on every call          */
} mm_fir;

typedef struct mm_fir_result {
    int64_t frames;
    int32_t channels;
    int32_t rate;
    int32_t K;
    int32_t _pad;
    int64_t clipped[2];        /* y outside the int16 range                          */
    int32_t peak[2];           /* max |delivered sample|, 0..32768                   */
    int32_t peak_unclipped[2]; /* max |y| before the clip (below 2^17)               */
} mm_fir_result;

/* The EBU R 128 report of a delivered signal (no reference counterpart): what an ITU-R
 * BS.1770-4 meter reads.  mm_meter.loudness is the reference's own measure (pyloudnorm on
 * the channel mean through float32 write-backs), which the chain normalises to; here every
 * channel is K-weighted and the channel energies are summed, so a centred (L = R) stereo
 * signal reads 10 log10 2 = 3.01 LU higher than there.
 * Signal s[c][n] on the int16 grid, x = s / 32768 in f64 (MM_OUT_F32 carries the same PCM
 * / 32768), R = rate, N = frames, 1 or 2 channels, each of channel weight 1.
 *   1. y_c = K-weighting of x_c in f64: the caller's two DF2T sections sos[2][5]
 *      (design.kweight_sections(R), the chain's design) in scipy.signal.lfilter's
 *      operation order from a zero state, nothing rounded to float32.
 *   2. Hops: B[i] = floor(i * R / 10) (int64), H = floor(10 * N / R) complete hops,
 *      e[i] = sum_c sum_{n in [B[i], B[i+1])} y_c[n]^2 for i < H; frames from B[H] on
 *      belong to no hop.
 *   3. A window of w hops at hop j (j + w <= H): z_w[j] = (e[j] + ... + e[j+w-1]) /
 *      (B[j+w] - B[j]), level l_w[j] = -0.691 + 10 log10 z_w[j].  Momentary: w = 4 (400 ms),
 *      short-term: w = 30 (3 s).
 *   4. momentary_max = max l_4, short_term_max = max l_30.
 *   5. Integrated loudness: J_a = {j : l_4[j] > -70}; relative_gate = -0.691 + 10 log10(
 *      mean_{J_a} z_4) - 10; J_g = {j in J_a : l_4[j] > relative_gate}; integrated =
 *      -0.691 + 10 log10(mean_{J_g} z_4).
 *   6. Loudness range (EBU Tech 3342): S_a = {j : l_30[j] > -70}; G_s = -0.691 + 10 log10(
 *      mean_{S_a} z_30) - 20; k[0..n) = {l_30[j] : j in S_a, l_30[j] > G_s} ascending;
 *      lra_low = k[((n-1) * 10 + 50) / 100], lra_high = k[((n-1) * 95 + 50) / 100] (integer
 *      division), lra = lra_high - lra_low, lra_blocks = n.
 *   7. H < 4: every figure is NaN.  H < 30: short_term_max, lra, lra_low, lra_high are NaN.
 *      J_a empty (silence): integrated = -inf, relative_gate NaN.  No gated short-term
 *      level: lra = 0, lra_blocks = 0, lra_low and lra_high NaN.
 * Sums run in index order; both gates are strict. */
typedef struct mm_r128 {
    int64_t frames;
    int32_t channels;
    int32_t rate;
    int64_t hops;              /* H                                                    */
    int64_t momentary_blocks;  /* windows of 4 hops: max(H - 3, 0)                     */
    int64_t short_term_blocks; /* windows of 30 hops: max(H - 29, 0)                   */
    int64_t lra_blocks;        /* n of step 6                                          */
    double integrated;         /* LUFS                                                 */
    double relative_gate;      /* LUFS, step 5                                         */
    double momentary_max;      /* LUFS                                                 */
    double short_term_max;     /* LUFS                                                 */
    double lra;                /* LU                                                   */
    double lra_low, lra_high;  /* LUFS: the 10th and 95th percentile levels of step 6  */
} mm_r128;

/* The delivery QC report of a delivered signal (no reference counterpart): what an ingest
 * check asks beyond loudness and true peak, as exact integer statements about the int16 grid.
 * Signal s[c][n] on the int16 grid (MM_OUT_F32 carries the same PCM / 32768 and is converted
 * back on load, as in the meter), CH = 1 or 2 channels, N frames with 0 <= N < 2^31, rate R.
 * Parameters: silence_lsb q in 0..32767, min_run r in 1..65535.
 *   1. Totals (int64, exact: sq <= 2^61): sum[c] = sum s, sq[c] = sum s^2, cross = sum s0 * s1
 *      (0 for mono); smin[c], smax[c] (0 when N == 0); or_bits[c] = OR of (uint16) s over n.
 *   2. Silence.  Frame n is silent when |s[c][n]| <= q for every channel.  lead_silence = the
 *      index of the first non-silent frame (N if none); trail_silence = N - 1 - the last
 *      non-silent index (N if none); silent_frames = their count; silence_longest /
 *      silence_longest_at = length and start of the longest maximal run of silent frames
 *      anywhere, the first among equals (no silent frame: 0, -1).  A dropout is such a run with
 *      at > 0 and at + len < N.
 *   3. Clip runs, per channel.  rail = +1 if s == 32767, -1 if s <= -32767, else 0.  A run is a
 *      maximal stretch of consecutive frames of equal non-zero rail.  clip_samples[c] = frames
 *      with rail != 0 (== mm_meter.clipped[c]); clip_runs[c] = runs of length >= r;
 *      clip_longest[c] / clip_longest_at[c] = the longest run and its start (the first of
 *      equals; none: 0, -1).
 *   4. Hops, as mm_r128's: B[i] = floor(i * R / 10), H = floor(10 * N / R) complete hops; per
 *      hop i < H three int64: a[i] = sum s0^2, b[i] = sum s1^2, x[i] = sum s0 * s1 over
 *      [B[i], B[i+1]) (mono: b = x = 0).  Frames from B[H] on belong to no hop.
 *   5. Correlation over time (stereo only), in 400 ms windows: a window is 4 hops at j with
 *      j + 4 <= H; A, Bw, X are its sums of a, b, x and n_w = B[j+4] - B[j].  It is gated in
 *      when A + Bw >= 2048 * n_w (mean square at least 32^2 a channel, about -60 dBFS: an
 *      integer comparison).  rho[j] = 0 if A == 0 or Bw == 0, else (double)X / sqrt((double)A *
 *      (double)Bw), every operation one correctly rounded IEEE operation.  corr_windows = the
 *      gated windows; corr_negative = those with X < 0 (exact); corr_min = the smallest rho of
 *      a gated window (NaN if none); corr_min_hop = the smallest j attaining it (-1 if none).
 *      Mono: 0, 0, NaN, -1.
 * Everything else a caller reads (DC offset, overall correlation, mono fold-down level, bit use,
 * dual mono, seconds, the dropout) derives from these integers (engine.qc_dict).  No verdicts:
 * thresholds are the caller's. */
typedef struct mm_qc {
    int64_t frames;
    int32_t channels;
    int32_t rate;
    int64_t hops;                /* H                                                    */
    int32_t silence_lsb;         /* q                                                    */
    int32_t min_run;             /* r                                                    */
    int64_t sum[2], sq[2], cross;
    int32_t smin[2], smax[2];
    uint32_t or_bits[2];
    int64_t lead_silence, trail_silence, silent_frames;
    int64_t silence_longest, silence_longest_at;
    int64_t clip_samples[2], clip_runs[2], clip_longest[2], clip_longest_at[2];
    int64_t corr_windows, corr_negative, corr_min_hop;
    double corr_min;
} mm_qc;

/* The spectrum report of a delivered signal (no reference counterpart): what it looks like over
 * frequency.  Welch's long-term average spectrum of each channel and the real part of their
 * cross-spectrum, and from those the 1/3-octave bands with a phase correlation a band.
 * Signal x[c][n] = the int16 grid / 32768 (MM_OUT_F32 carries it as it is and is converted back
 * on load, as in mm_qc), 1 or 2 channels, `frames` frames with 0 <= frames < 2^31, rate >= 2000.
 *   1. Frames.  Length N = 8192 at every rate, hop H = 4096, the periodic Hann window w[n] =
 *      0.5 - 0.5 cos(2 pi n / N).  Frame j covers [j H, j H + N); F = 0 if frames < N, else
 *      (frames - N) / H + 1.  A tail that fills no frame is dropped, as the R 128 gating blocks
 *      drop theirs.  F == 0 is "unmeasurable": n_frames = 0 and every bin, band and total is NaN.
 *   2. Bins, k = 0 .. N/2, with X_c,j[k] = sum_n w[n] x_c[j H + n] e^(-2 pi i k n / N):
 *        S_L[k] = (1/F) sum_j |X_L,j[k]|^2,  S_R[k] likewise,
 *        C[k]   = (1/F) sum_j Re(X_L,j[k] conj X_R,j[k]).
 *      The bin table is [N/2 + 1][3] double = {S_L, S_R, C}; mono has S_L and zeros beside it.
 *   3. Bands (mm_spectrum_bands, mm_spectrum_from_bins).  1/3-octave bands with base-10 centres
 *      f_m = 1000 * 10^(m / 10) and edges f_m * 10^(-1/20), f_m * 10^(+1/20), from the 20 Hz band
 *      (m = -17) to the last band whose lower edge is below rate / 2; that band ends at rate / 2.
 *      Bin k is the rectangle [(k - 1/2) rate / N, (k + 1/2) rate / N) clipped to [0, rate / 2]
 *      and enters a band with the fraction `frac` of that width that lies inside the band: the
 *      bands partition the power between their outer edges, no band is empty, and no rule asks
 *      where a bin's centre falls.  With the bin weight c_k = 1 for k = 0 and N/2 and 2 otherwise,
 *      a band's row is {ms_L, ms_R, ms_C, bins_in_band}: the mean squares sum frac c_k S[k] /
 *      (N * 3N/8) of S_L, S_R and C (3N/8 = sum w^2: a full-scale sine gives 1/2), and
 *      bins_in_band = sum frac c_k / 2, the fractions with the half-width bins 0 and N/2 counting
 *      as the halves they are, which is the band's width * N / rate: the 20 Hz band at 192 kHz
 *      rests on a fifth of a bin.
 *   4. total_ms[c] = sum_k c_k S_c[k] / (N * 3N/8), the mean square of the windowed frames.
 * Levels in dB, the correlation C_b / sqrt(L_b R_b) of a band, mid and side, the roll-off and the
 * occupied bandwidth derive from these numbers (engine.spectrum_dict).  Figures, not verdicts.
 * The FFT is float arithmetic: unlike the integer reports the restatements (numpy in the tests,
 * mm_spectrum_host in double, the kernels in single with double accumulators) agree to a
 * tolerance, not bit for bit; the GPU path is bit-identical to itself, a batch to single calls
 * and a master call's report to mm_spectrum_pcm on what that call delivered. */
typedef struct mm_spectrum {
    int64_t frames;
    int32_t channels;
    int32_t rate;
    int32_t n_fft;               /* N = 8192                                             */
    int32_t hop;                 /* H = 4096                                             */
    int64_t n_frames;            /* F                                                    */
    int32_t n_bands;             /* rows of the band table at this rate                  */
    int32_t _pad;
    double total_ms[2];          /* step 4 (mono: total_ms[1] = 0; F == 0: NaN)          */
} mm_spectrum;
#define MM_SPECTRUM_MAX_BANDS 80 /* bands at any int32 rate (38 at 192 kHz, 31 at 44.1 kHz) */

/* Bits of mm_job.meter_on and mm_delivery.meter_on: which reports of the delivered output
 * the master call makes (0 and 1 mean what they meant before the second bit). */
#define MM_REPORT_METER 1 /* mm_meter (mm_last_meters)                                  */
#define MM_REPORT_R128 2  /* mm_r128 (mm_last_r128), from the kweight.sos and the rate of
                             the job (a delivery: of its `loud` job, which must be set)  */
#define MM_REPORT_QC 4    /* mm_qc (mm_last_qc) with silence_lsb 1 and min_run 3, at the rate
                             of the job (a delivery: of its `loud` job, which must be set) */
#define MM_REPORT_SPECTRUM 8 /* mm_spectrum and its bin table (mm_last_spectrum,
                             mm_last_spectrum_bins), at the rate of the job (a delivery: of
                             its `loud` job, which must be set)                          */

/* What mm_job cannot carry for a delivery (mm_deliver*): the converter to another rate and,
 * acting on the delivered signal, the loudness target, the ceiling and the report. */
typedef struct mm_delivery {
    const mm_resampler *rs;  /* NULL: deliver at the job's own rate (the chain writes the
                                caller's output itself; mm_last_resample: MM_ERR_STATE)  */
    int32_t ceiling_q28;     /* 0 = off; else as mm_job.ceiling_q28                  */
    int32_t window;          /* the ceiling's look-ahead at rate_out (frames)        */
    int32_t meter_on;        /* MM_REPORT_METER: meter the delivered output (mm_last_meters);
                                MM_REPORT_R128: its R 128 report (mm_last_r128);
                                MM_REPORT_QC: its QC report (mm_last_qc), at loud's rate;
                                MM_REPORT_SPECTRUM: its spectrum report (mm_last_spectrum), at
                                loud's rate */
    int32_t level_clu;       /* the former pad: 0 = off (nothing new is queued); else the
                                loudness target in centi-LU, -4000 .. -500 (design.level_clu):
                                the delivered signal is levelled to it under the ceiling
                                (mm_level, mm_last_levels), which replaces the plain ceiling
                                call; needs `loud` for its kweight.sos and rate, as
                                MM_REPORT_R128 does                                      */
    const struct mm_job *loud; /* a job carrying the loudness geometry of the OUTPUT
                                (frames_proc = frames_out, channels, rate = rate_out,
                                kweight with tpb 256, blocks, segments), as for
                                mm_meter_device; NULL: peaks only.  The R 128 report
                                reads its kweight.sos and rate alone                 */
} mm_delivery;

/* Geometry of the compressor's envelope solve for a job (mm_solve_geometry: the
   planning arithmetic stage C runs on, computed on the host without a GPU). */
typedef struct mm_solve_geom {
    int32_t tps;             /* tiles per super-tile (a walker's unit)          */
    int32_t tile_rows;       /* M-plane rows per tile: T rounded up to whole walk
                                load blocks (extra rows hold M = 0)            */
    int32_t rows;            /* rows per column: tps * tile_rows + prefetch pad  */
    int32_t walk_block;      /* rows per walk load block (tile_rows is a multiple)  */
    int64_t cols_per_chunk;  /* super-tile columns per chunk (whole blocks of 64) */
    int64_t chunks;
    int64_t chunk_plane_bytes; /* one chunk's part of one band's M plane: walked
                                through 32-bit buffer offsets, < 2^31           */
    int64_t plane_bytes;     /* the three bands' M planes of the whole track     */
    int32_t col_block;       /* columns per comp_rms workgroup / pass-0 wave (64) (ABI 4) */
    int32_t rms_group_tiles; /* tiles per comp_rms workgroup: tps * col_block (ABI 4) */
} mm_solve_geom;

/* ---- context ------------------------------------------------------------ */
int mm_create(int device, mm_ctx **ctx);
int mm_destroy(mm_ctx *ctx);
const char *mm_last_error(mm_ctx *ctx);
int mm_sync(mm_ctx *ctx);
/* ABI version: 2 = mm_band.lut_key and mm_result.comp_jumped (round 3),
   mm_solve_geometry (round 4); 3 = mm_solve_geom.walk_block, the device loudness
   path in composable steps with a world check and the applied gain returned,
   device-pointer collectives (round 5); 4 = mm_job.sat_table / sat_key,
   mm_op_saturation_table, mm_np_sum_f32, mm_check_compressor_math,
   mm_solve_geom.col_block / rms_group_tiles (round 6); 5 = mm_job.meter_on, mm_meter and
   the metering entry points (mm_meter_device, mm_meter_pcm, mm_last_meters,
   mm_op_true_peak, mm_true_peak_host, mm_meter_span); also under 5, in the place of
   mm_job's trailing pad (a caller that zeroed it gets what it got): mm_job.ceiling_q28,
   mm_ceiling and the ceiling entry points (mm_ceiling_device, mm_ceiling_pcm,
   mm_ceiling_host, mm_last_ceilings, mm_ceiling_span, mm_ceiling_max_window); and, as new values
   of existing fields (no struct changed): mm_job.in_kind MM_IN_I24 / MM_IN_I32, mm_wav_info
   bits 24 / 32 with format 1, and the decode entry points (mm_pcm_decode_device,
   mm_op_pcm_decode, mm_pcm_decode_host, mm_pcm_decode_span); and, as new structs and entry
   points only (mm_job is unchanged): mm_resampler, mm_resample, mm_delivery, the converter
   (mm_resample_device, mm_resample_pcm, mm_resample_host, mm_resample_frames,
   mm_resample_span, mm_last_resample) and the delivery path (mm_deliver_device, mm_deliver,
   mm_deliver_wav); and, again as new structs and entry points only and a new value of an
   existing field (bit 1 of mm_job.meter_on and mm_delivery.meter_on): mm_r128 and the R 128
   report (mm_r128_from_hops, mm_r128_host, mm_r128_device, mm_r128_pcm, mm_op_r128_hops,
   mm_r128_span, mm_last_r128); and, as a new struct and entry points and in the place of
   mm_delivery's pad (a caller that zeroed it gets what it got): mm_delivery.level_clu, a
   delivery without a converter (rs == NULL), mm_level and the level entry points
   (mm_level_device, mm_level_pcm, mm_level_host, mm_op_level_gain, mm_last_levels,
   mm_level_span); and, as entry points only (no struct added or changed), the album
   (mm_r128_album_from_hops, mm_album_level_host, mm_album_r128_device, mm_album_r128_pcm,
   mm_op_r128_album_hops, mm_album_level_device, mm_album_level_pcm, mm_last_album); and, again
   as entry points only, the batch (mm_batch_ceiling_device, mm_batch_ceiling_pcm,
   mm_batch_level_device, mm_batch_level_pcm) and its converter (mm_batch_resample_device,
   mm_batch_resample_pcm); and, as a new struct and entry points and a new value of an
   existing field (bit 2 of mm_job.meter_on and mm_delivery.meter_on): mm_qc and the QC report
   (mm_qc_from_hops, mm_qc_host, mm_qc_device, mm_qc_pcm, mm_batch_qc_device, mm_batch_qc_pcm,
   mm_qc_span, mm_last_qc); and, in the same way (bit 3 of the two meter_on fields): mm_spectrum
   and the spectrum report (mm_spectrum_bands, mm_spectrum_from_bins, mm_spectrum_host,
   mm_spectrum_device, mm_spectrum_pcm, mm_batch_spectrum_device, mm_batch_spectrum_pcm,
   mm_last_spectrum, mm_last_spectrum_bins); and, as new structs and entry points only: mm_fir,
   mm_fir_result and the linear-phase FIR (mm_fir_device, mm_fir_pcm, mm_fir_host, mm_fir_span,
   mm_last_fir).  A caller
   built against an older header must
   refuse a library whose version differs from its own MM_ABI_VERSION. */
#define MM_ABI_VERSION 5
int mm_version(void);
/* The envelope-solve geometry of a job (no context, no GPU).  MM_ERR_ARG if a
   chunk's plane would not fit 32-bit offsets (no track length below 2^31 frames
   at rates up to 192 kHz does) or if comp_super is not 4 tiles (the rms kernel's
   workgroup shape). */
int mm_solve_geometry(const mm_job *job, mm_solve_geom *out);
/* Verification only (tests/test_gpu_record_base.py; an entry point added under ABI 5):
   after a chain with the multiband compressor on this context, the release-jump
   records of one band's active tiles, in compact order (chunk by chunk): tiles[i] =
   the tile's index on the track, mmax[i] = its largest M, records[16 i .. 16 i + 15]
   = its record (8 binades x 2 mantissa parities from the record's base; NaN where the
   reference walk left its binade).  Fills at most `cap` tiles and returns the number
   of active tiles in *count (a larger count than cap: nothing past cap was written).
   Read-only; MM_ERR_STATE without such a chain. */
int mm_solve_records(mm_ctx *ctx, int band, int64_t cap, int32_t *tiles, double *mmax, double *records,
                     int64_t *count);
/* sha256 prefix (16 hex digits) of the sources this library was built from
   (mastering_amd/srcsha.py: the csrc sources and this header) */
const char *mm_source_sha(void);

/* ---- whole chain -------------------------------------------------------- */
/* Host buffers: in = interleaved [frames_in*channels] of job->in_kind (f32 =
 * PCM16/32768, int16 PCM, packed 24-bit or int32 PCM), out = [frames_proc*channels] of out_kind.
 * Replaces AME:43-98 minus file/GCS IO. */
int mm_master(mm_ctx *ctx, const mm_job *job, const void *in, void *out, mm_result *res);
/* Same, with device-resident input/output (zero-copy; e.g. torch tensors). */
int mm_master_device(mm_ctx *ctx, const mm_job *job, const void *d_in, void *d_out, mm_result *res);

/* A batch of independent tracks (file sharding, BASELINE C3/C5): jobs[i] with
 * device input d_in[i] and output d_out[i]; up to MM_BATCH_STREAMS tracks run at
 * once on streams of their own (child contexts), res[i] (optional) as above. */
#define MM_BATCH_STREAMS 8
int mm_master_batch(mm_ctx *ctx, int n, const mm_job *jobs, const void *const *d_in, void *const *d_out,
                    mm_result *res);

/* ---- mastering report ----------------------------------------------------- */
/* Meter a device-resident signal, interleaved [frames][channels] of `kind`
 * (MM_OUT_I16, or MM_OUT_F32 = the same PCM / 32768: both give the same mm_meter).
 * loud: a job carrying the loudness geometry of this signal (frames_proc, channels,
 * rate, kweight with tpb 256, blocks, segments), or NULL for peaks only; a signal
 * shorter than one 0.4 s block gets loudness NaN, not an error.  The audio is never
 * altered.  Synchronous on return. */
int mm_meter_device(mm_ctx *ctx, const void *d_pcm, int kind, int64_t frames, int channels, const mm_job *loud,
                    mm_meter *out);
/* The same on a host buffer. */
int mm_meter_pcm(mm_ctx *ctx, const void *pcm, int kind, int64_t frames, int channels, const mm_job *loud,
                 mm_meter *out);
/* The meters of the last mm_master / mm_master_device / mm_master_wav (1) or
 * mm_master_batch (n, in job order; tracks whose job had meter_on == 0 report
 * frames 0) call on this context: copies min(cap, n) of them and returns n.
 * MM_ERR_STATE if that call did not meter. */
int mm_last_meters(mm_ctx *ctx, int cap, mm_meter *out);
/* The integer definition of mm_meter restated in plain C on the host (no context,
 * no GPU; loudness stays NaN): a CPU check of what the meter kernel computes. */
int mm_true_peak_host(const int16_t *pcm, int64_t frames, int channels, mm_meter *out);
/* Frames of m per workgroup of the meter kernel (where its seams lie). */
int mm_meter_span(void);

/* ---- EBU R 128 report ------------------------------------------------------- */
/* Steps 3-7 of mm_r128 on the hop energies e[0, hops) in plain C++ (no context, no GPU):
 * the one tail every path below ends in.  Fills every field but frames and channels (the
 * hop energies carry neither: 0).  MM_ERR_ARG for a null pointer or rate < 2000. */
int mm_r128_from_hops(const double *e, int64_t hops, int32_t rate, mm_r128 *out);
/* The definition restated sequentially on the host (no context, no GPU), interleaved
 * int16: its filter outputs are scipy.signal.lfilter's bit for bit.  hops_out (may be
 * NULL) receives the first min(H, hops_cap) hop energies.  MM_ERR_ARG as below. */
int mm_r128_host(const int16_t *pcm, int64_t frames, int channels, int32_t rate, const double sos[2][5],
                 double *hops_out, int64_t hops_cap, mm_r128 *out);
/* The report of a device-resident signal, interleaved [frames][channels] of `kind`
 * (MM_OUT_I16, or MM_OUT_F32 = the same PCM / 32768: both give the same mm_r128), with the
 * K-weighting sections sos of its rate.  MM_ERR_ARG, with words in mm_last_error, for
 * channels other than 1 or 2, a bad kind, rate < 2000 (the library's floor: a hop then has
 * at least 200 frames), frames >= 2^31 or a null pointer; frames == 0 gives a cleared
 * struct with NaN figures.  The audio is never altered.  Synchronous on return.  The sections
 * are not checked: design.kweight_sections(R) is a K-weighting only for R above ~3.1 kHz
 * (its shelf lies at 1500 Hz; at or below 3 kHz its poles leave the unit circle). */
int mm_r128_device(mm_ctx *ctx, const void *d_pcm, int kind, int64_t frames, int channels, int32_t rate,
                   const double sos[2][5], mm_r128 *out);
/* The same on a host buffer. */
int mm_r128_pcm(mm_ctx *ctx, const void *pcm, int kind, int64_t frames, int channels, int32_t rate,
                const double sos[2][5], mm_r128 *out);
/* The GPU pass's hop energies themselves for a host buffer (a per-stage operator, for
 * parity checks): copies the first min(H, cap) to hops_host and returns H. */
int mm_op_r128_hops(mm_ctx *ctx, const void *pcm, int kind, int64_t frames, int channels, int32_t rate,
                    const double sos[2][5], double *hops_host, int64_t cap);
/* Frames one workgroup of the K-weighting pass covers (256 lanes of one tile each). */
int mm_r128_span(void);
/* The R 128 reports of the last master call on this context, as mm_last_meters: 1, or n
 * for a batch in job order (frames 0 and NaN figures for a job without MM_REPORT_R128);
 * copies min(cap, n) and returns n.  MM_ERR_STATE if no job of that call asked for one. */
int mm_last_r128(mm_ctx *ctx, int cap, mm_r128 *out);

/* ---- delivery QC report ------------------------------------------------------ */
/* Step 5 of mm_qc on a stereo signal's hop table hops[H][3] = {a, b, x} in plain C++ (no
 * context, no GPU): the one tail the host restatement and the GPU path end in.  Sets hops,
 * rate, corr_windows, corr_negative, corr_min and corr_min_hop of *out and touches no other
 * field (the table carries no channel count: a mono caller keeps 0, 0, NaN, -1 without
 * calling).  MM_ERR_ARG for a null pointer, H < 0 or rate < 2000. */
int mm_qc_from_hops(const int64_t *hops, int64_t H, int32_t rate, mm_qc *out);
/* The definition restated sequentially on the host (no context, no GPU), interleaved int16.
 * hops_out (may be NULL) receives the whole table [H][3], H = floor(10 * frames / rate).
 * MM_ERR_ARG for channels other than 1 or 2, frames outside [0, 2^31), rate < 2000,
 * silence_lsb outside [0, 32767], min_run outside [1, 65535] or a null pointer. */
int mm_qc_host(const int16_t *pcm, int64_t frames, int channels, int32_t rate, int32_t silence_lsb, int32_t min_run,
               mm_qc *out, int64_t *hops_out);
/* The report of a device-resident signal, interleaved [frames][channels] of `kind` (MM_OUT_I16,
 * or MM_OUT_F32 = the same PCM / 32768: both give the same mm_qc): one memset, the span launch,
 * the fold launch and one read-back, then mm_qc_from_hops.  hops_out (may be NULL) as above.
 * MM_ERR_ARG as mm_qc_host, with words in mm_last_error, and for a bad kind.  The audio is
 * never altered.  Synchronous on return. */
int mm_qc_device(mm_ctx *ctx, const void *d_pcm, int kind, int64_t frames, int channels, int32_t rate,
                 int32_t silence_lsb, int32_t min_run, mm_qc *out, int64_t *hops_out);
/* The same on a host buffer. */
int mm_qc_pcm(mm_ctx *ctx, const void *pcm, int kind, int64_t frames, int channels, int32_t rate, int32_t silence_lsb,
              int32_t min_run, mm_qc *out, int64_t *hops_out);
/* The reports of n device-resident tracks of one kind, channel count and rate, 1 <= n <=
 * MM_ALBUM_TRACKS: out[t] is mm_qc_device's of track t alone (a run never joins across two
 * tracks and no frame of a neighbour is read), with one memset, two launches and one read-back
 * whatever n.  The results are also left behind mm_last_qc; the levels, ceilings and R 128
 * reports of the context's last call stay as they are.  MM_ERR_ARG, with words that name the
 * track and before anything is queued, for a track mm_qc_device refuses or a total of 2^31
 * frames or more.  Synchronous on return. */
int mm_batch_qc_device(mm_ctx *ctx, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                       int32_t rate, int32_t silence_lsb, int32_t min_run, mm_qc *out);
/* The same on host buffers. */
int mm_batch_qc_pcm(mm_ctx *ctx, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                    int32_t rate, int32_t silence_lsb, int32_t min_run, mm_qc *out);
/* Frames one workgroup of the span kernel covers (where its seams lie). */
int mm_qc_span(void);
/* The QC reports of the last master call (as mm_last_meters; frames 0: that job did not ask)
 * or mm_batch_qc_* call on this context: copies min(cap, n) and returns n.  MM_ERR_STATE if
 * that call made none. */
int mm_last_qc(mm_ctx *ctx, int cap, mm_qc *out);

/* ---- spectrum report ---------------------------------------------------------- */
/* The 1/3-octave bands at `rate` (step 3 of mm_spectrum; no context, no GPU): returns their
 * number n and writes min(cap, n) rows {lower edge, centre, upper edge} in Hz into
 * edges[cap][3].  MM_ERR_ARG for rate < 2000 or a null pointer with cap > 0. */
int mm_spectrum_bands(int32_t rate, int cap, double *edges);
/* Steps 3 and 4 on a bin table bins[N/2 + 1][3] in plain C++ in double (no context, no GPU): the
 * one tail the host restatement and the GPU path end in.  Sets every field of *out (n_frames
 * from `frames`) and, if `bands` is not NULL, writes n_bands rows {ms_L, ms_R, ms_C,
 * bins_in_band} into it (room for MM_SPECTRUM_MAX_BANDS rows always suffices).  NaN bins give
 * NaN figures.  MM_ERR_ARG as mm_spectrum_host. */
int mm_spectrum_from_bins(const double *bins, int64_t frames, int channels, int32_t rate, mm_spectrum *out, double *bands);
/* The definition restated sequentially on the host (no context, no GPU), interleaved int16,
 * with its own radix-2 FFT in double.  bands (may be NULL) as above; bins_out (may be NULL)
 * receives the bin table [N/2 + 1][3].  MM_ERR_ARG for channels other than 1 or 2, frames
 * outside [0, 2^31), rate < 2000 or a null pointer. */
int mm_spectrum_host(const int16_t *pcm, int64_t frames, int channels, int32_t rate, mm_spectrum *out, double *bands,
                     double *bins_out);
/* The report of a device-resident signal, interleaved [frames][channels] of `kind` (MM_OUT_I16,
 * or MM_OUT_F32 = the same PCM / 32768: both give the same bits): the frames launch, the fold
 * launch and one read-back, then mm_spectrum_from_bins.  bands and bins_out as above.
 * MM_ERR_ARG as mm_spectrum_host, with words in mm_last_error, and for a bad kind.  The audio
 * is never altered.  Synchronous on return. */
int mm_spectrum_device(mm_ctx *ctx, const void *d_pcm, int kind, int64_t frames, int channels, int32_t rate,
                       mm_spectrum *out, double *bands, double *bins_out);
/* The same on a host buffer. */
int mm_spectrum_pcm(mm_ctx *ctx, const void *pcm, int kind, int64_t frames, int channels, int32_t rate, mm_spectrum *out,
                    double *bands, double *bins_out);
/* The reports of n device-resident tracks of one kind, channel count and rate, 1 <= n <=
 * MM_ALBUM_TRACKS: out[t] and track t's bin table are mm_spectrum_device's of track t alone, bit
 * for bit (no frame of a neighbour is read; a track may begin at any frame offset of a shared
 * allocation), with two launches and one read-back whatever n.  The results are left behind
 * mm_last_spectrum and the tables behind mm_last_spectrum_bins; the other results of the
 * context's last call stay as they are.  MM_ERR_ARG, with words that name the track and before
 * anything is queued, for a track mm_spectrum_device refuses or a total of 2^31 frames or more.
 * Synchronous on return. */
int mm_batch_spectrum_device(mm_ctx *ctx, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                             int32_t rate, mm_spectrum *out);
/* The same on host buffers. */
int mm_batch_spectrum_pcm(mm_ctx *ctx, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                          int32_t rate, mm_spectrum *out);
/* The spectrum reports of the last master call (as mm_last_meters; frames 0 and NaN totals: that
 * job did not ask) or mm_batch_spectrum_* call on this context: copies min(cap, n) and returns
 * n.  MM_ERR_STATE if that call made none. */
int mm_last_spectrum(mm_ctx *ctx, int cap, mm_spectrum *out);
/* The bin table of track `track` of those reports: copies min(cap, N/2 + 1) rows of 3 doubles
 * and returns N/2 + 1 (NaN rows for a job that did not ask).  MM_ERR_STATE as mm_last_spectrum;
 * MM_ERR_ARG for a track outside them. */
int mm_last_spectrum_bins(mm_ctx *ctx, int track, int cap, double *bins);

/* ---- true-peak ceiling ----------------------------------------------------- */
/* Hold a device-resident signal, interleaved [frames][channels] of `kind` (MM_OUT_I16,
 * or MM_OUT_F32 = the same PCM / 32768), under the true-peak ceiling ceiling_q28 with a
 * look-ahead window of `window` frames (1 .. mm_ceiling_max_window()), in place, as
 * mm_ceiling defines.  MM_ERR_ARG for a ceiling or window out of range or frames beyond
 * the meter's limit.  Synchronous on return. */
int mm_ceiling_device(mm_ctx *ctx, void *d_pcm, int kind, int64_t frames, int channels, int32_t ceiling_q28,
                      int32_t window, mm_ceiling *out);
/* The same on a host buffer, in place. */
int mm_ceiling_pcm(mm_ctx *ctx, void *pcm, int kind, int64_t frames, int channels, int32_t ceiling_q28,
                   int32_t window, mm_ceiling *out);
/* The definition restated in plain C++ on the host (no context, no GPU), in place on
 * interleaved int16: a CPU check of what the ceiling kernels compute. */
int mm_ceiling_host(int16_t *pcm, int64_t frames, int channels, int32_t ceiling_q28, int32_t window,
                    mm_ceiling *out);
/* The ceilings of the last mm_master / mm_master_device / mm_master_wav (1) or
 * mm_master_batch (n, in job order; tracks whose job had ceiling_q28 == 0 report
 * frames 0) call on this context: copies min(cap, n) of them and returns n.
 * MM_ERR_STATE if that call set no ceiling. */
int mm_last_ceilings(mm_ctx *ctx, int cap, mm_ceiling *out);
/* Frames per workgroup of the kernel that applies the gains (where its seams lie). */
int mm_ceiling_span(void);
/* The largest look-ahead window, in frames (1024). */
int mm_ceiling_max_window(void);

/* ---- delivery to a loudness target -------------------------------------------- */
/* Level a device-resident signal, interleaved [frames][channels] of `kind` (MM_OUT_I16, or
 * MM_OUT_F32 = the same PCM / 32768), in place to level_clu under the ceiling ceiling_q28
 * (0: none; window as mm_ceiling_device), as mm_level defines, with the K-weighting
 * sections sos of its rate.  ceil_out (may be NULL) receives, when ceiling_q28 != 0, the
 * final mm_ceiling call at C on the delivered pass.  MM_ERR_ARG, with words in
 * mm_last_error and the context still usable, for level_clu outside [-4000, -500], a bad
 * kind, channels, ceiling or window, rate < 2000 or null sections.  Synchronous on return. */
int mm_level_device(mm_ctx *ctx, void *d_pcm, int kind, int64_t frames, int channels, int32_t rate,
                    const double sos[2][5], int32_t level_clu, int32_t ceiling_q28, int32_t window, mm_level *out,
                    mm_ceiling *ceil_out);
/* The same on a host buffer, in place. */
int mm_level_pcm(mm_ctx *ctx, void *pcm, int kind, int64_t frames, int channels, int32_t rate, const double sos[2][5],
                 int32_t level_clu, int32_t ceiling_q28, int32_t window, mm_level *out, mm_ceiling *ceil_out);
/* The definition restated in plain C++ on the host (no context, no GPU), in place on
 * interleaved int16: mm_ceiling_host, mm_r128_host and the gain under the same rule. */
int mm_level_host(int16_t *pcm, int64_t frames, int channels, int32_t rate, const double sos[2][5], int32_t level_clu,
                  int32_t ceiling_q28, int32_t window, mm_level *out, mm_ceiling *ceil_out);
/* The gain kernel alone on host buffers (a per-stage operator, for parity checks): n samples
 * of `kind` by gain_q16 in [2^8, 2^21], through device views that start src_off and dst_off
 * samples (0 .. 7) past a 16-byte boundary; dst_off < 0: in place.  *clipped and *peak are
 * the kernel's statistics (samples the clip moved; max |delivered sample|). */
int mm_op_level_gain(mm_ctx *ctx, const void *in, int kind, int64_t n, int src_off, int dst_off, int32_t gain_q16,
                     void *out_pcm, int64_t *clipped, int32_t *peak);
/* The levels of the last master call on this context, as mm_last_meters (a call without a
 * delivery, or a batch, sets none): copies min(cap, n) and returns n.  MM_ERR_STATE if that
 * call set no loudness target. */
int mm_last_levels(mm_ctx *ctx, int cap, mm_level *out);
/* Samples one workgroup of the gain kernel covers in whole 16-byte vectors (its seams lie
 * at multiples of this past the first 16-byte boundary of the destination). */
int mm_level_span(void);

/* ---- an album levelled as one programme -------------------------------------- */
/* One static gain for all tracks of an album: the album, measured as one programme, reads the
 * target, every track is held under the true-peak ceiling, and the loudness differences
 * between the tracks are kept (the album mode of ReplayGain 2.0 / EBU R 128 tools, which pool
 * the gating blocks of several programmes and never form a block across two of them).  No
 * reference counterpart.
 * The tracks are s_0 .. s_(n-1) on the int16 grid, 1 <= n <= MM_ALBUM_TRACKS, of N_t frames,
 * all of one rate, one channel count (1 or 2) and one PCM kind; mm_r128 / mm_ceiling accept
 * each of them alone, and the total frame count is below 2^31.
 *
 * Album R 128 figures (they generalise mm_r128_from_hops):
 *   - Track t has hop energies e_t[0 .. H_t) exactly as mm_r128 defines them (steps 1-2).
 *   - For w = 4 and w = 30 its windows z_(t,w)[j], l_(t,w)[j], j < H_t - w + 1, are those of
 *     step 3 on e_t alone: no window spans two tracks; a track with H_t < w contributes none.
 *   - The pool P_w is the tracks' windows back to back in track order.
 *   - momentary_max, relative_gate, integrated and momentary_blocks come from P_4 (steps 4-5);
 *     short_term_max, short_term_blocks, lra, lra_low, lra_high and lra_blocks from P_30
 *     (steps 4 and 6).  The gates and the percentile rule are mm_r128's, the sums running
 *     sequentially over the pool in pool order.
 *   - hops = sum H_t, frames = sum N_t.
 *   - P_4 empty: integrated is NaN; nothing above -70: -inf (as step 7).
 *   - With n = 1 every field equals mm_r128_from_hops' bit for bit.
 *
 * Album level: mm_level's rule with I(.) the album integrated loudness and y_k formed PER
 * TRACK from that track's kept source by the one gain g_k:
 *   - I_src not finite: UNMEASURABLE, each track then only gets its ceiling (ceil(s_t, C, W)).
 *   - C = 0: g_k is capped at g_peak = min(floor(32767 * 2^16 / max_t max|s_t|), 2^21);
 *     track t is gain(s_t, g_k).
 *   - C != 0, g_k <= ONE: track t is ceil(gain(s_t, g_k), C, W).
 *   - C != 0, g_k > ONE: track t is ceil(gain(ceil(s_t, C', W), g_k), C, W); C' and the cap on
 *     g_k are mm_level's: they do not depend on the track.
 *   - Steps 4 and 5 of mm_level decide, unchanged.
 *   - A track too short to have a window of its own still gets the gain and the ceiling.
 * In the resulting mm_level, frames, clipped and limited_frames are sums over the tracks and
 * min_gain_q16 is the minimum; the two limiter figures come from the limiting ceil call of
 * the delivered pass, as in mm_level. */
#define MM_ALBUM_TRACKS 256
/* The album R 128 figures from the tracks' hop energies back to back, e[0, sum track_hops), in
 * plain C++ (no context, no GPU): every field but frames and channels.  MM_ERR_ARG for a null
 * pointer, n outside [1, MM_ALBUM_TRACKS], a negative hop count or rate < 2000. */
int mm_r128_album_from_hops(const double *e, const int64_t *track_hops, int n, int32_t rate, mm_r128 *out);
/* The album level restated in plain C++ on the host (no context, no GPU), in place on n
 * interleaved int16 tracks: mm_ceiling_host, mm_r128_host and the gain in the one loop that
 * mm_level_host runs with n = 1.  *album and track_r128[n] (may be NULL) describe what was
 * delivered; track_ceil[n] (may be NULL) receives, when C != 0, every track's final
 * mm_ceiling call at C.  MM_ERR_ARG as mm_album_level_device. */
int mm_album_level_host(int16_t *const *pcm, const int64_t *frames, int n, int channels, int32_t rate,
                        const double sos[2][5], int32_t level_clu, int32_t ceiling_q28, int32_t window, mm_level *out,
                        mm_r128 *album, mm_r128 *track_r128, mm_ceiling *track_ceil);
/* The album R 128 report of n device-resident tracks, interleaved [frames[t]][channels] of
 * `kind`: every track is K-weighted in ONE launch and all hops are reduced in one more, with
 * one read-back.  The per-track reports are left behind mm_last_r128 (n, in track order).
 * MM_ERR_ARG, with words in mm_last_error and before anything is queued, for n outside
 * [1, MM_ALBUM_TRACKS], a track mm_r128_device refuses or a total of 2^31 frames or more.
 * The audio is never altered.  Synchronous on return. */
int mm_album_r128_device(mm_ctx *ctx, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                         int32_t rate, const double sos[2][5], mm_r128 *out);
/* The same on host buffers. */
int mm_album_r128_pcm(mm_ctx *ctx, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                      int32_t rate, const double sos[2][5], mm_r128 *out);
/* The album pass's hop energies themselves for host buffers, track after track (a per-stage
 * operator, for parity checks): copies the first min(sum H_t, cap) and returns sum H_t.  A
 * track's hops equal mm_op_r128_hops' of that track alone. */
int mm_op_r128_album_hops(mm_ctx *ctx, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                          int32_t rate, const double sos[2][5], double *hops_host, int64_t cap);
/* Level n device-resident tracks in place as one album (the album level above) to level_clu
 * under ceiling_q28 (0: none; window as mm_ceiling_device).  The mm_level and the album's
 * mm_r128 are left behind mm_last_album, the per-track reports of the delivered tracks behind
 * mm_last_r128 and, with a ceiling, mm_last_ceilings (n each, in track order).  The ceilings,
 * the gain and the measurement of a pass are each launched once over all tracks, as the batch
 * level's are, so the launches and synchronisations of a pass do not depend on n.  MM_ERR_ARG,
 * with words in mm_last_error, before anything is queued and with the context still usable,
 * for n outside [1, MM_ALBUM_TRACKS], a track mm_level_device refuses, level_clu outside
 * [-4000, -500] or a total of 2^31 frames or more.  Synchronous on return. */
int mm_album_level_device(mm_ctx *ctx, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                          int32_t rate, const double sos[2][5], int32_t level_clu, int32_t ceiling_q28, int32_t window);
/* The same on host buffers, in place. */
int mm_album_level_pcm(mm_ctx *ctx, void *const *pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                       const double sos[2][5], int32_t level_clu, int32_t ceiling_q28, int32_t window);
/* The result of the last mm_album_level_* call on this context.  MM_ERR_STATE if the last
 * call levelled no album. */
int mm_last_album(mm_ctx *ctx, mm_level *level, mm_r128 *album);

/* ---- a batch levelled track by track ----------------------------------------- */
/* The tracks of a batch are independent deliveries: every track t gets its OWN ceiling
 * ceiling_q28[t] and its OWN target level_clu[t], and what it receives is what the single-track
 * entry gives on that track alone, bit for bit, samples and statistics:
 *
 *   batch ceiling:  out[t] and track t as mm_ceiling_device(track t, ceiling_q28[t], window)
 *   batch level:    mm_level, mm_ceiling and track t as mm_level_device(track t, level_clu[t],
 *                   ceiling_q28[t], window); ceiling_q28[t] == 0: no ceiling for that track
 *                   (its gain is capped at its own sample peak); the R 128 report of track t
 *                   is mm_r128_device's of its delivered samples
 *
 * The tracks share one kind, channel count, rate and window.  Only the launch structure
 * differs from n calls: the need, apply, peak, trim, gain and K-weighting launches each cover
 * all tracks (csrc/ceiling.hip, tracks.hip, r128.hip), the tracks of a level advance one pass at a time, and the
 * launches and synchronisations of a pass do not depend on n. */

/* Hold n device-resident tracks, interleaved [frames[t]][channels] of `kind`, under their
 * ceilings in place; out[n] receives every track's mm_ceiling.  At most two synchronisations
 * (one when no track is trimmed).  MM_ERR_ARG, with words in mm_last_error that name the
 * track, before anything is queued and with the context still usable, for n outside
 * [1, MM_ALBUM_TRACKS], a track mm_ceiling_device refuses or a total of 2^31 frames or more.
 * Synchronous on return. */
int mm_batch_ceiling_device(mm_ctx *ctx, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                            const int32_t *ceiling_q28, int32_t window, mm_ceiling *out);
/* The same on host buffers, in place (an untouched track is not copied back). */
int mm_batch_ceiling_pcm(mm_ctx *ctx, void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                         const int32_t *ceiling_q28, int32_t window, mm_ceiling *out);
/* Level n device-resident tracks in place, track t to level_clu[t] under ceiling_q28[t] (0:
 * none).  The results are left behind mm_last_levels, mm_last_r128 (the delivered tracks') and,
 * when a track has a ceiling, mm_last_ceilings (n each, in track order; a track without a
 * ceiling leaves a cleared mm_ceiling with its channels).  MM_ERR_ARG as above, for n outside
 * [1, MM_ALBUM_TRACKS], a track mm_level_device refuses or a total of 2^31 frames or more.
 * Synchronous on return. */
int mm_batch_level_device(mm_ctx *ctx, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                          int32_t rate, const double sos[2][5], const int32_t *level_clu, const int32_t *ceiling_q28,
                          int32_t window);
/* The same on host buffers, in place. */
int mm_batch_level_pcm(mm_ctx *ctx, void *const *pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                       const double sos[2][5], const int32_t *level_clu, const int32_t *ceiling_q28, int32_t window);

/* ---- delivery at another sample rate ----------------------------------------- */
/* Convert a device-resident signal, interleaved [frames][channels] of `kind` (MM_OUT_I16,
 * or MM_OUT_F32 = the same PCM / 32768: both give the same integers), into d_out
 * ([frames_out][channels] of the same kind) as mm_resampler defines.  frames = 0 is valid
 * and gives frames_out = 0.  Synchronous on return. */
int mm_resample_device(mm_ctx *ctx, const void *d_in, int kind, int64_t frames, int channels, const mm_resampler *rs,
                       void *d_out, mm_resample *out);
/* The same on host buffers. */
int mm_resample_pcm(mm_ctx *ctx, const void *in, int kind, int64_t frames, int channels, const mm_resampler *rs,
                    void *out_pcm, mm_resample *out);
/* The definition restated in plain C++ on the host (no context, no GPU), interleaved
 * int16 in and out: a CPU check of what the kernel computes. */
int mm_resample_host(const int16_t *in, int64_t frames, int channels, const mm_resampler *rs, int16_t *out_pcm,
                     mm_resample *out);
/* *frames_out = ceil(frames * L / M). */
int mm_resample_frames(int64_t frames, int32_t L, int32_t M, int64_t *frames_out);
/* Output frames per workgroup of the converter's kernel (where its seams lie). */
int mm_resample_span(void);
/* Convert n device-resident tracks of one kind, channel count and rate pair, track t from
 * d_in[t] ([frames[t]][channels]) into d_out[t] ([ceil(frames[t] * L / M)][channels]); out[n]
 * receives every track's mm_resample.  No numerics are new: track t and out[t] are exactly
 * what mm_resample_device gives on that track alone; every position is relative to the
 * track's own start, the zero padding outside [0, frames[t]) included, so tracks that lie back
 * to back in one allocation never read or write a neighbour's frames (a pointer is aligned to
 * a frame, as for every entry).  Only the launch structure differs from n calls: one launch
 * covers the spans of all tracks (csrc/tracks.h), and a call costs one memset, one launch, one
 * read-back and one synchronisation whatever n (plus the taps upload when the table is not
 * the context's cached one); a call in which no track has frames launches nothing.
 * frames[t] == 0 is valid and gives frames_out == 0 (d_in[t] and d_out[t] may then be NULL).
 * MM_ERR_ARG, with words in mm_last_error that name the track, before anything is queued and
 * with the context still usable, for n outside [1, MM_ALBUM_TRACKS], a track
 * mm_resample_device refuses, a geometry or table it refuses, or a total of 2^31 input or
 * output frames or more.  Synchronous on return. */
int mm_batch_resample_device(mm_ctx *ctx, const void *const *d_in, int kind, const int64_t *frames, int n, int channels,
                             const mm_resampler *rs, void *const *d_out, mm_resample *out);
/* The same on host buffers. */
int mm_batch_resample_pcm(mm_ctx *ctx, const void *const *in, int kind, const int64_t *frames, int n, int channels,
                          const mm_resampler *rs, void *const *out_pcm, mm_resample *out);
/* mm_master_device / mm_master / mm_master_wav with a delivery: the chain runs into a
 * context buffer, the converter writes the caller's output ([frames_out][channels] of
 * job->out_kind; the WAV header carries rate_out and frames_out), then the delivery's
 * level, ceiling and report act on it, so all hold for what is delivered.  Without a
 * converter (rs == NULL) the chain writes the caller's output ([frames_proc][channels]) and
 * window is the ceiling's look-ahead at the job's rate.  level_clu != 0 needs `loud`
 * (MM_ERR_ARG otherwise).  The job must have
 * ceiling_q28 == 0 and meter_on == 0 (MM_ERR_ARG: they would act at the source rate) and
 * rs->rate_in == job->rate.  mm_result is the chain's (frames_out = frames_proc);
 * mm_last_meters and mm_last_ceilings report slot 0 as after mm_master. */
int mm_deliver_device(mm_ctx *ctx, const mm_job *job, const mm_delivery *dl, const void *d_in, void *d_out,
                      mm_result *res);
int mm_deliver(mm_ctx *ctx, const mm_job *job, const mm_delivery *dl, const void *in, void *out, mm_result *res);
int mm_deliver_wav(mm_ctx *ctx, const mm_job *job, const mm_delivery *dl, const char *in_path, const char *out_path,
                   mm_result *res);
/* The converter's statistics of the last mm_deliver* call on this context; MM_ERR_STATE
 * if the last master call was not a delivery. */
int mm_last_resample(mm_ctx *ctx, mm_resample *out);

/* ---- linear-phase FIR --------------------------------------------------------- */
/* Filter a device-resident signal, interleaved [frames][channels] of `kind` (MM_OUT_I16, or
 * MM_OUT_F32 = the same PCM / 32768: both give the same integers), into d_out (the same
 * shape and kind, another buffer: the filter runs out of place, and two ranges that overlap
 * anywhere are refused) as mm_fir defines.  frames = 0 is valid.  MM_ERR_ARG, with words in
 * mm_last_error and nothing written, for a table mm_fir refuses (a table whose nonzero taps_key and K are the context's cached ones is not read
 * again), more than 2 channels, frames outside [0, 2^31) or a bad kind.  Synchronous on return. */
int mm_fir_device(mm_ctx *ctx, const void *d_in, int kind, int64_t frames, int channels, const mm_fir *fir, void *d_out,
                  mm_fir_result *out);
/* The same on host buffers. */
int mm_fir_pcm(mm_ctx *ctx, const void *in, int kind, int64_t frames, int channels, const mm_fir *fir, void *out_pcm,
               mm_fir_result *out);
/* The definition restated in plain C++ with an int64 sum on the host (no context, no GPU),
 * interleaved int16 in and out: a CPU check of what the kernel computes.  Nothing outside
 * in[0, frames * channels) is read. */
int mm_fir_host(const int16_t *in, int64_t frames, int channels, const mm_fir *fir, int16_t *out_pcm, mm_fir_result *out);
/* Output frames per workgroup of the filter's kernel (where its seams lie). */
int mm_fir_span(void);
/* The statistics of the context's last mm_fir_device / mm_fir_pcm pass; MM_ERR_STATE if it
 * has run none. */
int mm_last_fir(mm_ctx *ctx, mm_fir_result *out);

/* ---- 24- and 32-bit integer PCM --------------------------------------------- */
/* Decode n_samples of `kind` (MM_IN_I24: any byte address; MM_IN_I32: 4-byte
 * aligned, MM_ERR_ARG otherwise) at the device pointer d_in into n_samples floats
 * at d_out, as MM_IN_I24 / MM_IN_I32 define.  Nothing outside the aligned dwords
 * that hold input bytes is read, nothing outside d_out[0, n_samples) written.
 * Synchronous on return. */
int mm_pcm_decode_device(mm_ctx *ctx, int kind, const void *d_in, int64_t n_samples, float *d_out);
/* The same on host buffers (a per-stage operator, like mm_op_pcm_to_float). */
int mm_op_pcm_decode(mm_ctx *ctx, int kind, const void *in, int64_t n_samples, float *out);
/* The definition restated in plain C++ on the host (no context, no GPU). */
int mm_pcm_decode_host(int kind, const void *in, int64_t n_samples, float *out);
/* Samples per workgroup pass of the decode kernel (where its seams lie). */
int mm_pcm_decode_span(void);

/* ---- WAV files (AME:43 decode, AME:98 export) ------------------------------ */
typedef struct mm_wav_info {
    int64_t frames;          /* whole frames in the data chunk                   */
    int64_t data_offset;     /* byte offset of the samples in the file           */
    int32_t rate;
    int32_t channels;
    int32_t format;          /* 1 = integer PCM, 3 = IEEE float32 (EXTENSIBLE resolved) */
    int32_t bits;            /* format 1: 16, 24 (packed) or 32; format 3: 32; for
                                EXTENSIBLE the container's bits (valid-bits are ignored:
                                samples are left-justified in the container)        */
} mm_wav_info;
/* Parse a RIFF/WAVE header (PCM 16/24/32-bit or float32; 24- and 32-bit PCM must
 * have nBlockAlign == channels * bits / 8).  ctx may be NULL (no message). */
int mm_wav_probe(mm_ctx *ctx, const char *path, mm_wav_info *info);
/* Master a WAV file into out_path (PCM16 WAV for MM_OUT_I16, float32 WAV for
 * MM_OUT_F32).  The samples stream from the file through pinned, double-buffered
 * staging into HBM as they are read (integer PCM crosses PCIe as it lies in the
 * file, 2, 3 or 4 bytes a sample, and is decoded on the GPU) and the output, 16-bit
 * whatever the input's width, streams back the same way.  job must be
 * built for the probed frames/rate/channels; its in_kind is ignored (taken from
 * the file). */
int mm_master_wav(mm_ctx *ctx, const mm_job *job, const char *in_path, const char *out_path, mm_result *res);

/* ---- staged entry points (time-sharded multi-GPU, parity probes) -------- */
/* Run AME:48-80 for this job's chunks into the context's int16 mix buffer and
 * the K-weighting per-tile aggregates (state carry-in assumed 0).  The context
 * copies the job's seg_bounds, block_lo and block_hi: the later staged calls read
 * the copies, so the job's arrays need not outlive this call. */
int mm_stage_chunks(mm_ctx *ctx, const mm_job *job, const void *d_in);
/* K-weighting end state of this job's range from a zero start: dim doubles. */
int mm_kweight_range_end(mm_ctx *ctx, double *end_state_host);
/* Per-segment K-weighted energies given a carry-in state (host [dim] or NULL);
 * writes n_segs doubles to host. */
int mm_hop_energies(mm_ctx *ctx, const double *carry_in_host, double *seg_energy_host);
/* Device-resident variant of mm_hop_energies + all-reduce + gating + mm_finalize
 * (VERDICT r03 item 7), in three composable steps (the collective in between may be
 * the library's communicator or torch.distributed over the same device buffer):
 * mm_shard_energies_device zeroes the caller's device vector d_full[n_global_segs]
 * and writes this rank's n_segs energies at seg_offset (synchronous on return);
 * mm_gate_finalize_device gates the whole track on the device (block b: segments
 * [blk_s0[b], blk_s1[b]), energies scaled by block_scale), applies the gain towards
 * `target` LUFS with the limiter, writes this rank's output to d_out and returns
 * {L, applied gain} in loudness_gain[2]. */
int mm_shard_energies_device(mm_ctx *ctx, const double *carry_in_host, int64_t n_global_segs, int64_t seg_offset,
                             double *d_full);
int mm_gate_finalize_device(mm_ctx *ctx, const double *d_full, int64_t n_global_segs, int64_t n_blocks,
                            const int32_t *blk_s0_host, const int32_t *blk_s1_host, double block_scale,
                            double target, void *d_out, double *loudness_gain);
/* All three with the library's communicator between them: `world` is the plan's rank
 * count; world > 1 needs mm_comm_init over exactly `world` ranks on this context
 * (MM_ERR_STATE otherwise: each rank would gate only its own part of the vector). */
int mm_shard_loudness_device(mm_ctx *ctx, const double *carry_in_host, int64_t n_global_segs, int64_t seg_offset,
                             int64_t n_blocks, const int32_t *blk_s0_host, const int32_t *blk_s1_host,
                             double block_scale, double target, int32_t world, void *d_out, double *loudness_gain);
/* Gated loudness from full-track segment energies (host, C restatement of
 * pyloudnorm's gating); returns L via *loudness. */
int mm_gate_loudness(const mm_job *job, const double *seg_energy, double *loudness);
/* numpy's float32 np.sum of x[0..n) (n <= 131072), on the host, through the reduction
 * program the device runs for pyloudnorm's block energies (8192-element buffer
 * chunks, pairwise leaves of <= 128 with eight accumulators): a CPU check that the
 * device sums in numpy's order. */
int mm_np_sum_f32(const float *x, int64_t n, float *out);
/* Verification entry (no reference counterpart): the compressor's device exp10 and
 * exact rms on host arrays of n arguments.  what 0: out[i] = exp10_tab(a[i]) (the
 * gain 10^y of comp_apply, y in [-3, 0]); what 1: out[i] = rms_exact1(a[i], b[i])
 * (comp_rms's audioop.rms: isqrt(floor(S / n)) for integer S = a[i] < 2^53 and
 * n = b[i] >= 1).  Checked by tests/test_compressor_math.py. */
int mm_check_compressor_math(mm_ctx *ctx, int what, const double *a, const double *b, int64_t n, double *out);
/* Apply gain + soft limiter + quantise (AME:84-89) to the staged mix. */
int mm_finalize(mm_ctx *ctx, double gain_linear, int use_gain, void *d_out);
/* Copy the staged pre-gain int16 mix (interleaved) to host (parity probe). */
int mm_read_mix(mm_ctx *ctx, int16_t *host_mix);

/* ---- timing (HIP events on the context stream) -------------------------- */
/* Enable per-kernel event timing; stats are averages over launches. */
int mm_timing(mm_ctx *ctx, int enable);
/* names: '\n'-joined kernel names into buf; ms/launches arrays of cap entries. */
int mm_kernel_stats(mm_ctx *ctx, char *names, int names_cap, double *total_ms, int64_t *launches, int cap);

/* ---- per-stage operators (AME:117-227, one stage at a time) --------------
 * The reference's public DSP helpers as standalone device operators, numpy in /
 * numpy out through host buffers (mastering_amd/ops.py mirrors their Python
 * signatures).  dtype is the sample type of a float input; an f32 input computes
 * in f32 (numpy's dtype rules for the reference's expressions), an f64 one in f64.
 * n counts samples, frames count [frames][channels] rows. */
#define MM_F32 0
#define MM_F64 1
/* audio_segment_to_float_array (AME:117-121): int16 -> f32 / 32768 */
int mm_op_pcm_to_float(mm_ctx *ctx, const int16_t *in, int64_t n, float *out);
/* apply_saturation (AME:128-134); percent != 0 (0 is the identity, no call) */
int mm_op_saturation(mm_ctx *ctx, int dtype, const void *in, int64_t n, double percent, void *out);
/* the same with the int16-grid table of mm_job.sat_table (table: [65536] f32, or
   NULL for the tanhf path): f32 inputs k / 32768 read entry k + 32768, others take
   tanhf; f64 inputs always compute in f64 */
int mm_op_saturation_table(mm_ctx *ctx, int dtype, const void *in, int64_t n, double percent, const float *table,
                           void *out);
/* apply_stereo_width (AME:136-144) on interleaved stereo [frames][2] */
int mm_op_stereo_width(mm_ctx *ctx, int dtype, const void *in, int64_t frames, double width, void *out);
/* float_array_to_audio_segment's samples (AME:123-126): clip, *32768, astype(int16) */
int mm_op_quantize(mm_ctx *ctx, int dtype, const void *in, int64_t n, int16_t *out);
/* soft_limiter (AME:224-227), in place like the reference */
int mm_op_soft_limiter(mm_ctx *ctx, int dtype, void *inout, int64_t n, double threshold);
/* samples * np.float64(gain) -> f64 (AME:222) */
int mm_op_gain(mm_ctx *ctx, int dtype, const void *in, int64_t n, double gain, double *out);
/* scipy.signal.sosfilt of ONE cascade (f->nsec 1..4 sections, all in branch 0,
 * tables for LB tiles/block = 256/channels) over each channel column of
 * [frames][channels], zero initial state; f64 out.  round_f32: every section's
 * output is rounded to f32 (pyloudnorm's lfilter write-backs; such a cascade runs
 * one launch per section, because the tile carry cannot hold a rounded hand-over).
 * f->tile in [1, 512] with 16 * (tile * channels + 1) * 8 <= 65536 bytes (the layout
 * transposes' LDS: tile <= 255 stereo, 511 mono), else MM_ERR_ARG.  Replaces
 * apply_eq_to_samples / apply_shelf_filter / apply_peak_filter (AME:146-194). */
int mm_op_sosfilt(mm_ctx *ctx, int dtype, const void *in, int64_t frames, int channels, const mm_iir *f,
                  int round_f32, double *out);
/* pyloudnorm Meter(rate).integrated_loudness of samples.mean(axis=1) (AME:213-218).
 * job: channels, frames_proc, kweight (tpb 256), loudness geometry, lufs_target.
 * out[0] = loudness (LUFS), out[1] = 10 ** ((lufs_target - L) / 20). */
int mm_op_loudness(mm_ctx *ctx, const mm_job *job, int dtype, const void *in, double *out);
/* Linear true peak of off-grid samples [frames][channels] (no reference counterpart):
 * the Annex 2 FIR of mm_meter in f64, y = sum_k H[p][k] * x[m-k] accumulated for
 * k = 0..11 in that order without contraction; out[c] = max |y| of channel c. */
int mm_op_true_peak(mm_ctx *ctx, int dtype, const void *in, int64_t frames, int channels, double *out);
/* The legacy engine's variants (main.py:94-192, mastering_amd/legacy.py):
 * saturation tanh(x*g)/g with g = 1 + 4*amount/100 (main.py:94-97); limiter
 * |x| > threshold -> tanh(x)*threshold (main.py:189-192); an EQ stage as the
 * parallel mix a*x + c*sosfilt(x) of its butter() filter (main.py:133-154: the
 * a*x product in f32 for f32 samples, numpy's rule), f64 out; and the compressor
 * + overlay on three given int16 band arrays (main.py:156-177, whose mid band is
 * LP4000(HP250(x)) rather than x - lo - hi). */
int mm_op_saturation_legacy(mm_ctx *ctx, int dtype, const void *in, int64_t n, double amount, void *out);
int mm_op_soft_limiter_legacy(mm_ctx *ctx, int dtype, void *inout, int64_t n, double threshold);
int mm_op_sosfilt_mix(mm_ctx *ctx, int dtype, const void *in, int64_t frames, int channels, const mm_iir *f,
                      double a, double c, double *out);
int mm_op_compress_bands(mm_ctx *ctx, const mm_job *job, const int16_t *lo, const int16_t *mid, const int16_t *hi,
                         int16_t *out);
/* apply_multiband_compressor (AME:196-210) on int16 PCM [frames][channels]:
 * job with multiband_on, in_kind MM_IN_I16, EQ/exciter/width/loudness off and one
 * chunk covering the input (tile * tiles_per_chunk >= frames_proc); out has the
 * input's frames (pydub overlay's ms re-slicing is the caller's). */
int mm_op_multiband(mm_ctx *ctx, const mm_job *job, const int16_t *in, int16_t *out);

/* ---- RCCL over xGMI ----------------------------------------------------- */
int mm_comm_unique_id(char id_out[128]);
int mm_comm_init(mm_ctx *ctx, int rank, int nranks, const char id[128]);
int mm_comm_destroy(mm_ctx *ctx);
/* In-place sum all-reduce of n doubles in host memory (staged through HBM). */
int mm_allreduce_sum_f64(mm_ctx *ctx, double *host_buf, int64_t n);
/* All-gather of n doubles per rank: out = [nranks * n]. */
int mm_allgather_f64(mm_ctx *ctx, const double *host_in, double *host_out, int64_t n);
/* The same two collectives on device buffers of this context's device (no host
 * staging; synchronous on return). */
int mm_allreduce_sum_f64_device(mm_ctx *ctx, double *d_buf, int64_t n);
int mm_allgather_f64_device(mm_ctx *ctx, const double *d_in, double *d_out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif
