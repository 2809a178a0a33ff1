// meter.hip — the mastering report: sample peak, ITU-R BS.1770-4 Annex 2 true peak
// (4x oversampling FIR, order 48) and the loudness of the delivered output.  No
// reference counterpart: the reference never measures what it wrote.
//
// On the int16 grid the Annex 2 filter is exact in integers: every tap is a
// multiple of 2^-13, so with C = H * 8192 the oversampled signal is
//   Y[m][p] = sum_{k<12} C[p][k] * s[m-k],  m in [0, N+11), p in 0..3
// in int32 (|Y| <= 16571 * 32768 < 2^31), and the linear true peak is max|Y| / 2^28.
// All results are integers combined with max / add: nothing depends on the launch
// geometry or on the order in which workgroups finish.
//
// This file owns the taps and the oversampler, on the device (tp_stage, tp_window, tp_frame)
// and on the host (tp_host): ceil_need and mm_ceiling_host in ceiling.hip run the same.
//
// Included at the end of mastering.hip (one translation unit), after ops.hip and
// loudness.hip (the host entry points use the context helpers, the operators' pointwise
// kernels and loudness_device) and pcm16.h.

namespace mm {

constexpr int METER_THREADS = 256;
constexpr int METER_FPT = 8;                            // output frames m per thread
constexpr int METER_SPAN = METER_THREADS * METER_FPT;   // frames of m per workgroup (mm_meter_span)
constexpr int METER_WGS_PER_CU = 4;                     // resident workgroups a launch is capped at, per CU
constexpr int METER_HALO = 12;                          // 11 frames of history + 1 so that windows start on a dword
constexpr int METER_LINE = (METER_SPAN + METER_HALO + 7) / 8 * 8;  // int16 per channel line in LDS (16-byte multiple)
constexpr int64_t METER_MAX_FRAMES = ((int64_t)1 << 31) - METER_SPAN;  // frames of a signal on the grid stay below this

// H * 8192 of BS.1770-4 Annex 2, phases 0 and 1 (2 and 3 are their reversals)
#define MM_TP_C0 14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68
#define MM_TP_C1 -239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155
#define MM_TP_C2 -155, 271, -477, 832, -1641, 6388, 3810, -1364, 730, -424, 240, -239
#define MM_TP_C3 -68, 122, -218, 390, -838, 7964, 1125, -487, 272, -161, 90, 14

struct TpTaps {
    int c[4][12];
};
__host__ __device__ constexpr TpTaps tp_taps() { return TpTaps{{{MM_TP_C0}, {MM_TP_C1}, {MM_TP_C2}, {MM_TP_C3}}}; }

// taps k = 2q (high half, meets the later sample) and 2q + 1 (low half) as one packed pair
__device__ __forceinline__ constexpr uint32_t tp_pair(int p, int q) {
    constexpr TpTaps t = tp_taps();
    return ((uint32_t)(uint16_t)t.c[p][2 * q + 1]) | ((uint32_t)(uint16_t)t.c[p][2 * q] << 16);
}

typedef short tp_v2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int tp_dot2(uint32_t samples, uint32_t taps, int acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(tp_v2, samples), __builtin_bit_cast(tp_v2, taps), acc, false);
}

// device result block of one metered signal (zeroed on the stream before the launch)
struct MeterDev {
    unsigned long long key[2];      // (true peak << 32) | (0xFFFFFFFF - frame): max = peak, smallest frame
    unsigned long long clipped[2];
    unsigned long long overs[2];
    int sample_peak[2];
    int _pad[2];
};

// The CH lines of the span at `base` and their halo, de-interleaved (zeros outside [0, N)).
template <int CH, typename T>
__device__ __forceinline__ void tp_stage(int16_t (&line)[CH][METER_LINE], const T *__restrict__ in, int64_t N, int64_t base) {
    const int64_t f0 = base - METER_HALO;  // frame of LDS index 0
    for (int i = threadIdx.x; i < METER_LINE; i += METER_THREADS) {
        const int64_t f = f0 + i;
        int s[CH] = {};
        if (f >= 0 && f < N) load_frame<CH, T>(in, f, s);
#pragma unroll
        for (int c = 0; c < CH; ++c) line[c][i] = (int16_t)s[c];
    }
    __syncthreads();
}

// The window of the METER_FPT frames m0 .. at line position pos = m0 - base (a multiple of
// 8): w[i] = s[m0 - 12 + i], i < 20, read as ten dwords D[i] = (w[2i], w[2i+1]) and kept in
// both packings, P[i] = (w[i], w[i+1]).
__device__ __forceinline__ void tp_window(const int16_t *pos, uint32_t (&P)[19]) {
    const uint4 *src = reinterpret_cast<const uint4 *>(pos);
    const uint4 a = src[0], b = src[1];
    const uint2 e = *reinterpret_cast<const uint2 *>(src + 2);
    const uint32_t D[10] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, e.x, e.y};
#pragma unroll
    for (int i = 0; i < 19; ++i) P[i] = (i & 1) ? ((D[i / 2] >> 16) | (D[i / 2 + 1] << 16)) : D[i / 2];
}

// |Y[m0 + j][p]| of a window: 6 packed dot products (the callers unroll over p < 4 and
// combine the four in their own way)
__device__ __forceinline__ int tp_frame(const uint32_t (&P)[19], int j, int p) {
    int acc = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) acc = tp_dot2(P[j + 11 - 2 * q], tp_pair(p, q), acc);
    return acc < 0 ? -acc : acc;  // |Y| <= 542994228: the negation cannot overflow
}

// A workgroup takes spans blockIdx.x, blockIdx.x + gridDim.x, ... in turn; one span
// is m in [base, base + METER_SPAN) of every channel.  The span and its halo are
// staged de-interleaved in LDS as int16 lines; a thread then owns METER_FPT
// consecutive m and reads its 20-sample window as ten dwords.  The pair
// (s[i], s[i+1]) that a tap pair meets is a window dword for even i and an
// alignbit of two neighbours for odd i: both packings are kept in registers, so the
// 48 MACs of a frame are 24 packed dot products whatever the parity of m.  A thread
// keeps its maxima and counts in registers over its spans (they come in ascending m,
// so a strict compare keeps the smallest frame of a tie); the workgroup reduces once
// at the end and issues one atomic per result word, which keeps the traffic on the
// result block's single cache line to a few thousand atomics however long the track.
template <int CH, typename T>
__global__ void __launch_bounds__(METER_THREADS) meter_i16_kernel(const T *__restrict__ in, int64_t N, int64_t spans,
                                                                  MeterDev *res) {
    __shared__ __attribute__((aligned(16))) int16_t line[CH][METER_LINE];
    __shared__ unsigned long long red_key[CH][METER_THREADS / 64];
    __shared__ unsigned red_clip[CH][METER_THREADS / 64], red_over[CH][METER_THREADS / 64];
    __shared__ int red_pk[CH][METER_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int best[CH], spk[CH];
    uint32_t best_m[CH];
    unsigned n_clip[CH], n_over[CH];  // <= METER_FPT per span and thread; a workgroup's sum stays below 2^32
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        best[c] = -1;
        spk[c] = 0;
        best_m[c] = 0;
        n_clip[c] = n_over[c] = 0;
    }
    for (int64_t span = blockIdx.x; span < spans; span += gridDim.x) {
        const int64_t base = span * METER_SPAN;
        tp_stage<CH, T>(line, in, N, base);
        const int64_t m0 = base + (int64_t)threadIdx.x * METER_FPT;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            uint32_t P[19];
            tp_window(&line[c][threadIdx.x * METER_FPT], P);
            unsigned cnt = 0;  // overs << 16 | clipped of this span
#pragma unroll
            for (int j = 0; j < METER_FPT; ++j) {
                int y[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) y[p] = tp_frame(P, j, p);
                const int pm = max(max(y[0], y[1]), max(y[2], y[3]));
                if (pm > best[c]) {  // strict: the smallest m of a tie stays
                    best[c] = pm;
                    best_m[c] = (uint32_t)(m0 + j);
                }
                cnt += pm > (1 << 28) ? 0x10000u : 0u;
                // s[m0 + j] = w[j + 12] = the high half of P[j + 11]
                const int s = (int)P[j + 11] >> 16;
                const int as = s < 0 ? -s : s;
                spk[c] = max(spk[c], as);
                cnt += as >= 32767 ? 1u : 0u;
            }
            n_clip[c] += cnt & 0xFFFFu;
            n_over[c] += cnt >> 16;
        }
        __syncthreads();  // the lines are free for the next span
    }
    if (best[0] < 0) return;  // a workgroup without a span (never launched: grid <= spans)
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        unsigned long long key = ((unsigned long long)(uint32_t)best[c] << 32) | (0xFFFFFFFFu - best_m[c]);
        key = wave_max_u64(key);
        const unsigned nc = wave_sum_u32(n_clip[c]), no = wave_sum_u32(n_over[c]);
        const int pk = wave_max_i32(spk[c]);
        if (lane == 0) {
            red_key[c][wave] = key;
            red_clip[c][wave] = nc;
            red_over[c][wave] = no;
            red_pk[c][wave] = pk;
        }
    }
    __syncthreads();
    if (threadIdx.x < CH) {
        const int c = threadIdx.x;
        unsigned long long key = 0;
        unsigned nc = 0, no = 0;
        int pk = 0;
        for (int w = 0; w < METER_THREADS / 64; ++w) {
            key = red_key[c][w] > key ? red_key[c][w] : key;
            nc += red_clip[c][w];
            no += red_over[c][w];
            pk = max(pk, red_pk[c][w]);
        }
        atomicMax(&res->key[c], key);
        if (nc) atomicAdd(&res->clipped[c], (unsigned long long)nc);
        if (no) atomicAdd(&res->overs[c], (unsigned long long)no);
        if (pk) atomicMax(&res->sample_peak[c], pk);
    }
}

// The off-grid operator: the same FIR in f64, y = sum_k H[p][k] * x[m-k] accumulated
// for k = 0..11 in that order (no contraction); max |y| per channel.  out[c] holds the
// bits of a non-negative double, which order like unsigned integers.
template <int CH, typename T>
__global__ void __launch_bounds__(256) meter_float_kernel(const T *__restrict__ in, int64_t N, unsigned long long *out) {
    constexpr TpTaps t = tp_taps();
    __shared__ unsigned long long red[CH][4];
    double best[CH];
    for (int c = 0; c < CH; ++c) best[c] = 0.0;
    const int64_t M = N + 11, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += stride) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            double x[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const int64_t f = m - k;
                x[k] = (f >= 0 && f < N) ? (double)in[f * CH + c] : 0.0;
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                double acc = __dmul_rn((double)t.c[p][0] / 8192.0, x[0]);
#pragma unroll
                for (int k = 1; k < 12; ++k) acc = __dadd_rn(acc, __dmul_rn((double)t.c[p][k] / 8192.0, x[k]));
                const double ay = fabs(acc);
                if (ay > best[c]) best[c] = ay;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < CH; ++c) {
        const unsigned long long v = wave_max_u64((unsigned long long)__double_as_longlong(best[c]));
        if (lane == 0) red[c][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < CH) {
        unsigned long long v = 0;
        for (int w = 0; w < 4; ++w) v = red[threadIdx.x][w] > v ? red[threadIdx.x][w] : v;
        if (v) atomicMax(&out[threadIdx.x], v);
    }
}

}  // namespace mm

// ======================================================= host entry points
namespace {

void meter_clear(mm_meter *m, int64_t frames, int channels) {
    memset(m, 0, sizeof *m);
    m->frames = frames;
    m->channels = channels;
    m->loudness = NAN;
}

// does `loud` carry the loudness geometry of a signal of these frames?
bool meter_has_geometry(const mm_job *loud, int64_t frames) {
    return loud && loud->kweight.nsec == 2 && loud->n_segs >= 1 && loud->n_blocks >= 1 && loud->seg_bounds &&
           loud->block_lo && loud->block_hi && loud->rate > 0 && 5 * frames >= 2 * (int64_t)loud->rate;
}

}  // namespace

// Queue one metering pass of a device-resident signal on the context's stream: the
// result block (zeroed on the stream first) is read by the caller after its sync.
// frames in [1, 2^31 - METER_SPAN), kind and channels already checked.
static int meter_launch(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, MeterDev *res) {
    HIPCHK(c, hipMemsetAsync(res, 0, sizeof(MeterDev), c->stream));
    const int64_t spans = tracks_need_spans(frames);
    const dim3 grid((unsigned)std::min<int64_t>(spans, (int64_t)METER_WGS_PER_CU * c->n_cus)), block(METER_THREADS);
    return dispatch_pcm(kind, channels, [&](auto ch, auto t) {
        using T = decltype(t);
        return launch(c, "meter_i16", meter_i16_kernel<ch, T>, grid, block, 0, static_cast<const T *>(d_pcm), frames, spans, res);
    });
}

// Meter a device-resident signal on the context's stream (synchronous on return).
static int meter_device(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, const mm_job *loud,
                        mm_meter *out) {
    if (!c || !out || (frames > 0 && !d_pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    static const char RANGE[] = "frames %lld out of range";  // (this stage's words print the count)
    if (const char *why = pcm_refusal(channels, frames, METER_MAX_FRAMES, RANGE))
        return why == RANGE ? set_err(c, MM_ERR_ARG, RANGE, (long long)frames) : set_err(c, MM_ERR_ARG, "%s", why);
    meter_clear(out, frames, channels);
    if (frames == 0) return MM_OK;
    if (loud && meter_has_geometry(loud, frames) && (loud->frames_proc != frames || loud->channels != channels))
        return set_err(c, MM_ERR_ARG, "loudness geometry built for %lld frames x %d ch", (long long)loud->frames_proc,
                       loud->channels);
    MeterDev *res;
    RET(get_buf(c, "meter_res", 1, &res));
    RET(meter_launch(c, d_pcm, kind, frames, channels, res));
    MeterDev h;
    HIPCHK(c, hipMemcpyAsync(&h, res, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int ch = 0; ch < channels; ++ch) {
        out->sample_peak[ch] = h.sample_peak[ch];
        out->true_peak_q28[ch] = (int32_t)(h.key[ch] >> 32);
        out->true_peak_frame[ch] = (int64_t)(0xFFFFFFFFu - (uint32_t)h.key[ch]);
        out->clipped[ch] = (int64_t)h.clipped[ch];
        out->overs[ch] = (int64_t)h.overs[ch];
    }
    if (meter_has_geometry(loud, frames)) {
        const void *f32 = d_pcm;
        if (kind == MM_OUT_I16) {  // decode as the reference does (AME:117-121), then its own measurement
            float *dec;
            RET(get_buf(c, "meter_f32", (size_t)frames * channels, &dec));
            PwArgs pa{};
            pa.n = frames * channels;
            pa.in = d_pcm;
            pa.out = dec;
            RET(launch(c, "meter_decode", pointwise_kernel<PW_PCM16, float>, dim3(pw_blocks(pa.n)), dim3(256), 0, pa));
            f32 = dec;
        }
        double lg[2];
        RET(loudness_device(c, loud, MM_F32, f32, lg));
        out->loudness = lg[0];
    }
    resolve_events(c);
    return MM_OK;
}

// max_p |Y_c[m][p]| in plain C++ on the host: the 12-tap loop of the definition, the one
// formulation behind mm_true_peak_host and mm_ceiling_host.
static int32_t tp_host(const int16_t *pcm, int64_t frames, int channels, int c, int64_t m) {
    constexpr TpTaps t = tp_taps();
    int32_t pm = 0;
    for (int p = 0; p < 4; ++p) {
        int32_t acc = 0;
        for (int k = 0; k < 12; ++k) {
            const int64_t f = m - k;
            if (f >= 0 && f < frames) acc += t.c[p][k] * (int32_t)pcm[f * channels + c];
        }
        pm = std::max(pm, acc < 0 ? -acc : acc);
    }
    return pm;
}

extern "C" {

int mm_meter_span(void) { return METER_SPAN; }

int mm_meter_device(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, const mm_job *loud,
                    mm_meter *out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return meter_device(c, d_pcm, kind, frames, channels, loud, out);
}

int mm_meter_pcm(mm_ctx *c, const void *pcm, int kind, int64_t frames, int channels, const mm_job *loud,
                 mm_meter *out) {
    if (!c) return MM_ERR_ARG;
    if (frames < 0 || (frames > 0 && !pcm) || (channels != 1 && channels != 2) || !pcm_kind_ok(kind))
        return set_err(c, MM_ERR_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    char *din;
    RET(pcm_upload(c, "meter_in", pcm, pcm_bytes(kind, frames, channels), &din));
    return meter_device(c, din, kind, frames, channels, loud, out);
}

int mm_last_meters(mm_ctx *c, int cap, mm_meter *out) {
    if (!c || cap < 0 || (cap > 0 && !out)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->meters.empty()) return set_err(c, MM_ERR_STATE, "the last master call did not meter");
    const int n = (int)c->meters.size();
    for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->meters[(size_t)i];
    return n;
}

int mm_op_true_peak(mm_ctx *c, int dtype, const void *in, int64_t frames, int channels, double *out) {
    if (!c || !out || (frames > 0 && !in)) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(check_dtype(c, dtype));
    if (channels != 1 && channels != 2) return set_err(c, MM_ERR_ARG, "channels must be 1 or 2");
    if (frames < 0 || frames >= ((int64_t)1 << 31) - 16) return set_err(c, MM_ERR_ARG, "frames out of range");
    for (int ch = 0; ch < channels; ++ch) out[ch] = 0.0;
    if (frames == 0) return MM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)frames * channels * dtype_size(dtype);
    char *din;
    unsigned long long *res;
    RET(get_buf(c, "op_in", bytes, &din));
    RET(get_buf(c, "meter_fres", 2, &res));
    HIPCHK(c, hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(res, 0, 16, c->stream));
    const dim3 grid(pw_blocks(frames + 11)), block(256);
    if (dtype == MM_F32) {
        if (channels == 2) RET(launch(c, "meter_float", meter_float_kernel<2, float>, grid, block, 0, (const float *)din, frames, res));
        else RET(launch(c, "meter_float", meter_float_kernel<1, float>, grid, block, 0, (const float *)din, frames, res));
    } else {
        if (channels == 2) RET(launch(c, "meter_float", meter_float_kernel<2, double>, grid, block, 0, (const double *)din, frames, res));
        else RET(launch(c, "meter_float", meter_float_kernel<1, double>, grid, block, 0, (const double *)din, frames, res));
    }
    unsigned long long h[2];
    HIPCHK(c, hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    for (int ch = 0; ch < channels; ++ch) memcpy(&out[ch], &h[ch], 8);
    return MM_OK;
}

// The integer definition restated in plain C++ on the host (no context, no GPU):
// what the meter_i16 kernel must reproduce field for field.  loudness stays NaN.
int mm_true_peak_host(const int16_t *pcm, int64_t frames, int channels, mm_meter *out) {
    if (!out || frames < 0 || (frames > 0 && !pcm) || (channels != 1 && channels != 2)) return MM_ERR_ARG;
    meter_clear(out, frames, channels);
    for (int c = 0; c < channels && frames > 0; ++c) {
        int32_t best = -1;
        int64_t best_m = 0;
        for (int64_t m = 0; m < frames + 11; ++m) {
            const int32_t pm = tp_host(pcm, frames, channels, c, m);
            if (pm > best) {
                best = pm;
                best_m = m;
            }
            if (pm > (1 << 28)) ++out->overs[c];
            if (m < frames) {
                const int32_t s = pcm[m * channels + c], as = s < 0 ? -s : s;
                out->sample_peak[c] = std::max(out->sample_peak[c], as);
                if (as >= 32767) ++out->clipped[c];
            }
        }
        out->true_peak_q28[c] = best;
        out->true_peak_frame[c] = best_m;
    }
    return MM_OK;
}

}  // extern "C"
