// fir.hip — an exact linear-phase FIR on the int16 grid: the stage a reference match (engine.
// match_pcm) applies its tonal curve with.  No reference counterpart.  Everything is
// defined in integers (include/mastering.h, mm_fir): with c[K] the caller's symmetric int32 taps
// (design.match_taps), K odd and H = (K - 1) / 2, output frame n of a channel is
//   acc = sum_{k<K} c[k] * s[n + H - k]        (s = 0 outside [0, N))
//   y   = (acc + 2^21) >> 22, delivered clipped to int16
// Frame n stays at frame n.  sum |c| < 2^24 (checked), so |acc| < 2^39: the sum is exact in
// int64 and just as exact as an f64 FMA chain in any order, folded or not.  The kernel sums in
// f64 FMAs (resample.hip says why), the host restatement in int64; the results are the same
// integers, so nothing depends on the launch geometry.
//
// The kernel (fir_span; fir_kernel runs it on the one signal of a call).  A workgroup owns
// FIR_SPAN consecutive output frames and stages the FIR_SPAN + K - 1 input frames they read,
// and FIR_GUARD more a side, in LDS, one dword a frame: a stereo frame packed with left in the
// low half (resample.hip: two int16 lines were 6.6 times slower), a mono sample as its int32.
// Against resample_span three things differ:
//   - the symmetry is folded: with d = |k - H| the pair c[H - d] = c[H + d] meets s[n + d] +
//     s[n - d], added as int32 and converted once, so a pair of taps costs one FMA an output;
//   - the taps are uniform: every lane needs the same c[H + d], kept on the device as doubles
//     (exact: |c| < 2^24) and read through a uniform read-only address, so they arrive in scalar
//     registers and feed the FMA directly, with no conversion and no vector load;
//   - a work item is FIR_R consecutive outputs, whose two sample windows slide through
//     registers: a step reads ONE new frame a side for its FIR_R outputs.  Lane t then reads
//     frame FIR_R * t + c with c uniform, a 4-dword stride that would meet 8 of the 32 banks; so
//     the line is kept de-interleaved by frame mod 4 (fir_phys): the lanes of a read are
//     consecutive dwords, and the uniform part of the address is scalar arithmetic.
// The pair loop runs in steps of 4 (the windows are rings of 4 registers with static slots);
// the device table is padded with zero taps to a multiple of 4, and the guard frames are what
// those zero taps meet (real samples or zeros: the products are exact zeros either way).
//
// Included in mastering.hip after resample.hip.

namespace mm {

constexpr int FIR_THREADS = 256;
constexpr int FIR_R = 4;                         // consecutive outputs per work item
constexpr int FIR_SPAN = FIR_THREADS * FIR_R;    // output frames per workgroup (mm_fir_span)
constexpr int FIR_MAX_K = 8191;
constexpr int FIR_GUARD = 4;                     // frames a side that only zero taps meet
constexpr int FIR_Q = 2312;                      // dwords of a residue's row: >= (FIR_SPAN + FIR_MAX_K - 1 + 2 * FIR_GUARD + 3) / 4,
                                                 // and = 8 mod 32, so that the staging writes of 32 lanes meet 32 banks
constexpr int64_t FIR_SUM_LIMIT = (int64_t)1 << 24;  // sum |c| below this
static_assert(FIR_R == 4, "the rings of fir_span have 4 static slots");
static_assert(4 * FIR_Q >= FIR_SPAN + FIR_MAX_K - 1 + 2 * FIR_GUARD + 3 && FIR_Q % 32 == 8, "FIR_Q");

// device result block of one pass (zeroed on the stream before the launch)
struct FirDev {
    unsigned long long clipped[2];
    int peak[2];
    int peak_unclipped[2];
};

struct FirArgs {
    int64_t N;   // frames
    int Hp;      // pairs of the device table: H rounded up to a multiple of 4
    int H;
    FirDev *st;
};

// LDS dword of staged frame i (frame 0 of the line is signal frame n0 - H - FIR_GUARD)
__device__ __forceinline__ int fir_phys(int i) { return (i & 3) * FIR_Q + (i >> 2); }

template <int CH>
__device__ __forceinline__ void fir_unpack(uint32_t d, int (&s)[CH]) {
    if constexpr (CH == 2) {
        s[0] = (int)(d << 16) >> 16;
        s[1] = (int)d >> 16;
    } else {
        s[0] = (int)d;
    }
}

// One span of one signal, `n0` its first output frame.  taps[0] = c[H], taps[d] = c[H + d] for
// d <= H and 0 for H < d <= Hp, as doubles.
template <int CH, typename T>
__device__ __forceinline__ void fir_span(const T *__restrict__ in, T *__restrict__ out, const double *__restrict__ taps,
                                         FirArgs a, int64_t n0) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[4 * FIR_Q];
    __shared__ unsigned red_clip[CH][FIR_THREADS / 64];
    __shared__ int red_pk[CH][FIR_THREADS / 64];
    __shared__ int red_un[CH][FIR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H;
    const int span = a.N - n0 < FIR_SPAN ? (int)(a.N - n0) : FIR_SPAN;
    // every frame a read below can meet: FIR_SPAN + 2 H + 2 FIR_GUARD of them, zero outside the signal
    const int len = FIR_SPAN + 2 * H + 2 * FIR_GUARD;
    const int64_t lo = n0 - H - FIR_GUARD;
    for (int i = tid; i < len; i += FIR_THREADS) {
        const int64_t f = lo + i;
        uint32_t d = 0u;
        if (f >= 0 && f < a.N) {
            if constexpr (CH == 2) {
                d = load_frame_packed<T>(in, f);
            } else {
                int s[1];
                load_frame<1, T>(in, f, s);
                d = (uint32_t)s[0];
            }
        }
        lds[fir_phys(i)] = d;
    }
    __syncthreads();
    // item tid: outputs FIR_R * tid + j; staged frame FIR_R * tid + c lies at lds[tid + fir_phys(c)]
    // (c uniform), and output j's own frame has c = cen + j
    const uint32_t *const mine = lds + tid;
    const int cen = H + FIR_GUARD;
    double acc[CH][FIR_R];
    int ringR[CH][4], ringL[CH][4];  // frame cen + e in ringR[e & 3]; frame cen - e in ringL[e & 3]
    {
        const double t0 = taps[0];
#pragma unroll
        for (int j = 0; j < FIR_R; ++j) {
            int s[CH];
            fir_unpack<CH>(mine[fir_phys(cen + j)], s);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                acc[c][j] = t0 * (double)s[c];
                ringR[c][j] = s[c];            // e = j (slot 0 is overwritten by the first step)
                ringL[c][(4 - j) & 3] = s[c];  // e = -j
            }
        }
    }
    // pairs d = d0 + u, d0 = 1 mod 4: at d the right window holds e in [d, d + 3] (new: d + 3),
    // the left window e in [d - 3, d] (new: d); output j meets frames cen + j + d and cen + j - d
    for (int d0 = 1; d0 <= a.Hp; d0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = d0 + u;
            const double t = taps[d];
            int sr[CH], sl[CH];
            fir_unpack<CH>(mine[fir_phys(cen + d + 3)], sr);
            fir_unpack<CH>(mine[fir_phys(cen - d)], sl);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                ringR[c][(u + 4) & 3] = sr[c];  // (d + 3) & 3
                ringL[c][(u + 1) & 3] = sl[c];  // d & 3
            }
#pragma unroll
            for (int j = 0; j < FIR_R; ++j)
#pragma unroll
                for (int c = 0; c < CH; ++c)
                    acc[c][j] = fma(t, (double)(ringR[c][(u + 1 + j) & 3] + ringL[c][(u + 5 - j) & 3]), acc[c][j]);
        }
    }
    unsigned n_clip[CH];
    int pk[CH], un[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        n_clip[c] = 0;
        pk[c] = un[c] = 0;
    }
#pragma unroll
    for (int j = 0; j < FIR_R; ++j) {
        const int o = FIR_R * tid + j;
        if (o >= span) continue;
        int y[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int v = (int)(((long long)acc[c][j] + (1ll << 21)) >> 22);  // arithmetic; |v| <= 2^17
            const int yc = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
            n_clip[c] += v != yc ? 1u : 0u;
            pk[c] = max(pk[c], yc < 0 ? -yc : yc);
            un[c] = max(un[c], v < 0 ? -v : v);
            y[c] = yc;
        }
        store_frame<CH, T>(out, n0 + o, y);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const unsigned nc = wave_sum_u32(n_clip[c]);
        const int p = wave_max_i32(pk[c]);
        const int q = wave_max_i32(un[c]);
        if (lane == 0) {
            red_clip[c][wave] = nc;
            red_pk[c][wave] = p;
            red_un[c][wave] = q;
        }
    }
    __syncthreads();
    if (tid < CH) {
        unsigned nc = 0;
        int p = 0, q = 0;
        for (int w = 0; w < FIR_THREADS / 64; ++w) {
            nc += red_clip[tid][w];
            p = max(p, red_pk[tid][w]);
            q = max(q, red_un[tid][w]);
        }
        if (nc) atomicAdd(&a.st->clipped[tid], (unsigned long long)nc);
        if (p) atomicMax(&a.st->peak[tid], p);
        if (q) atomicMax(&a.st->peak_unclipped[tid], q);
    }
}

template <int CH, typename T>
__global__ void __launch_bounds__(FIR_THREADS) fir_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                          const double *__restrict__ taps, FirArgs a) {
    fir_span<CH, T>(in, out, taps, a, (int64_t)blockIdx.x * FIR_SPAN);
}

}  // namespace mm

// ======================================================= host entry points
namespace {

// why K is not a table's length, or null
const char *fir_bad_length(int K) {
    return K < 3 || K > FIR_MAX_K || !(K & 1) ? "K must be odd and in [3, 8191]" : nullptr;
}

// why the table is refused, or null (K additions)
const char *fir_bad_table(const mm_fir *f) {
    if (!f || !f->taps) return "null filter or taps";
    if (const char *why = fir_bad_length(f->K)) return why;
    int64_t sum = 0;
    for (int k = 0; k < f->K; ++k) {
        const int64_t v = f->taps[k];
        if (f->taps[f->K - 1 - k] != f->taps[k]) return "the taps are not symmetric";
        sum += v < 0 ? -v : v;
    }
    return sum >= FIR_SUM_LIMIT ? "the taps have sum |c| >= 2^24" : nullptr;
}

const char *fir_bad_signal(int64_t frames, int channels) { return pcm_refusal(channels, frames, (int64_t)1 << 31); }

void fir_clear(mm_fir_result *o, int64_t frames, int channels, const mm_fir *f) {
    memset(o, 0, sizeof *o);
    o->frames = frames;
    o->channels = channels;
    o->rate = f->rate;
    o->K = f->K;
}

}  // namespace

// The device copy of the taps' upper half as doubles, padded with zero taps to a multiple of 4
// pairs (T[d] = c[H + d]), cached per context by the caller's content key (0: no key, checked
// and uploaded every call).
static int fir_taps_device(mm_ctx *c, const mm_fir *f, const double **out) {
    const int H = (f->K - 1) / 2, Hp = (H + 3) & ~3;
    double *D;
    if (f->taps_key && f->taps_key == c->fir_key && f->K == c->fir_K) {
        RET(get_buf(c, "fir_taps", (size_t)Hp + 1, &D));
        *out = D;
        return MM_OK;
    }
    if (const char *why = fir_bad_table(f)) return set_err(c, MM_ERR_ARG, "fir: %s", why);
    c->fir_key = 0;
    RET(get_buf(c, "fir_taps", (size_t)Hp + 1, &D));
    std::vector<double> t((size_t)Hp + 1, 0.0);
    for (int d = 0; d <= H; ++d) t[d] = (double)f->taps[H + d];
    HIPCHK(c, hipMemcpyAsync(D, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (t leaves scope)
    c->fir_key = f->taps_key;
    c->fir_K = f->K;
    *out = D;
    return MM_OK;
}

// Filter a device-resident signal into d_out (out of place; synchronous on return).
static int fir_device(mm_ctx *c, const void *d_in, int kind, int64_t frames, int channels, const mm_fir *f, void *d_out,
                      mm_fir_result *out) {
    if (!c || !out || !f || (frames > 0 && (!d_in || !d_out))) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = fir_bad_length(f->K)) return set_err(c, MM_ERR_ARG, "fir: %s", why);
    if (const char *why = fir_bad_signal(frames, channels)) return set_err(c, MM_ERR_ARG, "%s", why);
    {  // a workgroup reads its neighbours' frames while they write theirs: the two ranges must not meet
        const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out, bytes = pcm_bytes(kind, frames, channels);
        if (a < b + bytes && b < a + bytes) return set_err(c, MM_ERR_ARG, "fir: the filter runs out of place (d_in and d_out overlap)");
    }
    const double *taps;
    RET(fir_taps_device(c, f, &taps));
    fir_clear(out, frames, channels, f);
    c->fir_valid = false;
    if (frames > 0) {
        FirArgs a{};
        RET(get_buf(c, "fir_res", 1, &a.st));
        HIPCHK(c, hipMemsetAsync(a.st, 0, sizeof(FirDev), c->stream));
        a.N = frames;
        a.H = (f->K - 1) / 2;
        a.Hp = (a.H + 3) & ~3;
        const dim3 grid(blocks_for(frames, FIR_SPAN)), block(FIR_THREADS);
        RET(dispatch_pcm(kind, channels, [&](auto ch, auto t) {
            using T = decltype(t);
            return launch(c, "fir", fir_kernel<ch, T>, grid, block, 0, static_cast<const T *>(d_in), static_cast<T *>(d_out), taps,
                          a);
        }));
        FirDev h;
        HIPCHK(c, hipMemcpyAsync(&h, a.st, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int ch = 0; ch < channels; ++ch) {
            out->clipped[ch] = (int64_t)h.clipped[ch];
            out->peak[ch] = h.peak[ch];
            out->peak_unclipped[ch] = h.peak_unclipped[ch];
        }
        resolve_events(c);
    }
    c->fir = *out;
    c->fir_valid = true;
    return MM_OK;
}

extern "C" {

int mm_fir_span(void) { return FIR_SPAN; }

int mm_fir_device(mm_ctx *c, const void *d_in, int kind, int64_t frames, int channels, const mm_fir *f, void *d_out,
                  mm_fir_result *out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return fir_device(c, d_in, kind, frames, channels, f, d_out, out);
}

int mm_fir_pcm(mm_ctx *c, const void *in, int kind, int64_t frames, int channels, const mm_fir *f, void *out_pcm,
               mm_fir_result *out) {
    if (!c) return MM_ERR_ARG;
    if (!out || !f || (frames > 0 && (!in || !out_pcm)) || !pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (const char *why = fir_bad_length(f->K)) return set_err(c, MM_ERR_ARG, "fir: %s", why);
    if (const char *why = fir_bad_signal(frames, channels)) return set_err(c, MM_ERR_ARG, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = pcm_bytes(kind, frames, channels);
    char *din, *dout;
    RET(pcm_upload(c, "fir_in", in, bytes, &din));
    RET(get_buf(c, "fir_out", std::max<size_t>(bytes, 1), &dout));
    RET(fir_device(c, din, kind, frames, channels, f, dout, out));
    return pcm_download(c, out_pcm, dout, bytes);
}

// The definition restated in plain C++ on the host (no context, no GPU): what the kernel must
// reproduce, samples and statistics.  Nothing outside in[0, frames * channels) is read, nothing
// outside out_pcm[0, frames * channels) written.
int mm_fir_host(const int16_t *in, int64_t frames, int channels, const mm_fir *f, int16_t *out_pcm, mm_fir_result *out) {
    if (!out || !f || fir_bad_table(f) || fir_bad_signal(frames, channels)) return MM_ERR_ARG;
    if (frames > 0 && (!in || !out_pcm)) return MM_ERR_ARG;
    fir_clear(out, frames, channels, f);
    const int64_t K = f->K, H = (K - 1) / 2;
    for (int64_t n = 0; n < frames; ++n) {
        // the taps whose sample n + H - k lies in [0, frames)
        const int64_t k_lo = std::max<int64_t>(0, n + H - (frames - 1)), k_hi = std::min<int64_t>(K - 1, n + H);
        for (int ch = 0; ch < channels; ++ch) {
            int64_t acc = 0;
            for (int64_t k = k_lo; k <= k_hi; ++k) acc += (int64_t)f->taps[k] * in[(n + H - k) * channels + ch];
            const int64_t v = acc + ((int64_t)1 << 21);
            const int64_t y = v >= 0 ? v >> 22 : -((-v + (((int64_t)1 << 22) - 1)) >> 22);  // floor
            const int64_t d = std::min<int64_t>(32767, std::max<int64_t>(-32768, y));
            if (d != y) ++out->clipped[ch];
            out->peak[ch] = std::max(out->peak[ch], (int32_t)(d < 0 ? -d : d));
            out->peak_unclipped[ch] = std::max(out->peak_unclipped[ch], (int32_t)(y < 0 ? -y : y));
            out_pcm[n * channels + ch] = (int16_t)d;
        }
    }
    return MM_OK;
}

int mm_last_fir(mm_ctx *c, mm_fir_result *out) {
    if (!c || !out) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!c->fir_valid) return set_err(c, MM_ERR_STATE, "the context has not run a filter");
    *out = c->fir;
    return MM_OK;
}

}  // extern "C"
