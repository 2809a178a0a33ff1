// ceiling.hip — the true-peak ceiling: an exact look-ahead limiter on the delivered
// int16 output, and one static trim when the limiter leaves a residue.  No reference
// counterpart.  Everything is defined in integers (include/mastering.h, mm_ceiling):
//   P[m]  = max over channels and phases of |Y_c[m][p]|          (the meter's Y)
//   r[m]  = 2^16 if P[m] <= C_t, else floor(C_t * 2^16 / P[m]),  C_t = C - 8286
//   R[n]  = min r[n .. n+11]                (the m that sample n feeds), 2^16 outside
//   h[k]  = min R[k-W .. k+W],   g[n] = floor(sum h[n-W .. n+W] / (2W+1))   (<= R[n])
//   s'[n] = s[n] if g[n] == 2^16, else (s[n] * g[n] + 2^15) >> 16
// and, if the true peak TP1 of s' is still above C, every sample once more by
// g_t = floor(C_t * 2^16 / TP1): requantising moves |Y| by at most 8285.5 < 8286, so
// the trimmed peak is at most C_t + 8285.5 < C.
//
// Three span bodies.  ceil_need_span runs the meter's own oversampler (meter.hip: tp_stage,
// tp_window, tp_frame) and writes r - 1 as uint16 to a plane; ceil_apply_span
// stages the plane with its halo in LDS, forms both window minima by log-step doubling
// and the box sums from one LDS scan, and rewrites the samples in place; ceil_scale is
// pointwise.  The true peak after the limiter is the need body with its store switched off.
// All results are integers combined with min / max / add: nothing depends on the launch
// geometry.
//
// One launch structure, over n >= 1 tracks each with its own parameters (tracks.h: a track
// owns a run of workgroups, a workgroup finds its track by a search over at most 257 prefix
// sums, which are uniform reads, and at n = 1 reads none), so a pass costs the same launches
// and synchronisations for 1 track as for 256.  A single signal is the case n = 1.
//   ceil_tracks_need   ceil_need_span over all METER_SPAN spans; track t's r - 1 plane at a
//                      multiple of METER_SPAN of one plane buffer, TP0 into its CeilDev
//   ceil_tracks_apply  ceil_apply_span over all CEIL_SPAN spans; the early exit, the plane mask
//                      and the R mask are the track's own
//   ceil_tracks_peak   the linked true peak of every track (a track whose TP0 <= C was not
//                      touched: skipped)
//   ceil_tracks_trim   pointwise, the tracks with a residue only, each by its own g_t
// A workgroup of a track that takes no part exits on one uniform read of its parameters.
//
// Included at the end of mastering.hip after pcm16.h (frames, wave reductions, refusals,
// dispatch_pcm, the batch plumbing), tracks.h and meter.hip (the oversampler, tp_host).

namespace mm {

constexpr int CEIL_ONE = 1 << 16;
constexpr int CEIL_GUARD = 8286;     // > 16571 / 2: what requantising can add to |Y|
constexpr int CEIL_MAX_W = 1024;     // mm_ceiling_max_window
constexpr int CEIL_THREADS = 256;
constexpr int CEIL_SPAN = 4096;      // frames per ceil_apply workgroup (mm_ceiling_span)
constexpr int CEIL_RLEN = CEIL_SPAN + 4 * CEIL_MAX_W + 11;  // staged r of a span at the widest window
constexpr int CEIL_BUF = (CEIL_RLEN + 5 + 7) / 8 * 8;     // + what a packed pass may touch past a line's end
constexpr int CEIL_HLEN = CEIL_SPAN + 2 * CEIL_MAX_W;       // h of a span at the widest window

// device result block of one ceiling (zeroed on the stream before ceil_need)
struct CeilDev {
    unsigned tp0;                // max P (TP0)
    unsigned max_red;            // max (2^16 - g): the minimum gain, as a maximum of zero-initialised words
    unsigned long long limited;  // frames with g < 2^16
};

// floor(Ct * 2^16 / P) for 0 < Ct < P < 2^30.  The numerator is below 2^44 and exact in
// f64; a non-integer quotient lies at least 1/P > 2^-30 from an integer while the
// correctly rounded f64 quotient is within 2^-37 of it, so truncation already gives the
// floor.  The integer remainder check makes that independent of how the division rounds.
__device__ __forceinline__ int ceil_ratio(int Ct, int P) {
    const long long num = (long long)Ct << 16;
    int q = (int)((double)num / (double)P);
    const long long rem = num - (long long)q * P;
    q += rem < 0 ? -1 : (rem >= P ? 1 : 0);
    return q;
}

// One workgroup on the span of METER_SPAN frames m at `base`; a thread owns METER_FPT
// consecutive m (the meter's window layout).  With STORE it writes r[m] - 1 for all its m as
// one 16-byte store at span[thread * METER_FPT] (`span`: the plane at `base`, a 16-byte
// boundary): the plane holds whole spans, so every entry up to the plane's end is written
// (2^16 - 1 beyond N + 11, where P = 0).  The span's max P is folded into *tp with one atomic
// per workgroup.  Without STORE it is the linked true peak alone (ceil_tracks_peak).
template <int CH, typename T, bool STORE>
__device__ __forceinline__ void ceil_need_span(const T *__restrict__ in, int64_t N, int64_t base, int Ct,
                                               uint16_t *__restrict__ span, unsigned *tp) {
    __shared__ __attribute__((aligned(16))) int16_t line[CH][METER_LINE];
    __shared__ int red[METER_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    tp_stage<CH, T>(line, in, N, base);
    int pm[METER_FPT];
#pragma unroll
    for (int j = 0; j < METER_FPT; ++j) pm[j] = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        uint32_t P[19];
        tp_window(&line[c][threadIdx.x * METER_FPT], P);
#pragma unroll
        for (int j = 0; j < METER_FPT; ++j) {
#pragma unroll
            for (int p = 0; p < 4; ++p) pm[j] = max(pm[j], tp_frame(P, j, p));
        }
    }
    int best = 0;
    uint32_t r1[METER_FPT];  // r - 1
#pragma unroll
    for (int j = 0; j < METER_FPT; ++j) {
        best = max(best, pm[j]);
        if (STORE) r1[j] = pm[j] > Ct ? (uint32_t)(ceil_ratio(Ct, pm[j]) - 1) : (uint32_t)(CEIL_ONE - 1);
    }
    if (STORE) {
        uint4 o;
        o.x = r1[0] | (r1[1] << 16);
        o.y = r1[2] | (r1[3] << 16);
        o.z = r1[4] | (r1[5] << 16);
        o.w = r1[6] | (r1[7] << 16);
        static_assert(METER_FPT == 8, "one 16-byte store of eight uint16 per thread");
        *reinterpret_cast<uint4 *>(span + (int64_t)threadIdx.x * METER_FPT) = o;
    }
    best = wave_max_i32(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < METER_THREADS / 64; ++w) best = max(best, red[w]);
        if (best) atomicMax(tp, (unsigned)best);
    }
}

typedef unsigned short ceil_u16x2 __attribute__((ext_vector_type(2)));

// both uint16 halves of a dword at once (v_pk_min_u16)
__device__ __forceinline__ uint32_t ceil_min2(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(ceil_u16x2, a),
                                                                  __builtin_bit_cast(ceil_u16x2, b)));
}

// nxt[e] = min(cur[e], cur[e + off]) for e < n, two entries per dword: the partner pair is
// a dword for even off and a funnel shift of two neighbours for odd off.  The last dword
// may cover one entry past n, and the odd form reads one dword further: both stay inside
// the buffers (CEIL_BUF leaves 5 entries beyond the longest line), and what is computed
// past n is never read by a valid entry of a later pass.
__device__ __forceinline__ void ceil_min_pass(const uint16_t *cur, uint16_t *nxt, int n, int off) {
    const uint32_t *c = reinterpret_cast<const uint32_t *>(cur);
    uint32_t *o = reinterpret_cast<uint32_t *>(nxt);
    const int nd = (n + 1) >> 1, d = off >> 1;
    if (off & 1)
        for (int i = threadIdx.x; i < nd; i += CEIL_THREADS) o[i] = ceil_min2(c[i], (c[i + d] >> 16) | (c[i + d + 1] << 16));
    else
        for (int i = threadIdx.x; i < nd; i += CEIL_THREADS) o[i] = ceil_min2(c[i], c[i + d]);
    __syncthreads();
}

// out[i] = min cur[i .. i+K) for i < n_out, cur valid on [0, n_out + K - 1): minima over
// 2, 4, ... p <= K entries by doubling between the two buffers, then two overlapping
// windows of p.  Returns the buffer holding the result; every pass ends in a barrier.
__device__ __forceinline__ uint16_t *ceil_window_min(uint16_t *cur, uint16_t *nxt, int n_out, int K) {
    int valid = n_out + K - 1, step = 1;
    while (2 * step <= K) {
        valid -= step;
        ceil_min_pass(cur, nxt, valid, step);
        uint16_t *t = cur;
        cur = nxt;
        nxt = t;
        step *= 2;
    }
    ceil_min_pass(cur, nxt, n_out, K - step);
    return nxt;
}

// frame n of pcm by g, in place
template <int CH, typename T>
__device__ __forceinline__ void ceil_scale(T *pcm, int64_t n, int g) {
    int s[CH];
    load_frame<CH, T>(pcm, n, s);
#pragma unroll
    for (int c = 0; c < CH; ++c) s[c] = (s[c] * g + (1 << 15)) >> 16;  // |s * g| < 2^31: exact, arithmetic shift
    store_frame<CH, T>(pcm, n, s);
}

// One workgroup on the CEIL_SPAN frames n in [base, base + CEIL_SPAN) of one signal.  It needs h on
// [base - W, base + span + W), so R on [base - 2W, base + span + 2W) and r on 11 more:
// those r - 1 are staged in LDS as uint16 (2^16 - 1 outside the plane).  The signal's
// workgroups exit at once when TP0 <= C, and a workgroup whose staged r are all 2^16 writes
// nothing.  The box sums come from one exclusive scan of h in uint32
// ((span + 2W) * 2^16 < 2^32), divided by 2W + 1 with a multiply-high reciprocal
// rcp = floor(2^32 / (2W + 1)) and one correction.
template <int CH, typename T>
__device__ __forceinline__ void ceil_apply_span(T *__restrict__ pcm, int64_t N, int64_t plane_len,
                                                const uint16_t *__restrict__ plane, int C, int W, unsigned rcp, CeilDev *st,
                                                int64_t base) {
    __shared__ __attribute__((aligned(16))) uint16_t buf_a[CEIL_BUF], buf_b[CEIL_BUF];
    __shared__ uint32_t ps[CEIL_HLEN + 1];
    __shared__ uint32_t wsum[CEIL_THREADS / 64], wred[CEIL_THREADS / 64];
    if (st->tp0 <= (unsigned)C) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = 2 * W + 1;
    const int n_r = CEIL_SPAN + 4 * W + 11, n_R = CEIL_SPAN + 4 * W, n_h = CEIL_SPAN + 2 * W;
    const int64_t m_first = base - 2 * W;  // m (and j) of LDS index 0
    int limited = 0;
    for (int i = tid; i < n_r; i += CEIL_THREADS) {
        const int64_t m = m_first + i;
        const uint16_t v = (m >= 0 && m < plane_len) ? plane[m] : (uint16_t)(CEIL_ONE - 1);
        buf_a[i] = v;
        limited |= v != (uint16_t)(CEIL_ONE - 1);
    }
    if (!__syncthreads_or(limited)) return;
    // R - 1, masked to 2^16 - 1 outside [0, N)
    uint16_t *Rb = ceil_window_min(buf_a, buf_b, n_R, 12);
    for (int i = tid; i < n_R; i += CEIL_THREADS) {
        const int64_t j = m_first + i;
        if (j < 0 || j >= N) Rb[i] = (uint16_t)(CEIL_ONE - 1);
    }
    __syncthreads();
    // h - 1: index u is k = base - W + u
    const uint16_t *hb = ceil_window_min(Rb, Rb == buf_a ? buf_b : buf_a, n_h, D);
    // ps[u] = sum of h[v] for v < u
    const int per = (n_h + CEIL_THREADS - 1) / CEIL_THREADS;
    const int u0 = min(tid * per, n_h), u1 = min(u0 + per, n_h);
    uint32_t tot = 0;
    for (int u = u0; u < u1; ++u) tot += (uint32_t)hb[u] + 1u;
    uint32_t inc = tot;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t run = inc - tot;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    if (tid == 0) ps[0] = 0;
    for (int u = u0; u < u1; ++u) {
        run += (uint32_t)hb[u] + 1u;
        ps[u + 1] = run;
    }
    __syncthreads();
    unsigned count = 0;
    int red = 0;
    for (int t = tid; t < CEIL_SPAN; t += CEIL_THREADS) {
        const int64_t n = base + t;
        if (n >= N) break;
        const uint32_t sum = ps[t + D] - ps[t];  // h[n - W .. n + W]
        uint32_t g = __umulhi(sum, rcp);         // floor(sum / D) or one less
        g += sum - g * (uint32_t)D >= (uint32_t)D ? 1u : 0u;
        if (g == (uint32_t)CEIL_ONE) continue;
        ++count;
        red = max(red, CEIL_ONE - (int)g);
        ceil_scale<CH, T>(pcm, n, (int)g);
    }
    count = wave_sum_u32(count);
    red = wave_max_i32(red);
    if (lane == 0) {
        wsum[wave] = count;
        wred[wave] = (uint32_t)red;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CEIL_THREADS / 64; ++w) {
            count += wsum[w];
            red = max(red, (int)wred[w]);
        }
        if (count) atomicAdd(&st->limited, (unsigned long long)count);
        if (red) atomicMax(&st->max_red, (unsigned)red);
    }
}

static_assert(TRACKS_METER_SPAN == METER_SPAN && TRACKS_CEIL_SPAN == CEIL_SPAN && TRACKS_MAX == MM_ALBUM_TRACKS,
              "tracks.h restates the spans");

struct TrackDev {  // one a track, uploaded once a call
    void *pcm;
    int64_t frames;
};

struct TrackPar {  // one a track, uploaded once a launch sequence
    int C, Ct;     // the ceiling and C - CEIL_GUARD
    int g;         // the trim
    int active;    // 0: the track's workgroups exit at once
};

struct TracksArgs {
    const TrackDev *tr;
    const uint32_t *first_need, *first_apply;  // [n + 1] prefix sums of the two grids
    const TrackPar *par;
    uint16_t *plane;
    CeilDev *st;     // [n]
    unsigned *peak;  // [n] the linked true peak after the limiter / the trim
    int n, W;
    unsigned rcp;
};

template <int CH, typename T>
__global__ void __launch_bounds__(METER_THREADS) ceil_tracks_need_kernel(TracksArgs a) {
    const int t = tracks_find(a.first_need, a.n, blockIdx.x);
    const TrackPar p = a.par[t];
    if (!p.active) return;
    const TrackDev tr = a.tr[t];
    const int64_t base = (int64_t)(blockIdx.x - a.first_need[t]) * METER_SPAN;
    ceil_need_span<CH, T, true>(static_cast<const T *>(tr.pcm), tr.frames, base, p.Ct,
                                a.plane + tracks_plane_off(a.first_need, t) + base, &a.st[t].tp0);
}

template <int CH, typename T>
__global__ void __launch_bounds__(METER_THREADS) ceil_tracks_peak_kernel(TracksArgs a) {
    const int t = tracks_find(a.first_need, a.n, blockIdx.x);
    const TrackPar p = a.par[t];
    if (!p.active || a.st[t].tp0 <= (unsigned)p.C) return;
    const TrackDev tr = a.tr[t];
    const int64_t base = (int64_t)(blockIdx.x - a.first_need[t]) * METER_SPAN;
    ceil_need_span<CH, T, false>(static_cast<const T *>(tr.pcm), tr.frames, base, 0, nullptr, &a.peak[t]);
}

template <int CH, typename T>
__global__ void __launch_bounds__(CEIL_THREADS) ceil_tracks_apply_kernel(TracksArgs a) {
    const int t = tracks_find(a.first_apply, a.n, blockIdx.x);
    const TrackPar p = a.par[t];
    if (!p.active) return;
    const TrackDev tr = a.tr[t];
    const int64_t base = (int64_t)(blockIdx.x - a.first_apply[t]) * CEIL_SPAN;
    ceil_apply_span<CH, T>(static_cast<T *>(tr.pcm), tr.frames, tracks_plane_len(tr.frames),
                           a.plane + tracks_plane_off(a.first_need, t), p.C, a.W, a.rcp, &a.st[t], base);
}

// The static trim: the samples of the span's frames as one mono line
template <typename T>
__global__ void __launch_bounds__(CEIL_THREADS) ceil_tracks_trim_kernel(TracksArgs a, int channels) {
    const int t = tracks_find(a.first_apply, a.n, blockIdx.x);
    const TrackPar p = a.par[t];
    if (!p.active) return;
    const TrackDev tr = a.tr[t];
    const int64_t base = (int64_t)(blockIdx.x - a.first_apply[t]) * CEIL_SPAN;
    const int64_t s1 = (tr.frames < base + CEIL_SPAN ? tr.frames : base + CEIL_SPAN) * channels;
    for (int64_t i = base * channels + threadIdx.x; i < s1; i += CEIL_THREADS) ceil_scale<1, T>(static_cast<T *>(tr.pcm), i, p.g);
}

}  // namespace mm

// ======================================================= host entry points
namespace {

void ceiling_clear(mm_ceiling *o, int64_t frames, int channels, int32_t C, int32_t W) {
    memset(o, 0, sizeof *o);
    o->frames = frames;
    o->channels = channels;
    o->ceiling_q28 = C;
    o->window = W;
    o->min_gain_q16 = CEIL_ONE;
    o->trim_q16 = CEIL_ONE;
}

// why (C, W) on a signal of (frames, channels) is not a ceiling job, or null
const char *ceiling_bad_args(int64_t frames, int channels, int32_t C, int32_t W) {
    if (const char *why = pcm_refusal(channels, frames, METER_MAX_FRAMES)) return why;
    if (C < (1 << 24) || C > (1 << 28)) return "ceiling_q28 out of range [2^24, 2^28]";
    if (W < 1 || W > CEIL_MAX_W) return "ceiling window out of range [1, 1024]";
    return nullptr;
}

// what the limiter's launches found: TP0 and the statistics of `s`, and the linked true peak
// after the limiter, which is the delivered one until a trim runs
void ceiling_results(mm_ceiling *o, const CeilDev &s, int32_t tp_limited) {
    o->tp_in_q28 = (int32_t)s.tp0;
    o->tp_limited_q28 = o->tp_out_q28 = tp_limited;
    o->min_gain_q16 = CEIL_ONE - (int32_t)s.max_red;
    o->limited_frames = (int64_t)s.limited;
}

// the static trim of a residue tp_limited > C: provably under C (the file's head)
int32_t ceiling_trim_gain(int32_t C, int32_t tp_limited) { return (int32_t)(((int64_t)(C - CEIL_GUARD) << 16) / tp_limited); }

// The tracks of one call and the two grids over them: host tables, laid out once and uploaded
// with the parameters of every ceiling that runs on them.
struct CeilLayout {
    int n = 0, kind = 0, channels = 0;
    std::vector<TrackDev> tr;
    std::vector<uint32_t> first_need, first_apply;
};

void ceiling_layout(void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, CeilLayout &L) {
    L.n = n;
    L.kind = kind;
    L.channels = channels;
    L.tr.resize((size_t)n);
    std::vector<int64_t> need((size_t)n), apply((size_t)n);
    for (int t = 0; t < n; ++t) {
        L.tr[(size_t)t] = TrackDev{d_pcm[t], frames[t]};
        need[(size_t)t] = tracks_need_spans(frames[t]);
        apply[(size_t)t] = tracks_apply_spans(frames[t]);
    }
    L.first_need.resize((size_t)n + 1);
    L.first_apply.resize((size_t)n + 1);
    tracks_prefix(need.data(), n, L.first_need.data());
    tracks_prefix(apply.data(), n, L.first_apply.data());
}

// The ceiling over the tracks of a layout, in place: every track t with Cs[t] != 0 held under
// Cs[t] and out[t] filled; the other tracks and their out[t] are not touched.  One upload (the
// tracks, their parameters, the grids) and one memset (the result blocks, the peaks), then
// need, apply and the peak behind one synchronisation; the trims and their peak behind one
// more, when a track is left with a residue.  Nothing to do (no track with a ceiling and
// frames): nothing is queued.  Arguments already checked.  Synchronous on return.
int tracks_ceiling(mm_ctx *c, const CeilLayout &L, const int32_t *Cs, int32_t W, mm_ceiling *out) {
    const int n = L.n;
    const size_t N = (size_t)n, fb = (N + 1) * sizeof(uint32_t);
    const size_t o_par = N * sizeof(TrackDev), o_need = o_par + N * sizeof(TrackPar), o_apply = o_need + fb;
    std::vector<char> tab(o_apply + fb);  // (lives until the synchronisation behind its upload)
    TrackPar *par = reinterpret_cast<TrackPar *>(tab.data() + o_par);
    bool any = false;
    for (int t = 0; t < n; ++t) {
        par[t] = TrackPar{};
        if (!Cs[t]) continue;
        ceiling_clear(&out[t], L.tr[(size_t)t].frames, L.channels, Cs[t], W);
        if (L.tr[(size_t)t].frames == 0) continue;
        par[t] = TrackPar{Cs[t], Cs[t] - CEIL_GUARD, 0, 1};
        any = true;
    }
    if (!any) return MM_OK;
    memcpy(tab.data(), L.tr.data(), o_par);
    memcpy(tab.data() + o_need, L.first_need.data(), fb);
    memcpy(tab.data() + o_apply, L.first_apply.data(), fb);
    char *d_tab, *d_res;
    const size_t o_peak = N * sizeof(CeilDev), res_bytes = o_peak + N * sizeof(unsigned);
    TracksArgs a{};
    RET(get_buf(c, "ceil_tab", tab.size(), &d_tab));
    RET(get_buf(c, "ceil_res", res_bytes, &d_res));
    RET(get_buf(c, "ceil_r", (size_t)tracks_plane_total(L.first_need.data(), n), &a.plane));
    HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_res, 0, res_bytes, c->stream));
    a.tr = reinterpret_cast<const TrackDev *>(d_tab);
    a.par = reinterpret_cast<const TrackPar *>(d_tab + o_par);
    a.first_need = reinterpret_cast<const uint32_t *>(d_tab + o_need);
    a.first_apply = reinterpret_cast<const uint32_t *>(d_tab + o_apply);
    a.st = reinterpret_cast<CeilDev *>(d_res);
    a.peak = reinterpret_cast<unsigned *>(d_res + o_peak);
    a.n = n;
    a.W = W;
    a.rcp = (unsigned)(((uint64_t)1 << 32) / (uint64_t)(2 * W + 1));
    const dim3 gn(L.first_need[N]), bn(METER_THREADS), ga(L.first_apply[N]), ba(CEIL_THREADS);
    auto peak = [&]() {
        return dispatch_pcm(L.kind, L.channels, [&](auto ch, auto t) {
            using T = decltype(t);
            return launch(c, "ceil_tracks_peak", ceil_tracks_peak_kernel<ch, T>, gn, bn, 0, a);
        });
    };
    RET(dispatch_pcm(L.kind, L.channels, [&](auto ch, auto t) {
        using T = decltype(t);
        RET(launch(c, "ceil_tracks_need", ceil_tracks_need_kernel<ch, T>, gn, bn, 0, a));
        return launch(c, "ceil_tracks_apply", ceil_tracks_apply_kernel<ch, T>, ga, ba, 0, a);
    }));
    RET(peak());
    std::vector<char> hr(res_bytes);
    const CeilDev *hs = reinterpret_cast<const CeilDev *>(hr.data());
    const unsigned *hp = reinterpret_cast<const unsigned *>(hr.data() + o_peak);
    HIPCHK(c, hipMemcpyAsync(hr.data(), d_res, res_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bool trim = false;
    for (int t = 0; t < n; ++t) {  // (everything queued has run: the parameters become the trim's)
        if (!par[t].active) continue;
        const int32_t C = Cs[t];
        mm_ceiling *o = &out[t];
        const int32_t tp0 = (int32_t)hs[t].tp0;
        ceiling_results(o, hs[t], tp0 <= C ? tp0 : (int32_t)hp[t]);  // (untouched: ceil_tracks_peak skipped it)
        par[t].active = o->tp_limited_q28 > C;
        if (par[t].active) {  // the residue: one static trim
            par[t].g = o->trim_q16 = ceiling_trim_gain(C, o->tp_limited_q28);
            trim = true;
        }
    }
    if (trim) {
        HIPCHK(c, hipMemcpyAsync(d_tab + o_par, par, N * sizeof(TrackPar), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(a.peak, 0, N * sizeof(unsigned), c->stream));
        RET(dispatch_pcm(L.kind, 1, [&](auto, auto t) {
            using T = decltype(t);
            return launch(c, "ceil_tracks_trim", ceil_tracks_trim_kernel<T>, ga, ba, 0, a, L.channels);
        }));
        RET(peak());
        HIPCHK(c, hipMemcpyAsync(hr.data() + o_peak, a.peak, N * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int t = 0; t < n; ++t)
            if (par[t].active) out[t].tp_out_q28 = (int32_t)hp[t];
    }
    resolve_events(c);
    return MM_OK;
}

// Refuses what is not a batch to hold under ceilings, before anything is queued.
int batch_ceiling_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, const int32_t *C,
                        int32_t W) {
    return batch_check(c, pcm, kind, frames, n, channels, C != nullptr,
                       [&](int t) { return ceiling_bad_args(frames[t], channels, C[t], W); });
}

int batch_ceiling_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                         const int32_t *C, int32_t W, mm_ceiling *out) {
    CeilLayout L;
    ceiling_layout(d_pcm, kind, frames, n, channels, L);
    return tracks_ceiling(c, L, C, W, out);
}

}  // namespace

// The ceiling on a device-resident signal, in place (synchronous on return): a batch of one.
static int ceiling_device(mm_ctx *c, void *d_pcm, int kind, int64_t frames, int channels, int32_t C, int32_t W,
                          mm_ceiling *out) {
    if (!c || !out || (frames > 0 && !d_pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = ceiling_bad_args(frames, channels, C, W)) return set_err(c, MM_ERR_ARG, "%s", why);
    return batch_ceiling_device(c, &d_pcm, kind, &frames, 1, channels, &C, W, out);
}

extern "C" {

int mm_ceiling_span(void) { return CEIL_SPAN; }

int mm_ceiling_max_window(void) { return CEIL_MAX_W; }

int mm_ceiling_device(mm_ctx *c, void *d_pcm, int kind, int64_t frames, int channels, int32_t ceiling_q28,
                      int32_t window, mm_ceiling *out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return ceiling_device(c, d_pcm, kind, frames, channels, ceiling_q28, window, out);
}

int mm_ceiling_pcm(mm_ctx *c, void *pcm, int kind, int64_t frames, int channels, int32_t ceiling_q28, int32_t window,
                   mm_ceiling *out) {
    if (!c) return MM_ERR_ARG;
    if (!out || (frames > 0 && !pcm) || !pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (const char *why = ceiling_bad_args(frames, channels, ceiling_q28, window)) return set_err(c, MM_ERR_ARG, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = pcm_bytes(kind, frames, channels);
    char *dio;
    RET(pcm_upload(c, "ceil_io", pcm, bytes, &dio));
    RET(ceiling_device(c, dio, kind, frames, channels, ceiling_q28, window, out));
    if (out->tp_in_q28 <= ceiling_q28) return MM_OK;  // (an untouched signal is not copied back)
    return pcm_download(c, pcm, dio, bytes);
}

int mm_batch_ceiling_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                            const int32_t *ceiling_q28, int32_t window, mm_ceiling *out) {
    if (!c) return MM_ERR_ARG;
    if (!out) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(batch_ceiling_check(c, d_pcm, kind, frames, n, channels, ceiling_q28, window));
    HIPCHK(c, hipSetDevice(c->device));
    return batch_ceiling_device(c, d_pcm, kind, frames, n, channels, ceiling_q28, window, out);
}

int mm_batch_ceiling_pcm(mm_ctx *c, void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                         const int32_t *ceiling_q28, int32_t window, mm_ceiling *out) {
    if (!c) return MM_ERR_ARG;
    if (!out) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(batch_ceiling_check(c, pcm, kind, frames, n, channels, ceiling_q28, window));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "batch_io", pcm, kind, frames, n, channels, d));
    RET(batch_ceiling_device(c, d.data(), kind, frames, n, channels, ceiling_q28, window, out));
    std::vector<char> pick((size_t)n);  // (an untouched track is not copied back)
    for (int t = 0; t < n; ++t) pick[(size_t)t] = out[t].tp_in_q28 > ceiling_q28[t];
    return batch_download(c, pcm, d, kind, frames, n, channels, pick.data());
}

int mm_last_ceilings(mm_ctx *c, int cap, mm_ceiling *out) {
    if (!c || cap < 0 || (cap > 0 && !out)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->ceilings.empty()) return set_err(c, MM_ERR_STATE, "the last master call set no ceiling");
    const int n = (int)c->ceilings.size();
    for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->ceilings[(size_t)i];
    return n;
}

// The definition restated in plain C++ on the host (no context, no GPU), in place on
// interleaved int16: what the kernels must reproduce, samples and statistics.
int mm_ceiling_host(int16_t *pcm, int64_t frames, int channels, int32_t C, int32_t W, mm_ceiling *out) {
    if (!out || (frames > 0 && !pcm) || ceiling_bad_args(frames, channels, C, W)) return MM_ERR_ARG;
    ceiling_clear(out, frames, channels, C, W);
    if (frames == 0) return MM_OK;
    const int64_t N = frames, M = N + 11;
    const int64_t Ct = C - CEIL_GUARD;
    std::vector<int32_t> P((size_t)M);
    auto measure = [&]() {  // P[m], returns its maximum (the linked true peak)
        int32_t tp = 0;
        for (int64_t m = 0; m < M; ++m) {
            int32_t pm = 0;
            for (int c = 0; c < channels; ++c) pm = std::max(pm, tp_host(pcm, N, channels, c, m));
            P[(size_t)m] = pm;
            tp = std::max(tp, pm);
        }
        return tp;
    };
    auto scale = [&](int64_t n, int32_t g) {
        for (int c = 0; c < channels; ++c) {
            int16_t &s = pcm[n * channels + c];
            const int32_t v = (int32_t)s * g + (1 << 15);
            s = (int16_t)(v >= 0 ? v >> 16 : -((-v + 65535) >> 16));  // floor(v / 2^16): the arithmetic shift
        }
    };
    out->tp_in_q28 = out->tp_limited_q28 = out->tp_out_q28 = measure();
    if (out->tp_in_q28 <= C) return MM_OK;
    std::vector<int32_t> R((size_t)N), h((size_t)(N + 2 * (int64_t)W));
    for (int64_t n = 0; n < N; ++n) {
        int32_t v = CEIL_ONE;
        for (int64_t m = n; m < n + 12; ++m)
            v = std::min(v, P[(size_t)m] <= Ct ? CEIL_ONE : (int32_t)((Ct << 16) / P[(size_t)m]));
        R[(size_t)n] = v;
    }
    for (int64_t k = -W; k < N + W; ++k) {  // h[k] at index k + W; R = 2^16 outside [0, N)
        int32_t v = CEIL_ONE;
        for (int64_t j = std::max<int64_t>(k - W, 0); j <= std::min<int64_t>(k + W, N - 1); ++j) v = std::min(v, R[(size_t)j]);
        h[(size_t)(k + W)] = v;
    }
    int64_t sum = 0;
    for (int64_t u = 0; u < 2 * (int64_t)W; ++u) sum += h[(size_t)u];
    for (int64_t n = 0; n < N; ++n) {  // the box over h[n - W .. n + W] = indices n .. n + 2W
        sum += h[(size_t)(n + 2 * W)];
        const int32_t g = (int32_t)(sum / (2 * W + 1));
        sum -= h[(size_t)n];
        if (g == CEIL_ONE) continue;
        ++out->limited_frames;
        out->min_gain_q16 = std::min(out->min_gain_q16, g);
        scale(n, g);
    }
    out->tp_limited_q28 = out->tp_out_q28 = measure();
    if (out->tp_limited_q28 > C) {
        out->trim_q16 = ceiling_trim_gain(C, out->tp_limited_q28);
        for (int64_t n = 0; n < N; ++n) scale(n, out->trim_q16);
        out->tp_out_q28 = measure();
    }
    return MM_OK;
}

}  // extern "C"
