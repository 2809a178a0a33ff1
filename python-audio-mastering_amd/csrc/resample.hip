// resample.hip — deliver at another sample rate: an exact polyphase sample-rate converter
// on the int16 grid, and the delivery path that runs it between the chain and the ceiling
// (mm_deliver*).  No reference counterpart.  Everything is defined in integers
// (include/mastering.h, mm_resampler): with L / M the rate ratio in lowest terms and
// c[L][K] the caller's int32 taps (design.resample_taps), output frame n of a channel is
//   q = n * M, b = q / L, p = q % L
//   acc = sum_{k<K} c[p][k] * s[b + K/2 - k]        (s = 0 outside [0, N))
//   y   = (acc + 2^21) >> 22, delivered clipped to int16
// Every row has sum |c| < 2^24 (checked), so |acc| < 2^39: the sum is exact in int64 and
// just as exact as an f64 FMA chain in any order.  The kernel sums in f64 FMAs (full rate
// on this vector ALU, where the 64-bit integer multiply-add is a quarter-rate
// instruction), the host restatement in int64; the results are the same
// integers, so nothing depends on the launch geometry.
//
// One kernel (resample_tracks_kernel runs the body resample_span on the spans of every track
// of a call in one launch; a single signal is a call of one track).  A workgroup
// owns RS_SPAN consecutive output frames and stages the input
// frames they read in LDS: a line of int16 for mono, and for stereo one dword a frame
// (left in the low half).  Two de-interleaved int16 lines, as the meter stages its lines,
// were measured 6.6 times slower for stereo int16: the compiler fuses the reads of two
// neighbouring samples into one dword read at a 2-byte-aligned address, which the LDS
// serves slowly whenever the address is odd; a frame's dword is always aligned and
// halves the reads.  Outputs n and n + L share their phase, so a work item is RS_R
// outputs of one residue n mod L: each tap is loaded once and meets RS_R samples a
// channel.  The device copy of
// the taps is kept transposed and in output order, D[k][n mod L] = c[(n mod L) * M % L][k],
// so the lanes of a wave (consecutive n) read consecutive words of one row of D.
//
// Included in mastering.hip after pcm16.h (its frames and wave reductions are shared
// with the meter and the ceiling, not their line layout), meter.hip, ceiling.hip, level.hip
// (a delivery's refusals) and the WAV helpers.  mm_master / mm_deliver and mm_master_wav / mm_deliver_wav are here, one
// implementation each with the delivery optional.

namespace mm {

constexpr int RS_THREADS = 256;
constexpr int RS_SPAN = 1024;     // output frames per workgroup (mm_resample_span)
constexpr int RS_R = 4;           // outputs per work item (they share one row of taps)
constexpr int RS_LINE = 9216;     // frames a staged piece holds: a whole span up to M / L = 8 at K = 1024
constexpr int RS_MAX_K = 1024;
constexpr int RS_MAX_LM = 640;
constexpr int RS_SHIFT = 22;      // taps are multiples of 2^-22
constexpr int64_t RS_ROW_LIMIT = (int64_t)1 << 24;  // every row: sum |c| below this

// device result block of one conversion (zeroed on the stream before the launch)
struct RsDev {
    unsigned long long clipped[2];
    int peak[2];
};

struct RsArgs {
    int64_t N;          // input frames
    int64_t Nout;       // output frames
    int L, M, K;
    int sub;            // output frames per staged piece of a span: the largest whose input fits a line
    const int32_t *D;   // [K][L], output order
    RsDev *st;
};

// The workgroup's span is cut into pieces of a.sub outputs (one piece for every rate pair
// with M / L <= 8: a.sub == RS_SPAN); a piece starting at output m0 reads the input frames
// [lo, lo + len), lo = b(m0) - K/2 + 1, len = b(last) - b(m0) + K <= RS_LINE.  Item i of a
// piece of cnt outputs: residue r = i % min(L, cnt) and j-class jc = i / min(L, cnt); its
// outputs are o = r + (jc + jj * nJC) * L < cnt, jj < RS_R (interleaved j, so that with
// L = 1 the lanes of a wave are consecutive outputs).  An output beyond cnt computes on
// the item's first output's samples (always in range) and is not stored.
//
// resample_span is that workgroup: one span of one signal, `n0` its first output frame and
// every position relative to the signal's own start.
template <int CH, typename T>
__device__ __forceinline__ void resample_span(const T *__restrict__ in, T *__restrict__ out, RsArgs a, int64_t n0) {
    // mono: int16 samples; stereo: one dword a frame, left in the low half
    __shared__ __attribute__((aligned(16))) uint32_t lds[CH == 2 ? RS_LINE : RS_LINE / 2];
    int16_t *const line = reinterpret_cast<int16_t *>(lds);
    __shared__ unsigned red_clip[CH][RS_THREADS / 64];
    __shared__ int red_pk[CH][RS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, M = a.M, K = a.K;
    const int span = a.Nout - n0 < RS_SPAN ? (int)(a.Nout - n0) : RS_SPAN;
    unsigned n_clip[CH];
    int pk[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        n_clip[c] = 0;
        pk[c] = 0;
    }
    for (int s0 = 0; s0 < span; s0 += a.sub) {
        const int cnt = min(a.sub, span - s0);
        const int64_t m0 = n0 + s0;
        const int64_t q0 = m0 * M;  // < 2^31 * 640
        const int64_t b0 = q0 / L;
        const int p0 = (int)(q0 - b0 * L);
        const int rho0 = (int)(m0 % L);
        const int len = (int)(((m0 + cnt - 1) * M) / L - b0) + K;
        const int64_t lo = b0 - K / 2 + 1;  // frame of LDS index 0
        if (s0) __syncthreads();            // the lines are free for the next piece
        for (int i = tid; i < len; i += RS_THREADS) {
            const int64_t f = lo + i;
            const bool ok = f >= 0 && f < a.N;
            if constexpr (CH == 2) {
                lds[i] = ok ? load_frame_packed<T>(in, f) : 0u;
            } else {
                int s[1] = {};
                if (ok) load_frame<1, T>(in, f, s);
                line[i] = (int16_t)s[0];
            }
        }
        __syncthreads();
        const int Lc = min(L, cnt);
        const int J = (cnt + L - 1) / L, nJC = (J + RS_R - 1) / RS_R;
        const int items = Lc * nJC;
        for (int i = tid; i < items; i += RS_THREADS) {
            const int jc = i / Lc, r = i - jc * Lc;
            int rho = rho0 + r;  // (m0 + r) mod L: the row of D
            rho -= rho >= L ? L : 0;
            const int brel = (p0 + r * M) / L;  // b(m0 + r) - b0; r * M < 640 * 640
            int o[RS_R], base[RS_R];  // base: LDS index of the sample that meets tap 0
#pragma unroll
            for (int jj = 0; jj < RS_R; ++jj) {
                const int j = jc + jj * nJC;
                o[jj] = r + j * L;
                base[jj] = brel + (o[jj] < cnt ? j : jc) * M + K - 1;
            }
            double acc[CH][RS_R];
#pragma unroll
            for (int c = 0; c < CH; ++c)
#pragma unroll
                for (int jj = 0; jj < RS_R; ++jj) acc[c][jj] = 0.0;
            // two taps a step (K is even), the next pair loaded before this one is used, so
            // that a load's latency lies under a whole step of multiply-adds
            const int32_t *tp = a.D + rho;
            int32_t t0 = tp[0], t1 = tp[L];
            for (int k = 0; k < K; k += 2) {
                const double c0 = (double)t0, c1 = (double)t1;
                if (k + 2 < K) {
                    t0 = tp[(size_t)(k + 2) * L];
                    t1 = tp[(size_t)(k + 3) * L];
                }
#pragma unroll
                for (int jj = 0; jj < RS_R; ++jj) {
                    if constexpr (CH == 2) {
                        const uint32_t d0 = lds[base[jj] - k], d1 = lds[base[jj] - k - 1];
                        acc[0][jj] = fma(c0, (double)((int)(d0 << 16) >> 16), acc[0][jj]);
                        acc[1][jj] = fma(c0, (double)((int)d0 >> 16), acc[1][jj]);
                        acc[0][jj] = fma(c1, (double)((int)(d1 << 16) >> 16), acc[0][jj]);
                        acc[1][jj] = fma(c1, (double)((int)d1 >> 16), acc[1][jj]);
                    } else {
                        acc[0][jj] = fma(c0, (double)line[base[jj] - k], acc[0][jj]);
                        acc[0][jj] = fma(c1, (double)line[base[jj] - k - 1], acc[0][jj]);
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < RS_R; ++jj) {
                if (o[jj] >= cnt) continue;
                int y[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const long long v = ((long long)acc[c][jj] + (1ll << (RS_SHIFT - 1))) >> RS_SHIFT;  // arithmetic
                    const int yc = v > 32767 ? 32767 : (v < -32768 ? -32768 : (int)v);
                    n_clip[c] += v != yc ? 1u : 0u;
                    pk[c] = max(pk[c], yc < 0 ? -yc : yc);
                    y[c] = yc;
                }
                store_frame<CH, T>(out, m0 + o[jj], y);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const unsigned nc = wave_sum_u32(n_clip[c]);
        const int p = wave_max_i32(pk[c]);
        if (lane == 0) {
            red_clip[c][wave] = nc;
            red_pk[c][wave] = p;
        }
    }
    __syncthreads();
    if (tid < CH) {
        unsigned nc = 0;
        int p = 0;
        for (int w = 0; w < RS_THREADS / 64; ++w) {
            nc += red_clip[tid][w];
            p = max(p, red_pk[tid][w]);
        }
        if (nc) atomicAdd(&a.st->clipped[tid], (unsigned long long)nc);
        if (p) atomicMax(&a.st->peak[tid], p);
    }
}

static_assert(TRACKS_RS_SPAN == RS_SPAN, "tracks.h restates the span");

struct RsTrack {  // one a track, uploaded once a call
    const void *in;
    void *out;
    int64_t N, Nout;  // the track's own input and output frames
};

// One launch over the RS_SPAN spans of output frames of all tracks (tracks.h).  a.N, a.Nout and
// a.st are the launch's: st[n], and every workgroup takes N and Nout from its track
template <int CH, typename T>
__global__ void __launch_bounds__(RS_THREADS) resample_tracks_kernel(const RsTrack *tr, const uint32_t *first, int n, RsArgs a) {
    const int t = tracks_find(first, n, blockIdx.x);
    const RsTrack k = tr[t];
    a.N = k.N;
    a.Nout = k.Nout;
    a.st += t;
    resample_span<CH, T>(static_cast<const T *>(k.in), static_cast<T *>(k.out), a,
                         (int64_t)(blockIdx.x - first[t]) * RS_SPAN);
}

}  // namespace mm

// ======================================================= host entry points
namespace {

int64_t rs_gcd(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

int64_t rs_frames(int64_t frames, int L, int M) { return (frames * L + M - 1) / M; }

// why (L, M, K) is not a converter's geometry, or null
const char *resample_bad_geometry(int L, int M, int K) {
    if (K < 2 || K > RS_MAX_K || (K & 1)) return "K must be even and in [2, 1024]";
    if (L < 1 || M < 1 || L > RS_MAX_LM || M > RS_MAX_LM) return "L and M must be in [1, 640]";
    if (L == M || rs_gcd(L, M) != 1) return "L / M must be in lowest terms and not 1";
    return nullptr;
}

// why the table is refused, or null (the rows are summed: L * K additions)
const char *resample_bad_table(const mm_resampler *rs) {
    if (!rs || !rs->taps) return "null resampler or taps";
    if (const char *why = resample_bad_geometry(rs->L, rs->M, rs->K)) return why;
    if (rs->rate_in < 1 || rs->rate_out < 1 || (int64_t)rs->rate_in * rs->L != (int64_t)rs->rate_out * rs->M)
        return "rate_in * L must equal rate_out * M";
    for (int p = 0; p < rs->L; ++p) {
        int64_t sum = 0;
        for (int k = 0; k < rs->K; ++k) {
            const int64_t v = rs->taps[(size_t)p * rs->K + k];
            sum += v < 0 ? -v : v;
        }
        if (sum >= RS_ROW_LIMIT) return "a row of taps has sum |c| >= 2^24";
    }
    return nullptr;
}

// why (frames, channels) cannot be converted by this (checked) geometry, or null
const char *resample_bad_signal(int64_t frames, int channels, int L, int M) {
    if (const char *why = pcm_refusal(channels, frames, (int64_t)1 << 31)) return why;
    return rs_frames(frames, L, M) >= METER_MAX_FRAMES ? "output frames out of range" : nullptr;
}

// RsArgs.sub of a (checked) geometry: a piece of `sub` outputs reads
// ((sub - 1) * M + p0) / L + K <= (sub - 1) * M / L + 1 + K frames
int resample_sub(const mm_resampler *rs) {
    return (int)std::min<int64_t>(RS_SPAN, 1 + (int64_t)(RS_LINE - rs->K - 1) * rs->L / rs->M);
}

void resample_clear(mm_resample *o, int64_t frames, int channels, const mm_resampler *rs) {
    memset(o, 0, sizeof *o);
    o->frames_in = frames;
    o->frames_out = rs_frames(frames, rs->L, rs->M);
    o->channels = channels;
    o->rate_in = rs->rate_in;
    o->rate_out = rs->rate_out;
    o->L = rs->L;
    o->M = rs->M;
    o->K = rs->K;
}

}  // namespace

// The device copy of the taps, transposed and in output order (D[k][rho] = c[rho * M % L][k]),
// cached per context by the caller's content key (0: no key, checked and uploaded every call).
static int resample_taps_device(mm_ctx *c, const mm_resampler *rs, const int32_t **out) {
    int32_t *D;
    const size_t n = (size_t)rs->L * rs->K;
    if (rs->taps_key && rs->taps_key == c->rs_key && rs->L == c->rs_L && rs->M == c->rs_M && rs->K == c->rs_K) {
        RET(get_buf(c, "rs_taps", n, &D));
        *out = D;
        return MM_OK;
    }
    if (const char *why = resample_bad_table(rs)) return set_err(c, MM_ERR_ARG, "resampler: %s", why);
    c->rs_key = 0;
    RET(get_buf(c, "rs_taps", n, &D));
    std::vector<int32_t> t(n);
    for (int rho = 0; rho < rs->L; ++rho) {
        const int32_t *row = rs->taps + (size_t)((int64_t)rho * rs->M % rs->L) * rs->K;
        for (int k = 0; k < rs->K; ++k) t[(size_t)k * rs->L + rho] = row[k];
    }
    HIPCHK(c, hipMemcpyAsync(D, t.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (t leaves scope)
    c->rs_key = rs->taps_key;
    c->rs_L = rs->L;
    c->rs_M = rs->M;
    c->rs_K = rs->K;
    *out = D;
    return MM_OK;
}

// Refuses what is not a batch to convert (MM_ERR_ARG, the sentence names the track), before
// anything is queued.  The table itself is checked where it is uploaded (resample_taps_device),
// which queues nothing before it has refused.
static int batch_resample_check(mm_ctx *c, const void *const *in, int kind, const int64_t *frames, int n, int channels,
                                const mm_resampler *rs, void *const *out_pcm, const mm_resample *out) {
    if (n < 1 || n > MM_ALBUM_TRACKS) return set_err(c, MM_ERR_ARG, "batch: %d tracks out of range [1, %d]", n, MM_ALBUM_TRACKS);
    if (!in || !frames || !rs || !out_pcm || !out) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = resample_bad_geometry(rs->L, rs->M, rs->K)) return set_err(c, MM_ERR_ARG, "resampler: %s", why);
    int64_t total_in = 0, total_out = 0;
    for (int t = 0; t < n; ++t) {
        if (const char *why = resample_bad_signal(frames[t], channels, rs->L, rs->M))
            return set_err(c, MM_ERR_ARG, "batch: track %d: %s", t, why);
        if (frames[t] > 0 && (!in[t] || !out_pcm[t])) return set_err(c, MM_ERR_ARG, "batch: track %d: null pointer", t);
        total_in += frames[t];
        total_out += rs_frames(frames[t], rs->L, rs->M);
        if (total_in >= R128_MAX_FRAMES || total_out >= R128_MAX_FRAMES)
            return set_err(c, MM_ERR_ARG, "batch: track %d: 2^31 frames or more in all", t);
    }
    return MM_OK;
}

// Convert n device-resident tracks, track t from d_in[t] into d_out[t] (synchronous on return):
// one upload (the track table and, behind it, the n result blocks as zeros), one launch over the
// spans of all tracks, one read-back.  Arguments already checked, D the device copy of the taps
// (resample_taps_device).  The host table lives until the synchronisation at the end.
static int batch_resample_device(mm_ctx *c, const void *const *d_in, int kind, const int64_t *frames, int n, int channels,
                                 const mm_resampler *rs, const int32_t *D, void *const *d_out, mm_resample *out) {
    RsArgs a{};
    a.D = D;
    const size_t N = (size_t)n, tb = N * sizeof(RsTrack), o_st = (tb + (N + 1) * sizeof(uint32_t) + 7) & ~(size_t)7;
    std::vector<char> tab(o_st + N * sizeof(RsDev));  // the tracks, the grid's prefix sums, the zeroed results
    RsTrack *tr = reinterpret_cast<RsTrack *>(tab.data());
    uint32_t *first = reinterpret_cast<uint32_t *>(tab.data() + tb);
    std::vector<int64_t> wgs(N);
    for (int t = 0; t < n; ++t) {
        resample_clear(&out[t], frames[t], channels, rs);
        tr[t] = RsTrack{d_in[t], d_out[t], frames[t], out[t].frames_out};
        wgs[(size_t)t] = tracks_resample_spans(out[t].frames_out);
    }
    const uint32_t grid = tracks_prefix(wgs.data(), n, first);
    if (grid == 0) return MM_OK;  // no track has frames
    char *d_tab;
    RET(get_buf(c, "rs_tracks", tab.size(), &d_tab));
    HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
    a.st = reinterpret_cast<RsDev *>(d_tab + o_st);
    a.L = rs->L;
    a.M = rs->M;
    a.K = rs->K;
    a.sub = resample_sub(rs);
    RET(dispatch_pcm(kind, channels, [&](auto ch, auto t) {
        using T = decltype(t);
        return launch(c, "resample_tracks", resample_tracks_kernel<ch, T>, dim3(grid), dim3(RS_THREADS), 0,
                      reinterpret_cast<const RsTrack *>(d_tab), reinterpret_cast<const uint32_t *>(d_tab + tb), n, a);
    }));
    std::vector<RsDev> h(N);
    HIPCHK(c, hipMemcpyAsync(h.data(), a.st, N * sizeof(RsDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int t = 0; t < n; ++t)
        for (int ch = 0; ch < channels; ++ch) {
            out[t].clipped[ch] = (int64_t)h[(size_t)t].clipped[ch];
            out[t].peak[ch] = h[(size_t)t].peak[ch];
        }
    resolve_events(c);
    return MM_OK;
}

// Convert a device-resident signal into d_out (synchronous on return): a batch of one track.
static int resample_device(mm_ctx *c, const void *d_in, int kind, int64_t frames, int channels, const mm_resampler *rs,
                           void *d_out, mm_resample *out) {
    if (!c || !out || !rs || (frames > 0 && (!d_in || !d_out))) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = resample_bad_geometry(rs->L, rs->M, rs->K)) return set_err(c, MM_ERR_ARG, "resampler: %s", why);
    if (const char *why = resample_bad_signal(frames, channels, rs->L, rs->M)) return set_err(c, MM_ERR_ARG, "%s", why);
    const int32_t *D;
    RET(resample_taps_device(c, rs, &D));
    return batch_resample_device(c, &d_in, kind, &frames, 1, channels, rs, D, &d_out, out);
}

// why (job, delivery) is refused, or null
static const char *deliver_bad_args(const mm_job *j, const mm_delivery *dl) {
    if (!j || !dl) return "null job or delivery";
    if (j->ceiling_q28 || j->meter_on) return "the job's ceiling_q28 and meter_on act at the source rate: set the delivery's";
    if (j->channels != 1 && j->channels != 2) return "channels must be 1 or 2";
    int64_t frames = j->frames_proc;
    if (dl->rs) {
        if (const char *why = resample_bad_geometry(dl->rs->L, dl->rs->M, dl->rs->K)) return why;
        if (dl->rs->rate_in != j->rate) return "the resampler's rate_in is not the job's rate";
        if (const char *why = resample_bad_signal(j->frames_proc, j->channels, dl->rs->L, dl->rs->M)) return why;
        frames = rs_frames(j->frames_proc, dl->rs->L, dl->rs->M);
    }
    if (dl->level_clu) {
        if (!dl->loud || dl->loud->kweight.nsec != 2)
            return "a loudness target (level_clu) needs `loud`, a job with the K-weighting sections and the rate of the output";
        return level_bad_args(frames, j->channels, dl->loud->rate, dl->level_clu, dl->ceiling_q28, dl->window);
    }
    if (dl->ceiling_q28) return ceiling_bad_args(frames, j->channels, dl->ceiling_q28, dl->window);
    return nullptr;
}

// frames a master call delivers (dl null or without a converter: the chain's; else checked)
static int64_t delivered_frames(const mm_job *j, const mm_delivery *dl) {
    return dl && dl->rs ? rs_frames(j->frames_proc, dl->rs->L, dl->rs->M) : j->frames_proc;
}

// A master call on device-resident buffers.  Without a delivery (dl null) the plain chain:
// master_device.  With one, the chain into a context buffer and the converter into d_out (no
// converter: the chain into d_out), then the level or the ceiling and the report on what is
// delivered (slot 0 of mm_last_levels / _ceilings / _meters).
static int deliver_device(mm_ctx *c, const mm_job *j, const mm_delivery *dl, const void *d_in, void *d_out,
                          mm_result *res) {
    if (!dl) return master_device(c, j, d_in, d_out, res);
    if (const char *why = deliver_bad_args(j, dl)) return set_err(c, MM_ERR_ARG, "delivery: %s", why);
    const int kind = j->out_kind;
    int64_t frames = j->frames_proc;
    if (dl->rs) {
        char *mid;
        RET(get_buf(c, "deliver_mid", std::max<size_t>(pcm_bytes(kind, j->frames_proc, j->channels), 1), &mid));
        RET(master_device(c, j, d_in, mid, res));  // (the job asks for neither: its results stay empty)
        RET(resample_device(c, mid, kind, j->frames_proc, j->channels, dl->rs, d_out, &c->resample));
        frames = c->resample.frames_out;
    } else {
        RET(master_device(c, j, d_in, d_out, res));
    }
    results_reset(c, 1, dl->ceiling_q28, dl->meter_on, dl->level_clu);
    c->resample_valid = dl->rs != nullptr;
    return finish_delivered(c, d_out, kind, frames, j->channels, 0, dl->ceiling_q28, dl->window, dl->meter_on, dl->loud,
                            dl->level_clu);
}

// mm_master and mm_deliver: upload, the call on the device, download.
static int master_host(mm_ctx *c, const mm_job *j, const mm_delivery *dl, const void *in, void *out, mm_result *res) {
    RET(validate(c, j));
    if (const char *why = dl ? deliver_bad_args(j, dl) : nullptr) return set_err(c, MM_ERR_ARG, "delivery: %s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t in_bytes = (size_t)j->frames_in * j->channels * in_sample_bytes(j->in_kind);
    const size_t out_bytes = pcm_bytes(j->out_kind, delivered_frames(j, dl), j->channels);
    char *d_in, *d_out;
    RET(pcm_upload(c, "host_in", in, in_bytes, &d_in));
    RET(get_buf(c, "host_out", std::max<size_t>(out_bytes, 1), &d_out));
    RET(deliver_device(c, j, dl, d_in, d_out, res));
    RET(pcm_download(c, out, d_out, out_bytes));
    resolve_events(c);
    return MM_OK;
}

// mm_master_wav and mm_deliver_wav: file -> HBM, the call on the device, HBM -> file.  With
// a delivery the header carries the resampler's rate_out and the converter's frames_out.
static int master_wav(mm_ctx *c, const mm_job *jin, const mm_delivery *dl, const char *in_path, const char *out_path,
                      mm_result *res) {
    if (!jin || !in_path || !out_path) return set_err(c, MM_ERR_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    FileCloser in{fopen(in_path, "rb")};
    if (!in.f) return set_err(c, MM_ERR_ARG, "%s: cannot open", in_path);
    mm_job j;
    mm_wav_info wi;
    RET(wav_job(c, in.f, in_path, jin, &j, &wi));
    if (const char *why = dl ? deliver_bad_args(&j, dl) : nullptr) return set_err(c, MM_ERR_ARG, "delivery: %s", why);
    const size_t out_bytes = pcm_bytes(j.out_kind, delivered_frames(&j, dl), j.channels);
    if (out_bytes > 0xFFFFFFFFull - 36) return set_err(c, MM_ERR_ARG, "output larger than a RIFF file can hold");
    char *d_in, *d_out;
    RET(wav_stream_in(c, in.f, in_path, &j, &wi, &d_in));
    RET(get_buf(c, "host_out", std::max<size_t>(out_bytes, 1), &d_out));
    RET(deliver_device(c, &j, dl, d_in, d_out, res));
    return wav_stream_out(c, out_path, j.out_kind, j.channels, dl && dl->rs ? dl->rs->rate_out : j.rate, d_out, out_bytes);
}

extern "C" {

int mm_resample_span(void) { return RS_SPAN; }

int mm_resample_frames(int64_t frames, int32_t L, int32_t M, int64_t *frames_out) {
    if (!frames_out || frames < 0 || frames >= (int64_t)1 << 31 || L < 1 || M < 1 || L > RS_MAX_LM || M > RS_MAX_LM)
        return MM_ERR_ARG;
    *frames_out = rs_frames(frames, L, M);
    return MM_OK;
}

int mm_resample_device(mm_ctx *c, const void *d_in, int kind, int64_t frames, int channels, const mm_resampler *rs,
                       void *d_out, mm_resample *out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return resample_device(c, d_in, kind, frames, channels, rs, d_out, out);
}

int mm_resample_pcm(mm_ctx *c, const void *in, int kind, int64_t frames, int channels, const mm_resampler *rs, void *out_pcm,
                    mm_resample *out) {
    if (!c) return MM_ERR_ARG;
    if (!out || !rs || (frames > 0 && (!in || !out_pcm)) || !pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (const char *why = resample_bad_geometry(rs->L, rs->M, rs->K)) return set_err(c, MM_ERR_ARG, "resampler: %s", why);
    if (const char *why = resample_bad_signal(frames, channels, rs->L, rs->M)) return set_err(c, MM_ERR_ARG, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t out_bytes = pcm_bytes(kind, rs_frames(frames, rs->L, rs->M), channels);
    char *din, *dout;
    RET(pcm_upload(c, "rs_in", in, pcm_bytes(kind, frames, channels), &din));
    RET(get_buf(c, "rs_out", std::max<size_t>(out_bytes, 1), &dout));
    RET(resample_device(c, din, kind, frames, channels, rs, dout, out));
    return pcm_download(c, out_pcm, dout, out_bytes);
}

int mm_batch_resample_device(mm_ctx *c, const void *const *d_in, int kind, const int64_t *frames, int n, int channels,
                             const mm_resampler *rs, void *const *d_out, mm_resample *out) {
    if (!c) return MM_ERR_ARG;
    RET(batch_resample_check(c, d_in, kind, frames, n, channels, rs, d_out, out));
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t *D;
    RET(resample_taps_device(c, rs, &D));
    return batch_resample_device(c, d_in, kind, frames, n, channels, rs, D, d_out, out);
}

int mm_batch_resample_pcm(mm_ctx *c, const void *const *in, int kind, const int64_t *frames, int n, int channels,
                          const mm_resampler *rs, void *const *out_pcm, mm_resample *out) {
    if (!c) return MM_ERR_ARG;
    RET(batch_resample_check(c, in, kind, frames, n, channels, rs, out_pcm, out));
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t *D;
    RET(resample_taps_device(c, rs, &D));  // (a table it refuses: before a track is uploaded)
    std::vector<int64_t> frames_out((size_t)n);
    for (int t = 0; t < n; ++t) frames_out[(size_t)t] = rs_frames(frames[t], rs->L, rs->M);
    std::vector<void *> din, dout;
    RET(album_upload(c, "batch_rs_in", in, kind, frames, n, channels, din));
    RET(album_upload(c, "batch_rs_out", nullptr, kind, frames_out.data(), n, channels, dout));  // (laid out, nothing copied)
    RET(batch_resample_device(c, din.data(), kind, frames, n, channels, rs, D, dout.data(), out));
    return batch_download(c, out_pcm, dout, kind, frames_out.data(), n, channels, nullptr);
}

// The definition restated in plain C++ on the host (no context, no GPU): what the kernel
// must reproduce, samples and statistics.  Nothing outside in[0, frames * channels) is
// read, nothing outside out_pcm[0, frames_out * channels) written.
int mm_resample_host(const int16_t *in, int64_t frames, int channels, const mm_resampler *rs, int16_t *out_pcm,
                     mm_resample *out) {
    if (!out || !rs || resample_bad_table(rs) || resample_bad_signal(frames, channels, rs->L, rs->M)) return MM_ERR_ARG;
    if (frames > 0 && (!in || !out_pcm)) return MM_ERR_ARG;
    resample_clear(out, frames, channels, rs);
    const int64_t L = rs->L, M = rs->M, K = rs->K;
    for (int64_t n = 0; n < out->frames_out; ++n) {
        const int64_t q = n * M, b = q / L, p = q % L;
        const int32_t *row = rs->taps + (size_t)(p * K);
        for (int ch = 0; ch < channels; ++ch) {
            int64_t acc = 0;
            for (int64_t k = 0; k < K; ++k) {
                const int64_t f = b + K / 2 - k;
                if (f >= 0 && f < frames) acc += (int64_t)row[k] * in[f * channels + ch];
            }
            const int64_t v = acc + ((int64_t)1 << (RS_SHIFT - 1));
            const int64_t y = v >= 0 ? v >> RS_SHIFT : -((-v + (((int64_t)1 << RS_SHIFT) - 1)) >> RS_SHIFT);  // floor
            const int64_t d = std::min<int64_t>(32767, std::max<int64_t>(-32768, y));
            if (d != y) ++out->clipped[ch];
            out->peak[ch] = std::max(out->peak[ch], (int32_t)(d < 0 ? -d : d));
            out_pcm[n * channels + ch] = (int16_t)d;
        }
    }
    return MM_OK;
}

int mm_last_resample(mm_ctx *c, mm_resample *out) {
    if (!c || !out) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!c->resample_valid) return set_err(c, MM_ERR_STATE, "the last master call did not resample");
    *out = c->resample;
    return MM_OK;
}

int mm_deliver_device(mm_ctx *c, const mm_job *j, const mm_delivery *dl, const void *d_in, void *d_out, mm_result *res) {
    if (!c) return MM_ERR_ARG;
    if (!dl) return set_err(c, MM_ERR_ARG, "delivery: null job or delivery");
    HIPCHK(c, hipSetDevice(c->device));
    return deliver_device(c, j, dl, d_in, d_out, res);
}

int mm_master(mm_ctx *c, const mm_job *j, const void *in, void *out, mm_result *res) {
    return c ? master_host(c, j, nullptr, in, out, res) : MM_ERR_ARG;
}

int mm_deliver(mm_ctx *c, const mm_job *j, const mm_delivery *dl, const void *in, void *out, mm_result *res) {
    if (!c) return MM_ERR_ARG;
    if (!dl) return set_err(c, MM_ERR_ARG, "delivery: null job or delivery");
    return master_host(c, j, dl, in, out, res);
}

int mm_master_wav(mm_ctx *c, const mm_job *jin, const char *in_path, const char *out_path, mm_result *res) {
    return c ? master_wav(c, jin, nullptr, in_path, out_path, res) : MM_ERR_ARG;
}

int mm_deliver_wav(mm_ctx *c, const mm_job *jin, const mm_delivery *dl, const char *in_path, const char *out_path,
                   mm_result *res) {
    if (!c) return MM_ERR_ARG;
    if (!dl) return set_err(c, MM_ERR_ARG, "null argument");
    return master_wav(c, jin, dl, in_path, out_path, res);
}

}  // extern "C"
