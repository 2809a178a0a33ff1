// qc.hip — the delivery QC report of a delivered signal (mm_qc in include/mastering.h): the
// totals behind DC offset, correlation and bit use, digital silence at the head, the tail and
// inside, runs of full-scale samples, and the phase correlation in 400 ms windows.  No
// reference counterpart.  Every figure is an exact integer on the int16 grid; the one double,
// corr_min, comes from integers through mm_qc_from_hops, the tail that the host restatement
// (mm_qc_host: plain sequential loops) and the GPU path both end in.
//
// The GPU path is two launches on the context's stream.  The span kernel (qc_span: one
// workgroup a span of QC_SPAN frames, a thread QC_FPT consecutive frames of it, staged through
// LDS so that the global loads are whole lines) writes ONE fixed-size record a span with plain
// stores and adds its pieces of the hop sums into the zeroed [H][3] table, one integer atomic a
// hop piece after a workgroup reduction (integer adds commute: two runs are bit-identical, and
// there is no float atomic anywhere).  The fold kernel (qc_fold_kernel: one workgroup a track)
// then folds the track's records in span order, a contiguous chunk a thread and a tree in LDS,
// and writes the track's mm_qc integers; stream order gives it the records, so there is no
// in-kernel hand-off.
//
// Sums fold by addition.  Runs do not: a run of rail samples or of silence can cross any
// number of spans.  A segment of frames therefore carries, for each of the three run classes
// (rail of channel 0, rail of channel 1, silent), a QcRun: the open run at its head, the open
// run at its tail, whether the whole segment is one run, and of the runs closed on both sides
// inside it the longest (the first of equals, with its start on the track) and the count of
// those of min_run frames or more.  qc_run_join joins two adjacent segments and is
// associative; the same operator joins a thread's frames, the threads of a span and the spans
// of a track, and qc_run_finish lets the track's two ends close what is still open.
//
// The grid is the need grid of tracks.h (tracks_need_spans: it counts m in [0, frames + 11), so
// a track's last span may hold no frame and then writes an empty record, the operator's
// identity), laid over the spans of all tracks of a call: a single signal is a call of one
// track.  Included at the end of mastering.hip after r128.hip (r128_bound, r128_hop_of: the
// hops are the R 128 report's).

namespace mm {

constexpr int QC_THREADS = 256;
constexpr int QC_FPT = 8;                         // consecutive frames per thread
constexpr int QC_SPAN = QC_THREADS * QC_FPT;      // frames per workgroup (mm_qc_span)
constexpr int QC_HOP_PIECES = 12;                 // hops a span can meet: the first, then 11 of >= 200 frames
constexpr int QC_MIN_RATE = 2000;                 // the library's floor: hops of >= 200 frames
constexpr int64_t QC_MAX_FRAMES = (int64_t)1 << 31;
constexpr int QC_REPORT_LSB = 1, QC_REPORT_RUN = 3;  // silence_lsb and min_run of a master call's report (MM_REPORT_QC)
static_assert(QC_SPAN == TRACKS_METER_SPAN, "the span kernel runs on the need grid of tracks.h");
static_assert((QC_HOP_PIECES - 1) * (QC_MIN_RATE / 10) >= QC_SPAN, "B[h + 12] lies beyond the span that B[h + 1] lies in");
static_assert(QC_FPT <= QC_MIN_RATE / 10, "a thread's frames meet at most two hops");

struct QcRun {
    int head_v, head_len;  // the open run at the segment's first frame (len 0: none)
    int tail_v, tail_len;  // the open run at its last frame
    int whole;             // the segment is one run: the head and the tail are it
    int best_len, best_at; // the longest closed run, the first of equals, and its start on the track (none: 0, -1)
    int count;             // closed runs of min_run frames or more
};

__host__ __device__ __forceinline__ QcRun qc_run_none() { return QcRun{0, 0, 0, 0, 0, 0, -1, 0}; }

// one frame of class value v (0: no run)
__host__ __device__ __forceinline__ QcRun qc_run_frame(int v) {
    const int on = v != 0;
    return QcRun{v, on, v, on, on, 0, -1, 0};
}

// a run of len frames at `at` is closed; called in the order of `at`, so a strict compare
// keeps the first of equals
__host__ __device__ __forceinline__ void qc_run_close(QcRun &o, int len, int64_t at, int r) {
    if (len >= r) ++o.count;
    if (len > o.best_len) {
        o.best_len = len;
        o.best_at = (int)at;
    }
}

// a on [a_start, a_start + a_len) joined with b on the frames that follow; both hold frames
__host__ __device__ __forceinline__ QcRun qc_run_join(const QcRun &a, int64_t a_start, int64_t a_len, const QcRun &b, int r) {
    const int64_t seam = a_start + a_len;
    QcRun o{a.head_v, a.head_len, b.tail_v, b.tail_len, 0, a.best_len, a.best_at, a.count + b.count};
    if (a.tail_len > 0 && b.head_len > 0 && a.tail_v == b.head_v) {  // one run across the seam
        const int m = a.tail_len + b.head_len;
        if (a.whole && b.whole) {
            o.head_len = o.tail_len = m;
            o.whole = 1;
        } else if (a.whole) {
            o.head_len = m;
        } else if (b.whole) {
            o.tail_len = m;
        } else {
            qc_run_close(o, m, seam - a.tail_len, r);
        }
    } else {  // the seam closes what reaches it, unless that is the segment's own head or tail
        if (a.tail_len > 0 && !a.whole) qc_run_close(o, a.tail_len, seam - a.tail_len, r);
        if (b.head_len > 0 && !b.whole) qc_run_close(o, b.head_len, seam, r);
    }
    if (b.best_len > o.best_len) {
        o.best_len = b.best_len;
        o.best_at = b.best_at;
    }
    return o;
}

// the track's two ends close the open runs of its fold: the longest run, its start, the runs >= r
__host__ __device__ __forceinline__ void qc_run_finish(const QcRun &t, int64_t N, int r, int64_t *longest, int64_t *at,
                                                       int64_t *runs) {
    QcRun o{0, 0, 0, 0, 0, 0, -1, t.count};
    if (t.head_len > 0) qc_run_close(o, t.head_len, 0, r);
    if (t.best_len > o.best_len) {
        o.best_len = t.best_len;
        o.best_at = t.best_at;
    }
    if (t.tail_len > 0 && !t.whole) qc_run_close(o, t.tail_len, N - t.tail_len, r);
    *longest = o.best_len;
    *at = o.best_at;
    if (runs) *runs = o.count;
}

// what a span writes and the fold carries: a segment's totals and its three run classes
struct QcRec {
    int64_t start, len;  // the segment's frames on the track (len 0: the identity, nothing else is read)
    int64_t sum[2], sq[2], cross;
    int64_t clip[2], silent;
    int smin[2], smax[2];
    unsigned or_bits[2];
    QcRun run[3];        // rail of channel 0, rail of channel 1, silent
};

__host__ __device__ __forceinline__ QcRec qc_rec_join(const QcRec &a, const QcRec &b, int r) {
    if (a.len == 0) return b;
    if (b.len == 0) return a;
    QcRec o = a;
    o.len = a.len + b.len;
    o.cross = a.cross + b.cross;
    o.silent = a.silent + b.silent;
    for (int c = 0; c < 2; ++c) {
        o.sum[c] = a.sum[c] + b.sum[c];
        o.sq[c] = a.sq[c] + b.sq[c];
        o.clip[c] = a.clip[c] + b.clip[c];
        o.smin[c] = a.smin[c] < b.smin[c] ? a.smin[c] : b.smin[c];
        o.smax[c] = a.smax[c] > b.smax[c] ? a.smax[c] : b.smax[c];
        o.or_bits[c] = a.or_bits[c] | b.or_bits[c];
    }
    for (int k = 0; k < 3; ++k) o.run[k] = qc_run_join(a.run[k], a.start, a.len, b.run[k], r);
    return o;
}

// every integer of mm_qc from a track's fold (step 5's fields cleared: mm_qc_from_hops)
__host__ __device__ __forceinline__ void qc_finish(const QcRec &t, int64_t N, int channels, int rate, int64_t H, int q, int r,
                                                   mm_qc *o) {
    o->frames = N;
    o->channels = channels;
    o->rate = rate;
    o->hops = H;
    o->silence_lsb = q;
    o->min_run = r;
    const bool any = t.len != 0;
    o->cross = any ? t.cross : 0;
    o->silent_frames = any ? t.silent : 0;
    for (int c = 0; c < 2; ++c) {
        o->sum[c] = any ? t.sum[c] : 0;
        o->sq[c] = any ? t.sq[c] : 0;
        o->smin[c] = any ? t.smin[c] : 0;
        o->smax[c] = any ? t.smax[c] : 0;
        o->or_bits[c] = any ? t.or_bits[c] : 0u;
        o->clip_samples[c] = any ? t.clip[c] : 0;
        qc_run_finish(any ? t.run[c] : qc_run_none(), N, r, &o->clip_longest[c], &o->clip_longest_at[c], &o->clip_runs[c]);
    }
    const QcRun s = any ? t.run[2] : qc_run_none();
    qc_run_finish(s, N, r, &o->silence_longest, &o->silence_longest_at, nullptr);
    o->lead_silence = s.head_len;                   // (all silent: the head is the whole track, N)
    o->trail_silence = s.tail_len;
    o->corr_windows = o->corr_negative = 0;
    o->corr_min_hop = -1;
    o->corr_min = __builtin_nan("");
}

// one track of a launch
struct QcTrack {
    const void *pcm;
    int64_t N, H;   // frames, complete hops
    int64_t hop0;   // its first row of the hop table
};

struct QcLaunch {
    const QcTrack *tr;             // [n]
    const uint32_t *first;         // [n + 1] prefix sums of the tracks' spans (tracks.h)
    QcRec *rec;                    // [first[n]] a track's records at first[t]
    unsigned long long *hops;      // [sum H][3], zeroed on the stream
    mm_qc *out;                    // [n]
    int n, channels, rate, q, r;
};

struct QcRunSeg {
    QcRun run;
    int len;
};

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Span `span` of a track: its record into rec[span], its hop pieces into the track's table.
template <int CH, typename T>
__device__ __forceinline__ void qc_span(const T *__restrict__ in, const QcTrack &tr, int64_t span, int rate, int q, int r,
                                        QcRec *rec, unsigned long long *hops) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[QC_SPAN];  // a stereo frame as its dword, a mono one sign-extended
    __shared__ QcRunSeg seg[QC_THREADS];
    __shared__ unsigned long long hacc[QC_HOP_PIECES][3];
    __shared__ int bound[QC_HOP_PIECES + 1];  // where hop h_first + k begins, from the span's first frame (capped at its end)
    __shared__ QcRec wrec[QC_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t base = span * QC_SPAN;
    const int len = (int)max((int64_t)0, min((int64_t)QC_SPAN, tr.N - base));
    const int64_t h_first = r128_hop_of(base, rate);
    if (t <= QC_HOP_PIECES) bound[t] = (int)min((int64_t)QC_SPAN, r128_bound(h_first + t, rate) - base);
    if (t < QC_HOP_PIECES * 3) hacc[t / 3][t % 3] = 0;
    for (int i = t; i < QC_SPAN; i += QC_THREADS) {
        uint32_t d = 0;
        if (i < len) {
            if constexpr (CH == 2) {
                d = load_frame_packed<T>(in, base + i);
            } else {
                int s[1];
                load_frame<1, T>(in, base + i, s);
                d = (uint32_t)s[0];
            }
        }
        stage[i] = d;
    }
    __syncthreads();

    // the thread's frames r0 .. r0 + n - 1 of the span; hop piece k holds r0, piece k + 1 begins at nb
    const int r0 = t * QC_FPT, n = max(0, min(QC_FPT, len - r0));
    int k = 0;
    while (k + 1 < QC_HOP_PIECES && bound[k + 1] <= r0) ++k;
    const int nb = bound[k + 1];
    uint32_t d[QC_FPT];
    {
        const uint4 lo = *reinterpret_cast<const uint4 *>(&stage[r0]), hi = *reinterpret_cast<const uint4 *>(&stage[r0 + 4]);
        d[0] = lo.x, d[1] = lo.y, d[2] = lo.z, d[3] = lo.w, d[4] = hi.x, d[5] = hi.y, d[6] = hi.z, d[7] = hi.w;
    }
    QcRec me{};
    me.start = base + r0;
    me.len = n;
    me.smin[0] = me.smin[1] = 32767;
    me.smax[0] = me.smax[1] = -32768;
    unsigned long long pa[2] = {0, 0}, pb[2] = {0, 0};  // the squares of the two pieces ((-32768)^2 = 2^30: 64-bit from the second on)
    int64_t px[2] = {0, 0};
    int v[3][QC_FPT];
    int any_v[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < QC_FPT; ++j) {
        int s[2];
        s[0] = CH == 2 ? (int)(int16_t)(d[j] & 0xFFFFu) : (int)d[j];
        s[1] = CH == 2 ? (int)(int16_t)(d[j] >> 16) : 0;
        const bool in_range = j < n;
        bool silent = in_range;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int x = s[c], ax = x < 0 ? -x : x;
            const int rail = c < CH && in_range ? (x == 32767 ? 1 : (x <= -32767 ? -1 : 0)) : 0;
            v[c][j] = rail;
            any_v[c] |= rail;
            if (c < CH && in_range) {
                me.sum[c] += x;
                me.sq[c] += (int64_t)(x * x);
                me.smin[c] = min(me.smin[c], x);
                me.smax[c] = max(me.smax[c], x);
                me.or_bits[c] |= (unsigned)x & 0xFFFFu;
                me.clip[c] += rail != 0;
                silent = silent && ax <= q;
            }
        }
        v[2][j] = silent;
        any_v[2] |= silent;
        me.silent += silent;
        if (in_range) {
            const int p = r0 + j < nb ? 0 : 1;
            pa[p] += (unsigned long long)(s[0] * s[0]);
            if constexpr (CH == 2) {
                pb[p] += (unsigned long long)(s[1] * s[1]);
                px[p] += (int64_t)(s[0] * s[1]);
                me.cross += (int64_t)(s[0] * s[1]);
            }
        }
    }

    // the three run classes, each across the span's threads by a tree of joins; a class no
    // frame of the span belongs to (the rule in music) skips its tree
    QcRun span_run[3];
#pragma unroll
    for (int cls = 0; cls < 3; ++cls) {
        span_run[cls] = qc_run_none();
        if (CH == 1 && cls == 1) continue;
        if (!__syncthreads_or(any_v[cls] != 0)) continue;  // (uniform; 0 / 1, as ceil_apply passes it: its code stays the parent's)
        QcRun mine = qc_run_none();
        if (any_v[cls]) {
            mine = qc_run_frame(v[cls][0]);
#pragma unroll
            for (int j = 1; j < QC_FPT; ++j)
                if (j < n) mine = qc_run_join(mine, me.start, j, qc_run_frame(v[cls][j]), r);
        }
        seg[t] = QcRunSeg{mine, n};
        __syncthreads();
        for (int s = 1; s < QC_THREADS; s <<= 1) {
            if ((t & (2 * s - 1)) == 0) {
                const QcRunSeg A = seg[t], B = seg[t + s];  // (frames fill the threads from 0: A empty, then B too)
                if (A.len != 0 && B.len != 0) seg[t] = QcRunSeg{qc_run_join(A.run, me.start, A.len, B.run, r), A.len + B.len};
            }
            __syncthreads();
        }
        span_run[cls] = seg[0].run;
        __syncthreads();  // seg is free for the next class
    }

    // the totals: a butterfly in every wave, then thread 0 over the waves
    QcRec w = me;
    w.cross = wave_sum_i64(me.cross);
    w.silent = wave_sum_i64(me.silent);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        w.sum[c] = wave_sum_i64(me.sum[c]);
        w.sq[c] = wave_sum_i64(me.sq[c]);
        w.clip[c] = wave_sum_i64(me.clip[c]);
        w.smin[c] = -wave_max_i32(-me.smin[c]);
        w.smax[c] = wave_max_i32(me.smax[c]);
        unsigned ob = me.or_bits[c];
        for (int o = 32; o > 0; o >>= 1) ob |= __shfl_xor(ob, o);
        w.or_bits[c] = ob;
    }
    if (lane == 0) wrec[wave] = w;

    // the hop pieces into LDS: a wave that lies in one piece (the rule: a hop is 4410 frames at
    // 44.1 kHz, a wave's share 512) adds its totals once, any other wave lane by lane
    const int kf = __builtin_amdgcn_readfirstlane(k);
    if (__all(k == kf && r0 + QC_FPT <= nb)) {
        if (lane == 0) {
            if (w.sq[0]) atomicAdd(&hacc[kf][0], (unsigned long long)w.sq[0]);
            if (CH == 2 && w.sq[1]) atomicAdd(&hacc[kf][1], (unsigned long long)w.sq[1]);
            if (CH == 2 && w.cross) atomicAdd(&hacc[kf][2], (unsigned long long)w.cross);
        }
    } else {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (k + p >= QC_HOP_PIECES) continue;  // (never with frames: the static_asserts above)
            if (pa[p]) atomicAdd(&hacc[k + p][0], pa[p]);
            if (CH == 2 && pb[p]) atomicAdd(&hacc[k + p][1], pb[p]);
            if (CH == 2 && px[p]) atomicAdd(&hacc[k + p][2], (unsigned long long)px[p]);
        }
    }
    __syncthreads();
    if (t < QC_HOP_PIECES * 3) {  // one atomic a hop piece and column; from B[H] on a frame belongs to no hop
        const int64_t h = h_first + t / 3;
        const unsigned long long s = hacc[t / 3][t % 3];
        if (h < tr.H && s) atomicAdd(&hops[h * 3 + t % 3], s);
    }
    if (t == 0) {
        QcRec o = wrec[0];
        for (int i = 1; i < QC_THREADS / 64; ++i) {
            const QcRec &b = wrec[i];
            o.cross += b.cross;
            o.silent += b.silent;
            for (int c = 0; c < CH; ++c) {
                o.sum[c] += b.sum[c];
                o.sq[c] += b.sq[c];
                o.clip[c] += b.clip[c];
                o.smin[c] = min(o.smin[c], b.smin[c]);
                o.smax[c] = max(o.smax[c], b.smax[c]);
                o.or_bits[c] |= b.or_bits[c];
            }
        }
        if (CH == 1) {  // (the second channel of a mono signal: zeros, as mm_qc holds them)
            o.sum[1] = o.sq[1] = o.clip[1] = 0;
            o.smin[1] = o.smax[1] = 0;
            o.or_bits[1] = 0;
        }
        o.start = base;
        o.len = len;
        for (int cls = 0; cls < 3; ++cls) o.run[cls] = span_run[cls];
        rec[span] = o;
    }
}

// qc_span over the spans of all tracks: a record lands among its track's own, a hop piece in its
// track's own rows, and every frame index is the track's
template <int CH, typename T>
__global__ void __launch_bounds__(QC_THREADS) qc_tracks_kernel(QcLaunch L) {
    const int t = tracks_find(L.first, L.n, blockIdx.x);
    const QcTrack tr = L.tr[t];
    qc_span<CH, T>(static_cast<const T *>(tr.pcm), tr, (int64_t)(blockIdx.x - L.first[t]), L.rate, L.q, L.r,
                   L.rec + L.first[t], L.hops + 3 * tr.hop0);
}

// Workgroup t folds track t's records in span order: thread i the i-th contiguous chunk, then a
// tree of joins in LDS; thread 0 lets the track's ends close the open runs and writes its mm_qc.
__global__ void __launch_bounds__(QC_THREADS) qc_fold_kernel(QcLaunch L) {
    __shared__ QcRec tree[QC_THREADS];
    const int t = threadIdx.x;
    const QcTrack tr = L.tr[blockIdx.x];
    const QcRec *rec = L.rec + L.first[blockIdx.x];
    const int64_t S = (int64_t)L.first[blockIdx.x + 1] - (int64_t)L.first[blockIdx.x];
    const int64_t per = (S + QC_THREADS - 1) / QC_THREADS, i0 = min(S, t * per), i1 = min(S, i0 + per);
    QcRec acc{};  // (len 0: the identity)
    for (int64_t i = i0; i < i1; ++i) acc = qc_rec_join(acc, rec[i], L.r);
    tree[t] = acc;
    __syncthreads();
    for (int s = 1; s < QC_THREADS; s <<= 1) {
        if ((t & (2 * s - 1)) == 0) tree[t] = qc_rec_join(tree[t], tree[t + s], L.r);
        __syncthreads();
    }
    if (t == 0) qc_finish(tree[0], tr.N, L.channels, L.rate, tr.H, L.q, L.r, &L.out[blockIdx.x]);
}

}  // namespace mm

// ======================================================= host side
namespace {

void qc_clear(mm_qc *o, int64_t frames, int channels, int rate, int q, int r) {
    QcRec none{};
    qc_finish(none, frames, channels, rate, frames > 0 && rate > 0 ? 10 * frames / rate : 0, q, r, o);
}

// why a signal or a parameter is refused, or null (the words of mm_last_error)
const char *qc_refusal(int channels, int64_t frames, int rate, int q, int r) {
    if (rate < QC_MIN_RATE) return "rate below 2000 Hz";
    if (q < 0 || q > 32767) return "silence_lsb out of range [0, 32767]";
    if (r < 1 || r > 65535) return "min_run out of range [1, 65535]";
    return pcm_refusal(channels, frames, QC_MAX_FRAMES);
}

// The reports of n checked device-resident tracks into out[n] (synchronous on return): one
// upload of the track table, one memset of the results and the hop table, the span launch, the
// fold launch and one read-back, then the tail of step 5.  hops_out (may be null): the tables
// of all tracks back to back.  The host tables live until the synchronisation.
int qc_run(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate, int q, int r,
           mm_qc *out, int64_t *hops_out) {
    const size_t N = (size_t)n;
    std::vector<QcTrack> tr(N);
    std::vector<int64_t> wgs(N);
    std::vector<uint32_t> first(N + 1);
    int64_t hops = 0;
    for (int t = 0; t < n; ++t) {
        tr[(size_t)t] = QcTrack{d_pcm[t], frames[t], 10 * frames[t] / rate, hops};
        hops += tr[(size_t)t].H;
        wgs[(size_t)t] = tracks_need_spans(frames[t]);
    }
    const uint32_t grid = tracks_prefix(wgs.data(), n, first.data());
    const size_t tab_bytes = N * sizeof(QcTrack) + (N + 1) * sizeof(uint32_t);
    const size_t out_bytes = N * sizeof(mm_qc) + (size_t)hops * 3 * sizeof(int64_t);
    std::vector<char> tab(tab_bytes), back(out_bytes);
    memcpy(tab.data(), tr.data(), N * sizeof(QcTrack));
    memcpy(tab.data() + N * sizeof(QcTrack), first.data(), (N + 1) * sizeof(uint32_t));
    char *d_tab, *d_out;
    QcLaunch L{};
    RET(get_buf(c, "qc_tab", tab_bytes, &d_tab));
    RET(get_buf(c, "qc_out", out_bytes, &d_out));
    RET(get_buf(c, "qc_rec", std::max<size_t>(grid, 1), &L.rec));
    L.tr = reinterpret_cast<const QcTrack *>(d_tab);
    L.first = reinterpret_cast<const uint32_t *>(d_tab + N * sizeof(QcTrack));
    L.out = reinterpret_cast<mm_qc *>(d_out);
    L.hops = reinterpret_cast<unsigned long long *>(d_out + N * sizeof(mm_qc));
    L.n = n;
    L.channels = channels;
    L.rate = rate;
    L.q = q;
    L.r = r;
    HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_out, 0, out_bytes, c->stream));
    if (grid)
        RET(dispatch_pcm(kind, channels, [&](auto ch, auto t) {
            using T = decltype(t);
            return launch(c, "qc_tracks", qc_tracks_kernel<ch, T>, dim3(grid), dim3(QC_THREADS), 0, L);
        }));
    RET(launch(c, "qc_fold", qc_fold_kernel, dim3((unsigned)n), dim3(QC_THREADS), 0, L));
    HIPCHK(c, hipMemcpyAsync(back.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    memcpy(out, back.data(), N * sizeof(mm_qc));
    const int64_t *table = reinterpret_cast<const int64_t *>(back.data() + N * sizeof(mm_qc));
    for (int t = 0; t < n; ++t)
        if (channels == 2) mm_qc_from_hops(table + 3 * tr[(size_t)t].hop0, tr[(size_t)t].H, rate, &out[t]);
    if (hops_out && hops) memcpy(hops_out, table, (size_t)hops * 3 * sizeof(int64_t));
    return MM_OK;
}

// Refuses what is not a batch to check (MM_ERR_ARG, the sentence names the track), before
// anything is queued.
int batch_qc_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int rate, int q,
                   int r, const mm_qc *out) {
    return batch_check(c, pcm, kind, frames, n, channels, out != nullptr,
                       [&](int t) { return qc_refusal(channels, frames[t], rate, q, r); });
}

// The QC reports of n checked device-resident tracks (synchronous on return).  Only c->qcs is
// set: the levels, ceilings and R 128 reports of the context's last call stay.
int batch_qc_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate, int q,
                    int r, mm_qc *out) {
    RET(qc_run(c, d_pcm, kind, frames, n, channels, rate, q, r, out, nullptr));
    c->qcs.assign(out, out + n);
    return MM_OK;
}

}  // namespace

// The QC report of a device-resident signal (synchronous on return): a call of one track, which
// leaves the context's results as they are.
static int qc_device(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, int rate, int q, int r,
                     mm_qc *out, int64_t *hops_out) {
    if (!c || !out || (frames > 0 && !d_pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = qc_refusal(channels, frames, rate, q, r)) return set_err(c, MM_ERR_ARG, "QC: %s", why);
    return qc_run(c, &d_pcm, kind, &frames, 1, channels, rate, q, r, out, hops_out);
}

extern "C" {

int mm_qc_span(void) { return QC_SPAN; }

int mm_qc_from_hops(const int64_t *hops, int64_t H, int32_t rate, mm_qc *out) {
    if (!out || H < 0 || (H > 0 && !hops) || rate < QC_MIN_RATE) return MM_ERR_ARG;
    out->hops = H;
    out->rate = rate;
    out->corr_windows = out->corr_negative = 0;
    out->corr_min_hop = -1;
    out->corr_min = NAN;
    for (int64_t j = 0; j + 4 <= H; ++j) {
        int64_t A = 0, B = 0, X = 0;
        for (int k = 0; k < 4; ++k) {
            A += hops[3 * (j + k)];
            B += hops[3 * (j + k) + 1];
            X += hops[3 * (j + k) + 2];
        }
        if (A + B < 2048 * (r128_bound(j + 4, rate) - r128_bound(j, rate))) continue;  // below the gate
        ++out->corr_windows;
        if (X < 0) ++out->corr_negative;
        const double rho = A == 0 || B == 0 ? 0.0 : (double)X / std::sqrt((double)A * (double)B);
        if (out->corr_min_hop < 0 || rho < out->corr_min) {  // strict: the smallest j of a tie stays
            out->corr_min = rho;
            out->corr_min_hop = j;
        }
    }
    return MM_OK;
}

int mm_qc_host(const int16_t *pcm, int64_t frames, int channels, int32_t rate, int32_t silence_lsb, int32_t min_run,
               mm_qc *out, int64_t *hops_out) {
    if (!out || (frames > 0 && !pcm) || qc_refusal(channels, frames, rate, silence_lsb, min_run)) return MM_ERR_ARG;
    const int q = silence_lsb, r = min_run;
    qc_clear(out, frames, channels, rate, q, r);
    for (int c = 0; c < channels && frames > 0; ++c) {  // totals and clip runs, channel by channel
        out->smin[c] = out->smax[c] = pcm[c];
        int prev = 0;
        int64_t run = 0;
        for (int64_t n = 0; n < frames; ++n) {
            const int32_t s = pcm[n * channels + c];
            out->sum[c] += s;
            out->sq[c] += (int64_t)s * s;
            out->smin[c] = std::min(out->smin[c], s);
            out->smax[c] = std::max(out->smax[c], s);
            out->or_bits[c] |= (uint32_t)(uint16_t)s;
            const int rail = s == 32767 ? 1 : (s <= -32767 ? -1 : 0);
            run = rail != 0 && rail == prev ? run + 1 : (rail != 0 ? 1 : 0);
            prev = rail;
            if (rail != 0) ++out->clip_samples[c];
            if (run == r) ++out->clip_runs[c];  // (a run is counted once, when it reaches r)
            if (run > out->clip_longest[c]) {   // (strict, while it grows: the first of equals)
                out->clip_longest[c] = run;
                out->clip_longest_at[c] = n - run + 1;
            }
        }
    }
    int64_t run = 0, first_loud = -1, last_loud = -1;
    for (int64_t n = 0; n < frames; ++n) {
        bool silent = true;
        for (int c = 0; c < channels; ++c) silent = silent && std::abs((int32_t)pcm[n * channels + c]) <= q;
        if (channels == 2) out->cross += (int64_t)pcm[2 * n] * pcm[2 * n + 1];
        if (!silent) {
            run = 0;
            if (first_loud < 0) first_loud = n;
            last_loud = n;
            continue;
        }
        ++out->silent_frames;
        if (++run > out->silence_longest) {
            out->silence_longest = run;
            out->silence_longest_at = n - run + 1;
        }
    }
    out->lead_silence = first_loud < 0 ? frames : first_loud;
    out->trail_silence = last_loud < 0 ? frames : frames - 1 - last_loud;
    const int64_t H = out->hops;
    std::vector<int64_t> table((size_t)H * 3, 0);
    for (int64_t i = 0; i < H; ++i)
        for (int64_t n = r128_bound(i, rate); n < r128_bound(i + 1, rate); ++n) {
            const int64_t s0 = pcm[n * channels], s1 = channels == 2 ? pcm[n * channels + 1] : 0;
            table[(size_t)(3 * i)] += s0 * s0;
            table[(size_t)(3 * i + 1)] += s1 * s1;
            table[(size_t)(3 * i + 2)] += s0 * s1;
        }
    if (channels == 2) mm_qc_from_hops(table.data(), H, rate, out);
    if (hops_out && H) memcpy(hops_out, table.data(), (size_t)H * 3 * sizeof(int64_t));
    return MM_OK;
}

int mm_qc_device(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, int32_t rate, int32_t silence_lsb,
                 int32_t min_run, mm_qc *out, int64_t *hops_out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return qc_device(c, d_pcm, kind, frames, channels, rate, silence_lsb, min_run, out, hops_out);
}

int mm_qc_pcm(mm_ctx *c, const void *pcm, int kind, int64_t frames, int channels, int32_t rate, int32_t silence_lsb,
              int32_t min_run, mm_qc *out, int64_t *hops_out) {
    if (!c) return MM_ERR_ARG;
    if (!out || (frames > 0 && !pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = qc_refusal(channels, frames, rate, silence_lsb, min_run)) return set_err(c, MM_ERR_ARG, "QC: %s", why);
    HIPCHK(c, hipSetDevice(c->device));
    char *din;
    RET(pcm_upload(c, "qc_in", pcm, pcm_bytes(kind, frames, channels), &din));
    return qc_device(c, din, kind, frames, channels, rate, silence_lsb, min_run, out, hops_out);
}

int mm_batch_qc_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                       int32_t rate, int32_t silence_lsb, int32_t min_run, mm_qc *out) {
    if (!c) return MM_ERR_ARG;
    RET(batch_qc_check(c, d_pcm, kind, frames, n, channels, rate, silence_lsb, min_run, out));
    HIPCHK(c, hipSetDevice(c->device));
    return batch_qc_device(c, d_pcm, kind, frames, n, channels, rate, silence_lsb, min_run, out);
}

int mm_batch_qc_pcm(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                    int32_t silence_lsb, int32_t min_run, mm_qc *out) {
    if (!c) return MM_ERR_ARG;
    RET(batch_qc_check(c, pcm, kind, frames, n, channels, rate, silence_lsb, min_run, out));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "batch_qc_in", pcm, kind, frames, n, channels, d));
    return batch_qc_device(c, d.data(), kind, frames, n, channels, rate, silence_lsb, min_run, out);
}

int mm_last_qc(mm_ctx *c, int cap, mm_qc *out) {
    if (!c || cap < 0 || (cap > 0 && !out)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->qcs.empty()) return set_err(c, MM_ERR_STATE, "the last call made no QC report");
    const int n = (int)c->qcs.size();
    for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->qcs[(size_t)i];
    return n;
}

}  // extern "C"
