// tracks.hip — the ceiling, the level's gain and the sample-rate converter over n tracks at
// once, each track with its own parameters, and on them the level of everything the library
// levels: a single track, a batch (every track to its OWN R 128 target under its own true-peak
// ceiling) and an album (one gain for all tracks); and the conversion of a batch to another
// rate (the level, album and batch entries in include/mastering.h).  No reference counterpart.
//
// No numerics are defined here.  Per track the ceiling is mm_ceiling and the level mm_level,
// bit for bit, and the converter mm_resample: the kernels run the single-track bodies
// (ceiling.hip: ceil_need_span, ceil_apply_span, ceil_scale; level.hip: level_gain_span;
// resample.hip: resample_span), the decisions are level.hip's level_first / level_step /
// level_record / level_peak_cap, the gain's geometry and the kept sources its level_gain_geom
// and level_keep, and a ceiling's results ceiling.hip's ceiling_results.  What is
// here is the launch structure: one launch covers the spans of all tracks (tracks.h: a track
// owns a run of workgroups, a workgroup finds its track by a search over at most 257 prefix
// sums, which are uniform reads), so a pass costs the same launches and synchronisations for
// 1 track as for 256, where a call a track pays both n times.
//   ceil_tracks_need   ceil_need over all METER_SPAN spans; track t's r - 1 plane at a
//                      multiple of METER_SPAN of one plane buffer, TP0 into its CeilDev
//   ceil_tracks_apply  ceil_apply over all CEIL_SPAN spans; the early exit, the plane mask and
//                      the R mask are the track's own
//   ceil_tracks_peak   the linked true peak of every track: the need body with the plane
//                      store switched off (a track whose TP0 <= C was not touched: skipped)
//   ceil_tracks_trim   pointwise, the tracks with a residue only, each by its own g_t
//   level_tracks_gain  the level's gain (level_gain_span), its only kernel; head and tail single
//                      samples by a track's first workgroup
//   qc_tracks          the QC report's span kernel (qc.hip: qc_span) over all METER_SPAN spans;
//                      the fold that follows is qc.hip's own, one workgroup a track
//   spec_tracks        the spectrum report's frames kernel (spectrum.hip: spec_frames_group) over
//                      the groups of frames of all tracks (spectrum.h); the fold is spectrum.hip's
//   resample_tracks    the converter (resample.hip: resample_span) over all RS_SPAN spans of
//                      output frames; every position relative to the track's own start, the
//                      statistics into the track's RsDev (mm_batch_resample_*: one memset,
//                      one launch, one read-back whatever n)
// The per-track parameters of a launch are one small array uploaded per pass; a workgroup of
// a track that takes no part exits on one uniform read of it.
//
// The level has one driver, level_groups_device: the only loop over passes on the device.  It
// levels groups of consecutive tracks (LevelGroup: one target, one ceiling, one gain, one
// mm_level a group) and each entry only says what its groups are: mm_level_* and the end of a
// master call one group of one track, mm_batch_level_* n groups of one, mm_album_level_* one
// group of n.  The plain ceiling of one track (ceiling_device) and its reports are not here.
//
// Included last in mastering.hip, after album.hip (album_pass_prepare, album_pass_hops,
// album_reports measure the tracks of a pass; album_upload and batch_download move host
// tracks); tracks.h itself is included before meter.hip, whose grid counts its spans too.  The
// end of a master call, finish_delivered, closes the file: the level or the ceiling, then the
// reports.

namespace mm {

static_assert(TRACKS_METER_SPAN == METER_SPAN && TRACKS_CEIL_SPAN == CEIL_SPAN && TRACKS_RS_SPAN == RS_SPAN &&
                  TRACKS_MAX == MM_ALBUM_TRACKS,
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

// the samples of the span's frames as one mono line
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

struct GainTrack {  // one a track, uploaded once a launch
    const void *src;
    void *dst;
    int64_t n;  // samples
    int head, src_vec, g, active;
};

template <typename T>
__global__ void __launch_bounds__(LEVEL_THREADS) level_tracks_gain_kernel(const GainTrack *tr, const uint32_t *first, int n,
                                                                           LevelDev *st) {
    const int t = tracks_find(first, n, blockIdx.x);
    const GainTrack k = tr[t];
    if (!k.active) return;
    level_gain_span<T>(static_cast<const T *>(k.src), static_cast<T *>(k.dst), k.n, k.head, k.src_vec, k.g, st + t,
                       blockIdx.x - first[t]);
}

struct RsTrack {  // one a track, uploaded once a call
    const void *in;
    void *out;
    int64_t N, Nout;  // the track's own input and output frames
};

// a.N, a.Nout and a.st are the launch's: st[n], and every workgroup takes N and Nout from its track
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

// the QC report's span kernel (qc.hip: qc_span) over the spans of all tracks: a record lands among
// its track's own, a hop piece in its track's own rows, and every frame index is the track's
template <int CH, typename T>
__global__ void __launch_bounds__(QC_THREADS) qc_tracks_kernel(QcLaunch L) {
    const int t = tracks_find(L.first, L.n, blockIdx.x);
    const QcTrack tr = L.tr[t];
    qc_span<CH, T>(static_cast<const T *>(tr.pcm), tr, (int64_t)(blockIdx.x - L.first[t]), L.rate, L.q, L.r,
                   L.rec + L.first[t], L.hops + 3 * tr.hop0);
}

// the spectrum report's frames kernel (spectrum.hip: spec_frames_group) over the groups of all
// tracks: a record lands among its track's own, and every frame index is the track's
template <int CH, typename T>
__global__ void __launch_bounds__(SPEC_THREADS) spec_tracks_kernel(SpecLaunch L) {
    const int t = tracks_find(L.first, L.n, blockIdx.x);
    const SpecTrack tr = L.tr[t];
    spec_frames_group<CH, T>(static_cast<const T *>(tr.pcm), tr.F, (int64_t)(blockIdx.x - L.first[t]), L.tab,
                             L.rec + (size_t)blockIdx.x * SPEC_REC);
}

}  // namespace mm

// ======================================================= host
namespace {

// The tracks of one call and the grids over them, laid out and uploaded once.  The host
// tables live as long as the call, so the uploads need no synchronisation of their own.
struct TracksLayout {
    int n = 0, kind = 0, channels = 0;
    std::vector<TrackDev> tr;
    std::vector<uint32_t> first_need, first_apply, first_gain;
    TracksArgs a{};
    const uint32_t *d_first_gain = nullptr;
    // the parameters of the queued launches: untouched until the synchronisation behind them
    std::vector<TrackPar> par, par_trim;
    std::vector<GainTrack> gain[2];
};

int tracks_prepare(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, TracksLayout &L) {
    L.n = n;
    L.kind = kind;
    L.channels = channels;
    L.tr.resize((size_t)n);
    std::vector<int64_t> need((size_t)n), apply((size_t)n), gain((size_t)n);
    for (int t = 0; t < n; ++t) {
        L.tr[(size_t)t] = TrackDev{d_pcm[t], frames[t]};
        need[(size_t)t] = tracks_need_spans(frames[t]);
        apply[(size_t)t] = tracks_apply_spans(frames[t]);
        gain[(size_t)t] = level_gain_geom(d_pcm[t], d_pcm[t], kind, frames[t] * channels).wgs;  // (by the destination alone)
    }
    L.first_need.resize((size_t)n + 1);
    L.first_apply.resize((size_t)n + 1);
    L.first_gain.resize((size_t)n + 1);
    tracks_prefix(need.data(), n, L.first_need.data());
    tracks_prefix(apply.data(), n, L.first_apply.data());
    tracks_prefix(gain.data(), n, L.first_gain.data());
    TrackDev *d_tr;
    uint32_t *d_first;
    RET(get_buf(c, "tracks_tr", (size_t)n, &d_tr));
    RET(get_buf(c, "tracks_first", 3 * ((size_t)n + 1), &d_first));
    RET(get_buf(c, "tracks_r", (size_t)std::max<int64_t>(1, tracks_plane_total(L.first_need.data(), n)), &L.a.plane));
    RET(get_buf(c, "tracks_st", (size_t)n, &L.a.st));
    RET(get_buf(c, "tracks_peak", (size_t)n, &L.a.peak));
    const size_t fb = ((size_t)n + 1) * sizeof(uint32_t);
    HIPCHK(c, hipMemcpyAsync(d_tr, L.tr.data(), (size_t)n * sizeof(TrackDev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_first, L.first_need.data(), fb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_first + n + 1, L.first_apply.data(), fb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_first + 2 * (n + 1), L.first_gain.data(), fb, hipMemcpyHostToDevice, c->stream));
    L.a.tr = d_tr;
    L.a.first_need = d_first;
    L.a.first_apply = d_first + n + 1;
    L.d_first_gain = d_first + 2 * (n + 1);
    L.a.n = n;
    return MM_OK;
}

// The segmented ceiling, in place: every track t with Cs[t] != 0 held under Cs[t], out[t]
// filled as ceiling_device fills it; the other tracks and their out[t] are not touched.
// Need, apply and the peak behind one synchronisation; the trims and their peak behind one
// more, when a track is left with a residue.  Synchronous on return.
int tracks_ceiling(mm_ctx *c, TracksLayout &L, const int32_t *Cs, int32_t W, mm_ceiling *out) {
    const int n = L.n;
    bool any = false;
    L.par.assign((size_t)n, TrackPar{});
    for (int t = 0; t < n; ++t) {
        if (!Cs[t]) continue;
        ceiling_clear(&out[t], L.tr[(size_t)t].frames, L.channels, Cs[t], W);
        if (L.tr[(size_t)t].frames == 0) continue;
        L.par[(size_t)t] = TrackPar{Cs[t], Cs[t] - CEIL_GUARD, 0, 1};
        any = true;
    }
    if (!any) {  // nothing to queue; the layout's uploads may still be on the stream
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MM_OK;
    }
    TrackPar *d_par, *d_par_trim;
    RET(get_buf(c, "tracks_par", (size_t)n, &d_par));
    RET(get_buf(c, "tracks_par_trim", (size_t)n, &d_par_trim));
    HIPCHK(c, hipMemcpyAsync(d_par, L.par.data(), (size_t)n * sizeof(TrackPar), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(L.a.st, 0, (size_t)n * sizeof(CeilDev), c->stream));
    HIPCHK(c, hipMemsetAsync(L.a.peak, 0, (size_t)n * sizeof(unsigned), c->stream));
    TracksArgs a = L.a;
    a.par = d_par;
    a.W = W;
    a.rcp = (unsigned)(((uint64_t)1 << 32) / (uint64_t)(2 * W + 1));
    const dim3 gn(L.first_need[(size_t)n]), bn(METER_THREADS), ga(L.first_apply[(size_t)n]), ba(CEIL_THREADS);
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
    std::vector<CeilDev> hs((size_t)n);
    std::vector<unsigned> hp((size_t)n);
    HIPCHK(c, hipMemcpyAsync(hs.data(), L.a.st, (size_t)n * sizeof(CeilDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hp.data(), L.a.peak, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bool trim = false;
    L.par_trim.assign((size_t)n, TrackPar{});
    for (int t = 0; t < n; ++t) {
        if (!L.par[(size_t)t].active) continue;
        const int32_t C = Cs[t];
        mm_ceiling *o = &out[t];
        const int32_t tp0 = (int32_t)hs[(size_t)t].tp0;
        ceiling_results(o, hs[(size_t)t], tp0 <= C ? tp0 : (int32_t)hp[(size_t)t]);  // (untouched: ceil_tracks_peak skipped it)
        if (o->tp_limited_q28 > C) {  // the residue: one static trim
            const int gt = ceiling_trim_gain(C, o->tp_limited_q28);
            L.par_trim[(size_t)t] = TrackPar{C, C - CEIL_GUARD, gt, 1};
            o->trim_q16 = gt;
            trim = true;
        }
    }
    if (trim) {
        HIPCHK(c, hipMemcpyAsync(d_par_trim, L.par_trim.data(), (size_t)n * sizeof(TrackPar), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(L.a.peak, 0, (size_t)n * sizeof(unsigned), c->stream));
        a.par = d_par_trim;
        RET(dispatch_pcm(L.kind, 1, [&](auto, auto t) {
            using T = decltype(t);
            return launch(c, "ceil_tracks_trim", ceil_tracks_trim_kernel<T>, ga, ba, 0, a, L.channels);
        }));
        RET(peak());
        HIPCHK(c, hipMemcpyAsync(hp.data(), L.a.peak, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int t = 0; t < n; ++t)
            if (L.par_trim[(size_t)t].active) out[t].tp_out_q28 = (int32_t)hp[(size_t)t];
    }
    resolve_events(c);
    return MM_OK;
}

// One segmented gain, queued: every track t with g[t] != 0 from from[t] to to[t] (to[t] at its
// delivered buffer's offset within 16 bytes: the grid was laid out for it) by g[t], the
// statistics folded into st[t], which the caller zeroed on the stream.  `slot`: which of the
// layout's two parameter tables the launch keeps until the next synchronisation.
int tracks_gain_queue(mm_ctx *c, TracksLayout &L, int slot, const void *const *from, void *const *to, const int32_t *g,
                      LevelDev *st) {
    const int n = L.n;
    std::vector<GainTrack> &tab = L.gain[slot];
    tab.assign((size_t)n, GainTrack{});
    bool any = false;
    for (int t = 0; t < n; ++t) {
        const int64_t ns = L.tr[(size_t)t].frames * L.channels;
        if (!g[t] || ns == 0) continue;
        const LevelGeom geo = level_gain_geom(from[t], to[t], L.kind, ns);
        tab[(size_t)t] = GainTrack{from[t], to[t], ns, geo.head, geo.src_vec, (int)g[t], 1};
        any = true;
    }
    if (!any) return MM_OK;
    GainTrack *d_tab;
    RET(get_buf(c, slot ? "tracks_gain_b" : "tracks_gain_a", (size_t)n, &d_tab));
    HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), (size_t)n * sizeof(GainTrack), hipMemcpyHostToDevice, c->stream));
    const dim3 grid(L.first_gain[(size_t)n]), block(LEVEL_THREADS);
    return dispatch_pcm(L.kind, 1, [&](auto, auto t) {  // (pointwise: the samples as one mono line)
        using T = decltype(t);
        return launch(c, "level_tracks_gain", level_tracks_gain_kernel<T>, grid, block, 0, (const GainTrack *)d_tab,
                      L.d_first_gain, n, st);
    });
}

// Refuses what is not a batch (MM_ERR_ARG, the sentence in mm_last_error names the track),
// before anything is queued.  clu == null: a ceiling alone, which every track then has.
int batch_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                const double sos[2][5], const int32_t *clu, const int32_t *C, int32_t W) {
    if (n < 1 || n > MM_ALBUM_TRACKS) return set_err(c, MM_ERR_ARG, "batch: %d tracks out of range [1, %d]", n, MM_ALBUM_TRACKS);
    if (!pcm || !frames || !C || (clu && !sos)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    int64_t total = 0;
    for (int t = 0; t < n; ++t) {
        const char *why = clu ? level_bad_args(frames[t], channels, rate, clu[t], C[t], W) : ceiling_bad_args(frames[t], channels, C[t], W);
        if (why) return set_err(c, MM_ERR_ARG, "batch: track %d: %s", t, why);
        if (frames[t] > 0 && !pcm[t]) return set_err(c, MM_ERR_ARG, "batch: track %d: null pointer", t);
        total += frames[t];
        if (total >= R128_MAX_FRAMES) return set_err(c, MM_ERR_ARG, "batch: track %d: 2^31 frames or more in all", t);
    }
    return MM_OK;
}

// A group: `count` consecutive tracks of the call from `first` that share one target, one
// ceiling, one gain and one mm_level record.  A single track is one group of one track, a
// batch n groups of one, an album one group of n.
struct LevelGroup {
    int first, count;
    int32_t clu, C;
};

// The level of the groups of one call on device-resident tracks, in place (synchronous on
// return): the device's one loop over passes.  All groups run level.hip's rule in lockstep, a
// pass at a time, every launch over the tracks of all groups still active, and a group leaves
// the passes when its status is decided.  A group's loudness is the pooled figure of its own
// tracks (album.hip), which for a group of one is the track's own.  Arguments already checked.
// lv, pooled [ng]: every group's record and pooled report; ceil, rep [n]: every track's last
// ceiling at C (a cleared entry where its group has none) and the report of what it delivers.
int level_groups_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                        const double sos[2][5], const LevelGroup *groups, int ng, int32_t W, mm_level *lv, mm_r128 *pooled,
                        mm_ceiling *ceil, mm_r128 *rep) {
    const size_t N = (size_t)n;
    auto each = [&](int k, auto &&f) {  // f(t) for the tracks of group k
        for (int t = groups[k].first; t < groups[k].first + groups[k].count; ++t) f((size_t)t);
    };
    for (int k = 0; k < ng; ++k) {
        int64_t total = 0;
        each(k, [&](size_t t) {
            total += frames[t];
            memset(&ceil[t], 0, sizeof(mm_ceiling));
            ceil[t].channels = channels;
        });
        level_clear(&lv[k], total, channels, rate, groups[k].clu, groups[k].C, W);
    }
    TracksLayout L;
    RET(tracks_prepare(c, d_pcm, kind, frames, n, channels, L));
    // one segmented measurement of the groups `set`, each whole: pooled and rep of their tracks.
    // The pass is laid out for `measured` and stays while the next set is the same one.
    AlbumPass pass;
    std::vector<int> measured;
    std::vector<int64_t> f;
    auto measure = [&](const std::vector<int> &set) -> int {
        if (set != measured) {
            std::vector<const void *> p;
            f.clear();
            for (int k : set)
                each(k, [&](size_t t) {
                    p.push_back(d_pcm[t]);
                    f.push_back(frames[t]);
                });
            RET(album_pass_prepare(c, p.data(), kind, f.data(), (int)p.size(), channels, rate, sos, pass));
            measured = set;
        }
        std::vector<double> e;
        RET(album_pass_hops(c, pass, e));
        size_t i = 0;
        const double *ek = e.data();
        for (int k : set) {
            album_reports(ek, &pass.hops[i], &f[i], groups[k].count, rate, channels, &pooled[k], rep + groups[k].first);
            i += (size_t)groups[k].count;
            ek += pooled[k].hops;
        }
        return MM_OK;
    };
    std::vector<int> active((size_t)ng), quiet, again;
    for (int k = 0; k < ng; ++k) active[(size_t)k] = k;
    RET(measure(active));
    active.clear();
    std::vector<int32_t> Cs(N, 0);
    for (int k = 0; k < ng; ++k) {
        lv[k].source_lufs = pooled[k].integrated;
        if (std::isfinite(pooled[k].integrated)) {
            active.push_back(k);
            continue;
        }
        quiet.push_back(k);  // no window, or silence: its tracks only get their ceiling
        each(k, [&](size_t t) { Cs[t] = groups[k].C; });
    }
    if (std::any_of(Cs.begin(), Cs.end(), [](int32_t v) { return v != 0; })) RET(tracks_ceiling(c, L, Cs.data(), W, ceil));
    for (int k : quiet) {
        const int32_t C = groups[k].C;
        bool touched = false;
        each(k, [&](size_t t) { touched |= C && ceil[t].tp_in_q28 > C; });
        level_unmeasurable(&lv[k], ceil + groups[k].first, C ? groups[k].count : 0);
        if (touched) again.push_back(k);
    }
    if (!again.empty()) RET(measure(again));  // the reports describe what is delivered
    if (active.empty()) {
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the layout's uploads, where nothing else was queued)
        return MM_OK;
    }
    std::vector<char *> kept;
    RET(level_keep(c, "level_src", d_pcm, kind, frames, n, channels, kept));
    std::vector<const void *> src(kept.begin(), kept.end()), from(N, nullptr);
    std::vector<void *> keep_at(kept.begin(), kept.end()), to(N, nullptr);
    LevelDev *st, *st_copy;
    std::vector<LevelDev> hs(N), hs_copy(N);
    RET(get_buf(c, "level_res", N, &st));
    RET(get_buf(c, "level_res_copy", N, &st_copy));
    // the copies through the kernel at ONE (the identity), all tracks in one launch: they bring
    // max |s| of every track, which caps the gain of a group without a ceiling
    std::vector<int32_t> g(N, 0), g_copy(N, 0), next_g((size_t)ng, 0), g_peak((size_t)ng, LEVEL_GMAX);
    for (int k : active)
        each(k, [&](size_t t) {
            g_copy[t] = LEVEL_ONE;
            from[t] = d_pcm[t];
        });
    HIPCHK(c, hipMemsetAsync(st_copy, 0, N * sizeof(LevelDev), c->stream));
    RET(tracks_gain_queue(c, L, 0, from.data(), keep_at.data(), g_copy.data(), st_copy));
    HIPCHK(c, hipMemcpyAsync(hs_copy.data(), st_copy, N * sizeof(LevelDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k : active) {
        unsigned peak = 0;
        each(k, [&](size_t t) { peak = std::max(peak, hs_copy[t].peak); });
        if (!groups[k].C) g_peak[(size_t)k] = level_peak_cap((int32_t)peak);
        next_g[(size_t)k] = level_first(&lv[k]);
    }
    std::vector<LevelStep> step((size_t)ng);
    std::vector<mm_ceiling> ce_in(N);
    while (!active.empty()) {
        bool any_boost = false, any_C = false;
        std::fill(Cs.begin(), Cs.end(), 0);
        std::fill(g.begin(), g.end(), 0);
        std::fill(g_copy.begin(), g_copy.end(), 0);
        for (int k : active) {
            const LevelStep &s = step[(size_t)k] = level_step(groups[k].C, next_g[(size_t)k], g_peak[(size_t)k]);
            each(k, [&](size_t t) {
                g[t] = s.g;
                from[t] = s.boost ? d_pcm[t] : src[t];
                to[t] = d_pcm[t];
                if (s.boost) {
                    g_copy[t] = LEVEL_ONE;
                    Cs[t] = s.C_inner;
                }
            });
            any_boost |= s.boost;
            any_C |= groups[k].C != 0;
        }
        if (any_boost) {  // source -> delivered (the identity again), then the inner ceilings
            HIPCHK(c, hipMemsetAsync(st_copy, 0, N * sizeof(LevelDev), c->stream));
            RET(tracks_gain_queue(c, L, 0, src.data(), to.data(), g_copy.data(), st_copy));
            RET(tracks_ceiling(c, L, Cs.data(), W, ce_in.data()));
        }
        HIPCHK(c, hipMemsetAsync(st, 0, N * sizeof(LevelDev), c->stream));
        RET(tracks_gain_queue(c, L, 1, from.data(), to.data(), g.data(), st));
        HIPCHK(c, hipMemcpyAsync(hs.data(), st, N * sizeof(LevelDev), hipMemcpyDeviceToHost, c->stream));  // (behind the next sync)
        if (any_C) {
            std::fill(Cs.begin(), Cs.end(), 0);
            for (int k : active) each(k, [&](size_t t) { Cs[t] = groups[k].C; });
            RET(tracks_ceiling(c, L, Cs.data(), W, ceil));
        }
        RET(measure(active));
        std::vector<int> next;
        for (int k : active) {
            int64_t clipped = 0;
            each(k, [&](size_t t) { clipped += (int64_t)hs[t].clipped; });
            next_g[(size_t)k] = level_record(&lv[k], step[(size_t)k], pooled[k].integrated, clipped, ceil + groups[k].first,
                                             ce_in.data() + groups[k].first, groups[k].C ? groups[k].count : 0);
            if (next_g[(size_t)k]) next.push_back(k);
        }
        active.swap(next);
    }
    return MM_OK;
}

// The level of one track, in place (synchronous on return): one group of one.  ceil_out (may be
// null) receives the track's last ceiling at C when C != 0.
int level_track_device(mm_ctx *c, void *d_pcm, int kind, int64_t frames, int channels, int32_t rate, const double sos[2][5],
                       int32_t level_clu, int32_t C, int32_t W, mm_level *out, mm_ceiling *ceil_out) {
    if (!c || !out || !sos || (frames > 0 && !d_pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = level_bad_args(frames, channels, rate, level_clu, C, W)) return set_err(c, MM_ERR_ARG, "level: %s", why);
    const LevelGroup one{0, 1, level_clu, C};
    mm_r128 pooled, rep;
    mm_ceiling ce;
    RET(level_groups_device(c, &d_pcm, kind, &frames, 1, channels, rate, sos, &one, 1, W, out, &pooled, &ce, &rep));
    if (C && ceil_out) *ceil_out = ce;
    return MM_OK;
}

// The level of an album: one group of all n tracks.  Arguments already checked.  The results go
// behind mm_last_album, mm_last_r128 and mm_last_ceilings.
int album_level_run(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                    const double sos[2][5], int32_t level_clu, int32_t C, int32_t W) {
    results_reset(c);
    const LevelGroup all{0, n, level_clu, C};
    mm_level lv;
    mm_r128 pooled;
    std::vector<mm_ceiling> ceil((size_t)n);
    std::vector<mm_r128> rep((size_t)n);
    RET(level_groups_device(c, d_pcm, kind, frames, n, channels, rate, sos, &all, 1, W, &lv, &pooled, ceil.data(), rep.data()));
    c->r128s = rep;
    if (C) c->ceilings = ceil;
    c->albums.assign(1, lv);
    c->album_r128s.assign(1, pooled);
    return MM_OK;
}

// The level of a batch: n groups of one track, every track to its own target under its own
// ceiling.  Arguments already checked.  The results go behind mm_last_levels, mm_last_ceilings
// and mm_last_r128.
int batch_level_run(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                    const double sos[2][5], const int32_t *clu, const int32_t *C, int32_t W) {
    results_reset(c);
    const size_t N = (size_t)n;
    std::vector<LevelGroup> groups(N);
    for (int t = 0; t < n; ++t) groups[(size_t)t] = LevelGroup{t, 1, clu[t], C[t]};
    std::vector<mm_level> lv(N);
    std::vector<mm_ceiling> ceil(N);
    std::vector<mm_r128> pooled(N), rep(N);
    RET(level_groups_device(c, d_pcm, kind, frames, n, channels, rate, sos, groups.data(), n, W, lv.data(), pooled.data(),
                            ceil.data(), rep.data()));
    c->levels = lv;
    if (std::any_of(C, C + n, [](int32_t v) { return v != 0; })) c->ceilings = ceil;
    c->r128s = rep;
    return MM_OK;
}

int batch_ceiling_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                         const int32_t *C, int32_t W, mm_ceiling *out) {
    TracksLayout L;
    RET(tracks_prepare(c, d_pcm, kind, frames, n, channels, L));
    return tracks_ceiling(c, L, C, W, out);
}

// Refuses what is not a batch to convert (MM_ERR_ARG, the sentence names the track), before
// anything is queued.  The table itself is checked where it is uploaded (resample_taps_device),
// which queues nothing before it has refused.
int batch_resample_check(mm_ctx *c, const void *const *in, int kind, const int64_t *frames, int n, int channels,
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
// one memset of the n result blocks, one launch over the spans of all tracks, one read-back.
// Arguments already checked, D the device copy of the taps (resample_taps_device).  The host
// tables live until the synchronisation at the end.
int batch_resample_device(mm_ctx *c, const void *const *d_in, int kind, const int64_t *frames, int n, int channels,
                          const mm_resampler *rs, const int32_t *D, void *const *d_out, mm_resample *out) {
    RsArgs a{};
    a.D = D;
    const size_t N = (size_t)n;
    std::vector<RsTrack> tr(N);
    std::vector<int64_t> wgs(N);
    std::vector<uint32_t> first(N + 1);
    for (int t = 0; t < n; ++t) {
        resample_clear(&out[t], frames[t], channels, rs);
        tr[(size_t)t] = RsTrack{d_in[t], d_out[t], frames[t], out[t].frames_out};
        wgs[(size_t)t] = tracks_resample_spans(out[t].frames_out);
    }
    const uint32_t grid = tracks_prefix(wgs.data(), n, first.data());
    if (grid == 0) return MM_OK;  // no track has frames
    RsTrack *d_tr;
    uint32_t *d_first;
    RET(get_buf(c, "rs_tracks", N, &d_tr));
    RET(get_buf(c, "rs_tracks_first", N + 1, &d_first));
    RET(get_buf(c, "rs_tracks_res", N, &a.st));
    HIPCHK(c, hipMemcpyAsync(d_tr, tr.data(), N * sizeof(RsTrack), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_first, first.data(), (N + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(a.st, 0, N * sizeof(RsDev), c->stream));
    a.L = rs->L;
    a.M = rs->M;
    a.K = rs->K;
    a.sub = resample_sub(rs);
    RET(dispatch_pcm(kind, channels, [&](auto ch, auto t) {
        using T = decltype(t);
        return launch(c, "resample_tracks", resample_tracks_kernel<ch, T>, dim3(grid), dim3(RS_THREADS), 0,
                      (const RsTrack *)d_tr, (const uint32_t *)d_first, n, a);
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

// Refuses what is not a batch to check (MM_ERR_ARG, the sentence names the track), before
// anything is queued.
int batch_qc_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int rate, int q,
                   int r, const mm_qc *out) {
    if (n < 1 || n > MM_ALBUM_TRACKS) return set_err(c, MM_ERR_ARG, "batch: %d tracks out of range [1, %d]", n, MM_ALBUM_TRACKS);
    if (!pcm || !frames || !out) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    int64_t total = 0;
    for (int t = 0; t < n; ++t) {
        if (const char *why = qc_refusal(channels, frames[t], rate, q, r)) return set_err(c, MM_ERR_ARG, "batch: track %d: %s", t, why);
        if (frames[t] > 0 && !pcm[t]) return set_err(c, MM_ERR_ARG, "batch: track %d: null pointer", t);
        total += frames[t];
        if (total >= QC_MAX_FRAMES) return set_err(c, MM_ERR_ARG, "batch: track %d: 2^31 frames or more in all", t);
    }
    return MM_OK;
}

// The QC reports of n checked device-resident tracks (synchronous on return): qc.hip's qc_run
// with the span launch over all tracks.  Only c->qcs is set: the levels, ceilings and R 128
// reports of the context's last call stay.
int batch_qc_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate, int q,
                    int r, mm_qc *out) {
    RET(qc_run(c, d_pcm, frames, n, channels, rate, q, r, out, nullptr, [&](const QcLaunch &L, uint32_t grid) {
        return dispatch_pcm(kind, channels, [&](auto ch, auto t) {
            using T = decltype(t);
            return launch(c, "qc_tracks", qc_tracks_kernel<ch, T>, dim3(grid), dim3(QC_THREADS), 0, L);
        });
    }));
    c->qcs.assign(out, out + n);
    return MM_OK;
}

// Refuses what is not a batch to take the spectra of, as batch_qc_check does.
int batch_spectrum_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                         const mm_spectrum *out) {
    if (n < 1 || n > MM_ALBUM_TRACKS) return set_err(c, MM_ERR_ARG, "batch: %d tracks out of range [1, %d]", n, MM_ALBUM_TRACKS);
    if (!pcm || !frames || !out) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    int64_t total = 0;
    for (int t = 0; t < n; ++t) {
        if (const char *why = spectrum_refusal(channels, frames[t], rate)) return set_err(c, MM_ERR_ARG, "batch: track %d: %s", t, why);
        if (frames[t] > 0 && !pcm[t]) return set_err(c, MM_ERR_ARG, "batch: track %d: null pointer", t);
        total += frames[t];
        if (total >= SPEC_MAX_FRAMES) return set_err(c, MM_ERR_ARG, "batch: track %d: 2^31 frames or more in all", t);
    }
    return MM_OK;
}

// The spectrum reports of n checked device-resident tracks (synchronous on return):
// spectrum.hip's spectrum_run with the frames launch over all tracks.  Only c->spectra and the
// bin tables are set: the other results of the context's last call stay.
int batch_spectrum_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                          mm_spectrum *out) {
    std::vector<std::vector<double>> bins;
    RET(spectrum_run(c, d_pcm, frames, n, channels, rate, out, bins, [&](const SpecLaunch &L, uint32_t grid) {
        return dispatch_pcm(kind, channels, [&](auto ch, auto t) {
            using T = decltype(t);
            return launch(c, "spec_tracks", spec_tracks_kernel<ch, T>, dim3(grid), dim3(SPEC_THREADS), 0, L);
        });
    }));
    c->spectra.assign(out, out + n);
    c->spectrum_bins.swap(bins);
    return MM_OK;
}

}  // namespace

extern "C" {

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

int mm_batch_spectrum_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                             int32_t rate, mm_spectrum *out) {
    if (!c) return MM_ERR_ARG;
    RET(batch_spectrum_check(c, d_pcm, kind, frames, n, channels, rate, out));
    HIPCHK(c, hipSetDevice(c->device));
    return batch_spectrum_device(c, d_pcm, kind, frames, n, channels, rate, out);
}

int mm_batch_spectrum_pcm(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                          int32_t rate, mm_spectrum *out) {
    if (!c) return MM_ERR_ARG;
    RET(batch_spectrum_check(c, pcm, kind, frames, n, channels, rate, out));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "batch_spec_in", pcm, kind, frames, n, channels, d));
    return batch_spectrum_device(c, d.data(), kind, frames, n, channels, rate, out);
}

int mm_batch_ceiling_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                            const int32_t *ceiling_q28, int32_t window, mm_ceiling *out) {
    if (!c) return MM_ERR_ARG;
    if (!out) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(batch_check(c, d_pcm, kind, frames, n, channels, 0, nullptr, nullptr, ceiling_q28, window));
    HIPCHK(c, hipSetDevice(c->device));
    return batch_ceiling_device(c, d_pcm, kind, frames, n, channels, ceiling_q28, window, out);
}

int mm_batch_ceiling_pcm(mm_ctx *c, void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                         const int32_t *ceiling_q28, int32_t window, mm_ceiling *out) {
    if (!c) return MM_ERR_ARG;
    if (!out) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(batch_check(c, pcm, kind, frames, n, channels, 0, nullptr, nullptr, ceiling_q28, window));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "batch_io", pcm, kind, frames, n, channels, d));
    RET(batch_ceiling_device(c, d.data(), kind, frames, n, channels, ceiling_q28, window, out));
    std::vector<char> pick((size_t)n);  // (an untouched track is not copied back)
    for (int t = 0; t < n; ++t) pick[(size_t)t] = out[t].tp_in_q28 > ceiling_q28[t];
    return batch_download(c, pcm, d, kind, frames, n, channels, pick.data());
}

int mm_level_device(mm_ctx *c, void *d_pcm, int kind, int64_t frames, int channels, int32_t rate, const double sos[2][5],
                    int32_t level_clu, int32_t ceiling_q28, int32_t window, mm_level *out, mm_ceiling *ceil_out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return level_track_device(c, d_pcm, kind, frames, channels, rate, sos, level_clu, ceiling_q28, window, out, ceil_out);
}

int mm_level_pcm(mm_ctx *c, void *pcm, int kind, int64_t frames, int channels, int32_t rate, const double sos[2][5],
                 int32_t level_clu, int32_t ceiling_q28, int32_t window, mm_level *out, mm_ceiling *ceil_out) {
    if (!c) return MM_ERR_ARG;
    if (!out || !sos || (frames > 0 && !pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = level_bad_args(frames, channels, rate, level_clu, ceiling_q28, window))
        return set_err(c, MM_ERR_ARG, "level: %s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = pcm_bytes(kind, frames, channels);
    char *dio;
    RET(pcm_upload(c, "level_io", pcm, bytes, &dio));
    RET(level_track_device(c, dio, kind, frames, channels, rate, sos, level_clu, ceiling_q28, window, out, ceil_out));
    return pcm_download(c, pcm, dio, bytes);
}

// The gain alone on host buffers (a per-stage operator, for parity checks): n samples of `kind`
// by g, through device views that start src_off and dst_off samples (0 .. 7) past a 16-byte
// boundary; dst_off < 0: in place (src == dst).  The segmented launch over one mono track.
int mm_op_level_gain(mm_ctx *c, const void *in, int kind, int64_t n, int src_off, int dst_off, int32_t g, void *out_pcm,
                     int64_t *clipped, int32_t *peak) {
    if (!c) return MM_ERR_ARG;
    if (!clipped || !peak || (n > 0 && (!in || !out_pcm)) || n < 0 || n >= (int64_t)1 << 32 || src_off < 0 || src_off > 7 ||
        dst_off > 7)
        return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (g < LEVEL_GMIN || g > LEVEL_GMAX) return set_err(c, MM_ERR_ARG, "level: gain_q16 out of range [2^8, 2^21]");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t sb = pcm_sample_bytes(kind), bytes = (size_t)n * sb;
    char *a, *b;
    LevelDev *st, hs{};
    RET(get_buf(c, "level_op_a", bytes + 64, &a));
    RET(get_buf(c, "level_op_b", bytes + 64, &b));
    RET(get_buf(c, "level_res", 1, &st));
    const void *src = a + (size_t)src_off * sb;
    void *dst = dst_off < 0 ? const_cast<void *>(src) : b + (size_t)dst_off * sb;
    if (bytes) HIPCHK(c, hipMemcpyAsync(const_cast<void *>(src), in, bytes, hipMemcpyHostToDevice, c->stream));
    TracksLayout L;
    RET(tracks_prepare(c, &dst, kind, &n, 1, 1, L));
    HIPCHK(c, hipMemsetAsync(st, 0, sizeof(LevelDev), c->stream));
    RET(tracks_gain_queue(c, L, 0, &src, &dst, &g, st));
    HIPCHK(c, hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    RET(pcm_download(c, out_pcm, static_cast<const char *>(dst), bytes));
    resolve_events(c);
    *clipped = (int64_t)hs.clipped;
    *peak = (int32_t)hs.peak;
    return MM_OK;
}

int mm_album_level_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                          const double sos[2][5], int32_t level_clu, int32_t ceiling_q28, int32_t window) {
    if (!c) return MM_ERR_ARG;
    RET(album_check(c, d_pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window, true));
    HIPCHK(c, hipSetDevice(c->device));
    return album_level_run(c, d_pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window);
}

int mm_album_level_pcm(mm_ctx *c, void *const *pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                       const double sos[2][5], int32_t level_clu, int32_t ceiling_q28, int32_t window) {
    if (!c) return MM_ERR_ARG;
    RET(album_check(c, pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window, true));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "album_io", pcm, kind, frames, n, channels, d));
    RET(album_level_run(c, d.data(), kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window));
    return batch_download(c, pcm, d, kind, frames, n, channels, nullptr);
}

int mm_batch_level_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                          const double sos[2][5], const int32_t *level_clu, const int32_t *ceiling_q28, int32_t window) {
    if (!c) return MM_ERR_ARG;
    if (!level_clu) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(batch_check(c, d_pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window));
    HIPCHK(c, hipSetDevice(c->device));
    return batch_level_run(c, d_pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window);
}

int mm_batch_level_pcm(mm_ctx *c, void *const *pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                       const double sos[2][5], const int32_t *level_clu, const int32_t *ceiling_q28, int32_t window) {
    if (!c) return MM_ERR_ARG;
    if (!level_clu) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(batch_check(c, pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "batch_io", pcm, kind, frames, n, channels, d));
    RET(batch_level_run(c, d.data(), kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window));
    return batch_download(c, pcm, d, kind, frames, n, channels, nullptr);
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

}  // extern "C"

// The end of a master call for delivered buffer i (results_reset sized the call's results):
// the ceiling, or with a loudness target (level_clu, a delivery's) the level that contains
// it, then the reports, which so measure what is delivered: bit 0 of meter_on the
// meter, bit 1 the R 128 report (r128.hip) with the K-weighting sections and the rate of
// `loud`, which the level takes too, bit 2 the QC report (qc.hip) at that rate, bit 3 the
// spectrum report (spectrum.hip) at that rate.  A track that did not ask for what another track of the
// call asked for leaves a cleared entry.
static int finish_delivered(mm_ctx *c, void *d_out, int kind, int64_t frames, int channels, int i, int32_t ceiling_q28,
                            int32_t window, int meter_on, const mm_job *loud, int32_t level_clu) {
    if (level_clu) {
        if (!loud || loud->kweight.nsec != 2)
            return set_err(c, MM_ERR_ARG, "a loudness target needs a job with the K-weighting sections (kweight.sos)");
        RET(level_track_device(c, d_out, kind, frames, channels, loud->rate, loud->kweight.sos, level_clu, ceiling_q28, window,
                               &c->levels[(size_t)i], ceiling_q28 ? &c->ceilings[(size_t)i] : nullptr));
    } else if (ceiling_q28) RET(ceiling_device(c, d_out, kind, frames, channels, ceiling_q28, window, &c->ceilings[(size_t)i]));
    else if (!c->ceilings.empty()) c->ceilings[(size_t)i].channels = channels;
    if (meter_on & MM_REPORT_METER) RET(meter_device(c, d_out, kind, frames, channels, loud, &c->meters[(size_t)i]));
    else if (!c->meters.empty()) meter_clear(&c->meters[(size_t)i], 0, channels);
    if (meter_on & MM_REPORT_R128) {
        if (!loud || loud->kweight.nsec != 2)
            return set_err(c, MM_ERR_ARG, "the R 128 report needs a job with the K-weighting sections (kweight.sos)");
        RET(r128_device(c, d_out, kind, frames, channels, loud->rate, loud->kweight.sos, &c->r128s[(size_t)i]));
    } else if (!c->r128s.empty()) {
        r128_clear(&c->r128s[(size_t)i], 0, channels, 0);
    }
    if (meter_on & MM_REPORT_QC) {
        if (!loud) return set_err(c, MM_ERR_ARG, "the QC report needs a job with the rate of the delivered signal");
        RET(qc_device(c, d_out, kind, frames, channels, loud->rate, QC_REPORT_LSB, QC_REPORT_RUN, &c->qcs[(size_t)i], nullptr));
    } else if (!c->qcs.empty()) {
        qc_clear(&c->qcs[(size_t)i], 0, channels, 0, QC_REPORT_LSB, QC_REPORT_RUN);
    }
    if (meter_on & MM_REPORT_SPECTRUM) {
        if (!loud) return set_err(c, MM_ERR_ARG, "the spectrum report needs a job with the rate of the delivered signal");
        RET(spectrum_device(c, d_out, kind, frames, channels, loud->rate, &c->spectra[(size_t)i], &c->spectrum_bins[(size_t)i]));
    } else if (!c->spectra.empty()) {
        spectrum_clear(&c->spectra[(size_t)i], channels);
    }
    return MM_OK;
}
