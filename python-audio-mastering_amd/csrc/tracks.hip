// tracks.hip — the level of everything the library levels: a single track, a batch (every
// track to its OWN R 128 target under its own true-peak ceiling) and an album (one gain for all
// tracks) (the level, album and batch entries in include/mastering.h), and the end of a master
// call.  No reference counterpart.
//
// No numerics are defined here.  The decisions are level.hip's level_first / level_step /
// level_record / level_peak_cap, the gain's body, geometry and kept sources its level_gain_span,
// level_gain_geom and level_keep; a pass's ceilings are ceiling.hip's tracks_ceiling and its
// measurement r128.hip's AlbumPass with album.hip's pooled figures.  What is here:
//   level_tracks_gain    the level's gain, its only kernel: level_gain_span over the workgroups
//                        of all tracks (tracks.h), head and tail single samples by a track's
//                        first workgroup; tracks_gain_queue queues it
//   level_groups_device  the level's one driver, the only loop over passes on the device.  It
//                        levels groups of consecutive tracks (LevelGroup: one target, one
//                        ceiling, one gain, one mm_level a group) and each entry only says what
//                        its groups are: mm_level_* and the end of a master call one group of
//                        one track, mm_batch_level_* n groups of one, mm_album_level_* one group
//                        of n
//   mm_op_level_gain     the gain alone, for parity checks
//   finish_delivered     the end of a master call: the level or the ceiling, then the reports
// Every other stage over n tracks (the ceiling, the converter, the reports) is in its own file.

namespace mm {

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

}  // namespace mm

// ======================================================= host
namespace {

// The gain's grid over the tracks of one call, laid out by the destinations and uploaded once.
// The host tables live as long as the call, so the uploads need no synchronisation of their own.
struct GainLayout {
    int n = 0, kind = 0;
    std::vector<int64_t> samples;  // [n]
    std::vector<uint32_t> first;
    const uint32_t *d_first = nullptr;
    // the parameters of the queued launches: untouched until the synchronisation behind them
    std::vector<GainTrack> tab[2];
};

int gain_prepare(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, GainLayout &L) {
    L.n = n;
    L.kind = kind;
    L.samples.resize((size_t)n);
    std::vector<int64_t> wgs((size_t)n);
    for (int t = 0; t < n; ++t) {
        L.samples[(size_t)t] = frames[t] * channels;
        wgs[(size_t)t] = level_gain_geom(d_pcm[t], d_pcm[t], kind, L.samples[(size_t)t]).wgs;  // (by the destination alone)
    }
    L.first.resize((size_t)n + 1);
    tracks_prefix(wgs.data(), n, L.first.data());
    uint32_t *d_first;
    RET(get_buf(c, "tracks_first", (size_t)n + 1, &d_first));
    HIPCHK(c, hipMemcpyAsync(d_first, L.first.data(), ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    L.d_first = d_first;
    return MM_OK;
}

// One segmented gain, queued: every track t with g[t] != 0 from from[t] to to[t] (to[t] at its
// delivered buffer's offset within 16 bytes: the grid was laid out for it) by g[t], the
// statistics folded into st[t], which the caller zeroed on the stream.  `slot`: which of the
// layout's two parameter tables the launch keeps until the next synchronisation.
int tracks_gain_queue(mm_ctx *c, GainLayout &L, int slot, const void *const *from, void *const *to, const int32_t *g,
                      LevelDev *st) {
    const int n = L.n;
    std::vector<GainTrack> &tab = L.tab[slot];
    tab.assign((size_t)n, GainTrack{});
    bool any = false;
    for (int t = 0; t < n; ++t) {
        const int64_t ns = L.samples[(size_t)t];
        if (!g[t] || ns == 0) continue;
        const LevelGeom geo = level_gain_geom(from[t], to[t], L.kind, ns);
        tab[(size_t)t] = GainTrack{from[t], to[t], ns, geo.head, geo.src_vec, (int)g[t], 1};
        any = true;
    }
    if (!any) return MM_OK;
    GainTrack *d_tab;
    RET(get_buf(c, slot ? "tracks_gain_b" : "tracks_gain_a", (size_t)n, &d_tab));
    HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), (size_t)n * sizeof(GainTrack), hipMemcpyHostToDevice, c->stream));
    const dim3 grid(L.first[(size_t)n]), block(LEVEL_THREADS);
    return dispatch_pcm(L.kind, 1, [&](auto, auto t) {  // (pointwise: the samples as one mono line)
        using T = decltype(t);
        return launch(c, "level_tracks_gain", level_tracks_gain_kernel<T>, grid, block, 0, (const GainTrack *)d_tab,
                      L.d_first, n, st);
    });
}

// Refuses what is not a batch to level, before anything is queued.
int batch_level_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                      const double sos[2][5], const int32_t *clu, const int32_t *C, int32_t W) {
    return batch_check(c, pcm, kind, frames, n, channels, C && sos,
                       [&](int t) { return level_bad_args(frames[t], channels, rate, clu[t], C[t], W); });
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
    GainLayout L;
    CeilLayout ceils;
    RET(gain_prepare(c, d_pcm, kind, frames, n, channels, L));
    ceiling_layout(d_pcm, kind, frames, n, channels, ceils);
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
    if (std::any_of(Cs.begin(), Cs.end(), [](int32_t v) { return v != 0; })) RET(tracks_ceiling(c, ceils, Cs.data(), W, ceil));
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
            RET(tracks_ceiling(c, ceils, Cs.data(), W, ce_in.data()));
        }
        HIPCHK(c, hipMemsetAsync(st, 0, N * sizeof(LevelDev), c->stream));
        RET(tracks_gain_queue(c, L, 1, from.data(), to.data(), g.data(), st));
        HIPCHK(c, hipMemcpyAsync(hs.data(), st, N * sizeof(LevelDev), hipMemcpyDeviceToHost, c->stream));  // (behind the next sync)
        if (any_C) {
            std::fill(Cs.begin(), Cs.end(), 0);
            for (int k : active) each(k, [&](size_t t) { Cs[t] = groups[k].C; });
            RET(tracks_ceiling(c, ceils, Cs.data(), W, ceil));
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

}  // namespace

extern "C" {

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
    GainLayout L;
    RET(gain_prepare(c, &dst, kind, &n, 1, 1, L));
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
    RET(batch_level_check(c, d_pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window));
    HIPCHK(c, hipSetDevice(c->device));
    return batch_level_run(c, d_pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window);
}

int mm_batch_level_pcm(mm_ctx *c, void *const *pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                       const double sos[2][5], const int32_t *level_clu, const int32_t *ceiling_q28, int32_t window) {
    if (!c) return MM_ERR_ARG;
    if (!level_clu) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(batch_level_check(c, pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "batch_io", pcm, kind, frames, n, channels, d));
    RET(batch_level_run(c, d.data(), kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window));
    return batch_download(c, pcm, d, kind, frames, n, channels, nullptr);
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
