// album.hip — an album levelled as one programme: ONE static gain for all its tracks, which
// makes the album read the R 128 target with every track held under the true-peak ceiling
// (the album R 128 figures and the album level in include/mastering.h).  Loudness differences
// between the tracks are kept.  No reference counterpart.
//
// Two things live here.  The pooled figures: r128.hip's measuring pass (AlbumPass) gives the
// hop energies of every track of a call from two launches and one read-back; pooled figures
// come from the windows of the tracks back to back (no window spans two tracks) through
// r128_figures, the tail mm_r128_from_hops ends in; the per-track reports come from the same hop
// energies, so a pass measures once.  Every pass of the device's level loop (tracks.hip:
// level_groups_device) measures this way, whatever it levels.  And the host restatement of the
// level: level_group_host, the one pass loop in plain C++ over one group of n tracks, behind
// mm_level_host (n = 1) and mm_album_level_host.  Nothing is decided in it that level.hip does
// not decide.  The album's device entries are in tracks.hip, behind the driver.
//
// Included at the end of mastering.hip after level.hip.

namespace {

constexpr int ALBUM_TRACKS = MM_ALBUM_TRACKS;

// The windows of every track back to back in track order (the pools P_4 and P_30), then the
// one tail.  tracks (may be null, [n]): every track's own report from the same windows, as
// mm_r128_from_hops gives it (frames and channels 0), so that a measurement forms each
// window once.  track_hops and e already checked.
void album_from_hops(const double *e, const int64_t *track_hops, int n, int rate, mm_r128 *out, mm_r128 *tracks = nullptr) {
    r128_clear(out, 0, 0, rate);
    std::vector<double> z4, l4, z30, l30, z, l, zs, ls;
    int64_t off = 0;
    for (int t = 0; t < n; ++t) {
        const int64_t H = track_hops[t];
        r128_windows(e + off, H, rate, 4, z, l);
        r128_windows(e + off, H, rate, 30, zs, ls);
        if (tracks) {
            r128_clear(&tracks[t], 0, 0, rate);
            tracks[t].hops = H;
            r128_figures(z, l, zs, ls, &tracks[t]);
        }
        z4.insert(z4.end(), z.begin(), z.end());
        l4.insert(l4.end(), l.begin(), l.end());
        z30.insert(z30.end(), zs.begin(), zs.end());
        l30.insert(l30.end(), ls.begin(), ls.end());
        off += H;
    }
    out->hops = off;
    r128_figures(z4, l4, z30, l30, out);
}

// Refuses what is not an album (MM_ERR_ARG, the sentence in mm_last_error), before anything is
// queued: a level (clu != 0) also checks the target and, with C, the ceiling of every track.
int album_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                const double sos[2][5], int32_t clu, int32_t C, int32_t W, bool level) {
    if (n < 1 || n > ALBUM_TRACKS) return set_err(c, MM_ERR_ARG, "album: %d tracks out of range [1, %d]", n, ALBUM_TRACKS);
    if (!pcm || !frames || !sos) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    int64_t total = 0;
    for (int t = 0; t < n; ++t) {
        const char *why = level ? level_bad_args(frames[t], channels, rate, clu, C, W) : r128_refusal(channels, frames[t], rate);
        if (why) return set_err(c, MM_ERR_ARG, "album: track %d: %s", t, why);
        if (frames[t] > 0 && !pcm[t]) return set_err(c, MM_ERR_ARG, "album: track %d: null pointer", t);
        total += frames[t];
    }
    if (total >= R128_MAX_FRAMES) return set_err(c, MM_ERR_ARG, "album: total frames out of range");
    return MM_OK;
}

// The pooled report of n tracks and every track's own from their hop energies `e` (track after
// track, hops[t] of track t): the figures of album_from_hops with the frames and channels filled in.
void album_reports(const double *e, const int64_t *hops, const int64_t *frames, int n, int rate, int channels, mm_r128 *album,
                   mm_r128 *tracks) {
    album_from_hops(e, hops, n, rate, album, tracks);
    album->channels = channels;
    for (int t = 0; t < n; ++t) {
        tracks[t].frames = frames[t];
        tracks[t].channels = channels;
        album->frames += frames[t];
    }
}

// The album R 128 report of device-resident tracks (synchronous on return); the per-track
// reports land in c->r128s.  Arguments already checked.
int album_r128_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                      const double sos[2][5], mm_r128 *out) {
    AlbumPass pass;
    std::vector<double> e;
    std::vector<mm_r128> tr((size_t)n);
    RET(album_pass_prepare(c, d_pcm, kind, frames, n, channels, rate, sos, pass));
    RET(album_pass_hops(c, pass, e));
    album_reports(e.data(), pass.hops.data(), frames, n, rate, channels, out, tr.data());
    results_reset(c);
    c->r128s = tr;
    return MM_OK;
}

// The level of one group of n tracks restated in plain C++ on the host (no context, no GPU), in
// place on interleaved int16: mm_ceiling_host, mm_r128_host (for its hops), album_from_hops and
// the gain under level.hip's rule, the host's one loop over passes.  Arguments already checked.
// album: the group's pooled report; track_r128, track_ceil (may be null, [n]): every track's own.
int level_group_host(int16_t *const *pcm, const int64_t *frames, int n, int channels, int32_t rate, const double sos[2][5],
                     int32_t level_clu, int32_t C, int32_t W, mm_level *out, mm_r128 *album, mm_r128 *track_r128,
                     mm_ceiling *track_ceil) {
    int64_t total = 0;
    std::vector<int64_t> hops((size_t)n);
    for (int t = 0; t < n; ++t) {
        total += frames[t];
        hops[(size_t)t] = 10 * frames[t] / rate;
    }
    level_clear(out, total, channels, rate, level_clu, C, W);
    std::vector<mm_ceiling> ceil((size_t)n), ce_in((size_t)n);
    auto measure = [&]() -> int {  // the album's report and, where asked for, every track's
        std::vector<double> e;
        for (int t = 0; t < n; ++t) {
            const size_t off = e.size();
            e.resize(off + (size_t)hops[(size_t)t]);
            mm_r128 r;
            RET(mm_r128_host(pcm[t], frames[t], channels, rate, sos, e.data() + off, hops[(size_t)t], &r));
            if (track_r128) track_r128[t] = r;
        }
        album_from_hops(e.data(), hops.data(), n, rate, album);
        album->frames = total;
        album->channels = channels;
        return MM_OK;
    };
    auto done = [&]() {
        if (C && track_ceil)
            for (int t = 0; t < n; ++t) track_ceil[t] = ceil[(size_t)t];
        return MM_OK;
    };
    const int nc = C ? n : 0;  // ceilings a pass
    RET(measure());
    out->source_lufs = album->integrated;
    if (!std::isfinite(album->integrated)) {
        for (int t = 0; t < nc; ++t) RET(mm_ceiling_host(pcm[t], frames[t], channels, C, W, &ceil[(size_t)t]));
        level_unmeasurable(out, ceil.data(), nc);
        if (C) RET(measure());
        return done();
    }
    std::vector<std::vector<int16_t>> src((size_t)n);
    int32_t peak = 0;
    for (int t = 0; t < n; ++t) {
        src[(size_t)t].assign(pcm[t], pcm[t] + (size_t)(frames[t] * channels));
        for (int16_t s : src[(size_t)t]) peak = std::max(peak, std::abs((int32_t)s));
    }
    const int32_t g_peak = level_peak_cap(peak);
    int32_t g = level_first(out);
    while (g) {
        const LevelStep s = level_step(C, g, g_peak);
        int64_t clipped = 0;
        for (int t = 0; t < n; ++t) {
            const std::vector<int16_t> &x = src[(size_t)t];
            if (s.boost) {
                if (!x.empty()) memcpy(pcm[t], x.data(), x.size() * sizeof(int16_t));
                RET(mm_ceiling_host(pcm[t], frames[t], channels, s.C_inner, W, &ce_in[(size_t)t]));
                level_gain_host(pcm[t], pcm[t], x.size(), s.g, clipped);
            } else {
                level_gain_host(x.data(), pcm[t], x.size(), s.g, clipped);
            }
            if (C) RET(mm_ceiling_host(pcm[t], frames[t], channels, C, W, &ceil[(size_t)t]));
        }
        RET(measure());
        g = level_record(out, s, album->integrated, clipped, ceil.data(), ce_in.data(), nc);
    }
    return done();
}

}  // namespace

extern "C" {

int mm_r128_album_from_hops(const double *e, const int64_t *track_hops, int n, int32_t rate, mm_r128 *out) {
    if (!out || !track_hops || n < 1 || n > ALBUM_TRACKS || rate < R128_MIN_RATE) return MM_ERR_ARG;
    int64_t total = 0;
    for (int t = 0; t < n; ++t) {
        if (track_hops[t] < 0) return MM_ERR_ARG;
        total += track_hops[t];
    }
    if (total > 0 && !e) return MM_ERR_ARG;
    album_from_hops(e, track_hops, n, rate, out);
    return MM_OK;
}

// The definition restated in plain C++ on the host: a single track is a group of one.
int mm_level_host(int16_t *pcm, int64_t frames, int channels, int32_t rate, const double sos[2][5], int32_t level_clu,
                  int32_t C, int32_t W, mm_level *out, mm_ceiling *ceil_out) {
    if (!out || !sos || (frames > 0 && !pcm) || level_bad_args(frames, channels, rate, level_clu, C, W)) return MM_ERR_ARG;
    mm_r128 pooled;
    return level_group_host(&pcm, &frames, 1, channels, rate, sos, level_clu, C, W, out, &pooled, nullptr, ceil_out);
}

// And an album a group of its n tracks.
int mm_album_level_host(int16_t *const *pcm, const int64_t *frames, int n, int channels, int32_t rate,
                        const double sos[2][5], int32_t level_clu, int32_t C, int32_t W, mm_level *out, mm_r128 *album,
                        mm_r128 *track_r128, mm_ceiling *track_ceil) {
    if (!out || !album) return MM_ERR_ARG;
    RET(album_check(nullptr, (const void *const *)pcm, MM_OUT_I16, frames, n, channels, rate, sos, level_clu, C, W, true));
    return level_group_host(pcm, frames, n, channels, rate, sos, level_clu, C, W, out, album, track_r128, track_ceil);
}

int mm_album_r128_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                         int32_t rate, const double sos[2][5], mm_r128 *out) {
    if (!c) return MM_ERR_ARG;
    if (!out) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(album_check(c, d_pcm, kind, frames, n, channels, rate, sos, 0, 0, 0, false));
    HIPCHK(c, hipSetDevice(c->device));
    return album_r128_device(c, d_pcm, kind, frames, n, channels, rate, sos, out);
}

int mm_album_r128_pcm(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                      const double sos[2][5], mm_r128 *out) {
    if (!c) return MM_ERR_ARG;
    if (!out) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(album_check(c, pcm, kind, frames, n, channels, rate, sos, 0, 0, 0, false));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "album_io", pcm, kind, frames, n, channels, d));
    return album_r128_device(c, d.data(), kind, frames, n, channels, rate, sos, out);
}

int mm_op_r128_album_hops(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                          int32_t rate, const double sos[2][5], double *hops_host, int64_t cap) {
    if (!c) return MM_ERR_ARG;
    if (cap < 0 || (cap > 0 && !hops_host)) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(album_check(c, pcm, kind, frames, n, channels, rate, sos, 0, 0, 0, false));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "album_io", pcm, kind, frames, n, channels, d));
    AlbumPass pass;
    std::vector<double> e;
    RET(album_pass_prepare(c, d.data(), kind, frames, n, channels, rate, sos, pass));
    RET(album_pass_hops(c, pass, e));
    for (size_t i = 0; i < std::min(e.size(), (size_t)cap); ++i) hops_host[i] = e[i];
    return (int)std::min<size_t>(e.size(), (size_t)INT32_MAX);
}

int mm_last_album(mm_ctx *c, mm_level *level, mm_r128 *album) {
    if (!c || !level || !album) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->albums.empty()) return set_err(c, MM_ERR_STATE, "the last call levelled no album");
    *level = c->albums[0];
    *album = c->album_r128s[0];
    return MM_OK;
}

}  // extern "C"
