// album.hip — an album levelled as one programme: ONE static gain for all its tracks, which
// makes the album read the R 128 target with every track held under the true-peak ceiling
// (the album R 128 figures and the album level in include/mastering.h).  Loudness differences
// between the tracks are kept.  No reference counterpart.
//
// Nothing is decided here that level.hip does not decide: level_first, level_step and
// level_record run on the album's integrated loudness and the tracks' ceilings, the kept
// sources are level_keep's, the gain is level_gain's (on the host level_gain_host's) and the
// ceiling ceiling_device's, one call a track.  What is new is the measuring pass: r128.hip's album kernels K-weight
// every track in ONE launch and reduce all hops in one more, with one read-back of the
// album's hop energies and the look-back's error word, where n calls of r128_hops pay n
// synchronisations a pass.  The album's figures come from the pooled windows of the tracks
// (no window spans two tracks) through r128_figures, the tail mm_r128_from_hops ends in; the
// per-track reports come from the same hop energies, so a pass measures once.
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

// The segmented measuring pass of one album, laid out once a call: every track on a
// workgroup boundary, its hops at hop0[t] of the album's.
struct AlbumPass {
    R128AlbumArgs a{};
    unsigned nblk = 0;
    int kind = 0, channels = 0;
    std::vector<int64_t> hops;  // [n] H_t
    double *d_e = nullptr;
};

// Lays the pass out and uploads its tables (synchronous: the host tables are transient).
int album_pass_prepare(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                       const double sos[2][5], AlbumPass &p) {
    std::vector<R128Track> tracks((size_t)n);
    std::vector<int> wg_track;
    int64_t wg = 0, hop = 0;
    p.hops.resize((size_t)n);
    for (int t = 0; t < n; ++t) {
        const int64_t G = (frames[t] + R128_TILE - 1) / R128_TILE, nwg = (G + LB_THREADS - 1) / LB_THREADS;
        tracks[(size_t)t] = R128Track{d_pcm[t], frames[t], wg, hop};
        wg_track.insert(wg_track.end(), (size_t)nwg, t);
        p.hops[(size_t)t] = 10 * frames[t] / rate;
        wg += nwg;
        hop += p.hops[(size_t)t];
    }
    p.nblk = (unsigned)wg;
    p.kind = kind;
    p.channels = channels;
    p.a.n = n;
    p.a.rate = rate;
    p.a.H = hop;
    memcpy(p.a.sos, sos, sizeof p.a.sos);
    if (hop == 0) return MM_OK;  // nothing to measure: nothing is launched
    R128Track *d_tracks;
    int *d_wg;
    RET(get_buf(c, "album_tracks", (size_t)n, &d_tracks));
    RET(get_buf(c, "album_wg", (size_t)wg, &d_wg));
    RET(get_buf(c, "album_part", (size_t)wg * LB_THREADS * 2, &p.a.part));
    RET(get_buf(c, "album_part_hop", (size_t)wg * LB_THREADS, &p.a.part_hop));
    RET(get_buf(c, "album_hops", (size_t)hop, &p.d_e));
    HIPCHK(c, hipMemcpyAsync(d_tracks, tracks.data(), (size_t)n * sizeof(R128Track), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_wg, wg_track.data(), (size_t)wg * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    p.a.tracks = d_tracks;
    p.a.wg_track = d_wg;
    return MM_OK;
}

// One measurement: the album's hop energies into `e`, track after track.  Two launches, one
// read-back.  Synchronous on return.
int album_pass_hops(mm_ctx *c, const AlbumPass &p, std::vector<double> &e) {
    e.assign((size_t)p.a.H, 0.0);
    if (p.a.H == 0) return MM_OK;
    LbArgs lb{};
    RET(r128_upload_tables(c, p.a.sos, p.channels, lb));
    RET(lb_prepare(c, p.nblk, 1, lb));
    RET(get_buf(c, "r128_lb_error", 4, &lb.error));
    HIPCHK(c, hipMemsetAsync(lb.error, 0, 4, c->stream));
    const size_t lds = (size_t)lb_lds_bytes<8, 1>() + (size_t)R128_CHUNK * R128_ROW * sizeof(uint32_t);
    RET(dispatch_pcm(p.kind, p.channels, [&](auto ch, auto t) {
        using T = decltype(t);
        return launch(c, "r128_album_kweight", r128_album_kweight_kernel<ch, T>, dim3(p.nblk), dim3(LB_THREADS), lds, p.a, lb);
    }));
    RET(launch(c, "r128_album_reduce", r128_album_reduce_kernel, dim3(blocks_for(p.a.H, 4)), dim3(256), 0, p.a, p.d_e));
    unsigned err = 0;
    HIPCHK(c, hipMemcpyAsync(e.data(), p.d_e, (size_t)p.a.H * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&err, lb.error, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    if (err) return set_err(c, MM_ERR_STATE, "IIR look-back timed out");
    return MM_OK;
}

// The album's report and every track's from one measurement's hop energies.
void album_reports(const std::vector<double> &e, const AlbumPass &p, const int64_t *frames, mm_r128 *album,
                   std::vector<mm_r128> &tracks) {
    const int n = p.a.n;
    tracks.resize((size_t)n);
    album_from_hops(e.data(), p.hops.data(), n, p.a.rate, album, tracks.data());
    album->channels = p.channels;
    for (int t = 0; t < n; ++t) {
        tracks[(size_t)t].frames = frames[t];
        tracks[(size_t)t].channels = p.channels;
        album->frames += frames[t];
    }
}

// The album R 128 report of device-resident tracks (synchronous on return); the per-track
// reports land in c->r128s.  Arguments already checked.
int album_r128_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                      const double sos[2][5], mm_r128 *out) {
    AlbumPass pass;
    std::vector<double> e;
    std::vector<mm_r128> tr;
    RET(album_pass_prepare(c, d_pcm, kind, frames, n, channels, rate, sos, pass));
    RET(album_pass_hops(c, pass, e));
    album_reports(e, pass, frames, out, tr);
    results_reset(c);
    c->r128s = tr;
    return MM_OK;
}

// The album level on device-resident tracks, in place (synchronous on return).  Arguments
// already checked.  The results go behind mm_last_album, mm_last_r128 and mm_last_ceilings.
int album_level_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                       const double sos[2][5], int32_t level_clu, int32_t C, int32_t W) {
    results_reset(c);
    mm_level out;
    mm_r128 album;
    int64_t total = 0;
    for (int t = 0; t < n; ++t) total += frames[t];
    level_clear(&out, total, channels, rate, level_clu, C, W);
    AlbumPass pass;
    std::vector<double> e;
    std::vector<mm_r128> tr;
    std::vector<mm_ceiling> ceil((size_t)n), ce_in((size_t)n);
    RET(album_pass_prepare(c, d_pcm, kind, frames, n, channels, rate, sos, pass));
    auto measure = [&]() -> int {
        RET(album_pass_hops(c, pass, e));
        album_reports(e, pass, frames, &album, tr);
        return MM_OK;
    };
    auto done = [&]() {
        c->r128s = tr;
        if (C) c->ceilings = ceil;
        c->albums.assign(1, out);
        c->album_r128s.assign(1, album);
        return MM_OK;
    };
    const int nc = C ? n : 0;  // ceilings a pass
    RET(measure());
    out.source_lufs = album.integrated;
    if (!std::isfinite(album.integrated)) {  // no window, or silence: every track only gets its ceiling
        for (int t = 0; t < nc; ++t) RET(ceiling_device(c, d_pcm[t], kind, frames[t], channels, C, W, &ceil[(size_t)t]));
        level_unmeasurable(&out, ceil.data(), nc);
        if (C) RET(measure());  // the reports describe what is delivered
        return done();
    }
    std::vector<char *> src;
    std::vector<size_t> bytes((size_t)n);
    for (int t = 0; t < n; ++t) bytes[(size_t)t] = pcm_bytes(kind, frames[t], channels);
    LevelDev *st;
    std::vector<LevelDev> hs((size_t)n);
    RET(level_keep(c, "album_src", d_pcm, kind, frames, n, channels, src));
    RET(get_buf(c, "album_res", (size_t)n, &st));
    auto results = [&]() -> int {  // every slot of the pass, behind the next synchronisation
        HIPCHK(c, hipMemcpyAsync(hs.data(), st, (size_t)n * sizeof(LevelDev), hipMemcpyDeviceToHost, c->stream));
        return MM_OK;
    };
    int32_t g_peak = LEVEL_GMAX;
    if (C) {
        for (int t = 0; t < n; ++t)
            if (bytes[(size_t)t]) HIPCHK(c, hipMemcpyAsync(src[(size_t)t], d_pcm[t], bytes[(size_t)t], hipMemcpyDeviceToDevice, c->stream));
    } else {  // the copies through the kernel at ONE (the identity): they bring max_t max |s_t|
        HIPCHK(c, hipMemsetAsync(st, 0, (size_t)n * sizeof(LevelDev), c->stream));
        for (int t = 0; t < n; ++t) RET(level_gain_queue(c, d_pcm[t], src[(size_t)t], kind, frames[t] * channels, LEVEL_ONE, st + t));
        RET(results());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        unsigned peak = 0;
        for (const LevelDev &h : hs) peak = std::max(peak, h.peak);
        g_peak = level_peak_cap((int32_t)peak);
    }
    int32_t g = level_first(&out);
    while (g) {
        const LevelStep s = level_step(C, g, g_peak);
        HIPCHK(c, hipMemsetAsync(st, 0, (size_t)n * sizeof(LevelDev), c->stream));
        for (int t = 0; t < n; ++t) {
            const int64_t ns = frames[t] * channels;
            if (!s.boost) {
                RET(level_gain_queue(c, src[(size_t)t], d_pcm[t], kind, ns, s.g, st + t));
                continue;
            }
            if (bytes[(size_t)t]) HIPCHK(c, hipMemcpyAsync(d_pcm[t], src[(size_t)t], bytes[(size_t)t], hipMemcpyDeviceToDevice, c->stream));
            RET(ceiling_device(c, d_pcm[t], kind, frames[t], channels, s.C_inner, W, &ce_in[(size_t)t]));
            RET(level_gain_queue(c, d_pcm[t], d_pcm[t], kind, ns, s.g, st + t));
        }
        RET(results());
        for (int t = 0; t < nc; ++t) RET(ceiling_device(c, d_pcm[t], kind, frames[t], channels, C, W, &ceil[(size_t)t]));
        RET(measure());
        int64_t clipped = 0;
        for (const LevelDev &h : hs) clipped += (int64_t)h.clipped;
        g = level_record(&out, s, album.integrated, clipped, ceil.data(), ce_in.data(), nc);
    }
    return done();
}

// n host tracks into one context buffer, each on a 16-byte boundary: their device pointers
int album_upload(mm_ctx *c, const char *name, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                 std::vector<void *> &d) {
    size_t total = 0;
    for (int t = 0; t < n; ++t) total += (pcm_bytes(kind, frames[t], channels) + 15) & ~(size_t)15;
    char *base;
    RET(get_buf(c, name, std::max<size_t>(total, 1), &base));
    d.resize((size_t)n);
    for (int t = 0; t < n; ++t) {
        const size_t bytes = pcm_bytes(kind, frames[t], channels);
        d[(size_t)t] = base;
        if (bytes && pcm) HIPCHK(c, hipMemcpyAsync(base, pcm[t], bytes, hipMemcpyHostToDevice, c->stream));
        base += (bytes + 15) & ~(size_t)15;
    }
    return MM_OK;
}

// d[t] back into pcm[t] for the tracks `pick` names (null: all), synchronous
int batch_download(mm_ctx *c, void *const *pcm, const std::vector<void *> &d, int kind, const int64_t *frames, int n,
                   int channels, const char *pick) {
    for (int t = 0; t < n; ++t) {
        const size_t bytes = pcm_bytes(kind, frames[t], channels);
        if (bytes && (!pick || pick[t])) HIPCHK(c, hipMemcpyAsync(pcm[t], d[(size_t)t], bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
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

// The definition restated in plain C++ on the host (no context, no GPU), in place on
// interleaved int16: mm_ceiling_host, mm_r128_host (for its hops) and the gain, composed as
// mm_level_host composes them, under the same rule.
int mm_album_level_host(int16_t *const *pcm, const int64_t *frames, int n, int channels, int32_t rate,
                        const double sos[2][5], int32_t level_clu, int32_t C, int32_t W, mm_level *out, mm_r128 *album,
                        mm_r128 *track_r128, mm_ceiling *track_ceil) {
    if (!out || !album) return MM_ERR_ARG;
    RET(album_check(nullptr, (const void *const *)pcm, MM_OUT_I16, frames, n, channels, rate, sos, level_clu, C, W, true));
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

int mm_album_level_device(mm_ctx *c, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                          const double sos[2][5], int32_t level_clu, int32_t ceiling_q28, int32_t window) {
    if (!c) return MM_ERR_ARG;
    RET(album_check(c, d_pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window, true));
    HIPCHK(c, hipSetDevice(c->device));
    return album_level_device(c, d_pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window);
}

int mm_album_level_pcm(mm_ctx *c, void *const *pcm, int kind, const int64_t *frames, int n, int channels, int32_t rate,
                       const double sos[2][5], int32_t level_clu, int32_t ceiling_q28, int32_t window) {
    if (!c) return MM_ERR_ARG;
    RET(album_check(c, pcm, kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window, true));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "album_io", pcm, kind, frames, n, channels, d));
    RET(album_level_device(c, d.data(), kind, frames, n, channels, rate, sos, level_clu, ceiling_q28, window));
    return batch_download(c, pcm, d, kind, frames, n, channels, nullptr);
}

int mm_last_album(mm_ctx *c, mm_level *level, mm_r128 *album) {
    if (!c || !level || !album) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->albums.empty()) return set_err(c, MM_ERR_STATE, "the last call levelled no album");
    *level = c->albums[0];
    *album = c->album_r128s[0];
    return MM_OK;
}

}  // extern "C"
