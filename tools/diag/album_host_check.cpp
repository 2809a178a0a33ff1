// Stand-alone host check of mm_album_level_host and mm_r128_album_from_hops (an album levelled
// as one programme restated in plain C++, csrc/album.hip) for a sanitizer build: no context, no
// GPU, never loaded into Python.  Build the library's translation unit and this file into one
// program with the host side instrumented, and run it on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wno-unused-value -Wno-unused-result \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     python-audio-mastering_amd/csrc/mastering.hip tools/diag/album_host_check.cpp -lrccl -o album_host_check
// Every track is a heap block of exactly frames * channels samples, so an index that runs from
// one track into the next (the gain, a kept source, the composed mm_ceiling_host / mm_r128_host,
// the pooled windows) is an ASan report.  It replays the branches of the rule at 8 kHz, where
// half a second is five hops, on albums that hold a track too short for a window and an empty
// one, and checks what the definition promises whatever the pass count: every track's true peak
// under the ceiling, a REACHED album within 0.05 LU of the target, the album's report the pooled
// figures of the delivered tracks, without a ceiling every track equal to gain(source, gain_q16)
// computed here, and an album of one track equal to mm_level_host.  Both entries now run the one
// host loop (csrc/album.hip: level_group_host), so that last check compares the loop with itself
// and only guards the two wrappers; what the loop must deliver is pinned by
// tests/golden/level_host_parent.json (tests/test_level_golden.py).  Exits non-zero on any failure.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/mastering.h"

static int failures = 0;

#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++failures;                                             \
        }                                                           \
    } while (0)

static uint32_t rnd_state = 2463534242u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

// pyloudnorm's K-weighting sections (design.kweight_sections) of `rate`
static void kweight(double rate, double sos[2][5]) {
    const double G[2] = {4.0, 0.0}, Q[2] = {1.0 / std::sqrt(2.0), 0.5}, fc[2] = {1500.0, 38.0};
    for (int s = 0; s < 2; ++s) {
        const double A = std::pow(10.0, G[s] / 40.0), w0 = 2.0 * M_PI * (fc[s] / rate), al = std::sin(w0) / (2.0 * Q[s]);
        const double cw = std::cos(w0), sa = 2.0 * std::sqrt(A) * al;
        double b[3], a[3];
        if (s == 0) {
            b[0] = A * ((A + 1) + (A - 1) * cw + sa), b[1] = -2 * A * ((A - 1) + (A + 1) * cw), b[2] = A * ((A + 1) + (A - 1) * cw - sa);
            a[0] = (A + 1) - (A - 1) * cw + sa, a[1] = 2 * ((A - 1) - (A + 1) * cw), a[2] = (A + 1) - (A - 1) * cw - sa;
        } else {
            b[0] = (1 + cw) / 2, b[1] = -(1 + cw), b[2] = (1 + cw) / 2;
            a[0] = 1 + al, a[1] = -2 * cw, a[2] = 1 - al;
        }
        const double v[5] = {b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]};
        memcpy(sos[s], v, sizeof v);
    }
}

static const int RATE = 8000;
static const int32_t ONE = 1 << 16, C1 = 239243351;  // -1 dBTP

typedef std::vector<int16_t> Track;

// noise of peak `amp` with a louder second half (the limiter then bites on a part only)
static Track noise(int64_t frames, int ch, int amp) {
    Track p((size_t)(frames * ch));
    for (size_t i = 0; i < p.size(); ++i) {
        const int a = i >= p.size() / 2 ? amp : amp / 3;
        p[i] = (int16_t)((int64_t)(rnd() >> 16) * (2 * a + 1) / 65536 - a);
    }
    return p;
}

// the tracks as exactly-sized heap blocks of their own (an empty track: a null pointer)
struct Album {
    std::vector<std::unique_ptr<int16_t[]>> blocks;
    std::vector<int16_t *> ptr;
    std::vector<int64_t> frames;
    Album(const std::vector<Track> &src, int ch) {
        for (const Track &t : src) {
            blocks.emplace_back(t.empty() ? nullptr : new int16_t[t.size()]);
            if (!t.empty()) memcpy(blocks.back().get(), t.data(), t.size() * sizeof(int16_t));
            ptr.push_back(blocks.back().get());
            frames.push_back((int64_t)(t.size() / (size_t)ch));
        }
    }
};

static mm_level run(const std::vector<Track> &src, int ch, int clu, int32_t C, int32_t W, int want_status = -1) {
    double sos[2][5];
    kweight(RATE, sos);
    Album a(src, ch);
    const int n = (int)src.size();
    mm_level m;
    mm_r128 alb;
    std::vector<mm_r128> tr((size_t)n);
    std::vector<mm_ceiling> ce((size_t)n);
    CHECK(mm_album_level_host(a.ptr.data(), a.frames.data(), n, ch, RATE, sos, clu, C, W, &m, &alb, tr.data(), ce.data()) == MM_OK);
    int64_t total = 0;
    for (int64_t f : a.frames) total += f;
    CHECK(m.frames == total && m.channels == ch && m.rate == RATE && m.target_clu == clu && m.ceiling_q28 == C);
    CHECK(m.status >= MM_LEVEL_REACHED && m.status <= MM_LEVEL_UNMEASURABLE && m.passes >= 0 && m.passes <= MM_LEVEL_PASSES);
    if (want_status >= 0) CHECK(m.status == want_status);
    // the album's report is the pooled figures of the delivered tracks' own hop energies
    std::vector<double> e;
    std::vector<int64_t> hops;
    for (int t = 0; t < n; ++t) {
        const int64_t H = 10 * a.frames[(size_t)t] / RATE;
        const size_t off = e.size();
        e.resize(off + (size_t)H);
        mm_r128 r;
        CHECK(mm_r128_host(a.ptr[(size_t)t], a.frames[(size_t)t], ch, RATE, sos, e.data() + off, H, &r) == MM_OK);
        CHECK(memcmp(&r, &tr[(size_t)t], sizeof r) == 0);
        hops.push_back(H);
    }
    mm_r128 pooled;
    CHECK(mm_r128_album_from_hops(e.data(), hops.data(), n, RATE, &pooled) == MM_OK);
    pooled.frames = total;
    pooled.channels = ch;
    CHECK(memcmp(&pooled, &alb, sizeof alb) == 0);
    if (m.status == MM_LEVEL_UNMEASURABLE) {
        CHECK(m.passes == 0 && m.gain_q16 == ONE && std::isnan(m.loudness) && !std::isfinite(m.source_lufs));
        if (!C)
            for (int t = 0; t < n; ++t) CHECK(src[(size_t)t].empty() || memcmp(a.ptr[(size_t)t], src[(size_t)t].data(), src[(size_t)t].size() * 2) == 0);
    } else {
        CHECK(m.passes >= 1 && m.gain_q16 == m.pass_gain_q16[m.passes - 1] && m.loudness == m.pass_lufs[m.passes - 1]);
        CHECK(m.gain_q16 >= (1 << 8) && m.gain_q16 <= (1 << 21));
        for (int k = m.passes; k < MM_LEVEL_PASSES; ++k) CHECK(std::isnan(m.pass_lufs[k]) && m.pass_gain_q16[k] == 0);
        if (m.status == MM_LEVEL_REACHED) CHECK(std::fabs(m.loudness - clu / 100.0) <= 0.05);
        if (m.status == MM_LEVEL_PASSES_SPENT) CHECK(m.passes == MM_LEVEL_PASSES);
        CHECK(alb.integrated == m.loudness);
    }
    int64_t limited = 0;
    for (int t = 0; t < n; ++t) {
        const int64_t frames = a.frames[(size_t)t];
        if (C && frames > 0) {  // every track's true peak is under C
            mm_meter tp;
            CHECK(mm_true_peak_host(a.ptr[(size_t)t], frames, ch, &tp) == MM_OK);
            const int32_t peak = std::max(tp.true_peak_q28[0], ch == 2 ? tp.true_peak_q28[1] : 0);
            CHECK(peak <= C && ce[(size_t)t].tp_out_q28 == peak && ce[(size_t)t].ceiling_q28 == C && ce[(size_t)t].frames == frames);
            limited += ce[(size_t)t].limited_frames;
        } else if (!C && m.status != MM_LEVEL_UNMEASURABLE) {  // gain(source, g), restated
            for (size_t i = 0; i < src[(size_t)t].size(); ++i) {
                const int64_t v = (int64_t)src[(size_t)t][i] * m.gain_q16 + (1 << 15);
                const int64_t y = v >= 0 ? v >> 16 : -((-v + 65535) >> 16);
                if (a.ptr[(size_t)t][i] != y) {
                    CHECK(a.ptr[(size_t)t][i] == y);
                    break;
                }
            }
        }
    }
    if (!C) CHECK(m.clipped == 0 && m.limited_frames == 0 && m.min_gain_q16 == ONE);
    if (C && m.gain_q16 <= ONE) CHECK(m.limited_frames == limited);  // (the limiting call is then the final one)
    return m;
}

// n = 1 is mm_level_host: the same samples and the same struct (one loop behind both: the wrappers agree)
static void one_track(const Track &src, int ch, int clu, int32_t C, int32_t W) {
    double sos[2][5];
    kweight(RATE, sos);
    Album a({src}, ch);
    Track p = src;
    mm_level m, m1;
    mm_r128 alb;
    mm_ceiling ce, ce1;
    CHECK(mm_album_level_host(a.ptr.data(), a.frames.data(), 1, ch, RATE, sos, clu, C, W, &m, &alb, nullptr, &ce) == MM_OK);
    CHECK(mm_level_host(p.data(), a.frames[0], ch, RATE, sos, clu, C, W, &m1, &ce1) == MM_OK);
    CHECK(memcmp(&m, &m1, sizeof m) == 0);
    CHECK(p.empty() || memcmp(a.ptr[0], p.data(), p.size() * sizeof(int16_t)) == 0);
    if (C) CHECK(memcmp(&ce, &ce1, sizeof ce) == 0);
}

int main() {
    for (int ch = 1; ch <= 2; ++ch)
        for (int64_t frames : {(int64_t)4000, (int64_t)12345}) {
            // a loud track, a quiet one, one too short for a window (3 hops), an empty one, a mid one
            const std::vector<Track> hot = {noise(frames, ch, 32767), noise(6000, ch, 3000), noise(2500, ch, 32767), Track(),
                                            noise(frames / 2, ch, 12000)};
            const std::vector<Track> mid = {noise(frames, ch, 6000), noise(2500, ch, 9000), noise(5000, ch, 1500)};
            const std::vector<Track> quiet = {noise(3999, ch, 600), noise(frames, ch, 300), Track(), noise(1, ch, 600)};
            for (int32_t W : {1, 40, 1024}) {
                run(hot, ch, -2300, C1, W);                       // a cut, the limiter behind it
                run(mid, ch, -1400, C1, W);                       // a boost behind the limiter
                run(mid, ch, -500, C1, W);                        // more than the limiter leaves
                run(quiet, ch, -500, C1, W, MM_LEVEL_CAPPED);     // beyond the boost's cap
            }
            run(hot, ch, -2300, 0, 0, MM_LEVEL_REACHED);          // no ceiling: a cut
            std::vector<Track> spike = quiet;  // no ceiling: capped where a sample of ANY track would clip, here at once
            spike[3][0] = -32768;                                 // (in the one-frame track, which has no hop)
            const mm_level m = run(spike, ch, -500, 0, 0, MM_LEVEL_CAPPED);
            CHECK(m.passes == 1 && m.gain_q16 == ONE - 2);  // floor(32767 * 2^16 / 32768)
            run(mid, ch, -500, 0, 0);
            run(quiet, ch, -4000, 1 << 24, 16);                   // the lowest ceiling
            one_track(hot[0], ch, -2300, C1, 40);
            one_track(mid[0], ch, -1400, C1, 40);
            one_track(mid[0], ch, -500, 0, 0);
            one_track(hot[2], ch, -1400, C1, 40);                 // unmeasurable: the ceiling alone
        }
    for (int ch = 1; ch <= 2; ++ch)  // nothing to measure: no track with 4 hops, silence, no frames
        for (int32_t C : {0, C1}) {
            run({noise(3199, ch, 32767), noise(3199, ch, 20000), noise(1, ch, 32767)}, ch, -1400, C, 40, MM_LEVEL_UNMEASURABLE);
            run({Track((size_t)(8000 * ch), 0), Track((size_t)(4000 * ch), 0)}, ch, -1400, C, 40, MM_LEVEL_UNMEASURABLE);
            run({Track(), Track()}, ch, -1400, C, 40, MM_LEVEL_UNMEASURABLE);
        }
    {  // the pools: no window across two tracks
        std::vector<double> e(40, 1.0);
        const int64_t split[2] = {7, 33}, whole[1] = {40};
        mm_r128 a, b, c;
        CHECK(mm_r128_album_from_hops(e.data(), split, 2, RATE, &a) == MM_OK);
        CHECK(a.hops == 40 && a.momentary_blocks == 4 + 30 && a.short_term_blocks == 0 + 4);
        CHECK(mm_r128_album_from_hops(e.data(), whole, 1, RATE, &b) == MM_OK && mm_r128_from_hops(e.data(), 40, RATE, &c) == MM_OK);
        CHECK(memcmp(&b, &c, sizeof b) == 0 && b.momentary_blocks == 37 && b.short_term_blocks == 11);
    }
    {  // refused arguments
        double sos[2][5];
        kweight(RATE, sos);
        Album a({Track(200, (int16_t)100), Track(100, (int16_t)50)}, 2);
        mm_level m;
        mm_r128 alb;
        auto call = [&](int n, int ch, int rate, const double(*s)[5], int clu, int32_t C, int32_t W, mm_level *o, mm_r128 *al) {
            return mm_album_level_host(a.ptr.data(), a.frames.data(), n, ch, rate, s, clu, C, W, o, al, nullptr, nullptr);
        };
        CHECK(call(2, 2, RATE, sos, -1400, C1, 40, &m, &alb) == MM_OK);
        for (int n : {0, -1, MM_ALBUM_TRACKS + 1}) CHECK(call(n, 2, RATE, sos, -1400, C1, 40, &m, &alb) == MM_ERR_ARG);
        for (int clu : {0, -4001, -499, 1400}) CHECK(call(2, 2, RATE, sos, clu, C1, 40, &m, &alb) == MM_ERR_ARG);
        CHECK(call(2, 3, RATE, sos, -1400, C1, 40, &m, &alb) == MM_ERR_ARG);
        CHECK(call(2, 2, 1999, sos, -1400, C1, 40, &m, &alb) == MM_ERR_ARG);
        CHECK(call(2, 2, RATE, nullptr, -1400, C1, 40, &m, &alb) == MM_ERR_ARG);
        CHECK(call(2, 2, RATE, sos, -1400, (1 << 24) - 1, 40, &m, &alb) == MM_ERR_ARG);
        CHECK(call(2, 2, RATE, sos, -1400, C1, 0, &m, &alb) == MM_ERR_ARG);
        CHECK(call(2, 2, RATE, sos, -1400, C1, 1025, &m, &alb) == MM_ERR_ARG);
        CHECK(call(2, 2, RATE, sos, -1400, C1, 40, nullptr, &alb) == MM_ERR_ARG);
        CHECK(call(2, 2, RATE, sos, -1400, C1, 40, &m, nullptr) == MM_ERR_ARG);
        a.frames[1] = -1;
        CHECK(call(2, 2, RATE, sos, -1400, C1, 40, &m, &alb) == MM_ERR_ARG);
    }
    printf("album_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
