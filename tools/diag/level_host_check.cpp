// Stand-alone host check of mm_level_host (delivery to an R 128 loudness target restated in
// plain C++: csrc/album.hip's level_group_host over one track) for a sanitizer build: no
// context, no GPU, never loaded into Python.  Build the library's translation unit and this
// file into one program with the host side instrumented, and run it on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wno-unused-value -Wno-unused-result \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     python-audio-mastering_amd/csrc/mastering.hip tools/diag/level_host_check.cpp -lrccl -o level_host_check
// The signal is a heap block of exactly frames * channels samples, so a read or a write past
// the last frame by the gain, by the source copy or by the composed mm_ceiling_host /
// mm_r128_host is an ASan report.  It replays a few cases of each branch of the rule (no
// ceiling, a cut, a boost behind the limiter, the caps, too short to measure, silence) at
// 8 kHz, where half a second is five hops, and checks what the definition promises whatever
// the pass count: the true peak under the ceiling, no clipped sample without one, the
// delivered gain the last pass's, a REACHED loudness within 0.05 LU of the target, and,
// without a ceiling, the delivered samples equal to gain(source, gain_q16) computed here.
// Exits non-zero on any failure.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// noise of peak `amp` with a louder second half (the limiter then bites on a part only)
static std::vector<int16_t> noise(int64_t frames, int ch, int amp) {
    std::vector<int16_t> p((size_t)(frames * ch));
    for (size_t i = 0; i < p.size(); ++i) {
        const int a = i >= p.size() / 2 ? amp : amp / 3;
        p[i] = (int16_t)((int64_t)(rnd() >> 16) * (2 * a + 1) / 65536 - a);
    }
    return p;
}

static mm_level run(const std::vector<int16_t> &src, int ch, int clu, int32_t C, int32_t W, int want_status = -1) {
    double sos[2][5];
    kweight(RATE, sos);
    std::vector<int16_t> p = src;  // (exactly the samples: any access past them is reported)
    const int64_t frames = (int64_t)(p.size() / ch);
    mm_level m;
    mm_ceiling ce;
    CHECK(mm_level_host(p.data(), frames, ch, RATE, sos, clu, C, W, &m, C ? &ce : nullptr) == MM_OK);
    CHECK(m.frames == frames && m.channels == ch && m.rate == RATE && m.target_clu == clu && m.ceiling_q28 == C);
    CHECK(m.status >= MM_LEVEL_REACHED && m.status <= MM_LEVEL_UNMEASURABLE && m.passes >= 0 && m.passes <= MM_LEVEL_PASSES);
    if (want_status >= 0) CHECK(m.status == want_status);
    if (m.status == MM_LEVEL_UNMEASURABLE) {
        CHECK(m.passes == 0 && m.gain_q16 == ONE && std::isnan(m.loudness) && !std::isfinite(m.source_lufs));
        if (!C) CHECK(p == src);
    } else {
        CHECK(m.passes >= 1 && m.gain_q16 == m.pass_gain_q16[m.passes - 1] && m.loudness == m.pass_lufs[m.passes - 1]);
        CHECK(m.gain_q16 >= (1 << 8) && m.gain_q16 <= (1 << 21));
        for (int k = m.passes; k < MM_LEVEL_PASSES; ++k) CHECK(std::isnan(m.pass_lufs[k]) && m.pass_gain_q16[k] == 0);
        if (m.status == MM_LEVEL_REACHED) CHECK(std::fabs(m.loudness - clu / 100.0) <= 0.05);
        if (m.status == MM_LEVEL_PASSES_SPENT) CHECK(m.passes == MM_LEVEL_PASSES);
        mm_r128 r;  // the delivered loudness is the meter's on the delivered samples
        CHECK(mm_r128_host(p.data(), frames, ch, RATE, sos, nullptr, 0, &r) == MM_OK && r.integrated == m.loudness);
    }
    if (C && frames > 0) {
        mm_meter tp;
        CHECK(mm_true_peak_host(p.data(), frames, ch, &tp) == MM_OK);
        const int32_t peak = std::max(tp.true_peak_q28[0], ch == 2 ? tp.true_peak_q28[1] : 0);
        CHECK(peak <= C && ce.tp_out_q28 == peak && ce.ceiling_q28 == C && ce.frames == frames);
    } else if (m.status != MM_LEVEL_UNMEASURABLE) {
        CHECK(m.clipped == 0 && m.limited_frames == 0 && m.min_gain_q16 == ONE);
        for (size_t i = 0; i < p.size(); ++i) {  // gain(source, g), restated
            const int64_t v = (int64_t)src[i] * m.gain_q16 + (1 << 15);
            const int64_t y = v >= 0 ? v >> 16 : -((-v + 65535) >> 16);
            if (p[i] != y) {
                CHECK(p[i] == y);
                break;
            }
        }
    }
    return m;
}

int main() {
    for (int ch = 1; ch <= 2; ++ch)
        for (int64_t frames : {(int64_t)4000, (int64_t)8000, (int64_t)12345}) {
            const std::vector<int16_t> quiet = noise(frames, ch, 600), mid = noise(frames, ch, 6000),
                                       hot = noise(frames, ch, 32767);
            for (int32_t W : {1, 40, 1024}) {
                run(hot, ch, -2300, C1, W);                       // a cut, the limiter behind it
                run(mid, ch, -1400, C1, W);                       // a boost behind the limiter
                run(mid, ch, -500, C1, W);                        // more than the limiter leaves
                run(quiet, ch, -500, C1, W, MM_LEVEL_CAPPED);     // beyond the boost's cap
            }
            run(hot, ch, -2300, 0, 0, MM_LEVEL_REACHED);          // no ceiling: a cut
            std::vector<int16_t> spike = quiet;  // no ceiling: capped where a sample would clip, here at once
            spike[spike.size() / 3] = -32768;
            const mm_level m = run(spike, ch, -500, 0, 0, MM_LEVEL_CAPPED);
            CHECK(m.passes == 1 && m.gain_q16 == ONE - 2);  // floor(32767 * 2^16 / 32768)
            run(mid, ch, -500, 0, 0);
            run(quiet, ch, -4000, 1 << 24, 16);                   // the lowest ceiling
        }
    for (int ch = 1; ch <= 2; ++ch) {  // nothing to measure: fewer than 4 hops, silence, no frames
        for (int32_t C : {0, C1}) {
            run(noise(3199, ch, 32767), ch, -1400, C, 40, MM_LEVEL_UNMEASURABLE);
            run(noise(1, ch, 32767), ch, -1400, C, 40, MM_LEVEL_UNMEASURABLE);
            run(std::vector<int16_t>((size_t)(8000 * ch), 0), ch, -1400, C, 40, MM_LEVEL_UNMEASURABLE);
            run(std::vector<int16_t>(), ch, -1400, C, 40, MM_LEVEL_UNMEASURABLE);
        }
    }
    {  // refused arguments
        double sos[2][5];
        kweight(RATE, sos);
        std::vector<int16_t> p(200, (int16_t)100);
        mm_level m;
        CHECK(mm_level_host(p.data(), 100, 2, RATE, sos, -1400, C1, 40, &m, nullptr) == MM_OK);
        for (int clu : {0, -4001, -499, 1400}) CHECK(mm_level_host(p.data(), 100, 2, RATE, sos, clu, C1, 40, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(p.data(), 100, 3, RATE, sos, -1400, C1, 40, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(p.data(), 100, 2, 1999, sos, -1400, C1, 40, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(p.data(), 100, 2, RATE, nullptr, -1400, C1, 40, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(p.data(), 100, 2, RATE, sos, -1400, (1 << 24) - 1, 40, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(p.data(), 100, 2, RATE, sos, -1400, C1, 0, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(p.data(), 100, 2, RATE, sos, -1400, C1, 1025, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(nullptr, 100, 2, RATE, sos, -1400, C1, 40, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(p.data(), 100, 2, RATE, sos, -1400, C1, 40, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_host(p.data(), -1, 2, RATE, sos, -1400, C1, 40, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_level_span() > 0 && mm_level_span() % 8 == 0);
    }
    printf("level_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
