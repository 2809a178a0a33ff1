// Stand-alone host check of mm_r128_host and mm_r128_from_hops (the EBU R 128 report restated
// in plain C++, csrc/r128.hip) for a sanitizer build: no context, no GPU, never loaded into
// Python.  Build the library's translation unit and this file into one program with the
// host side instrumented, and run it on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wno-unused-value -Wno-unused-result \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     python-audio-mastering_amd/csrc/mastering.hip tools/diag/r128_host_check.cpp -lrccl -o r128_host_check
// The signal and the hop vector are heap blocks of exactly the elements the calls may touch
// (frames * channels samples, min(H, cap) energies), so a read past the last frame or a write
// past the last hop is an ASan report.  Shapes: mono and stereo, N = 1, N just below and
// above 0.4 s and 3 s (the first momentary and the first short-term window), the floor rate
// of 2000 Hz, a hop vector shorter than H.  Every hop energy is compared with the definition
// evaluated here (the same sequential filter, summed per channel first: another order), and
// the figures' NaN pattern with the definition's edge cases.  Exits non-zero on any failure.
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

static uint32_t rnd_state = 12345u;
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

static void run(int rate, int64_t N, int ch, int64_t cap_less = 0) {
    double sos[2][5];
    kweight(rate > 3100 ? rate : 8000.0, sos);  // (the design is unstable at or below 3 kHz: stable sections there)
    const int64_t H = 10 * N / rate, cap = H - cap_less > 0 ? H - cap_less : 0;
    std::vector<int16_t> pcm((size_t)(N * ch));
    for (auto &v : pcm) v = (int16_t)((int32_t)(rnd() >> 16) / 4 - 8192);
    std::vector<double> e((size_t)cap, -1.0);
    mm_r128 m;
    CHECK(mm_r128_host(pcm.data(), N, ch, rate, sos, cap ? e.data() : nullptr, cap, &m) == MM_OK);
    CHECK(m.frames == N && m.channels == ch && m.rate == rate && m.hops == H);
    CHECK(m.momentary_blocks == (H >= 4 ? H - 3 : 0) && m.short_term_blocks == (H >= 30 ? H - 29 : 0));
    CHECK(std::isnan(m.integrated) == (H < 4) && std::isnan(m.momentary_max) == (H < 4));
    CHECK(std::isnan(m.short_term_max) == (H < 30) && std::isnan(m.lra) == (H < 30));
    // the definition, one channel after the other
    std::vector<double> ref((size_t)H, 0.0);
    for (int c = 0; c < ch; ++c) {
        double z[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        for (int64_t n = 0; n < (H ? H * (int64_t)rate / 10 : 0); ++n) {
            double y = (double)pcm[(size_t)(n * ch + c)] / 32768.0;
            for (int s = 0; s < 2; ++s) {
                const double x = y, *q = sos[s];
                y = z[s][0] + q[0] * x;
                z[s][0] = (z[s][1] + x * q[1]) - y * q[3];
                z[s][1] = x * q[2] - y * q[4];
            }
            ref[(size_t)((10 * n + 9) / rate)] += y * y;
        }
    }
    for (int64_t i = 0; i < cap; ++i) CHECK(std::fabs(e[(size_t)i] - ref[(size_t)i]) <= 1e-11 * ref[(size_t)i]);  // (2 m 2^-53 for m <= 38400 terms)
    // the tail alone on the reference energies gives the same figures to rounding
    mm_r128 t;
    CHECK(mm_r128_from_hops(H ? ref.data() : nullptr, H, rate, &t) == MM_OK && t.hops == H && t.frames == 0);
    if (H >= 4) CHECK(std::fabs(t.integrated - m.integrated) <= 1e-9 && std::fabs(t.momentary_max - m.momentary_max) <= 1e-9);
    if (H >= 30) CHECK(std::fabs(t.lra - m.lra) <= 1e-9 && t.lra_blocks == m.lra_blocks && t.lra_blocks >= 1);
}

int main() {
    for (int ch = 1; ch <= 2; ++ch) {
        for (int rate : {44100, 48000, 2000, 192000})
            for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)(rate / 10 - 1), (int64_t)(4 * rate / 10 - 1), (int64_t)(4 * rate / 10),
                              (int64_t)(4 * rate / 10 + 1), (int64_t)(3 * rate - 1), (int64_t)(3 * rate), (int64_t)(3 * rate + 1)})
                run(rate, N, ch);
        run(44100, 321987, ch);
        run(44100, 321987, ch, 5);  // a hop vector shorter than H: only its elements are written
        run(2000, 6001, ch);
        run(2005, 6016, ch);        // hops of 200 and 201 frames
    }
    {  // refused arguments, and the tail's edge cases
        double sos[2][5];
        kweight(48000.0, sos);
        std::vector<int16_t> pcm(200, (int16_t)100);
        mm_r128 m;
        CHECK(mm_r128_host(pcm.data(), 100, 3, 48000, sos, nullptr, 0, &m) == MM_ERR_ARG);
        CHECK(mm_r128_host(pcm.data(), 100, 2, 1999, sos, nullptr, 0, &m) == MM_ERR_ARG);
        CHECK(mm_r128_host(pcm.data(), -1, 2, 48000, sos, nullptr, 0, &m) == MM_ERR_ARG);
        CHECK(mm_r128_host(pcm.data(), (int64_t)1 << 31, 2, 48000, sos, nullptr, 0, &m) == MM_ERR_ARG);
        CHECK(mm_r128_host(nullptr, 100, 2, 48000, sos, nullptr, 0, &m) == MM_ERR_ARG);
        CHECK(mm_r128_host(pcm.data(), 100, 2, 48000, nullptr, nullptr, 0, &m) == MM_ERR_ARG);
        CHECK(mm_r128_host(pcm.data(), 100, 2, 48000, sos, nullptr, 4, &m) == MM_ERR_ARG);
        CHECK(mm_r128_host(pcm.data(), 100, 2, 48000, sos, nullptr, 0, nullptr) == MM_ERR_ARG);
        CHECK(mm_r128_from_hops(nullptr, 3, 48000, &m) == MM_ERR_ARG && mm_r128_from_hops(nullptr, 0, 48000, nullptr) == MM_ERR_ARG);
        std::vector<double> zeros(40, 0.0);
        CHECK(mm_r128_from_hops(zeros.data(), 40, 48000, &m) == MM_OK);
        CHECK(m.integrated == -INFINITY && std::isnan(m.relative_gate) && m.lra == 0.0 && m.lra_blocks == 0);
        CHECK(std::isnan(m.lra_low) && std::isnan(m.lra_high) && m.short_term_max == -INFINITY);
        CHECK(mm_r128_span() > 0 && mm_r128_span() % 256 == 0 && mm_r128_span() / 256 <= 200);
    }
    printf("r128_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
