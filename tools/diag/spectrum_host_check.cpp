// Stand-alone host check of mm_spectrum_host and mm_spectrum_from_bins (the spectrum report
// restated in plain C++, csrc/spectrum.hip) and of csrc/spectrum.h (the frames, the groups a
// workgroup owns and where the records lie) for a sanitizer build: no context, no GPU, never
// loaded into Python.  Build the library's translation unit and this file into one program with
// the host side instrumented, and run it on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wno-unused-value -Wno-unused-result \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     python-audio-mastering_amd/csrc/mastering.hip tools/diag/spectrum_host_check.cpp -lrccl -o spectrum_host_check
// The signal, the bin table and the band table are heap blocks of exactly the elements the
// calls may touch (frames * channels samples, (N/2 + 1) * 3 bins, n_bands * 4 figures), so a
// read past the last frame or a write past the last band is an ASan report.  On signals of
// two frames the bins are compared with a direct O(N^2) DFT in long double of every 37th bin
// and the two end bins; the band table with the definition's overlap evaluated here in long
// double; the lengths are 0, 1, N - 1, N, N + H - 1, N + H and 3 N + 5, mono and stereo, at
// 2000, 44100 and 192000 Hz.  The layout: for every F the groups cover every frame once, in
// order, G is a function of F alone, a track has at most SPEC_R_MAX records, and the records of
// 1 to 3 tracks laid out by the prefix sums, written whole into a heap block of exactly the
// size the host allocates, neither overlap nor pass its end.
// Ends with "spectrum_host_check: 0 failure(s)"; exits non-zero on any failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mastering.h"
#include "../../python-audio-mastering_amd/csrc/spectrum.h"
#include "../../python-audio-mastering_amd/csrc/tracks.h"

using namespace mm;

static int failures = 0;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            if (failures < 20) fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static uint32_t rnd_state = 97531u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

static const long double PI_L = 3.141592653589793238462643383279502884L;

static bool close_to(double got, long double want, long double scale, long double rel) {
    return fabsl((long double)got - want) <= rel * scale;
}

static void run(int rate, int64_t frames, int ch, int what) {
    std::vector<int16_t> pcm((size_t)(frames * ch));
    for (size_t i = 0; i < pcm.size(); ++i) {
        const size_t n = i / (size_t)ch, c = i % (size_t)ch;
        switch (what) {
        case 0: pcm[i] = (int16_t)((int32_t)(rnd() >> 16) - 32768); break;                                  // noise, full scale
        case 1: pcm[i] = (int16_t)lrint(20000.0 * std::sin(0.0123 * (double)n * (c ? 3.0 : 1.0))); break;  // a sine a channel
        case 2: pcm[i] = (int16_t)(n == 4097 ? -32768 : 0); break;                                          // an impulse
        default: pcm[i] = 0; break;
        }
    }
    const int64_t F = spec_frames(frames);
    int n_bands = mm_spectrum_bands(rate, 0, nullptr);
    CHECK(n_bands > 0 && n_bands <= MM_SPECTRUM_MAX_BANDS);
    std::vector<double> edges((size_t)n_bands * 3), bands((size_t)n_bands * 4, -1.0), bins((size_t)SPEC_REC, -1.0);
    CHECK(mm_spectrum_bands(rate, n_bands, edges.data()) == n_bands);
    mm_spectrum m;
    memset(&m, 0x55, sizeof m);
    CHECK(mm_spectrum_host(frames ? pcm.data() : nullptr, frames, ch, rate, &m, bands.data(), bins.data()) == MM_OK);
    CHECK(m.frames == frames && m.channels == ch && m.rate == rate && m.n_fft == SPEC_N && m.hop == SPEC_HOP);
    CHECK(m.n_frames == F && m.n_bands == n_bands);
    if (F == 0) {
        for (double v : bins) CHECK(std::isnan(v));
        for (int b = 0; b < n_bands; ++b) CHECK(std::isnan(bands[(size_t)b * 4]) && bands[(size_t)b * 4 + 3] > 0.0);
        CHECK(std::isnan(m.total_ms[0]) && std::isnan(m.total_ms[1]));
        return;
    }
    // the bins by the definition, a direct DFT in long double (two frames at the most: O(N^2) a bin)
    long double pmax = 0.0L;
    for (int k = 0; k <= SPEC_N / 2; ++k) pmax = fmaxl(pmax, (long double)bins[(size_t)k * 3] + (long double)bins[(size_t)k * 3 + 1]);
    if (F <= 2) {
        std::vector<long double> w((size_t)SPEC_N), cs((size_t)SPEC_N), sn((size_t)SPEC_N);
        for (int n = 0; n < SPEC_N; ++n) {
            w[(size_t)n] = 0.5L - 0.5L * cosl(2.0L * PI_L * n / SPEC_N);
            cs[(size_t)n] = cosl(2.0L * PI_L * n / SPEC_N);
            sn[(size_t)n] = sinl(2.0L * PI_L * n / SPEC_N);
        }
        std::vector<int> ks{0, 1, SPEC_N / 2 - 1, SPEC_N / 2};
        for (int k = 37; k < SPEC_N / 2 - 1; k += 37) ks.push_back(k);
        for (int k : ks) {
            long double q[3] = {0.0L, 0.0L, 0.0L};
            for (int64_t f = 0; f < F; ++f) {
                long double xr[2] = {0.0L, 0.0L}, xi[2] = {0.0L, 0.0L};
                for (int c = 0; c < ch; ++c)
                    for (int n = 0; n < SPEC_N; ++n) {
                        const long double v = w[(size_t)n] * pcm[(size_t)((f * SPEC_HOP + n) * ch + c)] / 32768.0L;
                        const size_t a = (size_t)(((int64_t)k * n) % SPEC_N);
                        xr[c] += v * cs[a];
                        xi[c] -= v * sn[a];
                    }
                q[0] += xr[0] * xr[0] + xi[0] * xi[0];
                q[1] += xr[1] * xr[1] + xi[1] * xi[1];
                q[2] += xr[0] * xr[1] + xi[0] * xi[1];
            }
            for (int c = 0; c < 3; ++c) CHECK(close_to(bins[(size_t)k * 3 + c], q[c] / F, pmax, 1e-12L));
        }
    }
    // the bands and the totals by the definition's overlap, in long double
    const long double df = (long double)rate / SPEC_N, nyq = 0.5L * rate, norm = (long double)SPEC_N * (3.0L * SPEC_N / 8.0L);
    long double total[2] = {0.0L, 0.0L};
    for (int k = 0; k <= SPEC_N / 2; ++k)
        for (int c = 0; c < 2; ++c) total[c] += (k == 0 || k == SPEC_N / 2 ? 1.0L : 2.0L) * bins[(size_t)k * 3 + c];
    for (int c = 0; c < 2; ++c) CHECK(close_to(m.total_ms[c], total[c] / norm, total[0] / norm + total[1] / norm, 1e-12L));
    if (ch == 1) CHECK(m.total_ms[1] == 0.0);
    for (int b = 0; b < n_bands; ++b) {
        const long double lo = edges[(size_t)b * 3], hi = edges[(size_t)b * 3 + 2];
        CHECK(b == 0 || edges[(size_t)b * 3] == edges[(size_t)(b - 1) * 3 + 2]);
        CHECK(lo < hi && hi <= nyq && (b + 1 < n_bands || hi == nyq));
        long double s[3] = {0.0L, 0.0L, 0.0L};
        for (int k = 0; k <= SPEC_N / 2; ++k) {
            const long double bl = fmaxl(0.0L, (k - 0.5L) * df), bh = fminl(nyq, (k + 0.5L) * df);
            const long double ov = fminl(bh, hi) - fmaxl(bl, lo);
            if (ov <= 0.0L) continue;
            for (int c = 0; c < 3; ++c) s[c] += ov / (bh - bl) * (k == 0 || k == SPEC_N / 2 ? 1.0L : 2.0L) * bins[(size_t)k * 3 + c];
        }
        for (int c = 0; c < 3; ++c) CHECK(close_to(bands[(size_t)b * 4 + c], s[c] / norm, fabsl(s[0]) / norm + fabsl(s[1]) / norm + 1e-300L, 1e-11L));
        CHECK(close_to(bands[(size_t)b * 4 + 3], (hi - lo) / df, (hi - lo) / df, 1e-12L));
    }
    // the tail alone on the table gives the same bits
    std::vector<double> again((size_t)n_bands * 4, -2.0);
    mm_spectrum t;
    CHECK(mm_spectrum_from_bins(bins.data(), frames, ch, rate, &t, again.data()) == MM_OK);
    CHECK(memcmp(again.data(), bands.data(), again.size() * sizeof(double)) == 0 && memcmp(&t, &m, sizeof m) == 0);
}

static void layout() {
    for (int64_t F = 0; F <= 3 * (int64_t)SPEC_G0 * SPEC_R_MAX; F += (F < 3 * SPEC_G0 ? 1 : 1009)) {
        const int64_t G = spec_group(F), groups = spec_groups(F);
        CHECK(G >= SPEC_G0 && groups <= SPEC_R_MAX && (F == 0) == (groups == 0));
        int64_t next = 0;
        for (int64_t g = 0; g < groups; ++g) {
            int64_t f0;
            const int64_t n = spec_group_frames(F, g, &f0);
            CHECK(f0 == next && n >= 1 && n <= G);
            next = f0 + n;
        }
        CHECK(next == F);
    }
    CHECK(spec_frames(0) == 0 && spec_frames(SPEC_N - 1) == 0 && spec_frames(SPEC_N) == 1 && spec_frames(SPEC_N + SPEC_HOP - 1) == 1);
    CHECK(spec_frames(SPEC_N + SPEC_HOP) == 2 && spec_frames(((int64_t)1 << 31) - 1) == 524286);
    const int64_t len[6] = {0, 1, SPEC_G0, SPEC_G0 + 1, 3 * SPEC_G0 + 5, 2};
    for (int n = 1; n <= 3; ++n)
        for (int code = 0; code < 216; ++code) {
            int64_t wgs[3];
            uint32_t first[4];
            for (int t = 0, c = code; t < n; ++t, c /= 6) wgs[t] = spec_groups(len[c % 6]);
            const uint32_t grid = tracks_prefix(wgs, n, first);
            std::vector<uint8_t> owner((size_t)grid * SPEC_REC, 0);  // exactly what the host allocates
            for (uint32_t w = 0; w < grid; ++w) {
                const int t = tracks_find(first, n, w);
                CHECK(t >= 0 && t < n && w >= first[t] && w < first[t + 1]);
                for (int i = 0; i < SPEC_REC; ++i) {
                    uint8_t &o = owner.data()[(size_t)w * SPEC_REC + (size_t)i];  // (past the block: ASan)
                    CHECK(o == 0);
                    o = 1;
                }
            }
            for (uint8_t o : owner) CHECK(o == 1);
        }
}

int main() {
    for (int ch = 1; ch <= 2; ++ch)
        for (int rate : {2000, 44100, 192000})
            for (int64_t frames : {(int64_t)0, (int64_t)1, (int64_t)SPEC_N - 1, (int64_t)SPEC_N, (int64_t)SPEC_N + SPEC_HOP - 1,
                                   (int64_t)SPEC_N + SPEC_HOP, (int64_t)3 * SPEC_N + 5})
                for (int what = 0; what < 4; ++what) {
                    if (rate != 44100 && what != 0) continue;  // (the rate reaches the tail alone)
                    run(rate, frames, ch, what);
                }
    layout();
    {  // refused arguments
        std::vector<int16_t> pcm(200, (int16_t)100);
        std::vector<double> bins((size_t)SPEC_REC, 0.0);
        mm_spectrum m;
        CHECK(mm_spectrum_host(pcm.data(), 100, 3, 48000, &m, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_host(pcm.data(), 100, 2, 1999, &m, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_host(pcm.data(), -1, 2, 48000, &m, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_host(pcm.data(), (int64_t)1 << 31, 2, 48000, &m, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_host(nullptr, 100, 2, 48000, &m, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_host(pcm.data(), 100, 2, 48000, nullptr, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_host(pcm.data(), 100, 2, 48000, &m, nullptr, nullptr) == MM_OK && m.n_frames == 0);
        CHECK(mm_spectrum_from_bins(nullptr, 100, 2, 48000, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_from_bins(bins.data(), 100, 2, 48000, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_from_bins(bins.data(), 100, 2, 1999, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_spectrum_bands(1999, 0, nullptr) == MM_ERR_ARG && mm_spectrum_bands(48000, 1, nullptr) == MM_ERR_ARG);
    }
    printf("spectrum_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
