// Stand-alone host check of mm_fir_host (the linear-phase FIR restated in plain C++,
// csrc/fir.hip) for a sanitizer build: no context, no GPU, never loaded into Python.  Build the
// library's translation unit and this file into one program with the host side instrumented,
// and run it on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wno-unused-value -Wno-unused-result \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     python-audio-mastering_amd/csrc/mastering.hip tools/diag/fir_host_check.cpp -lrccl -o fir_host_check
// The input, the taps and the output are heap blocks of exactly the bytes the call may touch
// (frames * channels, K and frames * channels elements), so a read before the first frame, past
// the last one or past the taps, or a write past the last output frame, is an ASan report.
// Lengths run through N = 0, 1, 2, every N from H - 1 to K + 1 (K = 2047: mono, and stereo in
// steps of 97; K = 8191: N = 8192 alone) and 3 K + 7, with constants at both rails, and every output is compared with the definition evaluated here in __int128.
// Exits non-zero on any failure.
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

// Symmetric taps of both signs, up to 1.75 * 2^23 / K each with a positive bias, so that sum |c|
// lies below 2^24 and the DC gain of a long table near 1.5: the rails clip.
static std::vector<int32_t> table(int K) {
    std::vector<int32_t> c((size_t)K);
    const int H = (K - 1) / 2, a = (1 << 23) / K;
    for (int k = 0; k <= H; ++k) c[(size_t)k] = c[(size_t)(K - 1 - k)] = (int32_t)(rnd() % (uint32_t)(2 * a + 1)) - a / 4;
    return c;
}

static void run(int K, int64_t N, int ch, int fill) {
    const std::vector<int32_t> c = table(K);
    const int64_t H = (K - 1) / 2;
    mm_fir f;
    memset(&f, 0, sizeof f);
    f.rate = 48000;
    f.K = K;
    f.taps = c.data();
    std::vector<int16_t> in((size_t)(N * ch)), out((size_t)(N * ch), (int16_t)77);
    for (auto &v : in) v = fill == 0 ? (int16_t)(rnd() >> 16) : (int16_t)fill;
    mm_fir_result st;
    CHECK(mm_fir_host(N ? in.data() : nullptr, N, ch, &f, N ? out.data() : nullptr, &st) == MM_OK);
    CHECK(st.frames == N && st.channels == ch && st.K == K && st.rate == 48000);
    int64_t clipped[2] = {0, 0};
    int32_t peak[2] = {0, 0}, unclipped[2] = {0, 0};
    for (int64_t n = 0; n < N; ++n)
        for (int cc = 0; cc < ch; ++cc) {
            __int128 acc = 0;
            for (int k = 0; k < K; ++k) {
                const int64_t s = n + H - k;
                if (s >= 0 && s < N) acc += (__int128)c[(size_t)k] * in[(size_t)(s * ch + cc)];
            }
            acc += (__int128)1 << 21;
            const int64_t y = (int64_t)(acc >= 0 ? acc >> 22 : -((-acc + (((__int128)1 << 22) - 1)) >> 22));
            const int64_t d = y > 32767 ? 32767 : (y < -32768 ? -32768 : y);
            clipped[cc] += d != y;
            const int32_t a = (int32_t)(d < 0 ? -d : d), u = (int32_t)(y < 0 ? -y : y);
            peak[cc] = a > peak[cc] ? a : peak[cc];
            unclipped[cc] = u > unclipped[cc] ? u : unclipped[cc];
            CHECK(out[(size_t)(n * ch + cc)] == (int16_t)d);
        }
    for (int cc = 0; cc < ch; ++cc)
        CHECK(st.clipped[cc] == clipped[cc] && st.peak[cc] == peak[cc] && st.peak_unclipped[cc] == unclipped[cc]);
    if (fill && K >= 129) CHECK(clipped[0] > 0);
}

int main() {
    for (int K : {3, 5, 9, 129, 2047})
        for (int ch = 1; ch <= 2; ++ch) {
            const int64_t H = (K - 1) / 2;
            for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)(3 * K + 7)}) run(K, N, ch, 0);
            for (int64_t N = H - 1 > 0 ? H - 1 : 0; N <= K + 1; N += K > 200 && ch == 2 ? 97 : 1) run(K, N, ch, 0);
            for (int64_t N : {H, H + 1, (int64_t)K, (int64_t)(K + 1)}) run(K, N, ch, 0);
            run(K, 2 * K + 5, ch, 32767);  // a constant at both rails: the DC gain is above 1, so it clips
            run(K, 2 * K + 5, ch, -32768);
        }
    run(8191, 8192, 2, 0);
    {  // refused arguments: nothing is written
        std::vector<int32_t> c = table(9);
        std::vector<int16_t> in(24, (int16_t)1), out(24, (int16_t)77);
        mm_fir_result st;
        mm_fir f;
        memset(&f, 0, sizeof f);
        f.rate = 44100;
        f.K = 9;
        f.taps = c.data();
        CHECK(mm_fir_host(in.data(), 8, 1, &f, out.data(), &st) == MM_OK && st.frames == 8);
        for (auto &v : out) v = 77;
        CHECK(mm_fir_host(in.data(), 8, 3, &f, out.data(), &st) == MM_ERR_ARG);
        CHECK(mm_fir_host(nullptr, 8, 1, &f, out.data(), &st) == MM_ERR_ARG);
        CHECK(mm_fir_host(in.data(), 8, 1, &f, nullptr, &st) == MM_ERR_ARG);
        CHECK(mm_fir_host(in.data(), 8, 1, nullptr, out.data(), &st) == MM_ERR_ARG);
        CHECK(mm_fir_host(in.data(), -1, 1, &f, out.data(), &st) == MM_ERR_ARG);
        mm_fir bad = f;
        bad.K = 8;
        CHECK(mm_fir_host(in.data(), 8, 1, &bad, out.data(), &st) == MM_ERR_ARG);
        bad.K = 1;
        CHECK(mm_fir_host(in.data(), 8, 1, &bad, out.data(), &st) == MM_ERR_ARG);
        bad.K = 8193;
        CHECK(mm_fir_host(in.data(), 8, 1, &bad, out.data(), &st) == MM_ERR_ARG);
        bad = f;
        bad.taps = nullptr;
        CHECK(mm_fir_host(in.data(), 8, 1, &bad, out.data(), &st) == MM_ERR_ARG);
        c[1] += 1;  // one tap off symmetry
        CHECK(mm_fir_host(in.data(), 8, 1, &f, out.data(), &st) == MM_ERR_ARG);
        c[1] -= 1;
        std::vector<int32_t> full = {1 << 22, 0, 1 << 23, 0, 1 << 22};  // sum |c| = 2^24 exactly
        bad = f;
        bad.K = 5;
        bad.taps = full.data();
        CHECK(mm_fir_host(in.data(), 8, 1, &bad, out.data(), &st) == MM_ERR_ARG);
        full[2] -= 1;
        for (auto v : out) CHECK(v == 77);
        CHECK(mm_fir_host(in.data(), 8, 1, &bad, out.data(), &st) == MM_OK);
        CHECK(mm_fir_span() > 0);
    }
    printf("fir_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
