// Stand-alone host check of mm_ceiling_host (the true-peak ceiling restated in plain C++,
// csrc/ceiling.hip) for a sanitizer build: no context, no GPU, never loaded into Python.
// Build the library's translation unit and this file into one program with the host
// side instrumented, and run it on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wno-unused-value -Wno-unused-result \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     python-audio-mastering_amd/csrc/mastering.hip tools/diag/ceiling_host_check.cpp -lrccl -o ceiling_host_check
// It runs the boundary cases of tests/test_ceiling.py and the smallest and widest
// windows on short buffers (every index the host loops form lies at an edge), checks the
// guarantee tp_out <= C and that tp_in is the linked peak of mm_true_peak_host (the two
// share one host FIR), and exits non-zero on any failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

static mm_ceiling run(std::vector<int16_t> &pcm, int channels, int32_t C, int32_t W) {
    mm_ceiling m;
    const int rc = mm_ceiling_host(pcm.data(), (int64_t)(pcm.size() / channels), channels, C, W, &m);
    CHECK(rc == MM_OK);
    CHECK(m.tp_in_q28 <= C || m.tp_out_q28 <= C);
    return m;
}

int main() {
    const int32_t ONE = 1 << 16, GUARD = 8286;
    {  // a lone impulse: untouched at C == P, limited at C == P - 1
        const int32_t peak = 7964 * 20000;
        std::vector<int16_t> a(64, 0), b;
        a[30] = 20000;
        b = a;
        mm_ceiling m = run(a, 1, peak, 4);
        CHECK(m.limited_frames == 0 && m.tp_out_q28 == peak && a[30] == 20000);
        m = run(b, 1, peak - 1, 4);
        CHECK(m.limited_frames > 0 && b[30] == 19999 && m.tp_out_q28 <= peak - 1);
    }
    for (int32_t W : {1, 16}) {  // the smaller impulse at P == C_t keeps r = ONE, at C_t + 1 it does not
        const int32_t small = 15000, Ct = 7964 * small;
        const int at = 50 + 2 * W + 113;
        int64_t limited[2];
        for (int k = 0; k < 2; ++k) {
            std::vector<int16_t> p(400, 0);
            p[50] = 32767;
            p[at] = (int16_t)small;
            limited[k] = run(p, 1, Ct + GUARD - k, W).limited_frames;
        }
        CHECK(limited[1] == limited[0] + 4 * W + 13);
    }
    for (int channels : {1, 2})  // every window on buffers shorter and longer than it, full-scale noise
        for (int32_t W : {1, 2, 220, 1024})
            for (int64_t n : {1, 2, 11, 12, 13, 500, 3000}) {
                std::vector<int16_t> p((size_t)(n * channels));
                uint32_t s = (uint32_t)(n * 31 + W * 7 + channels);
                for (auto &v : p) v = (int16_t)((s = s * 1664525u + 1013904223u) >> 16);
                mm_meter tp;  // the meter's host restatement on the input: the same FIR, so the same peak
                CHECK(mm_true_peak_host(p.data(), n, channels, &tp) == MM_OK);
                const mm_ceiling m = run(p, channels, 1 << 27, W);
                CHECK(m.frames == n && m.window == W && m.min_gain_q16 <= ONE && m.trim_q16 <= ONE);
                CHECK(m.tp_in_q28 == std::max(tp.true_peak_q28[0], channels == 2 ? tp.true_peak_q28[1] : 0));
            }
    {  // zero frames and refused arguments
        mm_ceiling m;
        CHECK(mm_ceiling_host(nullptr, 0, 2, 1 << 27, 16, &m) == MM_OK && m.frames == 0);
        int16_t one = 0;
        CHECK(mm_ceiling_host(&one, 1, 1, (1 << 24) - 1, 16, &m) == MM_ERR_ARG);
        CHECK(mm_ceiling_host(&one, 1, 1, 1 << 27, 1025, &m) == MM_ERR_ARG);
        CHECK(mm_ceiling_host(&one, 1, 3, 1 << 27, 16, &m) == MM_ERR_ARG);
    }
    printf("ceiling_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
