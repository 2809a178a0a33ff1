// Stand-alone host check of mm_qc_host and mm_qc_from_hops (the delivery QC report restated in
// plain C++, csrc/qc.hip) for a sanitizer build: no context, no GPU, never loaded into Python.
// Build the library's translation unit and this file into one program with the host side
// instrumented, and run it on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Wno-unused-value -Wno-unused-result \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     python-audio-mastering_amd/csrc/mastering.hip tools/diag/qc_host_check.cpp -lrccl -o qc_host_check
// The signal and the hop table are heap blocks of exactly the elements the calls may touch
// (frames * channels samples, H * 3 sums), so a read past the last frame or a write past the
// last hop is an ASan report, and an overflowing sum a UBSan one.  Every field is compared
// with the definition evaluated here another way: the totals and hop sums in __int128 with the
// hop of a frame from its index, the runs from their starts (a frame whose predecessor differs)
// by walking forward, the gate in __int128.  Shapes: mono and stereo, N = 0, 1, 2, r - 1, r,
// one hop - 1 / + 0 / + 1, four hops - 1 / + 0 / + 1, at 2000, 11025, 44100 and 192000 Hz, on
// noise, on both rails and -32768, on clipped noise and on silence with a gap.  Exits non-zero
// on any failure.
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

typedef __int128 i128;

static uint32_t rnd_state = 2468u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

// the runs of equal non-zero v from their starts: samples, runs >= r, the longest and its start
static void runs_of(const std::vector<int> &v, int r, int64_t *samples, int64_t *runs, int64_t *longest, int64_t *at) {
    const int64_t N = (int64_t)v.size();
    *samples = *runs = *longest = 0;
    *at = -1;
    for (int64_t n = 0; n < N; ++n) {
        if (v[(size_t)n] == 0) continue;
        ++*samples;
        if (n > 0 && v[(size_t)(n - 1)] == v[(size_t)n]) continue;  // not a start
        int64_t len = 1;
        while (n + len < N && v[(size_t)(n + len)] == v[(size_t)n]) ++len;
        if (len >= r) ++*runs;
        if (len > *longest) {
            *longest = len;
            *at = n;
        }
    }
}

static void run(int rate, int64_t N, int ch, int what, int q, int r) {
    const int64_t H = 10 * N / rate;
    std::vector<int16_t> pcm((size_t)(N * ch));
    for (size_t i = 0; i < pcm.size(); ++i) {
        const int32_t noise = (int32_t)(rnd() >> 16) - 32768;
        switch (what) {
        case 0: pcm[i] = (int16_t)(noise / 2); break;
        case 1: pcm[i] = 32767; break;
        case 2: pcm[i] = -32767; break;
        case 3: pcm[i] = -32768; break;
        case 4: pcm[i] = (int16_t)(noise > 20000 ? 32767 : (noise < -20000 ? -32768 : noise)); break;  // clipped, both rails
        default: pcm[i] = (int16_t)((i / (size_t)ch) % 97 < 40 ? (int32_t)(rnd() % 3) - 1 : noise / 8); break;  // silent gaps
        }
    }
    std::vector<int64_t> table((size_t)(H * 3), -1);
    mm_qc m;
    CHECK(mm_qc_host(N ? pcm.data() : nullptr, N, ch, rate, q, r, &m, H ? table.data() : nullptr) == MM_OK);
    CHECK(m.frames == N && m.channels == ch && m.rate == rate && m.hops == H && m.silence_lsb == q && m.min_run == r);
    // totals and hop sums
    i128 sum[2] = {0, 0}, sq[2] = {0, 0}, cross = 0;
    std::vector<i128> ref((size_t)(H * 3), 0);
    int smin[2] = {0, 0}, smax[2] = {0, 0};
    uint32_t orb[2] = {0, 0};
    std::vector<int> rail[2], silent((size_t)N, 1);
    for (int c = 0; c < 2; ++c) rail[c].assign((size_t)N, 0);
    for (int64_t n = 0; n < N; ++n) {
        const int64_t h = (10 * n + 9) / rate;
        int s[2] = {pcm[(size_t)(n * ch)], ch == 2 ? pcm[(size_t)(n * ch + 1)] : 0};
        for (int c = 0; c < ch; ++c) {
            sum[c] += s[c];
            sq[c] += (i128)s[c] * s[c];
            smin[c] = n == 0 || s[c] < smin[c] ? s[c] : smin[c];
            smax[c] = n == 0 || s[c] > smax[c] ? s[c] : smax[c];
            orb[c] |= (uint16_t)s[c];
            rail[c][(size_t)n] = s[c] == 32767 ? 1 : (s[c] <= -32767 ? -1 : 0);
            if (std::abs(s[c]) > q) silent[(size_t)n] = 0;
        }
        cross += (i128)s[0] * s[1];
        if (h < H) {
            ref[(size_t)(3 * h)] += (i128)s[0] * s[0];
            ref[(size_t)(3 * h + 1)] += (i128)s[1] * s[1];
            ref[(size_t)(3 * h + 2)] += (i128)s[0] * s[1];
        }
    }
    CHECK((i128)m.cross == cross);
    for (int c = 0; c < 2; ++c) {
        CHECK((i128)m.sum[c] == sum[c] && (i128)m.sq[c] == sq[c] && m.smin[c] == smin[c] && m.smax[c] == smax[c] && m.or_bits[c] == orb[c]);
        int64_t samples, runs, longest, at;
        runs_of(rail[c], r, &samples, &runs, &longest, &at);
        CHECK(m.clip_samples[c] == samples && m.clip_runs[c] == runs && m.clip_longest[c] == longest && m.clip_longest_at[c] == at);
    }
    for (int64_t i = 0; i < H * 3; ++i) CHECK((i128)table[(size_t)i] == ref[(size_t)i]);
    int64_t samples, runs, longest, at, lead = 0, trail = 0;
    runs_of(silent, 1, &samples, &runs, &longest, &at);
    while (lead < N && silent[(size_t)lead]) ++lead;
    while (trail < N && silent[(size_t)(N - 1 - trail)]) ++trail;
    CHECK(m.silent_frames == samples && m.silence_longest == longest && m.silence_longest_at == at);
    CHECK(m.lead_silence == lead && m.trail_silence == trail);
    // step 5, and the tail alone on the table
    int64_t windows = 0, negative = 0, min_hop = -1;
    double rho_min = NAN;
    for (int64_t j = 0; ch == 2 && j + 4 <= H; ++j) {
        i128 A = 0, B = 0, X = 0;
        for (int k = 0; k < 4; ++k) A += ref[(size_t)(3 * (j + k))], B += ref[(size_t)(3 * (j + k) + 1)], X += ref[(size_t)(3 * (j + k) + 2)];
        if (A + B < (i128)2048 * ((j + 4) * (int64_t)rate / 10 - j * (int64_t)rate / 10)) continue;
        ++windows;
        negative += X < 0;
        const double rho = A == 0 || B == 0 ? 0.0 : (double)(int64_t)X / std::sqrt((double)(int64_t)A * (double)(int64_t)B);
        if (min_hop < 0 || rho < rho_min) rho_min = rho, min_hop = j;
    }
    CHECK(m.corr_windows == windows && m.corr_negative == negative && m.corr_min_hop == min_hop);
    CHECK(min_hop < 0 ? std::isnan(m.corr_min) : memcmp(&m.corr_min, &rho_min, 8) == 0);
    if (ch == 2) {
        mm_qc t;
        memset(&t, 0x55, sizeof t);
        CHECK(mm_qc_from_hops(H ? table.data() : nullptr, H, rate, &t) == MM_OK && t.hops == H && t.rate == rate);
        CHECK(t.corr_windows == windows && t.corr_negative == negative && t.corr_min_hop == min_hop);
        CHECK(min_hop < 0 ? std::isnan(t.corr_min) : memcmp(&t.corr_min, &rho_min, 8) == 0);
        CHECK(t.frames == 0x5555555555555555ll && t.cross == 0x5555555555555555ll);  // (no other field is touched)
    }
}

int main() {
    for (int ch = 1; ch <= 2; ++ch)
        for (int rate : {2000, 11025, 44100, 192000})
            for (int r : {1, 3, 7}) {
                const int64_t hop = rate / 10;
                for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)(r - 1), (int64_t)r, hop - 1, hop, hop + 1, 4 * hop - 1,
                                  4 * hop, 4 * hop + 1, 4 * hop + 2})
                    for (int what = 0; what < 6; ++what) run(rate, N, ch, what, r == 7 ? 0 : 1, r);
            }
    {  // refused arguments
        std::vector<int16_t> pcm(200, (int16_t)100);
        mm_qc m;
        CHECK(mm_qc_host(pcm.data(), 100, 3, 48000, 1, 3, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(pcm.data(), 100, 2, 1999, 1, 3, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(pcm.data(), -1, 2, 48000, 1, 3, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(pcm.data(), (int64_t)1 << 31, 2, 48000, 1, 3, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(nullptr, 100, 2, 48000, 1, 3, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(pcm.data(), 100, 2, 48000, -1, 3, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(pcm.data(), 100, 2, 48000, 32768, 3, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(pcm.data(), 100, 2, 48000, 1, 0, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(pcm.data(), 100, 2, 48000, 1, 65536, &m, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_host(pcm.data(), 100, 2, 48000, 1, 3, nullptr, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_from_hops(nullptr, 3, 48000, &m) == MM_ERR_ARG && mm_qc_from_hops(nullptr, 0, 48000, nullptr) == MM_ERR_ARG);
        CHECK(mm_qc_from_hops(nullptr, 0, 1999, &m) == MM_ERR_ARG && mm_qc_from_hops(nullptr, -1, 48000, &m) == MM_ERR_ARG);
        CHECK(mm_qc_span() > 0 && mm_qc_span() % 256 == 0);
    }
    printf("qc_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
