// Stand-alone host check of csrc/tracks.h (the layout of a launch over n tracks: prefix sums,
// the workgroup -> track search and the plane offsets) for a sanitizer build: no context, no
// GPU, never loaded into Python.  It includes that header only.  Build and run on the CPU:
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer \
//     tools/diag/tracks_layout_host_check.cpp -o tracks_layout_host_check && ./tracks_layout_host_check
// For every layout of 1 to 4 tracks with lengths drawn from {0, 1, 11, 12, S - 12, S - 11,
// S - 10, S, S + 1}, for every grid (S = TRACKS_METER_SPAN with the need grid's 11-frame tail,
// S = TRACKS_CEIL_SPAN for the apply grid, S = TRACKS_RS_SPAN for the converter's), it walks every workgroup of the grid and checks
// that the search returns the track and the span a plain loop over the tracks expects, that a
// track without a workgroup is never returned (in front, at the end, two in a row), that
// every plane offset is a multiple of TRACKS_METER_SPAN, and, by writing every span a need
// workgroup stores into a heap block of exactly the size the host allocates, that the planes
// neither overlap nor pass the buffer's end (a store past it is an ASan report).
// The converter's grid (tracks_resample_spans, S = TRACKS_RS_SPAN, lengths in output frames)
// goes through the same walk; there every workgroup also stores its span's output frames
// [n0, n0 + min(S, frames_out - n0)), n0 = (w - first[t]) * S, into a heap block of exactly
// frames_out entries of its track: every frame once, none past the end.
// Ends with "tracks_layout_host_check: 0 failure(s)"; exits non-zero on any failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../python-audio-mastering_amd/csrc/tracks.h"

using namespace mm;

static long failures = 0, layouts = 0, workgroups = 0;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            if (failures < 20) fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

enum Grid { APPLY = 0, NEED = 1, RESAMPLE = 2 };

static int64_t grid_span(int g) { return g == NEED ? TRACKS_METER_SPAN : g == APPLY ? TRACKS_CEIL_SPAN : TRACKS_RS_SPAN; }

static void check_layout(const int64_t *frames, int n, int g) {
    ++layouts;
    const bool need = g == NEED;
    std::vector<int64_t> wgs((size_t)n);
    for (int t = 0; t < n; ++t)
        wgs[(size_t)t] = need ? tracks_need_spans(frames[t]) : g == APPLY ? tracks_apply_spans(frames[t]) : tracks_resample_spans(frames[t]);
    std::vector<uint32_t> first((size_t)n + 1);
    const uint32_t grid = tracks_prefix(wgs.data(), n, first.data());
    const int64_t S = grid_span(g);
    // the grid covers every frame a workgroup must visit, and no span more
    uint32_t w = 0;
    for (int t = 0; t < n; ++t) {
        const int64_t reach = frames[t] > 0 ? frames[t] + (need ? 11 : 0) : 0;
        CHECK(wgs[(size_t)t] * S >= reach && (wgs[(size_t)t] == 0 || (wgs[(size_t)t] - 1) * S < reach));
        CHECK(first[(size_t)t] == w);
        for (int64_t s = 0; s < wgs[(size_t)t]; ++s, ++w) {  // what a plain loop expects of workgroup w
            ++workgroups;
            const int got = tracks_find(first.data(), n, w);
            CHECK(got == t);
            CHECK(got >= 0 && got < n && wgs[(size_t)got] > 0);
            CHECK((int64_t)(w - first[(size_t)got]) == s);
        }
    }
    CHECK(w == grid && first[(size_t)n] == grid);
    if (g == RESAMPLE) {  // what resample_tracks_kernel's workgroups store, track by track
        for (uint32_t v = 0; v < grid; ++v) CHECK(wgs[(size_t)tracks_find(first.data(), n, v)] > 0);
        for (int t = 0; t < n; ++t) {
            std::vector<uint8_t> seen((size_t)frames[t], 0);
            for (uint32_t v = first[(size_t)t]; v < first[(size_t)t + 1]; ++v) {
                const int64_t n0 = (int64_t)(v - first[(size_t)t]) * S;
                CHECK(n0 < frames[t]);
                const int64_t span = frames[t] - n0 < S ? frames[t] - n0 : S;
                for (int64_t i = 0; i < span; ++i) {
                    uint8_t &o = seen.data()[n0 + i];  // (past the block: ASan)
                    CHECK(o == 0);
                    o = 1;
                }
            }
            for (int64_t i = 0; i < frames[t]; ++i) CHECK(seen[(size_t)i] == 1);
        }
        return;
    }
    if (!need) return;
    // the planes: one heap block of exactly what the host allocates, every need span stored once
    const int64_t total = tracks_plane_total(first.data(), n);
    std::vector<uint8_t> owner((size_t)total, 0);
    int64_t end = 0;
    for (int t = 0; t < n; ++t) {
        const int64_t off = tracks_plane_off(first.data(), t), len = tracks_plane_len(frames[t]);
        CHECK(off % TRACKS_METER_SPAN == 0 && len % TRACKS_METER_SPAN == 0);
        CHECK(off >= end);                                // no overlap with the planes before
        CHECK(len == 0 || len >= frames[t] + 11);         // ceil_apply reads r on [0, frames + 11)
        CHECK(off + len <= total);
        for (int64_t s = 0; s < wgs[(size_t)t]; ++s)
            for (int64_t i = 0; i < TRACKS_METER_SPAN; ++i) {
                uint8_t &o = owner.data()[off + s * TRACKS_METER_SPAN + i];  // (past the block: ASan)
                CHECK(o == 0);
                o = (uint8_t)(t + 1);
            }
        end = off + len;
    }
    CHECK(end == total);
    for (int64_t i = 0; i < total; ++i) CHECK(owner[(size_t)i] != 0);  // and the buffer holds nothing else
}

int main() {
    for (int g = APPLY; g <= RESAMPLE; ++g) {
        const int64_t S = grid_span(g);
        const int64_t len[9] = {0, 1, 11, 12, S - 12, S - 11, S - 10, S, S + 1};
        for (int n = 1; n <= 4; ++n) {
            int idx[4] = {0, 0, 0, 0};
            for (;;) {
                int64_t frames[4];
                for (int t = 0; t < n; ++t) frames[t] = len[idx[t]];
                check_layout(frames, n, g);
                int k = 0;
                while (k < n && ++idx[k] == 9) idx[k++] = 0;
                if (k == n) break;
            }
        }
    }
    // the widest search: TRACKS_MAX tracks, every other one empty
    {
        std::vector<int64_t> frames((size_t)TRACKS_MAX);
        for (int t = 0; t < TRACKS_MAX; ++t) frames[(size_t)t] = (t & 1) ? 0 : 1 + 1000 * (t % 7);
        check_layout(frames.data(), TRACKS_MAX, NEED);
        check_layout(frames.data(), TRACKS_MAX, APPLY);
        check_layout(frames.data(), TRACKS_MAX, RESAMPLE);
    }
    printf("%ld layouts, %ld workgroups\n", layouts, workgroups);
    printf("tracks_layout_host_check: %ld failure(s)\n", failures);
    return failures ? 1 : 0;
}
