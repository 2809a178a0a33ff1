// tracks.h — the layout of a launch over n tracks (the ceiling, the converter, the QC and
// spectrum reports and the level's gain, each in its own file): every track owns a run of
// consecutive workgroups, one a span of its frames, and a workgroup finds its track by a
// search over the prefix sums of those runs.  Plain integer arithmetic, host and device
// alike, with no other header of the library: the tables the host uploads, the kernels and
// the stand-alone check tools/diag/tracks_layout_host_check.cpp all go through it.
//
//   first[t]  = workgroups of the tracks before t (first[0] = 0, first[n] = the grid)
//   track of workgroup w = the largest t with first[t] <= w   (w < first[n])
// A track without a workgroup (no frames) has first[t] == first[t + 1] and is never found:
// the largest such t is the track that follows, and after the last track with workgroups
// first[t] == first[n] > w.  The converter's grid counts spans of OUTPUT frames
// (tracks_resample_spans of ceil(frames * L / M)).  The need grid's prefix sums also place
// the planes: track t's r - 1 plane holds whole spans at first_need[t] * TRACKS_METER_SPAN of
// one buffer of first_need[n] * TRACKS_METER_SPAN entries, so planes neither overlap nor
// leave their spans' 16-byte alignment.  A single signal is the case n = 1 of the same launch
// (the search then reads no table); meter.hip counts its spans with the same functions.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MM_TRACKS_HD __host__ __device__
#else
#define MM_TRACKS_HD
#endif

namespace mm {

constexpr int TRACKS_MAX = 256;           // MM_ALBUM_TRACKS
constexpr int TRACKS_METER_SPAN = 2048;   // METER_SPAN: frames m of a need / peak workgroup
constexpr int TRACKS_CEIL_SPAN = 4096;    // CEIL_SPAN: frames n of an apply / trim workgroup
constexpr int TRACKS_RS_SPAN = 1024;      // RS_SPAN: output frames of a converter workgroup

// workgroups of a track of `frames` frames on the need / peak grid (m in [0, frames + 11))
MM_TRACKS_HD inline int64_t tracks_need_spans(int64_t frames) {
    return frames > 0 ? (frames + 11 + TRACKS_METER_SPAN - 1) / TRACKS_METER_SPAN : 0;
}

// on the apply / trim grid (n in [0, frames))
MM_TRACKS_HD inline int64_t tracks_apply_spans(int64_t frames) {
    return frames > 0 ? (frames + TRACKS_CEIL_SPAN - 1) / TRACKS_CEIL_SPAN : 0;
}

// on the converter's grid (output frames n in [0, frames_out))
MM_TRACKS_HD inline int64_t tracks_resample_spans(int64_t frames_out) {
    return frames_out > 0 ? (frames_out + TRACKS_RS_SPAN - 1) / TRACKS_RS_SPAN : 0;
}

// first[0 .. n] from the workgroups of every track; returns the grid
MM_TRACKS_HD inline uint32_t tracks_prefix(const int64_t *wgs, int n, uint32_t *first) {
    uint32_t run = 0;
    for (int t = 0; t < n; ++t) {
        first[t] = run;
        run += (uint32_t)wgs[t];
    }
    first[n] = run;
    return run;
}

// the track of workgroup w < first[n] (at most 8 steps for n <= 256)
MM_TRACKS_HD inline int tracks_find(const uint32_t *first, int n, uint32_t w) {
    int lo = 0, hi = n;  // first[lo] <= w < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

// track t's plane in the one plane buffer: offset, length (whole spans) and the buffer's size
MM_TRACKS_HD inline int64_t tracks_plane_off(const uint32_t *first_need, int t) {
    return (int64_t)first_need[t] * TRACKS_METER_SPAN;
}
MM_TRACKS_HD inline int64_t tracks_plane_len(int64_t frames) { return tracks_need_spans(frames) * TRACKS_METER_SPAN; }
MM_TRACKS_HD inline int64_t tracks_plane_total(const uint32_t *first_need, int n) { return tracks_plane_off(first_need, n); }

}  // namespace mm
