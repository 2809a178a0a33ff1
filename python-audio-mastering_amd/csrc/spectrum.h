// spectrum.h — the geometry of the spectrum report (spectrum.hip; mm_spectrum in
// include/mastering.h): the frames of a signal, the groups of frames a workgroup owns and
// where a track's records lie.  Plain integer arithmetic, host and device alike, with no other
// header of the library: the tables the host uploads, the kernels and the stand-alone check
// tools/diag/spectrum_host_check.cpp all go through it.
//
//   F = frames of a signal of `frames` samples a channel: 0 below SPEC_N, else
//       (frames - SPEC_N) / SPEC_HOP + 1; frame j covers [j * SPEC_HOP, j * SPEC_HOP + SPEC_N)
//   G = frames a workgroup owns, a function of F ALONE (so a track of a batch is cut as the
//       same track alone is): max(SPEC_G0, ceil(F / SPEC_R_MAX))
//   groups = ceil(F / G); group g owns frames [g * G, min(F, (g + 1) * G))
//   a record = SPEC_REC doubles ([SPEC_BINS][3]); track t's records lie at first[t] * SPEC_REC
//       of one buffer of first[n] * SPEC_REC doubles, first[] the prefix sums of the groups
//       (tracks.h: tracks_prefix, tracks_find)
// A record is 98 328 bytes.  A whole group of SPEC_G0 = 16 frames reads 16 * 4096 new sample
// frames, 131 072 bytes of mono int16, so the records of a call stay below the bytes of its
// int16 input from 45 frames on (mono; stereo: from 9), and SPEC_R_MAX bounds them at 50 MB a
// track whatever its length.  Below that a signal has at most three records.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MM_SPEC_HD __host__ __device__
#else
#define MM_SPEC_HD
#endif

namespace mm {

constexpr int SPEC_N = 8192;                // frame length, at every rate
constexpr int SPEC_HOP = 4096;              // hop
constexpr int SPEC_BINS = SPEC_N / 2 + 1;   // k = 0 .. N/2
constexpr int SPEC_REC = SPEC_BINS * 3;     // doubles of a record and of a bin table: S_L, S_R, C a bin
constexpr int SPEC_G0 = 16;                 // frames a workgroup owns at least
constexpr int SPEC_R_MAX = 512;             // records a track has at most

MM_SPEC_HD inline int64_t spec_frames(int64_t frames) { return frames < SPEC_N ? 0 : (frames - SPEC_N) / SPEC_HOP + 1; }

MM_SPEC_HD inline int64_t spec_group(int64_t F) {
    const int64_t need = (F + SPEC_R_MAX - 1) / SPEC_R_MAX;
    return need > SPEC_G0 ? need : SPEC_G0;
}

MM_SPEC_HD inline int64_t spec_groups(int64_t F) {
    const int64_t G = spec_group(F);
    return (F + G - 1) / G;
}

// the frames of group g: [*f0, *f0 + returned count)
MM_SPEC_HD inline int64_t spec_group_frames(int64_t F, int64_t g, int64_t *f0) {
    const int64_t G = spec_group(F);
    *f0 = g * G;
    return F - *f0 < G ? F - *f0 : G;
}

}  // namespace mm
