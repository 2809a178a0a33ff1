// loudness.h — the loudness tail's owner: numpy's float32 np.sum as a program and
// the limits it is built against, the segment ranges of the gating blocks, and
// struct Loudness, the one holder of what the context keeps for the tail (the block
// programs on the device, the cached segment geometry, the staged job's geometry).
// The program part needs no HIP (tools/diag/np_sum_program_check.cpp includes it
// with MM_LOUDNESS_HOST_ONLY); gate.hip takes the limits from here.  Loudness's
// methods are defined in loudness.hip, after the context they work on.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/mastering.h"

// ---- numpy's float32 np.sum as a program (gate.hip kw_blocks_kernel) ----------
constexpr int KB_CHUNK = 8192;   // numpy's reduction buffer (elements)
constexpr int KB_VMAX = 1536;    // leaves + nodes of one block (76 800 frames at 192 kHz: 1199)
constexpr int KB_PMAX = 2560;    // ints of one program (192 kHz: 2430); programs start 16-byte aligned

// The reduction tree of np.sum over n contiguous float32 values: 8192-element
// buffer chunks summed in order, each chunk numpy's pairwise recursion (leaves of
// <= 128 elements).  Serialised as gate.hip's program layout.
struct PwBuild {
    std::vector<int32_t> loff, llen;        // leaves in order
    std::vector<int32_t> na, nb, nh;        // nodes: operands (>= 0 leaf, < 0 node ~k) and height
    std::vector<int32_t> chunk_leaf;
};
inline int32_t pw_node(PwBuild &b, int32_t va, int32_t vb, int32_t ha, int32_t hb, int32_t *h) {
    b.na.push_back(va);
    b.nb.push_back(vb);
    *h = std::max(ha, hb) + 1;
    b.nh.push_back(*h);
    return ~(int32_t)(b.na.size() - 1);
}
inline int32_t pw_rec(PwBuild &b, int32_t off, int32_t m, int32_t *h) {
    if (m <= 128) {  // numpy: m < 8 sequential, else eight accumulators + tail
        b.loff.push_back(off);
        b.llen.push_back(m);
        *h = 0;
        return (int32_t)b.loff.size() - 1;
    }
    int32_t n2 = m / 2;
    n2 -= n2 % 8;
    int32_t ha, hb;
    const int32_t va = pw_rec(b, off, n2, &ha);
    const int32_t vb = pw_rec(b, off + n2, m - n2, &hb);
    return pw_node(b, va, vb, ha, hb, h);
}
// appends the program of np.sum over n elements to `out`
inline void pw_build(int64_t n, std::vector<int32_t> &out) {
    PwBuild b;
    int32_t acc = 0, hacc = 0;
    const int64_t nch = (n + KB_CHUNK - 1) / KB_CHUNK;
    for (int64_t c = 0; c < nch; ++c) {
        b.chunk_leaf.push_back((int32_t)b.loff.size());
        int32_t h;
        const int32_t v = pw_rec(b, (int32_t)(c * KB_CHUNK), (int32_t)std::min<int64_t>(KB_CHUNK, n - c * KB_CHUNK), &h);
        if (c == 0) {  // res = 0 + pairwise(chunk 0): exact (sums of squares are >= +0)
            acc = v;
            hacc = h;
        } else {
            acc = pw_node(b, acc, v, hacc, h, &hacc);
        }
    }
    b.chunk_leaf.push_back((int32_t)b.loff.size());
    const int32_t nl = (int32_t)b.loff.size(), nn = (int32_t)b.na.size();
    // nodes sorted by height (stable): a level reads only lower ones
    std::vector<int32_t> order(nn), pos(nn);
    for (int32_t k = 0; k < nn; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return b.nh[x] < b.nh[y]; });
    for (int32_t k = 0; k < nn; ++k) pos[order[k]] = k;
    auto vidx = [&](int32_t v) { return v >= 0 ? v : nl + pos[~v]; };
    const int32_t nlev = nn ? b.nh[order[nn - 1]] : 0;
    out.push_back(nl);
    out.push_back(nn);
    out.push_back(nlev);
    out.push_back((int32_t)nch);
    out.push_back(n == 0 ? -1 : vidx(acc));
    out.insert(out.end(), b.chunk_leaf.begin(), b.chunk_leaf.end());
    out.insert(out.end(), b.loff.begin(), b.loff.end());
    out.insert(out.end(), b.llen.begin(), b.llen.end());
    for (int32_t k = 0; k < nn; ++k) out.push_back(vidx(b.na[order[k]]));
    for (int32_t k = 0; k < nn; ++k) out.push_back(vidx(b.nb[order[k]]));
    for (int32_t L = 0, k = 0; L <= nlev; ++L) {  // level L: nodes of height L + 1
        while (k < nn && b.nh[order[k]] <= L) ++k;
        out.push_back(k);
    }
}
// The program evaluated on the host with the device's operation order (CPU check
// against np.sum: mm_np_sum_f32).
inline float pw_eval(const int32_t *P, const float *x) {
    const int nl = P[0], nn = P[1], nch = P[3], root = P[4];
    const int32_t *loff = P + 5 + nch + 1, *llen = loff + nl, *na = llen + nl, *nb = na + nn;
    std::vector<float> val((size_t)nl + nn);
    for (int li = 0; li < nl; ++li) {
        const float *e = x + loff[li];
        const int len = llen[li];
        float res;
        if (len < 8) {
            res = e[0];
            for (int i = 1; i < len; ++i) res = res + e[i];
        } else {
            float r[8];
            for (int q = 0; q < 8; ++q) r[q] = e[q];
            int i = 8;
            for (; i < len - (len & 7); i += 8)
                for (int q = 0; q < 8; ++q) r[q] = r[q] + e[i + q];
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (; i < len; ++i) res = res + e[i];
        }
        val[li] = res;
    }
    for (int k = 0; k < nn; ++k) val[nl + k] = val[na[k]] + val[nb[k]];
    return root < 0 ? 0.0f : val[root];
}

// Frames [lo, hi) of a gating block as the range of the S segments (bounds B[0..S])
// that begin in it.
inline std::pair<int64_t, int64_t> seg_range(const int64_t *B, int64_t S, int64_t lo, int64_t hi) {
    return {std::min<int64_t>(std::lower_bound(B, B + S + 1, lo) - B, S),
            std::min<int64_t>(std::lower_bound(B, B + S + 1, hi) - B, S)};
}

#ifndef MM_LOUDNESS_HOST_ONLY
namespace mm {
struct KbArgs;
}

// The gating blocks of a chain's line and, for a timeline of several tracks
// (n_trk > 0), each track's first gating block, first tile and the end of its real
// frames, on the device (unit_geometry).
struct TrackTable {
    int n_trk = 0;
    int64_t n_blocks = 0;
    int64_t *trk_blk = nullptr, *trk_tile0 = nullptr, *trk_end = nullptr;
};

// Segment geometry of ONE line on the device (a staged range, the operator): the
// segment bounds and every gating block as a segment range.
struct SegGeom {
    int64_t n_segs = 0, n_blocks = 0;
    int64_t *bounds = nullptr;
    int32_t *s0 = nullptr, *s1 = nullptr;
};

struct Loudness {
    // exact block energies (kw_blocks_kernel): per block its first frame, length and
    // program; prog == null: the device holds no programs
    int64_t *kb_lo = nullptr;
    int32_t *kb_n = nullptr, *kb_prog_of = nullptr, *kb_prog = nullptr;
    std::vector<int64_t> kb_cache;   // block geometry the programs on the device were built for
    int kb_nvals = 0, kb_pints = 0;  // the largest program's values and ints (kw_blocks' LDS)
    std::vector<int64_t> geom_cache;  // segment geometry already on the device (upload_geometry)
    std::vector<int64_t> job_segb, job_lo, job_hi;  // the staged job's geometry (own_job)

    // Per-block programs on the device for blocks [lo_b, hi_b) of a line.
    int kb_upload(mm_ctx *c, const int64_t *lo, const int64_t *hi, size_t nb);
    // The program fields of kw_blocks_kernel's arguments, from the last kb_upload.
    void kb_fill(mm::KbArgs &kb) const;
    // A single line's segment geometry (uploaded only when it changes).
    int upload_geometry(mm_ctx *c, const mm_job *j, SegGeom *g);
    // A staged job keeps its geometry here: later calls read the library's memory.
    void own_job(mm_job *j) {
        auto take = [](std::vector<int64_t> &v, const int64_t *&p, int64_t n) {
            if (!p) return;
            v.assign(p, p + std::max<int64_t>(n, 0));
            p = v.data();
        };
        take(job_segb, j->seg_bounds, j->n_segs + 1);
        take(job_lo, j->block_lo, j->n_blocks);
        take(job_hi, j->block_hi, j->n_blocks);
    }
};
#endif
