// control.h — the chain's control block: its typed readback header, its layout as
// one pure function, and ChainCtl, the one owner of the block, of the mapped host
// block its readback area arrives in, and of what is known about their contents.
// The layout part needs no HIP (tools/diag/control_layout_check.cpp includes it
// with MM_CONTROL_LAYOUT_ONLY); the rest follows common.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mastering.h"

// Head of the readback area (the first bytes of the control block, brought to the
// host once per chain pass); the per-chunk active counts, int32 [3][chunks], follow.
struct RbHead {
    unsigned lb_error, pad0[3];    // IIR look-back timeout (never expected)
    unsigned flags[16];            // sweep k flagged a stale successor
    unsigned long long walked[2];  // frames re-walked, frames jumped by the fix-up sweeps
    double lg[2];                  // a single track's loudness and gain
    unsigned pad1[4];
};
static_assert(offsetof(RbHead, lb_error) == 0 && offsetof(RbHead, flags) == 16 && offsetof(RbHead, walked) == 80 &&
                  offsetof(RbHead, lg) == 96 && sizeof(RbHead) == 128 && 3 * sizeof(int32_t) == 12,
              "the readback layout: head, then 12 bytes per chunk");

// finalize's done counters (FinArgs::done: FIN_DONE_LINES lines of 128 B and the top one)
constexpr size_t CTL_DONE_BYTES = 65 * 128;

// ticket and status words of a look-back launch of nblk blocks
inline size_t lb_flag_bytes(int64_t nblk) { return ((16 + (size_t)nblk * 4) + 15) / 16 * 16; }

// Byte offsets within the control block: the readback area, finalize's done
// counters, the sweeps' claim stamps [3][cols] followed by the column-block counts
// [3][cols / 64], then the eq / crossover / K-weighting look-back regions.
struct CtlLayout {
    int64_t chunks, cols;      // the solve's chunks and super-tile columns (0: no compressor)
    size_t rb_bytes, rb_area;  // readback bytes brought to the host; their area (a multiple of 256)
    size_t done, claims, cbtot, claim_area;  // (claim_area: bytes from `claims`, a multiple of 256)
    size_t region, lb[3];      // bytes of each look-back region; their offsets
    size_t bytes;
};

// nblk, nblk_kw: look-back blocks of the chunk stages and of a K-weighting stage that
// follows (0: none; sub-tile lanes can make it the larger); sg: the solve (null: none)
inline CtlLayout ctl_layout(unsigned nblk, unsigned nblk_kw, const mm_solve_geom *sg) {
    CtlLayout l{};
    l.chunks = sg ? sg->chunks : 0;
    l.cols = sg ? sg->chunks * sg->cols_per_chunk : 0;
    l.rb_bytes = sizeof(RbHead) + 12 * (size_t)l.chunks;
    l.done = l.rb_area = (l.rb_bytes + 255) / 256 * 256;
    l.claims = l.done + CTL_DONE_BYTES;
    l.cbtot = l.claims + (size_t)3 * l.cols * 4;
    l.claim_area = ((size_t)(3 * l.cols + 3 * l.cols / 64) * 4 + 255) / 256 * 256;
    l.region = lb_flag_bytes(std::max(nblk, nblk_kw));
    for (int r = 0; r < 3; ++r) l.lb[r] = l.claims + l.claim_area + r * l.region;
    l.bytes = l.lb[0] + 3 * l.region;
    return l;
}

#ifndef MM_CONTROL_LAYOUT_ONLY
static_assert(CTL_DONE_BYTES == (size_t)(mm::FIN_DONE_LINES + 1) * 128, "FinArgs::done");

// The control block of the chain in flight.  One memset at the chain's start zeroes
// it; the chain's last finalize launch (the tail) hands the readback area to the
// mapped host block and leaves the whole block zeroed, so a chain after a completed
// one starts with no fill and ends with no copy; without a tail, ONE copy at the end.
// Its state, changed only by the operations below:
//  * clean_ptr, clean_bytes: the device block is zero from clean_ptr up to clean_bytes
//    (the last chain's tail zeroed it; null: not known to be zero);
//  * fresh[r]: look-back region r is still zero (a region is fresh until its first use);
//  * flags_fresh: the sweep flags are zero as well;
//  * tail: the last queued finalize hands the readback area over;
//  * kept: an extension after a tail hand-over starts from a zeroed block, so the
//    per-chunk active counts (comp_rms, once per chain) and the earlier passes'
//    re-walked counts are held here and merged into the last readback.
struct ChainCtl {
    CtlLayout lay{};
    char *block = nullptr;                  // device block ("ctl")
    char *rb = nullptr, *rb_dev = nullptr;  // mapped host block and its device address
    size_t rb_cap = 0, clean_bytes = 0;
    char *clean_ptr = nullptr;
    bool fresh[3] = {false, false, false}, flags_fresh = false, tail = false;
    struct {
        bool on = false;
        std::vector<int32_t> tot;
        unsigned long long walked[2] = {0, 0};
    } kept;

    // the readback as the host reads it after the sync, and as the kernels write it
    const RbHead &head() const { return *reinterpret_cast<const RbHead *>(rb); }
    int32_t *host_totals() const { return reinterpret_cast<int32_t *>(rb + sizeof(RbHead)); }
    int32_t totals(int band, int64_t chunk) const { return host_totals()[band * lay.chunks + chunk]; }
    RbHead *dev() const { return reinterpret_cast<RbHead *>(block); }
    int32_t *dev_totals(int band) const { return reinterpret_cast<int32_t *>(block + sizeof(RbHead)) + band * lay.chunks; }
    uint32_t *claims(int band) const { return reinterpret_cast<uint32_t *>(block + lay.claims) + band * lay.cols; }
    int32_t *cbtot(int band) const { return reinterpret_cast<int32_t *>(block + lay.cbtot) + band * (lay.cols / 64); }

    // Begin a chain on blk (l.bytes): zeroed here unless the last chain's tail left it so.
    hipError_t begin(const CtlLayout &l, char *blk, hipStream_t s) {
        if (blk != clean_ptr || l.bytes > clean_bytes) {
            if (hipError_t e = hipMemsetAsync(blk, 0, l.bytes, s)) return e;
        }
        clean_ptr = nullptr;
        lay = l;
        block = blk;
        fresh[0] = fresh[1] = fresh[2] = flags_fresh = true;
        tail = kept.on = false;
        kept.walked[0] = kept.walked[1] = 0;
        return hipSuccess;
    }
    // Look-back region r (0 eq, 1 crossover, 2 K-weighting) for a launch of nblk blocks:
    // given out once and only to a launch it was sized for; null: the launch zeroes words of its own.
    char *take_region(int r, int64_t nblk) {
        if (r < 0 || !fresh[r] || lb_flag_bytes(nblk) > lay.region) return nullptr;
        fresh[r] = false;
        return block + lay.lb[r];
    }
    // The sweep flags for a round of sweeps, zeroed unless they still are (the walked count accumulates).
    hipError_t take_flags(hipStream_t s, unsigned **flags) {
        *flags = dev()->flags;
        const bool zero = flags_fresh;
        flags_fresh = false;
        return zero ? hipSuccess : hipMemsetAsync(*flags, 0, sizeof(RbHead::flags), s);
    }
    hipError_t ensure_rb() {
        const size_t bytes = lay.rb_bytes + 64;
        if (rb_cap >= bytes) return hipSuccess;
        if (hipError_t e = free()) return e;
        // mapped and coherent: the chain's last finalize block writes it directly
        if (hipError_t e = hipHostMalloc((void **)&rb, bytes, hipHostMallocMapped | hipHostMallocCoherent)) return e;
        if (hipError_t e = hipHostGetDevicePointer((void **)&rb_dev, rb, 0)) return e;
        rb_cap = bytes;
        return hipSuccess;
    }
    // A finalize launch: the chain's tail (fa given) hands the readback area over in that
    // launch (FinArgs::ctl) instead of a copy after it; any other one (null) does not.
    hipError_t attach_tail(mm::FinArgs *fa) {
        tail = false;
        if (!fa || !block) return hipSuccess;
        if (hipError_t e = ensure_rb()) return e;
        fa->ctl = block;
        fa->ctl_bytes = (int64_t)lay.bytes;
        fa->rb_area = (int64_t)lay.claims;  // (zeroed last: the readback area and the done counters)
        fa->rb_bytes = (int)lay.rb_bytes;
        fa->rb_host = rb_dev;
        fa->done = reinterpret_cast<unsigned *>(block + lay.done);
        tail = true;
        return hipSuccess;
    }
    // Queue ONE D2H copy of everything the host checks after the chain: the readback area.
    hipError_t queue_copy(hipStream_t s) {
        if (hipError_t e = ensure_rb()) return e;
        return hipMemcpyAsync(rb, block, lay.rb_bytes, hipMemcpyDeviceToHost, s);
    }
    // Before a resumed solve's next pass: hold what the handed-over readback carries
    // (a copied readback: the device words accumulate).
    void keep() {
        if (!tail) return;
        if (!kept.on) kept.tot.assign(host_totals(), host_totals() + 3 * lay.chunks);
        for (int i = 0; i < 2; ++i) kept.walked[i] += head().walked[i];
        kept.on = flags_fresh = true;
    }
    // After the chain's last pass: merge what keep() held, and note a zeroed block.
    void finish() {
        if (kept.on) {
            memcpy(host_totals(), kept.tot.data(), kept.tot.size() * sizeof(int32_t));
            for (int i = 0; i < 2; ++i) reinterpret_cast<RbHead *>(rb)->walked[i] += kept.walked[i];
            kept.on = false;
        }
        clean_ptr = tail ? block : nullptr;
        clean_bytes = lay.bytes;
    }
    hipError_t free() {
        const hipError_t e = rb ? hipHostFree(rb) : hipSuccess;
        rb = rb_dev = nullptr;
        rb_cap = 0;
        return e;
    }
};
#endif
