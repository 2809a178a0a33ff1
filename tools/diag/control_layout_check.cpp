// Stand-alone host check of the chain's control-block layout (ctl_layout and RbHead,
// csrc/control.h) against the formulas the host code used before the layout had one
// owner, written out literally below: no context, no GPU, never loaded into Python.
// Only the layout part of the header is compiled (no HIP); build it instrumented and
// run it on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//     tools/diag/control_layout_check.cpp -o control_layout_check
// Exits non-zero on any failure.
#include <cstdio>

#define MM_CONTROL_LAYOUT_ONLY
#include "../../python-audio-mastering_amd/csrc/control.h"

static int failures = 0;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

// nblk / nblk_kw: look-back blocks of the chunk stages / the K-weighting stage;
// nch chunks of spc columns (spc a multiple of 64; 0 chunks: no compressor)
static void run(unsigned nblk, unsigned nblk_kw, int64_t nch, int64_t spc) {
    mm_solve_geom sg{};
    sg.chunks = nch;
    sg.cols_per_chunk = spc;
    const CtlLayout l = ctl_layout(nblk, nblk_kw, nch ? &sg : nullptr);

    // the earlier host code, literally: setup_control called with max(nblk, nblk_kw) ...
    const unsigned nb = nblk > nblk_kw ? nblk : nblk_kw;
    const size_t region = ((16 + (size_t)nb * 4) + 15) / 16 * 16;
    // ... and the claim words of stage_front, which mm_op_compress_bands wrote another way
    const int64_t claims = 3 * nch * spc + 3 * nch * spc / 64;
    CHECK(claims == 3 * nch * spc * 65 / 64);
    const size_t rb_bytes = 128 + (size_t)12 * nch;
    const size_t rba = (rb_bytes + 255) / 256 * 256, cla = ((size_t)claims * 4 + 255) / 256 * 256;
    const size_t fin_done = (size_t)(64 + 1) * 128;
    const size_t bytes = rba + fin_done + cla + 3 * region;

    CHECK(l.bytes == bytes);
    CHECK(l.rb_bytes == rb_bytes);                // queue_readback's copy, FinArgs::rb_bytes
    CHECK(l.rb_area == rba);
    CHECK(l.done == rba);                         // FinArgs::done
    CHECK(l.claims == rba + fin_done);            // ctl_claims, and FinArgs::rb_area
    CHECK(l.cbtot == l.claims + (size_t)3 * nch * spc * 4);  // "claims + 3 NS" in words
    CHECK(l.claim_area == cla);
    CHECK(l.region == region);
    for (int r = 0; r < 3; ++r) CHECK(l.lb[r] == rba + fin_done + cla + r * region);
    CHECK(l.chunks == nch && l.cols == nch * spc);

    // the properties the kernels rely on
    CHECK(l.region % 16 == 0 && l.rb_area % 256 == 0 && l.claim_area % 256 == 0);
    CHECK(l.rb_bytes % 4 == 0 && l.bytes % 4 == 0 && l.claims % 4 == 0);  // finalize zeroes words
    for (int r = 0; r < 3; ++r) CHECK(l.lb[r] % 16 == 0);
    // the areas in order, none overlapping its successor, the last ending with the block
    CHECK(l.rb_bytes <= l.rb_area);
    CHECK(l.done == l.rb_area && l.done + CTL_DONE_BYTES == l.claims);
    CHECK(l.cbtot + (size_t)3 * (l.cols / 64) * 4 <= l.claims + l.claim_area);  // claims + cbtot fit
    CHECK(l.claims + l.claim_area == l.lb[0]);
    CHECK(l.lb[0] + l.region == l.lb[1] && l.lb[1] + l.region == l.lb[2] && l.lb[2] + l.region == l.bytes);
    CHECK(lb_flag_bytes(nblk) <= l.region && lb_flag_bytes(nblk_kw) <= l.region);  // both stages' launches fit
}

int main() {
    static_assert(offsetof(RbHead, lb_error) == 0 && offsetof(RbHead, flags) == 16 && offsetof(RbHead, walked) == 80 &&
                      offsetof(RbHead, lg) == 96 && sizeof(RbHead) == 128,
                  "RB_ERR, RB_FLAGS, RB_WALKED, RB_LG, RB_TOTALS");
    run(1, 0, 0, 0);        // no compressor, one block
    run(1, 1, 1, 64);       // one chunk of 64 columns
    run(3, 9, 2, 128);      // K-weighting blocks above the chunk stages' (three sub-tile lanes per tile)
    run(9, 3, 2, 128);
    // 2 hours of 96 kHz stereo: 691.2 M frames in 225-frame tiles, 30 s chunks of 12800 tiles
    // (3200 columns), 128 tiles per look-back block; K-weighting at 256 lanes per block, 1 or 3 per tile
    run(24000, 12000, 240, 3200);
    run(24000, 36000, 240, 3200);
    for (unsigned nblk = 1; nblk < 40; ++nblk)  // every residue of the roundings
        for (int64_t nch = 0; nch < 45; ++nch) run(nblk, nblk / 2, nch, 64 * (1 + nch % 3));
    printf("control_layout_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
