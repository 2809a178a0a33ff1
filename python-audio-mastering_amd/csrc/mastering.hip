// mastering.hip — host side of the C-ABI (include/mastering.h), one translation
// unit: the launch sequence of the chain (a unit of n >= 1 tracks between two
// syncs), the batch scheduler and the context entry points.  The chain's control
// block is control.h, the loudness tail's state loudness.h, the context that holds
// both context.h, followed by decode.hip (24/32-bit PCM input).  ops.hip (the
// per-stage operators) and loudness.hip (the loudness tail, its operator and the
// time-sharded entry points) follow the chain, before the units that call
// line_loudness; wav.hip, comm.hip, then pcm16.h, meter.hip, r128.hip, qc.hip, spectrum.hip, ceiling.hip, level.hip,
// resample.hip (with mm_master* / mm_deliver*: a master call with or without a delivery), fir.hip, album.hip
// and tracks.hip (the level's driver and the end of a master call) come at the end.
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/mastering.h"
#include "iir.hip"
#include "kernels.hip"
#include "compressor.hip"
#include "gate.hip"

using namespace mm;

#include "control.h"
#include "loudness.h"
#include "context.h"
#include "decode.hip"

// tracks.hip: the end of a master call for delivered buffer i, the level (a delivery's) or the
// ceiling and then the report
static int finish_delivered(mm_ctx *c, void *d_out, int kind, int64_t frames, int channels, int i, int32_t ceiling_q28,
                            int32_t window, int meter_on, const mm_job *loud, int32_t level_clu = 0);

// ------------------------------------------------------- look-back plumbing
// Transition tables of one filter stage (uploaded only when they change).
static int upload_tables(mm_ctx *c, const char *name, const mm_iir &f, LbArgs &lb) {
    const size_t n = (size_t)(MM_TILE_POW + MM_BLK_POW) * 64;
    std::vector<double> host(n);
    memcpy(host.data(), f.phi_tile_pow, sizeof f.phi_tile_pow);
    memcpy(host.data() + MM_TILE_POW * 64, f.phi_blk_pow, sizeof f.phi_blk_pow);
    const std::string key = std::string("tab_") + name;
    double *d;
    RET(get_buf(c, key.c_str(), n, &d));
    std::vector<double> &cached = c->mats_cache[key];
    if (cached != host) {
        HIPCHK(c, hipMemcpyAsync(d, host.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // host vector is transient
        cached = host;
    }
    lb.pw_tile = d;
    lb.pw_blk = d + MM_TILE_POW * 64;
    return MM_OK;
}

// Zero-state weights of one stage over a whole tile of T frames (pass 1 of the
// crossover as a product, XoArgs::zw): row n is the state after the tile from a
// zero state with a unit input at frame n and zeros elsewhere, W[n] = A^(T-1-n) B
// (A: one zero-input frame, B: the state one frame after a unit input), evaluated
// in long double and rounded once.  Branch 0 is sections [0, nsec_branch0), branch 1
// the rest, both fed by the stage input (csrc/lookback.h's layout).
static void zs_weights(const mm_iir &f, int T, std::vector<double> &W) {
    const int nsec = f.nsec, nb0 = f.nsec_branch0;
    auto step = [&](const long double *z, long double x, long double *o) {
        for (int br = 0; br < 2; ++br) {
            long double u = x;
            for (int s = br ? nb0 : 0; s < (br ? nsec : nb0); ++s) {
                const double *c = f.sos[s];
                const long double y = (long double)c[0] * u + z[2 * s];
                o[2 * s] = (long double)c[1] * u - (long double)c[3] * y + z[2 * s + 1];
                o[2 * s + 1] = (long double)c[2] * u - (long double)c[4] * y;
                u = y;
            }
        }
    };
    W.assign((size_t)T * 8, 0.0);
    long double v[8] = {0}, t[8] = {0}, zero[8] = {0};
    step(zero, 1.0L, v);
    for (int n = T - 1; n >= 0; --n) {
        for (int d = 0; d < 2 * nsec; ++d) W[(size_t)n * 8 + d] = (double)v[d];
        step(v, 0.0L, t);
        for (int d = 0; d < 8; ++d) v[d] = t[d];
    }
}

// The stage's zero-state weights on the device (rebuilt only when its sections or
// the tile change); null for a section count outside 1..4 (pass 1 then runs the
// recurrence).
static int upload_zw(mm_ctx *c, const char *name, const mm_iir &f, int T, const double **out) {
    *out = nullptr;
    if (f.nsec < 1 || f.nsec > 4) return MM_OK;
    std::vector<double> key(f.sos[0], f.sos[0] + 20);
    key.push_back((double)T);
    key.push_back((double)f.nsec);
    key.push_back((double)f.nsec_branch0);
    const std::string kname = std::string("zw_") + name;
    double *d;
    RET(get_buf(c, kname.c_str(), (size_t)T * 8, &d));
    std::vector<double> &cached = c->mats_cache[kname];
    if (cached != key) {
        std::vector<double> W;
        zs_weights(f, T, W);
        HIPCHK(c, hipMemcpyAsync(d, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // host vector is transient
        cached = key;
    }
    *out = d;
    return MM_OK;
}

// Per-launch look-back state for nblk blocks of CH lines.  region: the chain's
// pre-zeroed control region of this stage (ChainCtl::take_region) and its error
// word; otherwise (-1, or a region already used) the ticket and the status words
// are zeroed by a private memset right before the launch, and the caller of a
// launch outside a chain sets lb.error.
static int lb_prepare(mm_ctx *c, int64_t nblk, int ch, LbArgs &lb, int region = -1) {
    char *flags = c->ctl.take_region(region, nblk);
    if (!flags) {
        const size_t flag_bytes = lb_flag_bytes(nblk);
        RET(get_buf(c, "lb_flags", flag_bytes, &flags));
        HIPCHK(c, hipMemsetAsync(flags, 0, flag_bytes, c->stream));
    }
    lb.ticket = reinterpret_cast<unsigned *>(flags);
    lb.status = reinterpret_cast<unsigned *>(flags + 16);
    RET(get_buf(c, "lb_agg", (size_t)nblk * ch * 8, &lb.agg));
    RET(get_buf(c, "lb_incl", (size_t)nblk * ch * 8, &lb.incl));
    if (region >= 0) lb.error = &c->ctl.dev()->lb_error;
    lb.init = nullptr;
    return MM_OK;
}

static int validate(mm_ctx *c, const mm_job *j) {
    if (!j) return set_err(c, MM_ERR_ARG, "null job");
    if (j->channels != 1 && j->channels != 2) return set_err(c, MM_ERR_ARG, "channels must be 1 or 2");
    if (!in_sample_bytes(j->in_kind)) return set_err(c, MM_ERR_ARG, "in_kind %d", j->in_kind);
    if (j->tile < 16 || j->tile > 512) return set_err(c, MM_ERR_ARG, "tile %d out of range [16, 512]", j->tile);
    if (j->tiles_per_chunk < 1) return set_err(c, MM_ERR_ARG, "tiles_per_chunk < 1");
    if (j->frames_proc < 0 || j->frames_in < 0) return set_err(c, MM_ERR_ARG, "negative frame count");
    if (j->frames_proc >= (int64_t)1 << 31 || j->frames_in >= (int64_t)1 << 31)
        return set_err(c, MM_ERR_ARG, "track longer than 2^31 frames (32-bit frame indexing)");
    if (j->eq.nsec < 0 || j->eq.nsec > 4) return set_err(c, MM_ERR_ARG, "eq.nsec %d", j->eq.nsec);
    if (j->ceiling_q28 && (j->ceiling_q28 < (1 << 24) || j->ceiling_q28 > (1 << 28)))
        return set_err(c, MM_ERR_ARG, "ceiling_q28 %d out of range [2^24, 2^28]", j->ceiling_q28);
    const int tpb = LB_THREADS / j->channels;
    if (j->eq.nsec > 0 && j->eq.tpb != tpb) return set_err(c, MM_ERR_ARG, "eq tables built for %d tiles/block, need %d", j->eq.tpb, tpb);
    if (j->multiband_on && j->xover.tpb != tpb) return set_err(c, MM_ERR_ARG, "crossover tables built for %d tiles/block", j->xover.tpb);
    if (j->lufs_on && j->kweight.tpb != LB_THREADS) return set_err(c, MM_ERR_ARG, "K-weighting tables built for %d tiles/block", j->kweight.tpb);
    if (j->eq.nsec > 0 && j->eq.tile != j->tile) return set_err(c, MM_ERR_ARG, "eq tables built for %d-frame tiles", j->eq.tile);
    if (j->multiband_on && j->xover.tile != j->tile) return set_err(c, MM_ERR_ARG, "crossover tables built for %d-frame tiles", j->xover.tile);
    if (j->lufs_on && (j->kweight.tile < 1 || j->tile % j->kweight.tile != 0))
        return set_err(c, MM_ERR_ARG, "K-weighting tables built for %d-frame (sub-)tiles, not a divisor of %d",
                       j->kweight.tile, j->tile);
    if (j->multiband_on) {
        if (j->xover.nsec != 4 || j->xover.nsec_branch0 != 2) return set_err(c, MM_ERR_ARG, "crossover must be 2+2 sections");
        for (int b = 0; b < 3; ++b) {
            if (!j->band[b].lut) return set_err(c, MM_ERR_ARG, "band %d: missing table", b);
            if (j->band[b].look < 0) return set_err(c, MM_ERR_ARG, "band %d: look < 0", b);
            if (!(j->band[b].release_frames >= 1.0) || !(j->band[b].attack_frames > 0.0))
                return set_err(c, MM_ERR_ARG, "band %d: release must span >= 1 frame", b);
            // r0 must be the table's first nonzero row and every row from it on nonzero: the
            // tiles with an active frame (rms >= r0: cnt, comp_describe's live tiles) are then
            // exactly the tiles with a nonzero M (the ones comp_rms_t writes a record for).
            // The two rows at r0 are checked for every job, the whole column unless this
            // context checked a table of the same content key against the same r0 last.
            const double *lt = j->band[b].lut;
            const int64_t r0 = j->band[b].r0;
            const uint64_t key = j->band[b].lut_key;
            bool ok = r0 >= 0 && r0 <= 32769 && (r0 == 0 || lt[4 * (r0 - 1)] == 0.0) &&
                      (r0 > 32768 || lt[4 * r0] != 0.0);
            if (ok && (key == 0 || c->lut_ok_key[b] != key || c->lut_ok_r0[b] != r0)) {
                for (int64_t r = 0; r <= 32768 && ok; ++r) ok = (lt[4 * r] != 0.0) == (r >= r0);
                c->lut_ok_key[b] = ok ? key : 0;
                c->lut_ok_r0[b] = r0;
            }
            if (!ok) return set_err(c, MM_ERR_ARG, "band %d: r0 %lld is not the table's first nonzero row", b, (long long)r0);
        }
    }
    if (j->lufs_on) {
        if (j->kweight.nsec != 2) return set_err(c, MM_ERR_ARG, "K-weighting must be 2 sections");
        if (j->n_segs < 1 || !j->seg_bounds || !j->block_lo || !j->block_hi || j->n_blocks < 1)
            return set_err(c, MM_ERR_ARG, "missing loudness geometry");
        for (int64_t s = 0; s < j->n_segs; ++s) {
            int64_t b0 = j->seg_bounds[s], b1 = std::min<int64_t>(j->seg_bounds[s + 1], j->frames_proc);
            if (b1 > b0 && b1 - b0 < j->tile && s + 1 < j->n_segs)
                return set_err(c, MM_ERR_ARG, "loudness segment %lld shorter than a tile", (long long)s);
        }
    }
    return MM_OK;
}

static void fill_sos(double dst[4][5], const mm_iir &f, int n) {
    for (int s = 0; s < 4; ++s)
        for (int k = 0; k < 5; ++k) dst[s][k] = s < n ? f.sos[s][k] : 0.0;
}

template <int NS>
static int launch_eq_ns(mm_ctx *c, int ch, unsigned nblk, const EqArgs &ea, const LbArgs &lb, int64_t K) {
    if (ch == 2) {
        const size_t lds = eq_lds_bytes<NS, 2>();
        if (ea.in16) return launch(c, "eq", eq_kernel<NS, 2, true>, dim3(nblk), dim3(LB_THREADS), lds, ea, lb, K);
        return launch(c, "eq", eq_kernel<NS, 2, false>, dim3(nblk), dim3(LB_THREADS), lds, ea, lb, K);
    }
    const size_t lds = eq_lds_bytes<NS, 1>();
    if (ea.in16) return launch(c, "eq", eq_kernel<NS, 1, true>, dim3(nblk), dim3(LB_THREADS), lds, ea, lb, K);
    return launch(c, "eq", eq_kernel<NS, 1, false>, dim3(nblk), dim3(LB_THREADS), lds, ea, lb, K);
}

static int launch_eq(mm_ctx *c, int nsec, int ch, unsigned nblk, const EqArgs &ea, const LbArgs &lb, int64_t K) {
    switch (nsec) {
        case 1: return launch_eq_ns<1>(c, ch, nblk, ea, lb, K);
        case 2: return launch_eq_ns<2>(c, ch, nblk, ea, lb, K);
        case 3: return launch_eq_ns<3>(c, ch, nblk, ea, lb, K);
        default: return launch_eq_ns<4>(c, ch, nblk, ea, lb, K);
    }
}

// --------------------------------------------------- compressor sweeps
// Fix-up sweeps are queued without a host sync: sweep k writes flag k (some
// successor may be stale) and exits at once if sweep k-1 flagged nothing.
// Convergence is checked at the chain's single sync (evaluate_chain); a rare
// unconverged batch is extended there (MM_COMP_SWEEPS sets the queued count).
constexpr int COMP_SWEEPS = 8;  // queued by a context's first solve (a sweep after a quiet one exits at once)

static int comp_sweeps(mm_ctx *c, int n) {
    Solve &sv = c->comp;
    CompArgs &ca = sv.ca;
    const int64_t NS = ca.GS;
    unsigned *flags;
    HIPCHK(c, c->ctl.take_flags(c->stream, &flags));
    for (int k = 0; k < n; ++k) {
        ca.sweep_idx = (int)sv.stamp;
        ca.stamp = ++sv.stamp;
        ca.heads = ca.stamp > 1 ? 1 : 0;  // the chain's first sweep is a Jacobi step
        ca.changed = flags + k;
        const unsigned int *prevf = k > 0 ? flags + (k - 1) : nullptr;
        RET(launch(c, "comp_fix", comp_fix_kernel, dim3(blocks_for(NS, 64), 3), dim3(64), 0, ca, prevf));
    }
    sv.pending = n;
    return MM_OK;
}

// gains + overlay into q2, every tile starting from its stored entry state
static int comp_back(mm_ctx *c) {
    const CompArgs &ca = c->comp.ca;
    const int64_t nchunks = ca.GS / ca.SPC;  // (chunk-aligned blocks of APPLY_TILES tiles)
    return launch(c, "comp_apply", comp_apply_kernel,
                  dim3((unsigned)(nchunks * ((ca.K + APPLY_TILES - 1) / APPLY_TILES))), dim3(3 * APPLY_TILES), 0, ca);
}

static int queue_readback(mm_ctx *c) {
    HIPCHK(c, c->ctl.queue_copy(c->stream));
    return MM_OK;
}

// After the stream has drained: reports look-back timeouts (never expected: a
// block only waits on blocks that started before it) and whether the queued
// sweeps converged.
static int evaluate_chain(mm_ctx *c, bool *converged) {
    Solve &sv = c->comp;
    if (c->ctl.head().lb_error) return set_err(c, MM_ERR_STATE, "IIR look-back timed out");
    if (sv.on && sv.ca.trace) {  // MM_FIX_TRACE: the three slowest walkers of every sweep
        const int64_t NS = sv.ca.GS;
        std::vector<uint32_t> tr((size_t)16 * 3 * NS * 4);
        HIPCHK(c, hipMemcpy(tr.data(), sv.ca.trace, tr.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (const char *path = getenv("MM_FIX_TRACE_DUMP")) {  // every walker record: [sweep][band][super-tile][4]
            if (FILE *f = fopen(path, "wb")) {
                fwrite(tr.data(), sizeof(uint32_t), tr.size(), f);
                fclose(f);
            }
        }
        for (int k = 0; k < 16; ++k) {
            std::vector<std::pair<uint32_t, int64_t>> v;
            int64_t nw = 0;
            for (int64_t i = 0; i < 3 * NS; ++i) {
                const uint32_t *r = &tr[((size_t)k * 3 * NS + i) * 4];
                if (r[0] || r[3]) {
                    v.push_back({r[0], i});
                    ++nw;
                }
            }
            if (v.empty()) continue;
            std::sort(v.rbegin(), v.rend());
            fprintf(stderr, "sweep %d: %lld walkers;", k, (long long)nw);
            for (size_t q = 0; q < std::min<size_t>(3, v.size()); ++q) {
                const uint32_t *r = &tr[((size_t)k * 3 * NS + v[q].second) * 4];
                fprintf(stderr, " [band %lld st %lld: %.1f us walked %u jumped %u visited %u]",
                        (long long)(v[q].second / NS), (long long)(v[q].second % NS), r[0] / 100.0, r[1], r[2],
                        r[3]);
            }
            fprintf(stderr, "\n");
        }
    }
    *converged = true;
    if (sv.on && sv.pending) {
        const unsigned *flags = c->ctl.head().flags;
        int k = 0;
        while (k < sv.pending && flags[k]) ++k;
        sv.iters += k;
        *converged = k < sv.pending;
        sv.pending = 0;
        // the solve needed `iters` flagged sweeps and one quiet one: queue that + 1
        if (*converged) sv.queue = std::min(16, std::max(3, sv.iters + 2));
        if (!*converged && sv.iters >= c->job.comp_max_iters)
            return set_err(c, MM_ERR_STATE, "compressor did not converge in %d sweeps", sv.iters);
    }
    return MM_OK;
}

// The chain's one sync, its readback queued: a rare unconverged solve is resumed
// with 8 more sweeps, the back end and `requeue_tail` (what follows the apply and
// brings the next readback) until it has converged (ChainCtl::keep / finish merge
// what the passes' readbacks carried).
template <typename Tail>
static int solve_to_convergence(mm_ctx *c, Tail requeue_tail) {
    for (;;) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bool converged;
        RET(evaluate_chain(c, &converged));
        if (converged) break;
        c->ctl.keep();
        RET(comp_sweeps(c, 8));
        RET(comp_back(c));
        RET(requeue_tail());
    }
    c->ctl.finish();
    return MM_OK;
}

// A chain without a tail (the staged entry points, the operators): ONE copy of the
// readback area, then the sync.
static int chain_check(mm_ctx *c) {
    RET(queue_readback(c));
    return solve_to_convergence(c, [c] { return queue_readback(c); });
}

// Geometry of the envelope solve (the C-ABI's mm_solve_geometry): TPS tiles per
// super-tile (the job's comp_super frames rounded to whole tiles), columns per
// chunk in whole blocks of 64 (comp_rms stores; a wave's columns lie in one
// chunk), plane rows per tile and per column, and each chunk's own plane (32-bit
// buffer offsets within it at any track length).
static int solve_geometry(const mm_job *j, mm_solve_geom *g) {
    const int K = j->tiles_per_chunk, T = j->tile;
    if (K < 1 || T < 1 || j->frames_proc < 0) return MM_ERR_ARG;
    const int64_t G = (j->frames_proc + T - 1) / T;
    *g = mm_solve_geom{};
    g->tps = std::max(1, std::min((j->comp_super + T / 2) / T, DESC_MAX_TPS));  // (comp_describe: 64 TPS threads)
    if (g->tps != RMS_TPS) return MM_ERR_ARG;  // comp_rms_t's workgroup: RMS_TPS positions x 64 columns
    g->col_block = 64;
    g->rms_group_tiles = RMS_TPS * 64;
    g->chunks = (G + K - 1) / K;
    g->cols_per_chunk = (((int64_t)K + g->tps - 1) / g->tps + 63) / 64 * 64;
    g->walk_block = WB;
    g->tile_rows = (T + WB - 1) / WB * WB;
    g->rows = g->tps * g->tile_rows + WALK_PAD;
    g->chunk_plane_bytes = (int64_t)g->rows * g->cols_per_chunk * 8;
    g->plane_bytes = 3 * g->chunks * g->chunk_plane_bytes;
    return g->chunk_plane_bytes < ((int64_t)1 << 31) ? MM_OK : MM_ERR_ARG;
}

// Begin a chain: its control block, laid out by ctl_layout (control.h).
static int begin_chain(mm_ctx *c, unsigned nblk, unsigned nblk_kw, const mm_solve_geom *sg) {
    const CtlLayout lay = ctl_layout(nblk, nblk_kw, sg);
    char *blk;
    RET(get_buf(c, "ctl", lay.bytes, &blk));
    HIPCHK(c, c->ctl.begin(lay, blk, c->stream));
    return MM_OK;
}

// Stage C (AME:207-210): per-band pydub compressor envelope solve + gains +
// overlay of the three int16 band planes (tile-major) into q2.  tile_e holds the
// crossover's per-tile band energies ([3][E, tail][G]).  Queues everything up to
// the apply; convergence is checked at the chain's sync.
// FNV-1a over the job fields the envelope solve's sweep count depends on
static uint64_t comp_signature(const mm_job *j) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const void *p, size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    };
    mix(&j->frames_proc, sizeof j->frames_proc);
    mix(&j->rate, sizeof j->rate);
    mix(&j->tile, sizeof j->tile);
    mix(&j->tiles_per_chunk, sizeof j->tiles_per_chunk);
    mix(&j->comp_super, sizeof j->comp_super);
    for (const mm_band &b : j->band) {
        mix(&b.thresh_rms, sizeof b.thresh_rms);
        mix(&b.attack_frames, sizeof b.attack_frames);
        mix(&b.release_frames, sizeof b.release_frames);
        mix(&b.look, sizeof b.look);
        mix(&b.r0, sizeof b.r0);
        mix(&b.lut_key, sizeof b.lut_key);
    }
    return h;
}

// pad: a fused timeline's tracks with padding, n_pad {end, end of the last chunk}
// pairs on the device for comp_trim_kernel (0: none).
static int stage_compress(mm_ctx *c, const mm_job *j, short2 *const bands[3], const double *tile_e, short2 **q2_out,
                          const int64_t *pad = nullptr, int n_pad = 0) {
    const int T = j->tile, ch = j->channels, K = j->tiles_per_chunk;
    const int64_t N = j->frames_proc;
    const int64_t G = c->G;
    const int64_t TG = (int64_t)T * std::max<int64_t>(G, 1);
    CompArgs ca{};
    ca.N_proc = N;
    ca.G = G;
    ca.T = T;
    ca.K = K;
    ca.ch = ch;
    ca.warmup = j->comp_warmup;
    mm_solve_geom sg;
    if (solve_geometry(j, &sg) != MM_OK)
        return set_err(c, MM_ERR_ARG, "chunk of %d tiles too large for one envelope-solve plane", K);
    const int64_t nchunks = sg.chunks;
    ca.TPS = sg.tps;
    ca.SPC = sg.cols_per_chunk;
    ca.GS = nchunks * ca.SPC;
    const int64_t NS = ca.GS;
    short2 *q2;
    RET(get_buf(c, "q2", TG, &q2));
    ca.q_out = q2;
    *q2_out = q2;
    double *st, *ends, *luts, *tstc, *descc, *mmax, *mmaxc, *ced, *cedc;
    RET(get_buf(c, "comp_start", (size_t)3 * NS, &st));
    RET(get_buf(c, "comp_end", (size_t)3 * NS, &ends));
    RET(get_buf(c, "comp_lut", (size_t)3 * 32769, &luts));
    const int64_t NC = nchunks * K;  // compact indices
    RET(get_buf(c, "comp_mmax", (size_t)3 * G, &mmax));
    RET(get_buf(c, "comp_tstc", (size_t)3 * NC, &tstc));
    RET(get_buf(c, "comp_mmaxc", (size_t)3 * NC, &mmaxc));
    RET(get_buf(c, "comp_ced", (size_t)6 * G, &ced));
    RET(get_buf(c, "comp_cedc", (size_t)6 * NC, &cedc));
    RET(get_buf(c, "comp_descc", (size_t)3 * DREC * NC, &descc));
    double *desc_g;
    RET(get_buf(c, "comp_desc_g", (size_t)3 * DREC * std::max<int64_t>(G, 1), &desc_g));
    int32_t *ranks, *tls, *nacts;
    RET(get_buf(c, "comp_rank", (size_t)3 * G, &ranks));
    RET(get_buf(c, "comp_tl", (size_t)3 * NC, &tls));
    RET(get_buf(c, "comp_nact", (size_t)3 * nchunks, &nacts));
    ca.jumps = getenv("MM_COMP_NOJUMP") ? 0 : 1;  // diagnostics: results must not change
    ca.sjump = ca.jumps && !getenv("MM_COMP_NOSJUMP") && ca.TPS == SJ_TPS ? 1 : 0;
    ca.e_tiles = E_TILES;
    double *sdesc;
    int32_t *se0s;
    RET(get_buf(c, "comp_sdesc", ca.sjump ? (size_t)3 * NS * SREC : 1, &sdesc));
    RET(get_buf(c, "comp_se0", ca.sjump ? (size_t)3 * NS : 1, &se0s));
    ca.walked = c->ctl.dev()->walked;  // (zeroed and read back with the control block, as total / claim / cbtot)
    ca.trace = nullptr;
    if (getenv("MM_FIX_TRACE")) {  // diagnostics: per-walker sweep records, printed by evaluate_chain
        RET(get_buf(c, "comp_trace", (size_t)16 * 3 * NS * 4, &ca.trace));
        HIPCHK(c, hipMemsetAsync(ca.trace, 0, (size_t)16 * 3 * NS * 4 * sizeof(uint32_t), c->stream));
    }
    ca.TP = sg.tile_rows;
    ca.RP = sg.rows;
    ca.chunk_elems = sg.chunk_plane_bytes / 8;  // SPC / 64 column blocks of 64 x RP
    const int64_t ms_elems = ca.chunk_elems * nchunks;
    int32_t *cnt;
    RET(get_buf(c, "comp_cnt", (size_t)3 * G, &cnt));
    for (int b = 0; b < 3; ++b) {
        double *msb;
        char nm[16];
        snprintf(nm, sizeof nm, "comp_ms%d", b);
        RET(get_buf(c, nm, (size_t)ms_elems, &msb));
        ca.Ms[b] = msb;
        ca.E[b] = tile_e + (size_t)(2 * b) * G;
        ca.tail[b] = tile_e + (size_t)(2 * b + 1) * G;
        ca.band[b] = bands[b];
        ca.lut[b] = luts + (size_t)b * 32769;
        // cached by content key (a host pointer may be reused by another table once the
        // caller frees one): upload when the key differs or is unknown
        if (j->band[b].lut_key == 0 || c->lut_key[b] != j->band[b].lut_key) {
            // the M column of the host's {M, M/A, M/R, 0} rows
            HIPCHK(c, hipMemcpy2DAsync(luts + (size_t)b * 32769, sizeof(double), j->band[b].lut,
                                       4 * sizeof(double), sizeof(double), 32769, hipMemcpyHostToDevice,
                                       c->stream));
            c->lut_key[b] = j->band[b].lut_key;
        }
        ca.r0[b] = (uint32_t)j->band[b].r0;
        ca.look[b] = j->band[b].look;
        ca.attack_frames[b] = j->band[b].attack_frames;
        ca.release_frames[b] = j->band[b].release_frames;
        ca.rcp_attack[b] = 1.0 / j->band[b].attack_frames;
        ca.rcp_release[b] = 1.0 / j->band[b].release_frames;
        ca.cnt[b] = cnt + (size_t)b * G;
        ca.mmax[b] = mmax + (size_t)b * G;
        ca.total[b] = c->ctl.dev_totals(b);
        ca.rank[b] = ranks + (size_t)b * G;
        ca.nact[b] = nacts + (size_t)b * nchunks;
        ca.tl[b] = tls + (size_t)b * NC;
        ca.mmaxc[b] = mmaxc + (size_t)b * NC;
        ca.ced[b] = ced + (size_t)2 * b * G;
        ca.cedc[b] = cedc + (size_t)2 * b * NC;
        ca.tstc[b] = tstc + (size_t)b * NC;
        ca.descc[b] = descc + (size_t)b * DREC * NC;
        ca.desc_g[b] = desc_g + (size_t)b * DREC * G;
        // the fixed record base: no state exceeds the table's largest M (its last row: the
        // table is nondecreasing), so JB binades down from that M's hold every state at or
        // above 2^e0fix (a table without a positive M has no active tile: any base does)
        const double mtop = j->band[b].lut[(size_t)4 * 32768];
        ca.e0fix[b] = (mtop > 0.0 ? std::max(ilogb(mtop), -900) : 0) - (JB - 1);
        ca.start[b] = st + (size_t)b * NS;
        ca.end[b] = ends + (size_t)b * NS;
        ca.claim[b] = c->ctl.claims(b);
        ca.sdesc[b] = ca.sjump ? sdesc + (size_t)b * NS * SREC : nullptr;
        ca.se0[b] = ca.sjump ? se0s + (size_t)b * NS : nullptr;
        ca.cbtot[b] = c->ctl.cbtot(b);
    }
    // column block = one workgroup (RMS_TPS x 64 tiles): gathers / stores through LDS
    RET(launch(c, "comp_rms", comp_rms_t_kernel, dim3((unsigned)(NS / 64), 3), dim3(256), 0, ca));
    if (n_pad > 0)  // a timeline: the padding's frames leave the per-chunk statistics
        RET(launch(c, "comp_trim", comp_trim_kernel, dim3((unsigned)n_pad, 3), dim3(64), 0, ca, pad));
    RET(launch(c, "comp_describe", comp_describe_kernel, dim3((unsigned)(NS / 64), 3), dim3(64 * ca.TPS), 0, ca));
    RET(launch(c, "comp_pass0", comp_pass0_kernel, dim3(blocks_for(NS, PASS0_BLOCK), 3), dim3(PASS0_BLOCK), 0, ca));
    Solve &sv = c->comp;
    sv.on = true;
    sv.ca = ca;
    sv.stamp = 0;
    sv.iters = sv.pending = 0;
    // as many as the last solve on this context needed (+ 1 spare) when this job has
    // the same compressor settings and geometry: a stream of similar jobs queues few
    // idle sweeps and rarely resumes from the host; a job with other settings or
    // another length starts from COMP_SWEEPS again (a P_HOT job after P_FULL ones
    // would otherwise resume from the host)
    const uint64_t sig = comp_signature(j);
    if (sig != sv.sig) {
        sv.queue = 0;
        sv.sig = sig;
    }
    int sweeps = sv.queue > 0 ? sv.queue : COMP_SWEEPS;
    if (const char *e = getenv("MM_COMP_SWEEPS")) sweeps = std::max(1, std::min(16, atoi(e)));  // tests / tuning
    RET(comp_sweeps(c, sweeps));
    RET(comp_back(c));
    return MM_OK;
}

// Look-back blocks of the K-weighting stage over G tiles: one lane per sub-tile of
// kweight.tile frames (design.kweight_sub).
static unsigned kw_nblk(const mm_job *j, int64_t G) {
    return blocks_for(std::max<int64_t>(G, 1) * (j->tile / std::max(1, j->kweight.tile)), LB_THREADS);
}

// ------------------------------------------------------------ chain A..C
// nblk_kw: the blocks of the K-weighting stage that will follow on this line (0: none);
// pad, n_pad: as stage_compress
static int stage_front(mm_ctx *c, const mm_job *j, const void *d_in, unsigned nblk_kw, const int64_t *pad = nullptr,
                       int n_pad = 0) {
    mm_job jf;
    if (j->in_kind == MM_IN_I24 || j->in_kind == MM_IN_I32) {
        // 24/32-bit PCM: decoded once for the line (a fused timeline is one run of
        // samples), and the job goes on as MM_IN_F32 on those floats
        const int64_t n = j->frames_in * j->channels;
        float *dec;
        RET(get_buf(c, "pcm_dec", (size_t)std::max<int64_t>(n, 1), &dec));
        RET(pcm_decode(c, j->in_kind, d_in, n, dec));
        jf = *j;
        jf.in_kind = MM_IN_F32;
        j = &jf;
        d_in = dec;
    }
    const int T = j->tile, ch = j->channels, K = j->tiles_per_chunk;
    const int64_t N = j->frames_proc;
    const int64_t G = (N + T - 1) / T;
    const int64_t TG = (int64_t)T * std::max<int64_t>(G, 1);
    c->G = G;
    c->job = *j;
    c->staged = false;
    short2 *q1;
    RET(get_buf(c, "q1", TG, &q1));
    const int tpb = LB_THREADS / ch;
    const unsigned nblk = blocks_for(std::max<int64_t>(G, 1), tpb);
    mm_solve_geom sg{};
    if (j->multiband_on) solve_geometry(j, &sg);  // (checked by stage_compress)
    RET(begin_chain(c, nblk, nblk_kw, j->multiband_on ? &sg : nullptr));

    EqArgs ea{};
    ea.in = j->in_kind == MM_IN_I16 ? nullptr : static_cast<const float *>(d_in);
    ea.in16 = j->in_kind == MM_IN_I16 ? static_cast<const int16_t *>(d_in) : nullptr;
    ea.N_in = j->frames_in;
    ea.N_proc = N;
    ea.G = G;
    ea.T = T;
    ea.sat.keep = j->sat_keep;
    ea.sat.mix = j->sat_mix;
    ea.sat.drive = j->sat_drive;
    ea.sat.on = j->sat_on;
    ea.sat.tab = nullptr;
    ea.sat.corr = nullptr;
    if (j->sat_on && j->sat_table) {  // the exciter's int16-grid table, uploaded when its key changes
        float *tab;
        uint32_t *corr;
        RET(get_buf(c, "sat_tab", 65536, &tab));
        RET(get_buf(c, "sat_corr", SAT_CORR_WORDS, &corr));
        ea.sat.tab = tab;
        if (j->sat_key == 0 || c->sat_key != j->sat_key) {  // once per table: build the codes, count exceptions
            unsigned *exc;
            RET(get_buf(c, "sat_exc", 1, &exc));
            HIPCHK(c, hipMemcpyAsync(tab, j->sat_table, 65536 * sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemsetAsync(exc, 0, sizeof(unsigned), c->stream));
            RET(launch(c, "sat_corr", sat_corr_kernel, dim3((SAT_CORR_WORDS + 255) / 256), dim3(256), 0, ea.sat, corr,
                       exc));
            unsigned e1 = 1;
            HIPCHK(c, hipMemcpyAsync(&e1, exc, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->sat_codes = e1 == 0;
            c->sat_key = j->sat_key;
        }
        // codes when complete (else, and for A/B: a full-table gather per sample)
        if (c->sat_codes && !getenv("MM_SAT_GATHER")) ea.sat.corr = corr;
        if (ea.sat.tab && !ea.sat.corr && j->eq.nsec > 0 && N > 0) {
            // the EQ kernel takes the exciter only as tanhf + codes: the table case runs
            // as a pointwise pre-pass into a decoded f32 input, and the EQ without it
            const int64_t n = j->frames_in * ch;
            float *pre;
            RET(get_buf(c, "sat_pre", (size_t)std::max<int64_t>(n, 1), &pre));
            if (n > 0)
                RET(launch(c, "sat_pre", sat_pre_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, ea.in, ea.in16, n,
                           ea.sat, pre));
            ea.in = pre;
            ea.in16 = nullptr;
            ea.sat.on = 0;
        }
    }
    ea.width = j->width;
    ea.width_on = j->width_on && ch == 2;
    ea.q_out = reinterpret_cast<int16_t *>(q1);
    if (j->eq.nsec > 0) RET(get_buf(c, "eq_xs", (size_t)TG * 2, &ea.xs));
    if (G > 0) {
        // --- stage A: saturation -> EQ -> width -> int16 (AME:55-63)
        if (j->eq.nsec == 0) {
            const unsigned nf = blocks_for(N, 256);
            if (ch == 2) RET(launch(c, "pre_pointwise", pre_pointwise_kernel<2>, dim3(nf), dim3(256), 0, ea));
            else RET(launch(c, "pre_pointwise", pre_pointwise_kernel<1>, dim3(nf), dim3(256), 0, ea));
        } else {
            fill_sos(ea.sos, j->eq, j->eq.nsec);
            LbArgs lb{};
            RET(upload_tables(c, "eq", j->eq, lb));
            RET(lb_prepare(c, nblk, ch, lb, 0));
            RET(launch_eq(c, j->eq.nsec, ch, nblk, ea, lb, K));
        }
    }
    short2 *mix = q1;
    const unsigned nb = blocks_for(std::max<int64_t>(G, 1), 256);
    if (j->multiband_on && G > 0) {
        // --- stage B: crossover + band quantisation (AME:196-206)
        short2 *bands[3];
        RET(get_buf(c, "band0", TG, &bands[0]));
        RET(get_buf(c, "band1", TG, &bands[1]));
        RET(get_buf(c, "band2", TG, &bands[2]));
        XoArgs xa{};
        xa.N_proc = N;
        xa.G = G;
        xa.T = T;
        fill_sos(xa.sos, j->xover, 4);
        xa.q_in = reinterpret_cast<const int16_t *>(q1);
        for (int b = 0; b < 3; ++b) xa.band[b] = reinterpret_cast<int16_t *>(bands[b]);
        double *tile_e;  // [3][E, tail][G]
        RET(get_buf(c, "comp_tile_e", (size_t)6 * G, &tile_e));
        for (int b = 0; b < 3; ++b) {
            xa.E[b] = tile_e + (size_t)(2 * b) * G;
            xa.tail[b] = tile_e + (size_t)(2 * b + 1) * G;
            const int r = j->band[b].look % T;
            xa.tail_from[b] = r ? T - r : T;
        }
        LbArgs lb{};
        RET(upload_tables(c, "xover", j->xover, lb));
        if ((size_t)T * 8 * sizeof(double) <= (size_t)lb_lds_bytes<8, 1>())  // (the weights alias its LDS)
            RET(upload_zw(c, "xover", j->xover, T, &xa.zw));
        RET(lb_prepare(c, nblk, ch, lb, 1));
        if (ch == 2)
            RET(launch(c, "xover", xover_kernel<2>, dim3(nblk), dim3(LB_THREADS), lb_lds_bytes<8, 2>(), xa, lb,
                       (int64_t)K));
        else
            RET(launch(c, "xover", xover_kernel<1>, dim3(nblk), dim3(LB_THREADS), lb_lds_bytes<8, 1>(), xa, lb,
                       (int64_t)K));

        // --- stage C: 3-band compressor + overlay (AME:207-210)
        short2 *q2;
        RET(stage_compress(c, j, bands, tile_e, &q2, pad, n_pad));
        mix = q2;
    } else {
        c->comp.on = false;
    }
    c->mix = mix;
    c->staged = true;
    return MM_OK;
}

// One track of the staged mix to its output: G tiles from tile g_off on.  `tail`:
// the chain's last finalize launch, which hands the readback area over.
static int finalize(mm_ctx *c, const mm_job *j, int64_t G, int64_t g_off, double gain, const double *gain_dev,
                    int use_gain, void *d_out, bool tail = false) {
    FinArgs fa{};
    HIPCHK(c, c->ctl.attach_tail(tail && G > 0 ? &fa : nullptr));
    if (G == 0) return MM_OK;
    fa.N_proc = j->frames_proc;
    fa.G = G;
    fa.Gs = c->G;
    fa.g_off = g_off;
    fa.T = j->tile;
    fa.ch = j->channels;
    fa.out_kind = j->out_kind;
    fa.use_gain = use_gain;
    fa.gain = gain;
    fa.gain_dev = gain_dev;
    fa.mix = c->mix;
    fa.out = d_out;
    const size_t lds = (size_t)FIN_TILES * (j->tile + 1) * sizeof(short2);
    if (fa.ch == 2)
        return launch(c, "finalize", finalize_kernel<2>, dim3(blocks_for(G, FIN_TILES)), dim3(256), lds, fa);
    return launch(c, "finalize", finalize_kernel<1>, dim3(blocks_for(G, FIN_TILES)), dim3(256), lds, fa);
}

// Stage the chunk chain of a range (time-sharded ranks) to convergence.  The staged
// job outlives this call, so its loudness arrays become the library's copies.
static int stage_chunks(mm_ctx *c, const mm_job *j, const void *d_in) {
    RET(validate(c, j));
    RET(stage_front(c, j, d_in, j->lufs_on ? kw_nblk(j, (j->frames_proc + j->tile - 1) / j->tile) : 0u));
    c->loud.own_job(&c->job);
    return chain_check(c);
}

// the per-stage operators (AME:117-227 one at a time), then the loudness tail
#include "ops.hip"
#include "loudness.hip"

// ------------------------------------------------------------------ units
// What a context runs between two syncs: n >= 1 tracks with the same settings,
// mastered as ONE line.  A single track (mm_master*, a batch's lone tracks) is a
// unit of one and keeps its own geometry: its job goes to the chunk stages as it
// is, the line is its ceil(frames / tile) tiles, and L and the gain arrive with the
// tail's readback.  A fused unit (n > 1: a same-settings run of mm_master_batch,
// BASELINE C3/C5 on one GPU) is a timeline: track i occupies whole chunks
// [off_i, off_i + n_i * CF) of it, its last chunk zero-padded; every per-chunk
// stage (EQ, crossover, compressor: AME:48-77 restarts them per chunk) then runs
// once over all tracks with the single-track kernels, and the padding changes none
// of a track's frames because it follows them and every stage is causal.  The
// K-weighting line restarts at each track start and gives padding frames zero
// energy; the gating runs one block per track; finalize writes every track to its
// own output.  One launch per stage covers the whole batch (n times one track's
// lanes), which fills the GPU where a single track's latency-bound launches leave
// most SIMDs idle.
struct Unit {
    int n = 1;
    const mm_job *J = nullptr;        // [n]
    const void *const *in = nullptr;  // [n] device inputs
    void *const *out = nullptr;       // [n] device outputs
    // the timeline's layout (n > 1: unit_layout)
    std::vector<int64_t> off;  // [n + 1] first timeline frame of each track (and the end)
    std::vector<int64_t> nch;  // [n] chunks of each track
    int64_t P = 0;             // timeline frames
    TrackTable geom;           // gating blocks and track table on the device (unit_geometry)
    std::vector<int64_t> pad;  // {track end, end of its last chunk} of the tracks that end inside a chunk
};

static bool same_iir(const mm_iir &a, const mm_iir &b) { return memcmp(&a, &b, sizeof a) == 0; }

// jobs that differ only in their track (length, loudness geometry): one timeline
static bool fusable(const mm_job *J, int n) {
    const mm_job &a = J[0];
    for (int i = 0; i < n; ++i) {
        const mm_job &b = J[i];
        if (b.frames_proc <= 0) return false;
        if (i == 0) continue;
        if (b.channels != a.channels || b.rate != a.rate || b.tile != a.tile || b.tiles_per_chunk != a.tiles_per_chunk ||
            b.sat_keep != a.sat_keep || b.sat_mix != a.sat_mix || b.sat_drive != a.sat_drive || b.sat_on != a.sat_on ||
            (b.sat_table == nullptr) != (a.sat_table == nullptr) || b.sat_key != a.sat_key ||
            b.width != a.width || b.width_on != a.width_on || b.multiband_on != a.multiband_on ||
            b.lufs_on != a.lufs_on || b.out_kind != a.out_kind || b.in_kind != a.in_kind ||
            b.comp_warmup != a.comp_warmup || b.comp_max_iters != a.comp_max_iters || b.comp_super != a.comp_super)
            return false;
        if (!same_iir(a.eq, b.eq)) return false;
        if (a.lufs_on && (b.lufs_target != a.lufs_target || b.block_scale != a.block_scale || !same_iir(a.kweight, b.kweight)))
            return false;
        if (a.multiband_on) {
            if (!same_iir(a.xover, b.xover)) return false;
            for (int k = 0; k < 3; ++k) {
                const mm_band &x = a.band[k], &y = b.band[k];
                if (x.thresh_rms != y.thresh_rms || x.attack_frames != y.attack_frames ||
                    x.release_frames != y.release_frames || x.look != y.look || x.r0 != y.r0)
                    return false;
                const bool keyed = x.lut_key != 0 && y.lut_key != 0;
                if (keyed ? x.lut_key != y.lut_key
                          : (x.lut != y.lut && memcmp(x.lut, y.lut, (size_t)32769 * 4 * sizeof(double)) != 0))
                    return false;
            }
        }
    }
    return true;
}

static bool unit_layout(Unit *p) {
    const mm_job *J = p->J;
    const int n = p->n;
    const int64_t CF = (int64_t)J[0].tile * J[0].tiles_per_chunk;
    p->off.assign((size_t)n + 1, 0);
    p->nch.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        p->nch[i] = (J[i].frames_proc + CF - 1) / CF;
        p->off[i + 1] = p->off[i] + p->nch[i] * CF;
    }
    p->P = p->off[n];
    return p->P < ((int64_t)1 << 31);  // 32-bit frame indexing
}

// Loudness geometry of the unit's line, uploaded before anything is queued (its one
// sync then waits on nothing).  A unit of one: the block programs of the track's
// own blocks, cached on the context.  A timeline: every track's first gating block,
// first tile and the end of its real frames, and the block programs of every
// track's own blocks at its timeline offset.
static int unit_geometry(mm_ctx *c, Unit *p) {
    const mm_job *J = p->J;
    const int n = p->n;
    p->geom = TrackTable{};
    if (n == 1) {
        p->geom.n_blocks = J->n_blocks;
        return c->loud.kb_upload(c, J->block_lo, J->block_hi, (size_t)J->n_blocks);
    }
    const int T = J[0].tile;
    std::vector<int64_t> tblk((size_t)n + 1), tt0((size_t)n), tend((size_t)n), lo, hi;
    for (int i = 0; i < n; ++i) {
        const int64_t o = p->off[i];
        tblk[i] = (int64_t)lo.size();
        for (int64_t b = 0; b < J[i].n_blocks; ++b) {
            lo.push_back(o + J[i].block_lo[b]);
            hi.push_back(o + J[i].block_hi[b]);
        }
        tt0[i] = o / T;
        tend[i] = o + J[i].frames_proc;
    }
    tblk[n] = (int64_t)lo.size();
    RET(c->loud.kb_upload(c, lo.data(), hi.data(), lo.size()));
    p->geom.n_blocks = (int64_t)lo.size();
    p->geom.n_trk = n;
    RET(get_buf(c, "fz_trk_blk", tblk.size(), &p->geom.trk_blk));
    RET(get_buf(c, "fz_trk_tile0", tt0.size(), &p->geom.trk_tile0));
    RET(get_buf(c, "fz_trk_end", tend.size(), &p->geom.trk_end));
    HIPCHK(c, hipMemcpyAsync(p->geom.trk_blk, tblk.data(), tblk.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p->geom.trk_tile0, tt0.data(), tt0.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p->geom.trk_end, tend.data(), tend.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // host vectors are transient
    return MM_OK;
}

// Loudness of the staged line, every track's finalize (the last launch hands the
// readback area over), and the readback: what follows the chunk stages, and again
// an extended solve.
static int unit_tail(mm_ctx *c, const Unit &u) {
    const mm_job &j0 = u.J[0];
    const bool fused = u.n > 1, lufs = j0.lufs_on && c->G > 0;
    // lg[2i] = L, lg[2i+1] = gain: a single track's in the readback area
    double *lg = c->ctl.dev()->lg;
    if (fused) RET(get_buf(c, "fz_lg", (size_t)2 * u.n, &lg));
    if (lufs) RET(line_loudness(c, &j0, fused ? u.P : j0.frames_proc, u.geom, lg));
    for (int i = 0; i < u.n; ++i)
        RET(finalize(c, &u.J[i], fused ? u.nch[i] * j0.tiles_per_chunk : c->G, fused ? u.off[i] / j0.tile : 0, 1.0,
                     lufs ? lg + 2 * i + 1 : nullptr, j0.lufs_on, u.out[i], i == u.n - 1));
    return c->ctl.tail ? MM_OK : queue_readback(c);
}

// Queue a unit without host round trips: loudness geometry (uploaded first: its
// sync waits on an idle stream), for a timeline its input (in place when the tracks
// already lie back to back on whole chunks, else gathered with the padding zeroed),
// the chunk stages, then the tail.
static int unit_enqueue(mm_ctx *c, Unit &u) {
    RET(validate(c, u.J));
    const mm_job &j0 = u.J[0];
    const bool fused = u.n > 1;
    const int64_t G = ((fused ? u.P : j0.frames_proc) + j0.tile - 1) / j0.tile;
    const bool lufs = j0.lufs_on && G > 0;  // (G == 0: a single empty track; fusable tracks have frames)
    if (lufs) RET(unit_geometry(c, &u));
    const mm_job *line = &j0;
    const void *tin = u.in[0];
    mm_job tj;
    const int64_t *pad = nullptr;
    if (fused) {
        const size_t fb = (size_t)j0.channels * in_sample_bytes(j0.in_kind);
        bool in_place = true;
        for (int i = 0; i < u.n && in_place; ++i)
            in_place = u.J[i].frames_in == u.off[i + 1] - u.off[i] &&
                       static_cast<const char *>(u.in[i]) == static_cast<const char *>(u.in[0]) + u.off[i] * fb;
        if (!in_place) {
            char *buf;
            RET(get_buf(c, "fz_in", (size_t)u.P * fb, &buf));
            for (int i = 0; i < u.n; ++i) {
                const int64_t len = u.off[i + 1] - u.off[i], nin = std::min(u.J[i].frames_in, len);
                if (nin > 0)
                    HIPCHK(c, hipMemcpyAsync(buf + u.off[i] * fb, u.in[i], nin * fb, hipMemcpyDeviceToDevice, c->stream));
                if (len > nin) HIPCHK(c, hipMemsetAsync(buf + (u.off[i] + nin) * fb, 0, (len - nin) * fb, c->stream));
            }
            tin = buf;
        }
        tj = j0;  // the timeline as one job (loudness is per track)
        tj.frames_in = tj.frames_proc = u.P;
        tj.lufs_on = 0;
        line = &tj;
        u.pad.clear();  // (the unit outlives the copy: unit_complete syncs)
        for (int i = 0; i < u.n && j0.multiband_on; ++i)
            if (u.off[i] + u.J[i].frames_proc < u.off[i + 1]) {
                u.pad.push_back(u.off[i] + u.J[i].frames_proc);
                u.pad.push_back(u.off[i + 1]);
            }
        if (!u.pad.empty()) {
            int64_t *d;
            RET(get_buf(c, "fz_pad", u.pad.size(), &d));
            HIPCHK(c, hipMemcpyAsync(d, u.pad.data(), u.pad.size() * 8, hipMemcpyHostToDevice, c->stream));
            pad = d;
        }
    }
    RET(stage_front(c, line, tin, lufs ? kw_nblk(&j0, G) : 0u, pad, pad ? (int)(u.pad.size() / 2) : 0));
    return unit_tail(c, u);
}

// The unit's one sync: checks the compressor's convergence (a rare unconverged
// solve is extended and the tail re-run) and reads the results.
static int unit_complete(mm_ctx *c, const Unit &u, mm_result *res) {
    RET(solve_to_convergence(c, [&] { return unit_tail(c, u); }));
    if (!res) return MM_OK;
    const mm_job &j0 = u.J[0];
    const bool fused = u.n > 1, lufs = j0.lufs_on && c->G > 0;
    const RbHead &rb = c->ctl.head();
    const Solve &sv = c->comp;
    const double *lg = rb.lg;
    std::vector<double> l2;
    if (fused && lufs) {  // (only a timeline's L and gains lie outside the readback area)
        double *d;
        RET(get_buf(c, "fz_lg", (size_t)2 * u.n, &d));
        l2.resize((size_t)2 * u.n);
        HIPCHK(c, hipMemcpy(l2.data(), d, l2.size() * sizeof(double), hipMemcpyDeviceToHost));
        lg = l2.data();
    }
    const int64_t nchk = c->ctl.lay.chunks, CF = (int64_t)j0.tile * j0.tiles_per_chunk;
    for (int i = 0; i < u.n; ++i) {
        mm_result &r = res[i];
        r.loudness = j0.lufs_on ? (lufs ? lg[2 * i] : -INFINITY) : NAN;  // no frames: pyloudnorm raised earlier
        r.gain_linear = j0.lufs_on ? (lufs ? lg[2 * i + 1] : INFINITY) : 1.0;
        r.frames_out = u.J[i].frames_proc;
        r.comp_iters = sv.iters;  // one solve for the whole unit
        r.comp_active = 0;             // summed over the track's own chunks (no compressor: no counts)
        for (int b = 0; b < 3 && sv.on; ++b)
            for (int64_t k = fused ? u.off[i] / CF : 0; k < (fused ? u.off[i + 1] / CF : nchk); ++k)
                r.comp_active += c->ctl.totals(b, k);
        // the unit's solve statistics are reported once, on its first track (sums over
        // a batch's results then count every unit once)
        r.comp_walked = i == 0 && sv.on ? (int64_t)rb.walked[0] : 0;
        r.comp_jumped = i == 0 && sv.on ? (int64_t)rb.walked[1] : 0;
    }
    return MM_OK;
}

// The per-call results of a master call (mm_last_meters, mm_last_r128, mm_last_qc, mm_last_spectrum,
// mm_last_ceilings, mm_last_levels, mm_last_resample): none at its start; before its end one entry for each of
// the n delivered buffers of what any of them asked for (meter_on: the reports asked for, bits or-ed).
static void results_reset(mm_ctx *c, int n = 0, bool ceiling = false, int meter_on = 0, bool level = false) {
    c->meters.assign(meter_on & MM_REPORT_METER ? (size_t)n : 0, mm_meter{});
    c->r128s.assign(meter_on & MM_REPORT_R128 ? (size_t)n : 0, mm_r128{});
    c->qcs.assign(meter_on & MM_REPORT_QC ? (size_t)n : 0, mm_qc{});
    c->spectra.assign(meter_on & MM_REPORT_SPECTRUM ? (size_t)n : 0, mm_spectrum{});
    c->spectrum_bins.assign(c->spectra.size(), std::vector<double>());
    c->ceilings.assign(ceiling ? (size_t)n : 0, mm_ceiling{});
    c->levels.assign(level ? (size_t)n : 0, mm_level{});
    c->albums.clear();
    c->album_r128s.clear();
    c->resample_valid = false;
}

// The chain's ceiling window: round-half-even(rate / 200) = 5 ms, within [1, 1024]
// (design.ceiling_window).
static int ceiling_window(int rate) {
    int q = rate / 200;
    const int rem = rate % 200;
    if (rem > 100 || (rem == 100 && (q & 1))) ++q;
    return std::min(mm_ceiling_max_window(), std::max(1, q));
}

static int master_device(mm_ctx *c, const mm_job *j, const void *d_in, void *d_out, mm_result *res) {
    results_reset(c);
    Unit u;
    u.J = j;
    u.in = &d_in;
    u.out = &d_out;
    RET(unit_enqueue(c, u));
    RET(unit_complete(c, u, res));
    results_reset(c, 1, j->ceiling_q28, j->meter_on);
    return finish_delivered(c, d_out, j->out_kind, j->frames_proc, j->channels, 0, j->ceiling_q28, ceiling_window(j->rate),
                            j->meter_on, j);
}

// The units of a batch: one track, or consecutive same-settings tracks fused into one
// timeline.  A run of such tracks is split into max(2, ceil(frames / cap)) units of
// about equal length (cap MM_FUSE_MAX_FRAMES, default 150 M frames): two units in
// flight on two streams overlap one unit's latency-bound tail with the other's
// front (C3 8 x 3 min: 14.5 G frames/s as 2 units, 14.2 as 1, 13.7 as 4; C5 16 x 3
// min at 96 kHz: 12.6 as 2, 12.3 as 4, 12.0 as 1, 11.0 unfused), and the cap
// keeps a unit's compacted envelope arrays to a few GB.
static std::vector<Unit> batch_units(const mm_job *J, const void *const *d_in, void *const *d_out, int n) {
    int64_t cap = 150000000;
    if (const char *e = getenv("MM_FUSE_MAX_FRAMES")) cap = std::max<int64_t>(1, atoll(e));
    const bool fuse = !getenv("MM_BATCH_STREAMS_ONLY");
    auto padded = [&](int i) {
        const int64_t CF = (int64_t)J[i].tile * J[i].tiles_per_chunk;
        return (J[i].frames_proc + CF - 1) / CF * CF;
    };
    auto unit = [&](int first, int count) {
        Unit u;
        u.n = count;
        u.J = J + first;
        u.in = d_in + first;
        u.out = d_out + first;
        return u;
    };
    std::vector<Unit> units;
    for (int i = 0; i < n;) {
        int run = 1;  // maximal run of tracks fusable with track i
        int64_t total = padded(i);
        while (fuse && i + run < n) {
            const mm_job pair[2] = {J[i], J[i + run]};
            if (!fusable(pair, 2)) break;
            total += padded(i + run);
            ++run;
        }
        const int parts = (int)std::min<int64_t>(run, std::max<int64_t>(std::min(2, run), (total + cap - 1) / cap));
        int64_t acc = 0;
        int k = i;
        for (int q = 0; q < parts; ++q) {  // close unit q once it holds about (q+1)/parts of the run
            const int first = k;
            if (q + 1 == parts) {
                k = i + run;
            } else {
                const int64_t goal = total * (q + 1) / parts;
                acc += padded(k++);
                while (k < i + run - (parts - q - 1) && acc + padded(k) / 2 <= goal) acc += padded(k++);
            }
            Unit u = unit(first, k - first);
            if (u.n > 1 && !unit_layout(&u)) {  // over 2^31 frames: one by one
                for (int t = first; t < k; ++t) units.push_back(unit(t, 1));
                continue;
            }
            units.push_back(std::move(u));
        }
        i += run;
    }
    return units;
}

// =================================================================== C-ABI
extern "C" {

int mm_version(void) { return MM_ABI_VERSION; }

int mm_solve_geometry(const mm_job *j, mm_solve_geom *out) {
    if (!j || !out) return MM_ERR_ARG;
    return solve_geometry(j, out);
}

// Verification only: the last chain's release-jump records of one band, active tile
// by active tile in compact order (the solve's buffers stay on the context)
int mm_solve_records(mm_ctx *c, int band, int64_t cap, int32_t *tiles, double *mmax, double *records,
                     int64_t *count) {
    if (!c || !count || band < 0 || band > 2 || cap < 0 || (cap > 0 && (!tiles || !mmax || !records)))
        return set_err(c, MM_ERR_ARG, "bad arguments");
    const Solve &sv = c->comp;
    if (!sv.on) return set_err(c, MM_ERR_STATE, "no envelope solve on this context");
    const CompArgs &ca = sv.ca;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t nchunks = ca.GS / ca.SPC;
    std::vector<int32_t> nact((size_t)nchunks);
    HIPCHK(c, hipMemcpy(nact.data(), ca.nact[band], (size_t)nchunks * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (int64_t ch = 0; ch < nchunks; ++ch) {
        const int64_t na = nact[(size_t)ch], take = std::max<int64_t>(0, std::min(na, cap - n));
        const int64_t ci = ch * ca.K;
        if (take > 0) {
            HIPCHK(c, hipMemcpy(tiles + n, ca.tl[band] + ci, (size_t)take * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(mmax + n, ca.mmaxc[band] + ci, (size_t)take * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(records + n * DREC, ca.descc[band] + ci * DREC, (size_t)take * DREC * sizeof(double),
                                hipMemcpyDeviceToHost));
        }
        n += na;
    }
    *count = n;
    return MM_OK;
}

#ifndef MM_SOURCE_SHA
#define MM_SOURCE_SHA "unknown"
#endif
const char *mm_source_sha(void) { return MM_SOURCE_SHA; }

int mm_create(int device, mm_ctx **out) {
    if (!out) return MM_ERR_ARG;
    *out = nullptr;
    mm_ctx *c = new mm_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) {
        delete c;
        return MM_ERR_HIP;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return MM_ERR_HIP;
    }
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
        c->n_cus = ncu;
    *out = c;
    return MM_OK;
}

int mm_destroy(mm_ctx *c) {
    if (!c) return MM_OK;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->comm) ncclCommDestroy(c->comm);
    resolve_events(c);
    for (auto e : c->free_events) hipEventDestroy(e);
    for (auto &kv : c->bufs)
        if (kv.second.p) hipFree(kv.second.p);
    for (int b = 0; b < 2; ++b) {
        if (c->pin[b]) hipHostFree(c->pin[b]);
        if (c->pin_ev[b]) hipEventDestroy(c->pin_ev[b]);
    }
    c->ctl.free();
    for (mm_ctx *k : c->children) mm_destroy(k);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return MM_OK;
}

const char *mm_last_error(mm_ctx *c) { return c ? c->err : "null context"; }

int mm_sync(mm_ctx *c) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    return MM_OK;
}

int mm_master_device(mm_ctx *c, const mm_job *j, const void *d_in, void *d_out, mm_result *res) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return master_device(c, j, d_in, d_out, res);
}

// A batch of independent tracks (BASELINE C3/C5 on one GPU), cut into units
// (batch_units: same-settings runs fused into one timeline, else units of one);
// unit u runs on child context u % S (own stream and buffers, S = min(units,
// MM_BATCH_STREAMS)), so up to S units are in flight at once and their
// latency-bound kernels fill each other's idle SIMDs.  Units are completed in
// submission order; a child's next unit is queued as soon as its previous one
// has been checked.
int mm_master_batch(mm_ctx *c, int n, const mm_job *jobs, const void *const *d_in, void *const *d_out,
                    mm_result *res) {
    if (!c || n < 0 || (n > 0 && (!jobs || !d_in || !d_out))) return set_err(c, MM_ERR_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < n; ++i) RET(validate(c, &jobs[i]));
    results_reset(c);
    std::vector<Unit> units = batch_units(jobs, d_in, d_out, n);
    const int nu = (int)units.size();
    const int S = std::min(nu, MM_BATCH_STREAMS);
    while ((int)c->children.size() < S) {
        mm_ctx *k = nullptr;
        if (mm_create(c->device, &k) != MM_OK) return set_err(c, MM_ERR_HIP, "cannot create a batch stream");
        c->children.push_back(k);
    }
    for (int s = 0; s < S; ++s) {
        c->children[s]->timing = c->timing;
    }
    auto complete = [&](mm_ctx *k, const Unit &u) { return unit_complete(k, u, res ? res + (u.J - jobs) : nullptr); };
    std::vector<int> cur((size_t)S, -1);
    int next = 0;
    auto fail = [&](mm_ctx *k) {
        set_err(c, MM_ERR_STATE, "batch job: %s", k->err);
        for (int s = 0; s < S; ++s) hipStreamSynchronize(c->children[s]->stream);
        return MM_ERR_STATE;
    };
    for (int s = 0; s < S && next < nu; ++s, ++next) {
        cur[s] = next;
        if (unit_enqueue(c->children[s], units[next]) != MM_OK) return fail(c->children[s]);
    }
    for (int done = 0; done < nu;) {
        for (int s = 0; s < S; ++s) {
            if (cur[s] < 0) continue;
            mm_ctx *k = c->children[s];
            if (complete(k, units[cur[s]]) != MM_OK) return fail(k);
            ++done;
            cur[s] = -1;
            if (next < nu) {
                cur[s] = next;
                if (unit_enqueue(k, units[next]) != MM_OK) return fail(k);
                ++next;
            }
        }
    }
    for (int s = 0; s < S; ++s) {  // per-kernel timing of the children lands in the parent's stats
        mm_ctx *k = c->children[s];
        resolve_events(k);
        for (auto &nm : k->stat_order) {
            auto it = c->stats.find(nm);
            if (it == c->stats.end()) {
                c->stat_order.push_back(nm);
                it = c->stats.emplace(nm, KStat{}).first;
            }
            it->second.ms += k->stats[nm].ms;
            it->second.n += k->stats[nm].n;
        }
        k->stats.clear();
        k->stat_order.clear();
    }
    int meter = 0;
    bool ceiling = false;
    for (int i = 0; i < n; ++i) meter |= jobs[i].meter_on;
    for (int i = 0; i < n; ++i) ceiling = ceiling || jobs[i].ceiling_q28;
    results_reset(c, n, ceiling, meter);
    for (int i = 0; i < n; ++i) {
        const mm_job &j = jobs[i];
        RET(finish_delivered(c, d_out[i], j.out_kind, j.frames_proc, j.channels, i, j.ceiling_q28, ceiling_window(j.rate),
                             j.meter_on, &j));
    }
    return MM_OK;
}

int mm_stage_chunks(mm_ctx *c, const mm_job *j, const void *d_in) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return stage_chunks(c, j, d_in);
}

int mm_finalize(mm_ctx *c, double gain_linear, int use_gain, void *d_out) {
    if (!c || !c->staged) return set_err(c, MM_ERR_STATE, "no staged job");
    return finalize(c, &c->job, c->G, 0, gain_linear, nullptr, use_gain, d_out);
}

int mm_read_mix(mm_ctx *c, int16_t *host_mix) {
    if (!c || !c->staged) return set_err(c, MM_ERR_STATE, "no staged job");
    const mm_job *j = &c->job;
    const int64_t N = j->frames_proc;
    if (N == 0) return MM_OK;
    int16_t *tmp;
    RET(get_buf(c, "mix_nat", (size_t)N * j->channels, &tmp));
    RET(launch(c, "mix_to_natural", mix_to_natural_kernel, dim3(blocks_for(N, 256)), dim3(256), 0,
               (const short2 *)c->mix, tmp, c->G, j->tile, N, j->channels));
    HIPCHK(c, hipMemcpyAsync(host_mix, tmp, (size_t)N * j->channels * sizeof(int16_t), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

int mm_timing(mm_ctx *c, int enable) {
    if (!c) return MM_ERR_ARG;
    c->timing = enable != 0;
    if (!enable) {
        c->stats.clear();
        c->stat_order.clear();
    }
    return MM_OK;
}

int mm_kernel_stats(mm_ctx *c, char *names, int names_cap, double *total_ms, int64_t *launches, int cap) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    std::string joined;
    int n = 0;
    for (auto &nm : c->stat_order) {
        if (n >= cap) break;
        total_ms[n] = c->stats[nm].ms;
        launches[n] = c->stats[nm].n;
        if (n) joined += "\n";
        joined += nm;
        ++n;
    }
    if (names && names_cap > 0) {
        strncpy(names, joined.c_str(), (size_t)names_cap - 1);
        names[names_cap - 1] = 0;
    }
    return n;
}

}  // extern "C"

// the WAV file path, the collectives, metering
#include "wav.hip"
#include "comm.hip"
#include "pcm16.h"
#include "tracks.h"  // the span counts of every grid over frames, one track or many
#include "meter.hip"
#include "r128.hip"
#include "qc.hip"
#include "spectrum.hip"
#include "ceiling.hip"
#include "level.hip"
#include "resample.hip"
#include "fir.hip"
#include "album.hip"
#include "tracks.hip"
