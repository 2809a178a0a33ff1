// mastering.hip — host side of the C-ABI (include/mastering.h), one translation
// unit: the launch sequence of the chain (a unit of n >= 1 tracks between two
// syncs), loudness gating, the batch scheduler and the staged / time-sharded entry
// points.  The chain's control block is control.h, the context that holds it
// context.h, followed by decode.hip (24/32-bit PCM input);
// wav.hip, comm.hip, ops.hip, then pcm16.h, meter.hip, ceiling.hip and resample.hip (with
// mm_master* / mm_deliver*: a master call with or without a delivery) come at the end.
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
#include "context.h"
#include "decode.hip"

// ceiling.hip: the end of a master call for delivered buffer i, the ceiling and then the report
static int finish_delivered(mm_ctx *c, void *d_out, int kind, int64_t frames, int channels, int i, int32_t ceiling_q28,
                            int32_t window, int meter_on, const mm_job *loud);

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

// ------------------------------------------------------------ K-weighting
// Loudness geometry of a line on the device: segment bounds, every gating block as a
// segment range, and for a timeline of several tracks (n_trk > 0) each track's
// first tile, the end of its real frames and its first gating block.
struct LineGeom {
    int n_trk = 0;
    int64_t n_segs = 0, n_blocks = 0;
    int64_t *bounds = nullptr, *trk_blk = nullptr, *trk_tile0 = nullptr, *trk_end = nullptr;
    int32_t *s0 = nullptr, *s1 = nullptr;
};

// Frames [lo, hi) of a gating block as the range of the S segments (bounds B[0..S])
// that begin in it.
static std::pair<int64_t, int64_t> seg_range(const int64_t *B, int64_t S, int64_t lo, int64_t hi) {
    return {std::min<int64_t>(std::lower_bound(B, B + S + 1, lo) - B, S),
            std::min<int64_t>(std::lower_bound(B, B + S + 1, hi) - B, S)};
}

// A single track's geometry (kept on the context, uploaded only when it changes).
static int upload_geometry(mm_ctx *c, const mm_job *j, LineGeom *g) {
    std::vector<int64_t> key;
    key.reserve((size_t)(j->n_segs + 3 + 2 * j->n_blocks));
    key.push_back(j->n_segs);
    key.insert(key.end(), j->seg_bounds, j->seg_bounds + j->n_segs + 1);
    key.push_back(j->n_blocks);
    key.insert(key.end(), j->block_lo, j->block_lo + j->n_blocks);
    key.insert(key.end(), j->block_hi, j->block_hi + j->n_blocks);
    *g = LineGeom{};
    g->n_segs = j->n_segs;
    g->n_blocks = j->n_blocks;
    RET(get_buf(c, "kw_bounds", (size_t)j->n_segs + 1, &g->bounds));
    RET(get_buf(c, "gate_s0", (size_t)j->n_blocks, &g->s0));
    RET(get_buf(c, "gate_s1", (size_t)j->n_blocks, &g->s1));
    if (key == c->geom_cache) return MM_OK;
    std::vector<int32_t> s0((size_t)j->n_blocks), s1((size_t)j->n_blocks);
    const int64_t S = j->n_segs;
    for (int64_t b = 0; b < j->n_blocks; ++b) {
        const auto r = seg_range(j->seg_bounds, S, j->block_lo[b], j->block_hi[b]);
        s0[b] = (int32_t)r.first;
        s1[b] = (int32_t)r.second;
    }
    HIPCHK(c, hipMemcpyAsync(g->bounds, j->seg_bounds, (S + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(g->s0, s0.data(), s0.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(g->s1, s1.data(), s1.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // host vectors are transient
    c->geom_cache = key;
    return MM_OK;
}

// ---- numpy's float32 np.sum as a program (gate.hip kw_blocks_kernel) ----------
// The reduction tree of np.sum over n contiguous float32 values: 8192-element
// buffer chunks summed in order, each chunk numpy's pairwise recursion (leaves of
// <= 128 elements).  Serialised as gate.hip's program layout.
struct PwBuild {
    std::vector<int32_t> loff, llen;        // leaves in order
    std::vector<int32_t> na, nb, nh;        // nodes: operands (>= 0 leaf, < 0 node ~k) and height
    std::vector<int32_t> chunk_leaf;
};
static int32_t pw_node(PwBuild &b, int32_t va, int32_t vb, int32_t ha, int32_t hb, int32_t *h) {
    b.na.push_back(va);
    b.nb.push_back(vb);
    *h = std::max(ha, hb) + 1;
    b.nh.push_back(*h);
    return ~(int32_t)(b.na.size() - 1);
}
static int32_t pw_rec(PwBuild &b, int32_t off, int32_t m, int32_t *h) {
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
static void pw_build(int64_t n, std::vector<int32_t> &out) {
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
static float pw_eval(const int32_t *P, const float *x) {
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

// Per-block programs on the device: blocks [lo_b, hi_b) of the line; one program
// per distinct length (the clamped last blocks of a track differ).  The blocks the
// device already holds are recognised without building anything: a unit calls this
// before its first launch, on the step's critical path.
static int kb_upload(mm_ctx *c, const int64_t *lo, const int64_t *hi, size_t nb) {
    if (c->kb_prog && c->kb_cache.size() == 2 * nb && std::equal(lo, lo + nb, c->kb_cache.begin()) &&
        std::equal(hi, hi + nb, c->kb_cache.begin() + nb))
        return MM_OK;
    std::vector<int64_t> key(lo, lo + nb), n(nb);
    key.insert(key.end(), hi, hi + nb);
    for (size_t b = 0; b < nb; ++b) n[b] = hi[b] - lo[b];
    RET(get_buf(c, "kb_lo", std::max<size_t>(nb, 1), &c->kb_lo));
    RET(get_buf(c, "kb_prog_of", std::max<size_t>(nb, 1), &c->kb_prog_of));
    RET(get_buf(c, "kb_n", std::max<size_t>(nb, 1), &c->kb_n));
    std::map<int64_t, int32_t> at;
    std::vector<int32_t> prog, of(nb), n32(nb);
    int nvals = 1, pints = 4;
    for (size_t b = 0; b < nb; ++b) {
        if (n[b] < 0 || n[b] > 16 * KB_CHUNK) return set_err(c, MM_ERR_ARG, "loudness block of %lld frames", (long long)n[b]);
        auto it = at.find(n[b]);
        if (it == at.end()) {
            const int32_t o = (int32_t)prog.size();
            pw_build(n[b], prog);
            if (prog[o] + prog[o + 1] > KB_VMAX || (int64_t)prog.size() - o > KB_PMAX)
                return set_err(c, MM_ERR_ARG, "loudness block program too large");
            while (prog.size() % 4) prog.push_back(0);  // (16-byte aligned programs: int4 copies)
            nvals = std::max(nvals, prog[o] + prog[o + 1]);
            pints = std::max(pints, (int)(prog.size() - o));
            it = at.emplace(n[b], o).first;
        }
        of[b] = it->second;
        n32[b] = (int32_t)n[b];
    }
    c->kb_prog = nullptr;  // (get_buf may move it: re-fetched below)
    prog.resize(prog.size() + pints, 0);  // every block copies the largest program's length
    RET(get_buf(c, "kb_prog", prog.size(), &c->kb_prog));
    if (nb) {
        HIPCHK(c, hipMemcpyAsync(c->kb_lo, lo, nb * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->kb_prog_of, of.data(), nb * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->kb_n, n32.data(), nb * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->kb_prog, prog.data(), prog.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // host vectors are transient
    c->kb_cache = key;
    c->kb_nvals = nvals;
    c->kb_pints = pints;
    return MM_OK;
}

// The K-weighting kernel's arguments for the staged mix of G tiles holding `frames`
// frames: one lane per sub-tile of kweight.tile frames (design.kweight_sub), `sub`
// per tile.  The caller adds its mode's outputs and, for a timeline, the track tables.
static KwArgs kw_args(const mm_ctx *c, const mm_job *j, int64_t frames, int64_t G) {
    KwArgs ka{};
    ka.sub = j->tile / j->kweight.tile;
    ka.N_proc = frames;
    ka.G = G * ka.sub;
    ka.T = j->kweight.tile;
    ka.Gt = G;
    ka.ch = j->channels;
    for (int s_ = 0; s_ < 2; ++s_)
        for (int k = 0; k < 5; ++k) ka.sos[s_][k] = j->kweight.sos[s_][k];
    ka.mix = reinterpret_cast<const int16_t *>(c->mix);
    return ka;
}

// Queue the K-weighting of the staged line (SQ: pass 2 writes the f32 squares, else
// the segment partials); a time-sharded range starts from `carry_in_host`.
template <bool SQ>
static int kweight_run(mm_ctx *c, const mm_job *j, const KwArgs &ka, const double *carry_in_host = nullptr) {
    LbArgs lb{};
    RET(upload_tables(c, "kweight", j->kweight, lb));
    const unsigned nblk = blocks_for(ka.G, LB_THREADS);
    RET(lb_prepare(c, nblk, 1, lb, 2));
    if (carry_in_host) {
        double *init;
        RET(get_buf(c, "kw_init", 8, &init));
        HIPCHK(c, hipMemcpyAsync(init, carry_in_host, 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // pageable source
        lb.init = init;
    }
    return launch(c, "kweight", kweight_kernel<SQ>, dim3(nblk), dim3(LB_THREADS), lb_lds_bytes<4, 1>(), ka, lb);
}

// Segment energies of a line (round 5's loudness, and the time-sharded ranks'):
// K-weighting + f64 energies per segment of `g`.  Returns the device segment-energy
// vector; `line_end` receives the state after the last frame when requested.
static int kweight_segments(mm_ctx *c, const mm_job *j, int64_t frames, const LineGeom &g,
                            const double *carry_in_host, double *line_end, double **seg_out) {
    KwArgs ka = kw_args(c, j, frames, c->G);
    double *seg;
    RET(get_buf(c, "kw_part", (size_t)std::max<int64_t>(ka.G, 1) * 2, &ka.part));
    RET(get_buf(c, "kw_part_seg", (size_t)std::max<int64_t>(ka.G, 1), &ka.part_seg));
    RET(get_buf(c, "kw_seg", (size_t)g.n_segs, &seg));
    ka.n_segs = g.n_segs;
    ka.seg_bounds = g.bounds;
    ka.line_end = line_end;
    ka.n_trk = g.n_trk;
    ka.trk_tile0 = g.trk_tile0;
    ka.trk_end = g.trk_end;
    RET(kweight_run<false>(c, j, ka, carry_in_host));
    RET(launch(c, "seg_reduce", seg_reduce_kernel, dim3(blocks_for(g.n_segs, 4)), dim3(256), 0, ka, seg));  // wave per segment
    *seg_out = seg;
    return MM_OK;
}

// The staged job's segment energies (time-sharded ranks: carry-in state, range end state).
static int kweight_staged(mm_ctx *c, const double *carry_in_host, double *line_end, double **seg_out) {
    LineGeom g;
    RET(upload_geometry(c, &c->job, &g));
    return kweight_segments(c, &c->job, c->job.frames_proc, g, carry_in_host, line_end, seg_out);
}

// The exact loudness of a line (single track or fused timeline, AME:212-218): the
// K-weighting in lfilter's order writing np.square's f32 values, then pyloudnorm's
// block energies in numpy's reduction order (kw_blocks_kernel) into zl [2 nb].
// The block programs must be on the device (kb_upload) before this is queued.
static int kweight_exact(mm_ctx *c, const mm_job *j, int64_t frames, const LineGeom &g, double **zl_out) {
    const int64_t G = c->G, nb = g.n_blocks;
    float *sq;
    double *zl;
    const int Tt = j->tile, TP = (Tt + 3) / 4 * 4;  // padded tile stride (16-byte stores and loads)
    if (((KB_CHUNK - 1) / Tt + 2) * (TP / 4) > KB_LD * KB_THREADS)
        return set_err(c, MM_ERR_ARG, "tile of %d frames: the loudness block loads do not cover a chunk", Tt);
    RET(get_buf(c, "kw_sq", (size_t)(G * TP), &sq));
    RET(get_buf(c, "gate_zl", (size_t)std::max<int64_t>(2 * nb, 2), &zl));
    KwArgs ka = kw_args(c, j, frames, G);
    ka.n_trk = g.n_trk;
    ka.trk_tile0 = g.trk_tile0;
    ka.trk_end = g.trk_end;
    ka.sq = sq;
    ka.sq_tp = TP;
    RET(kweight_run<true>(c, j, ka));
    if (nb > 0) {
        KbArgs kb{};
        kb.sq = sq;
        kb.T = Tt;
        kb.TP = TP;
        kb.n_blocks = nb;
        kb.blk_lo = c->kb_lo;
        kb.blk_prog = c->kb_prog_of;
        kb.blk_n = c->kb_n;
        kb.prog = c->kb_prog;
        kb.scale = (float)j->block_scale;  // Python float * np.float32: the constant rounded to f32 (NEP 50)
        kb.zl = zl;
        kb.stage_floats = ((KB_CHUNK - 1) / Tt + 2) * TP;  // the padded tile runs a chunk can span
        kb.nvals = 2 * c->kb_nvals;  // (two value buffers)
        kb.pints = c->kb_pints;
        const size_t lds = (size_t)kb_lds_bytes(kb.stage_floats, kb.nvals, kb.pints);
        // persistent: as many workgroups as fit at once (a multiple of 8: the XCD-aware block mapping)
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, (160 * 1024) / (int64_t)(lds + 64)));  // (and VGPRs)
        const unsigned grid = (unsigned)std::min<int64_t>((nb + 7) / 8 * 8, (int64_t)c->n_cus * per_cu / 8 * 8);
        RET(launch(c, "kw_blocks", kw_blocks_kernel, dim3(std::max(grid, 8u)), dim3(KB_THREADS), lds, kb));
    }
    *zl_out = zl;
    return MM_OK;
}

// Host-returning variant (time-sharded ranks: carry-in state, range end state).
static int kweight_energies(mm_ctx *c, const double *carry_in_host, double *seg_host, double *range_end_host) {
    double *lend, *seg;
    RET(get_buf(c, "kw_lend", 8, &lend));
    RET(kweight_staged(c, carry_in_host, range_end_host ? lend : nullptr, &seg));
    if (range_end_host)
        HIPCHK(c, hipMemcpyAsync(range_end_host, lend, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (seg_host)
        HIPCHK(c, hipMemcpyAsync(seg_host, seg, c->job.n_segs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return chain_check(c);
}

// the gate: block energies and levels from the segment energies in parallel (unless
// ga.zl already holds them: the exact path), then one workgroup per track
static int gate_launch(mm_ctx *c, GateArgs ga, unsigned n_tracks) {
    if (!ga.zl) {
        RET(get_buf(c, "gate_zl", (size_t)(2 * ga.n_blocks), &ga.zl));
        RET(launch(c, "gate_blocks", gate_blocks_kernel, dim3(blocks_for(ga.n_blocks, GATE_BLK_THREADS)),
                   dim3(GATE_BLK_THREADS), 0, ga));
    }
    return launch(c, "gate", gate_kernel, dim3(n_tracks), dim3(GATE_THREADS), 0, ga);
}

// Loudness and gain of every track of the staged line on the device (no host round
// trip) into out[2i] = L, out[2i+1] = gain: exactly pyloudnorm's block energies, or
// with MM_LOUDNESS_SEGMENTS round 5's f64 segment energies (A/B builds).  The
// line's geometry must be on the device (unit_geometry) before this is queued.
static int line_loudness(mm_ctx *c, const mm_job *j, int64_t frames, const LineGeom &g, double *out) {
    GateArgs ga{};
    ga.n_blocks = g.n_blocks;
    ga.target = j->lufs_target;
    ga.out = out;
    ga.trk_blk = g.trk_blk;
    if (getenv("MM_LOUDNESS_SEGMENTS")) {
        double *seg;
        RET(kweight_segments(c, j, frames, g, nullptr, nullptr, &seg));
        ga.blk_s0 = g.s0;
        ga.blk_s1 = g.s1;
        ga.seg = seg;
        ga.scale = j->block_scale;
    } else {
        RET(kweight_exact(c, j, frames, g, &ga.zl));
    }
    return gate_launch(c, ga, (unsigned)std::max(g.n_trk, 1));
}

// numpy's float32 np.sum over x[0..n) evaluated on the host through the same
// program the device runs for pyloudnorm's block energies (CPU check of pw_build).
extern "C" int mm_np_sum_f32(const float *x, int64_t n, float *out) {
    if (!out || n < 0 || (n > 0 && !x) || n > 16 * KB_CHUNK) return MM_ERR_ARG;
    std::vector<int32_t> prog;
    pw_build(n, prog);
    *out = pw_eval(prog.data(), x);
    return MM_OK;
}

// pyloudnorm 0.1.1 integrated_loudness gating (mono, G=1), restated.
extern "C" int mm_gate_loudness(const mm_job *j, const double *seg_energy, double *loudness) {
    if (!j || !seg_energy || !loudness) return MM_ERR_ARG;
    const int64_t nb = j->n_blocks;
    std::vector<double> z((size_t)nb), l((size_t)nb);
    for (int64_t b = 0; b < nb; ++b) {
        const auto r = seg_range(j->seg_bounds, j->n_segs, j->block_lo[b], j->block_hi[b]);
        double acc = 0.0;
        for (int64_t s = r.first; s < r.second; ++s) acc += seg_energy[s];
        z[b] = j->block_scale * acc;
        l[b] = -0.691 + 10.0 * std::log10(z[b]);
    }
    double sum = 0.0;
    int64_t cnt = 0;
    for (int64_t b = 0; b < nb; ++b)
        if (l[b] >= -70.0) {
            sum += z[b];
            ++cnt;
        }
    double mean_abs = cnt ? sum / (double)cnt : NAN;
    double gamma_r = -0.691 + 10.0 * std::log10(mean_abs) - 10.0;
    sum = 0.0;
    cnt = 0;
    for (int64_t b = 0; b < nb; ++b)
        if (l[b] > gamma_r && l[b] > -70.0) {
            sum += z[b];
            ++cnt;
        }
    double zavg = cnt ? sum / (double)cnt : 0.0;  // np.nan_to_num(mean([])) == 0
    *loudness = -0.691 + 10.0 * std::log10(zavg);
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

// Stage the chunk chain of a range (time-sharded ranks) to convergence.
static int stage_chunks(mm_ctx *c, const mm_job *j, const void *d_in) {
    RET(validate(c, j));
    RET(stage_front(c, j, d_in, j->lufs_on ? kw_nblk(j, (j->frames_proc + j->tile - 1) / j->tile) : 0u));
    return chain_check(c);
}

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
    LineGeom geom;             // loudness geometry on the device (unit_geometry)
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
// own blocks (or its segment tables), cached on the context.  A timeline: every
// track's segment bounds shifted to its offset (a bound shared with the previous
// track's end is not repeated; the gap between a track's last bound and the next
// track start is a padding segment no gating block reads), every track's blocks as
// segment ranges of that list, and the block programs at the timeline offsets.
static int unit_geometry(mm_ctx *c, Unit *p) {
    const mm_job *J = p->J;
    const int n = p->n;
    if (n == 1) {
        if (getenv("MM_LOUDNESS_SEGMENTS")) return upload_geometry(c, J, &p->geom);
        p->geom = LineGeom{};
        p->geom.n_blocks = J->n_blocks;
        return kb_upload(c, J->block_lo, J->block_hi, (size_t)J->n_blocks);
    }
    const int T = J[0].tile;
    std::vector<int64_t> bounds, tblk((size_t)n + 1), tt0((size_t)n), tend((size_t)n);
    std::vector<int32_t> s0, s1;
    for (int i = 0; i < n; ++i) {
        const mm_job &j = J[i];
        const int64_t o = p->off[i];
        int64_t base;
        if (!bounds.empty() && bounds.back() == o + j.seg_bounds[0]) {
            base = (int64_t)bounds.size() - 1;
        } else {
            base = (int64_t)bounds.size();
            bounds.push_back(o + j.seg_bounds[0]);
        }
        for (int64_t s = 1; s <= j.n_segs; ++s) bounds.push_back(o + j.seg_bounds[s]);
        tblk[i] = (int64_t)s0.size();
        for (int64_t b = 0; b < j.n_blocks; ++b) {
            const auto r = seg_range(j.seg_bounds, j.n_segs, j.block_lo[b], j.block_hi[b]);
            s0.push_back((int32_t)(base + r.first));
            s1.push_back((int32_t)(base + r.second));
        }
        tt0[i] = o / T;
        tend[i] = o + j.frames_proc;
    }
    tblk[n] = (int64_t)s0.size();
    {  // the exact path's blocks: every track's own blocks at its timeline offset
        std::vector<int64_t> lo, hi;
        for (int i = 0; i < n; ++i)
            for (int64_t b = 0; b < J[i].n_blocks; ++b) {
                lo.push_back(p->off[i] + J[i].block_lo[b]);
                hi.push_back(p->off[i] + J[i].block_hi[b]);
            }
        RET(kb_upload(c, lo.data(), hi.data(), lo.size()));
    }
    if (bounds.back() < p->P) bounds.push_back(p->P);  // the last track's padding
    p->geom.n_segs = (int64_t)bounds.size() - 1;
    p->geom.n_blocks = (int64_t)s0.size();
    p->geom.n_trk = n;
    RET(get_buf(c, "fz_bounds", bounds.size(), &p->geom.bounds));
    RET(get_buf(c, "fz_trk_blk", tblk.size(), &p->geom.trk_blk));
    RET(get_buf(c, "fz_trk_tile0", tt0.size(), &p->geom.trk_tile0));
    RET(get_buf(c, "fz_trk_end", tend.size(), &p->geom.trk_end));
    RET(get_buf(c, "fz_s0", std::max<size_t>(s0.size(), 1), &p->geom.s0));
    RET(get_buf(c, "fz_s1", std::max<size_t>(s1.size(), 1), &p->geom.s1));
    HIPCHK(c, hipMemcpyAsync(p->geom.bounds, bounds.data(), bounds.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p->geom.trk_blk, tblk.data(), tblk.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p->geom.trk_tile0, tt0.data(), tt0.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p->geom.trk_end, tend.data(), tend.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (!s0.empty()) {
        HIPCHK(c, hipMemcpyAsync(p->geom.s0, s0.data(), s0.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(p->geom.s1, s1.data(), s1.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
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

// The per-call results of a master call (mm_last_meters, mm_last_ceilings, mm_last_resample):
// none at its start; before its end one entry for each of the n delivered buffers of what
// any of them asked for.
static void results_reset(mm_ctx *c, int n = 0, bool ceiling = false, bool meter = false) {
    c->meters.assign(meter ? (size_t)n : 0, mm_meter{});
    c->ceilings.assign(ceiling ? (size_t)n : 0, mm_ceiling{});
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
    bool meter = false, ceiling = false;
    for (int i = 0; i < n; ++i) meter = meter || jobs[i].meter_on;
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

int mm_kweight_range_end(mm_ctx *c, double *end_state_host) {
    if (!c || !c->staged) return set_err(c, MM_ERR_STATE, "no staged job");
    if (c->G == 0) {
        for (int k = 0; k < 4; ++k) end_state_host[k] = 0.0;
        return MM_OK;
    }
    return kweight_energies(c, nullptr, nullptr, end_state_host);
}

int mm_hop_energies(mm_ctx *c, const double *carry_in_host, double *seg_energy_host) {
    if (!c || !c->staged) return set_err(c, MM_ERR_STATE, "no staged job");
    if (c->G == 0) {
        for (int64_t s = 0; s < c->job.n_segs; ++s) seg_energy_host[s] = 0.0;
        return MM_OK;
    }
    return kweight_energies(c, carry_in_host, seg_energy_host, nullptr);
}

// Time-sharded loudness with the energy vector in HBM, in three steps a caller can
// compose with any collective between them (the library's communicator, or
// torch.distributed over the same device buffer):
//  1. mm_shard_energies_device: zero the caller's whole-track vector d_full and write
//     this rank's segment energies at seg_offset (a rank's segments are consecutive
//     global ones);
//  2. a sum all-reduce of d_full over the ranks (mm_allreduce_sum_f64_device);
//  3. mm_gate_finalize_device: pyloudnorm's gating of the whole track on the device,
//     the gain towards `target` applied by finalize straight from device memory;
//     returns L and the gain it applied.
int mm_shard_energies_device(mm_ctx *c, const double *carry_in_host, int64_t n_global_segs, int64_t seg_offset,
                             double *d_full) {
    if (!c || !c->staged) return set_err(c, MM_ERR_STATE, "no staged job");
    const int64_t nl = c->job.n_segs;
    if (!d_full || n_global_segs < 1 || seg_offset < 0 || seg_offset + nl > n_global_segs)
        return set_err(c, MM_ERR_ARG, "shard energies: segments [%lld, %lld) outside [0, %lld)",
                       (long long)seg_offset, (long long)(seg_offset + nl), (long long)n_global_segs);
    HIPCHK(c, hipMemsetAsync(d_full, 0, (size_t)n_global_segs * sizeof(double), c->stream));
    if (c->G > 0 && nl > 0) {
        double *seg;
        RET(kweight_staged(c, carry_in_host, nullptr, &seg));
        HIPCHK(c, hipMemcpyAsync(d_full + seg_offset, seg, (size_t)nl * sizeof(double), hipMemcpyDeviceToDevice,
                                 c->stream));
    }
    return chain_check(c);  // (synchronises the stream: d_full is complete on return)
}

int mm_gate_finalize_device(mm_ctx *c, const double *d_full, int64_t n_global_segs, int64_t n_blocks,
                            const int32_t *blk_s0_host, const int32_t *blk_s1_host, double block_scale,
                            double target, void *d_out, double *loudness_gain_host) {
    if (!c || !c->staged) return set_err(c, MM_ERR_STATE, "no staged job");
    if (!d_full || n_global_segs < 1 || n_blocks < 1 || !blk_s0_host || !blk_s1_host || !loudness_gain_host)
        return set_err(c, MM_ERR_ARG, "gate: bad segment or block geometry");
    for (int64_t b = 0; b < n_blocks; ++b)
        if (blk_s0_host[b] < 0 || blk_s1_host[b] < blk_s0_host[b] || blk_s1_host[b] > n_global_segs)
            return set_err(c, MM_ERR_ARG, "gate: block %lld has segments [%d, %d) outside [0, %lld)",
                           (long long)b, blk_s0_host[b], blk_s1_host[b], (long long)n_global_segs);
    double *gout;
    int32_t *s0, *s1;
    RET(get_buf(c, "shard_gate", 2, &gout));
    RET(get_buf(c, "shard_blk0", (size_t)n_blocks, &s0));
    RET(get_buf(c, "shard_blk1", (size_t)n_blocks, &s1));
    HIPCHK(c, hipMemcpyAsync(s0, blk_s0_host, (size_t)n_blocks * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s1, blk_s1_host, (size_t)n_blocks * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    GateArgs ga{};
    ga.n_blocks = n_blocks;
    ga.blk_s0 = s0;
    ga.blk_s1 = s1;
    ga.seg = d_full;
    ga.scale = block_scale;
    ga.target = target;
    ga.out = gout;
    RET(gate_launch(c, ga, 1));
    RET(finalize(c, &c->job, c->G, 0, 1.0, gout + 1, 1, d_out));
    // L and the gain finalize applied (gate.hip's device expression, not a host recomputation)
    HIPCHK(c, hipMemcpyAsync(loudness_gain_host, gout, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

// Steps 1-3 with the library's own communicator.  `world` is the plan's rank count:
// a multi-rank plan needs this context's RCCL communicator over exactly that many
// ranks, or every rank would gate only its own part of the vector (and return a
// different, wrong loudness) — refused instead.
int mm_shard_loudness_device(mm_ctx *c, const double *carry_in_host, int64_t n_global_segs, int64_t seg_offset,
                             int64_t n_blocks, const int32_t *blk_s0_host, const int32_t *blk_s1_host,
                             double block_scale, double target, int32_t world, void *d_out,
                             double *loudness_gain_host) {
    if (!c) return MM_ERR_ARG;
    if (world < 1) return set_err(c, MM_ERR_ARG, "shard loudness: world %d", world);
    if (world > 1 && (!c->comm || c->nranks != world))
        return set_err(c, MM_ERR_STATE, "shard loudness: a %d-rank plan needs this context's communicator over %d "
                       "ranks (have %d)", world, world, c->comm ? c->nranks : 0);
    double *full;
    RET(get_buf(c, "shard_seg", (size_t)std::max<int64_t>(n_global_segs, 1), &full));
    RET(mm_shard_energies_device(c, carry_in_host, n_global_segs, seg_offset, full));
    if (world > 1) RET(mm_allreduce_sum_f64_device(c, full, n_global_segs));
    return mm_gate_finalize_device(c, full, n_global_segs, n_blocks, blk_s0_host, blk_s1_host, block_scale, target,
                                   d_out, loudness_gain_host);
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

// the WAV file path, the collectives, per-stage operators (AME:117-227 one at a time), metering
#include "wav.hip"
#include "comm.hip"
#include "ops.hip"
#include "pcm16.h"
#include "meter.hip"
#include "ceiling.hip"
#include "resample.hip"
