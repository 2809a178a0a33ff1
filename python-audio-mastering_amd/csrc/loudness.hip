// loudness.hip — the loudness tail on the host (AME:212-222): what Loudness
// (loudness.h) keeps on the device, the exact block energies of a chain's line
// (line_loudness), the f64 segment energies of a staged range (the time-sharded
// entry points) and of the operator's line (mm_op_loudness), and the gate.
// Included by mastering.hip after finalize, chain_check and ops.hip (the operator's
// tile-major kernels) and before the units, which call line_loudness.

// One program per distinct block length (the clamped last blocks of a track
// differ).  The blocks the device already holds are recognised without building
// anything: a unit calls this before its first launch, on the step's critical path.
int Loudness::kb_upload(mm_ctx *c, const int64_t *lo, const int64_t *hi, size_t nb) {
    if (kb_prog && kb_cache.size() == 2 * nb && std::equal(lo, lo + nb, kb_cache.begin()) &&
        std::equal(hi, hi + nb, kb_cache.begin() + nb))
        return MM_OK;
    kb_prog = nullptr;  // no programs held until this upload completes (a failed one leaves none)
    std::vector<int64_t> key(lo, lo + nb), n(nb);
    key.insert(key.end(), hi, hi + nb);
    for (size_t b = 0; b < nb; ++b) n[b] = hi[b] - lo[b];
    RET(get_buf(c, "kb_lo", std::max<size_t>(nb, 1), &kb_lo));
    RET(get_buf(c, "kb_prog_of", std::max<size_t>(nb, 1), &kb_prog_of));
    RET(get_buf(c, "kb_n", std::max<size_t>(nb, 1), &kb_n));
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
    prog.resize(prog.size() + pints, 0);  // every block copies the largest program's length
    int32_t *d_prog;
    RET(get_buf(c, "kb_prog", prog.size(), &d_prog));
    if (nb) {
        HIPCHK(c, hipMemcpyAsync(kb_lo, lo, nb * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(kb_prog_of, of.data(), nb * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(kb_n, n32.data(), nb * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_prog, prog.data(), prog.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // host vectors are transient
    kb_prog = d_prog;
    kb_cache = key;
    kb_nvals = nvals;
    kb_pints = pints;
    return MM_OK;
}

void Loudness::kb_fill(KbArgs &kb) const {
    kb.blk_lo = kb_lo;
    kb.blk_prog = kb_prog_of;
    kb.blk_n = kb_n;
    kb.prog = kb_prog;
    kb.nvals = 2 * kb_nvals;  // (two value buffers)
    kb.pints = kb_pints;
}

int Loudness::upload_geometry(mm_ctx *c, const mm_job *j, SegGeom *g) {
    std::vector<int64_t> key;
    key.reserve((size_t)(j->n_segs + 3 + 2 * j->n_blocks));
    key.push_back(j->n_segs);
    key.insert(key.end(), j->seg_bounds, j->seg_bounds + j->n_segs + 1);
    key.push_back(j->n_blocks);
    key.insert(key.end(), j->block_lo, j->block_lo + j->n_blocks);
    key.insert(key.end(), j->block_hi, j->block_hi + j->n_blocks);
    *g = SegGeom{};
    g->n_segs = j->n_segs;
    g->n_blocks = j->n_blocks;
    RET(get_buf(c, "kw_bounds", (size_t)j->n_segs + 1, &g->bounds));
    RET(get_buf(c, "gate_s0", (size_t)j->n_blocks, &g->s0));
    RET(get_buf(c, "gate_s1", (size_t)j->n_blocks, &g->s1));
    if (key == geom_cache) return MM_OK;
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
    geom_cache = key;
    return MM_OK;
}

// ------------------------------------------------------------ K-weighting
// The K-weighting kernel's arguments for the staged mix of G tiles holding `frames`
// frames: one lane per sub-tile of kweight.tile frames (design.kweight_sub), `sub`
// per tile.  The caller adds its mode's outputs and, for a timeline, the track table.
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

// The staged job's f64 segment energies (time-sharded ranks: carry-in state, range
// end state): K-weighting + energies per segment of the job's own geometry.  Returns
// the device segment-energy vector; `line_end` receives the state after the last
// frame when requested.
static int kweight_segments(mm_ctx *c, const double *carry_in_host, double *line_end, double **seg_out) {
    const mm_job *j = &c->job;
    SegGeom g;
    RET(c->loud.upload_geometry(c, j, &g));
    KwArgs ka = kw_args(c, j, j->frames_proc, c->G);
    double *seg;
    RET(get_buf(c, "kw_part", (size_t)std::max<int64_t>(ka.G, 1) * 2, &ka.part));
    RET(get_buf(c, "kw_part_seg", (size_t)std::max<int64_t>(ka.G, 1), &ka.part_seg));
    RET(get_buf(c, "kw_seg", (size_t)g.n_segs, &seg));
    ka.n_segs = g.n_segs;
    ka.seg_bounds = g.bounds;
    ka.line_end = line_end;
    // one line, never a timeline: kweight_kernel<false> with n_trk > 0 is not reached from the host
    RET(kweight_run<false>(c, j, ka, carry_in_host));
    RET(launch(c, "seg_reduce", seg_reduce_kernel, dim3(blocks_for(g.n_segs, 4)), dim3(256), 0, ka, seg));  // wave per segment
    *seg_out = seg;
    return MM_OK;
}

// Host-returning variant (mm_kweight_range_end, mm_hop_energies).
static int kweight_energies(mm_ctx *c, const double *carry_in_host, double *seg_host, double *range_end_host) {
    double *lend, *seg;
    RET(get_buf(c, "kw_lend", 8, &lend));
    RET(kweight_segments(c, carry_in_host, range_end_host ? lend : nullptr, &seg));
    if (range_end_host)
        HIPCHK(c, hipMemcpyAsync(range_end_host, lend, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (seg_host)
        HIPCHK(c, hipMemcpyAsync(seg_host, seg, c->job.n_segs * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return chain_check(c);
}

// The exact loudness of a line (single track or fused timeline, AME:212-218): the
// K-weighting in lfilter's order writing np.square's f32 values, then pyloudnorm's
// block energies in numpy's reduction order (kw_blocks_kernel) into zl [2 nb].
// The block programs must be on the device (kb_upload) before this is queued.
static int kweight_exact(mm_ctx *c, const mm_job *j, int64_t frames, const TrackTable &t, double **zl_out) {
    const int64_t G = c->G, nb = t.n_blocks;
    float *sq;
    double *zl;
    const int Tt = j->tile, TP = (Tt + 3) / 4 * 4;  // padded tile stride (16-byte stores and loads)
    if (((KB_CHUNK - 1) / Tt + 2) * (TP / 4) > KB_LD * KB_THREADS)
        return set_err(c, MM_ERR_ARG, "tile of %d frames: the loudness block loads do not cover a chunk", Tt);
    RET(get_buf(c, "kw_sq", (size_t)(G * TP), &sq));
    RET(get_buf(c, "gate_zl", (size_t)std::max<int64_t>(2 * nb, 2), &zl));
    KwArgs ka = kw_args(c, j, frames, G);
    ka.n_trk = t.n_trk;
    ka.trk_tile0 = t.trk_tile0;
    ka.trk_end = t.trk_end;
    ka.sq = sq;
    ka.sq_tp = TP;
    RET(kweight_run<true>(c, j, ka));
    if (nb > 0) {
        KbArgs kb{};
        kb.sq = sq;
        kb.T = Tt;
        kb.TP = TP;
        kb.n_blocks = nb;
        kb.scale = (float)j->block_scale;  // Python float * np.float32: the constant rounded to f32 (NEP 50)
        kb.zl = zl;
        kb.stage_floats = ((KB_CHUNK - 1) / Tt + 2) * TP;  // the padded tile runs a chunk can span
        c->loud.kb_fill(kb);
        const size_t lds = (size_t)kb_lds_bytes(kb.stage_floats, kb.nvals, kb.pints);
        // persistent: as many workgroups as fit at once (a multiple of 8: the XCD-aware block mapping)
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, (160 * 1024) / (int64_t)(lds + 64)));  // (and VGPRs)
        const unsigned grid = (unsigned)std::min<int64_t>((nb + 7) / 8 * 8, (int64_t)c->n_cus * per_cu / 8 * 8);
        RET(launch(c, "kw_blocks", kw_blocks_kernel, dim3(std::max(grid, 8u)), dim3(KB_THREADS), lds, kb));
    }
    *zl_out = zl;
    return MM_OK;
}

// ------------------------------------------------------------------- gate
// block energies and levels from the segment energies in parallel (unless ga.zl
// already holds them: the exact path), then one workgroup per track
static int gate_launch(mm_ctx *c, GateArgs ga, unsigned n_tracks) {
    if (!ga.zl) {
        RET(get_buf(c, "gate_zl", (size_t)(2 * ga.n_blocks), &ga.zl));
        RET(launch(c, "gate_blocks", gate_blocks_kernel, dim3(blocks_for(ga.n_blocks, GATE_BLK_THREADS)),
                   dim3(GATE_BLK_THREADS), 0, ga));
    }
    return launch(c, "gate", gate_kernel, dim3(n_tracks), dim3(GATE_THREADS), 0, ga);
}

// Loudness and gain of every track of the staged line on the device (no host round
// trip) into out[2i] = L, out[2i+1] = gain: exactly pyloudnorm's block energies.
// The line's geometry must be on the device (unit_geometry) before this is queued.
static int line_loudness(mm_ctx *c, const mm_job *j, int64_t frames, const TrackTable &t, double *out) {
    GateArgs ga{};
    ga.n_blocks = t.n_blocks;
    ga.target = j->lufs_target;
    ga.out = out;
    ga.trk_blk = t.trk_blk;
    RET(kweight_exact(c, j, frames, t, &ga.zl));
    return gate_launch(c, ga, (unsigned)std::max(t.n_trk, 1));
}

// ------------------------------------------------------------ the operator
// The job of mm_op_loudness / loudness_device: samples of `dtype`, K-weighting
// tables built for LB_THREADS lanes of its own tile, segments of at least a tile.
static int loudness_check(mm_ctx *c, const mm_job *j, int dtype) {
    RET(check_dtype(c, dtype));
    const int64_t N = j->frames_proc;
    if (j->channels != 1 && j->channels != 2) return set_err(c, MM_ERR_ARG, "channels must be 1 or 2");
    if (N < 1 || N >= (int64_t)1 << 31) return set_err(c, MM_ERR_ARG, "frames %lld out of range", (long long)N);
    if (j->kweight.nsec != 2 || j->kweight.tpb != LB_THREADS) return set_err(c, MM_ERR_ARG, "K-weighting tables");
    if (j->n_segs < 1 || !j->seg_bounds || !j->block_lo || !j->block_hi || j->n_blocks < 1)
        return set_err(c, MM_ERR_ARG, "missing loudness geometry");
    const int T = j->kweight.tile;  // the K-weighting tables' (sub-)tile
    if (T < 1 || T > 512) return set_err(c, MM_ERR_ARG, "K-weighting tables built for %d-frame tiles", T);
    size_t lds;
    RET(transpose_lds(c, T, 1, &lds));  // the mono line's transpose
    for (int64_t s = 0; s + 1 < j->n_segs; ++s)
        if (std::min<int64_t>(j->seg_bounds[s + 1], N) - j->seg_bounds[s] < T)
            return set_err(c, MM_ERR_ARG, "loudness segment shorter than a tile");
    return MM_OK;
}

// The device part of mm_op_loudness (and the meter's output loudness): din = the
// job's [frames_proc][channels] samples of `dtype` in device memory (left unchanged);
// out (host) as mm_op_loudness.  Synchronous on return.
static int loudness_device(mm_ctx *c, const mm_job *j, int dtype, const void *din, double *out) {
    RET(loudness_check(c, j, dtype));
    const int ch = j->channels, T = j->kweight.tile;
    const int64_t N = j->frames_proc, G = (N + T - 1) / T;
    const size_t esz = dtype_size(dtype);
    const void *mono = din;
    if (ch == 2) {  // mean(axis=1) on the device, then the mono line
        char *dmono;
        RET(get_buf(c, "op_mono", (size_t)N * esz, &dmono));
        PwArgs pa{};
        pa.n = N;
        pa.in = din;
        pa.out = dmono;
        if (dtype == MM_F32) RET(launch(c, "op_mono", pointwise_kernel<PW_MONO, float>, dim3(pw_blocks(N)), dim3(256), 0, pa));
        else RET(launch(c, "op_mono", pointwise_kernel<PW_MONO, double>, dim3(pw_blocks(N)), dim3(256), 0, pa));
        mono = dmono;
    }
    double *tm;
    RET(get_buf(c, "op_tm", (size_t)G * T, &tm));
    const unsigned nb = blocks_for(G, OPS_TILES);
    size_t lds;
    RET(transpose_lds(c, T, 1, &lds));
    if (dtype == MM_F32)
        RET(launch(c, "to_tile_major", to_tile_major_kernel<float, 1>, dim3(nb), dim3(256), lds, (const float *)mono, tm,
                   N, G, T));
    else
        RET(launch(c, "to_tile_major", to_tile_major_kernel<double, 1>, dim3(nb), dim3(256), lds, (const double *)mono,
                   tm, N, G, T));
    RET(iir_in_place(c, &j->kweight, N, 1, G, tm, dtype == MM_F32));
    // segment energies -> gating on the device (gate.hip)
    double *seg, *gout;
    SegGeom g;
    RET(c->loud.upload_geometry(c, j, &g));
    KwArgs ka{};  // a mono f64 line tiled by the K-weighting tile itself, one lane per tile:
    ka.N_proc = N;  // tile_energy / seg_reduce read the tiling, the segments and the partials only
    ka.G = ka.Gt = G;
    ka.T = T;
    ka.sub = 1;
    ka.ch = 1;
    ka.n_segs = g.n_segs;
    ka.seg_bounds = g.bounds;
    RET(get_buf(c, "op_part", (size_t)G * 2, &ka.part));
    RET(get_buf(c, "op_part_seg", (size_t)G, &ka.part_seg));
    RET(get_buf(c, "op_seg", (size_t)g.n_segs, &seg));
    RET(get_buf(c, "op_gate", 2, &gout));
    RET(launch(c, "op_tile_energy", tile_energy_kernel, dim3(blocks_for(G, 256)), dim3(256), 0, ka, (const double *)tm));
    RET(launch(c, "op_seg_reduce", seg_reduce_kernel, dim3(blocks_for(g.n_segs, 4)), dim3(256), 0, ka, seg));
    GateArgs ga{};
    ga.n_blocks = g.n_blocks;
    ga.blk_s0 = g.s0;
    ga.blk_s1 = g.s1;
    ga.seg = seg;
    ga.scale = j->block_scale;
    ga.target = j->lufs_target;
    ga.out = gout;
    RET(gate_launch(c, ga, 1));
    HIPCHK(c, hipMemcpyAsync(out, gout, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    return MM_OK;
}

// =================================================================== C-ABI
extern "C" {

// pyloudnorm Meter(rate).integrated_loudness of samples.mean(axis=1) (AME:213-218):
// mono in the input's dtype, K-weighting (f32 write-backs for an f32 input), segment
// energies, gating; out[0] = L, out[1] = 10 ** ((job->lufs_target - L) / 20).
int mm_op_loudness(mm_ctx *c, const mm_job *j, int dtype, const void *in, double *out) {
    if (!c || !j || !out || (j->frames_proc > 0 && !in)) return set_err(c, MM_ERR_ARG, "bad arguments");
    RET(loudness_check(c, j, dtype));  // (before the upload is sized; loudness_device checks whatever it is given)
    HIPCHK(c, hipSetDevice(c->device));
    const size_t in_bytes = (size_t)j->frames_proc * j->channels * dtype_size(dtype);
    char *din;
    RET(get_buf(c, "op_in", in_bytes, &din));
    HIPCHK(c, hipMemcpyAsync(din, in, in_bytes, hipMemcpyHostToDevice, c->stream));
    return loudness_device(c, j, dtype, din, out);
}

// numpy's float32 np.sum over x[0..n) evaluated on the host through the same
// program the device runs for pyloudnorm's block energies (CPU check of pw_build).
int mm_np_sum_f32(const float *x, int64_t n, float *out) {
    if (!out || n < 0 || (n > 0 && !x) || n > 16 * KB_CHUNK) return MM_ERR_ARG;
    std::vector<int32_t> prog;
    pw_build(n, prog);
    *out = pw_eval(prog.data(), x);
    return MM_OK;
}

// pyloudnorm 0.1.1 integrated_loudness gating (mono, G=1), restated.
int mm_gate_loudness(const mm_job *j, const double *seg_energy, double *loudness) {
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
        RET(kweight_segments(c, carry_in_host, nullptr, &seg));
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

}  // extern "C"
