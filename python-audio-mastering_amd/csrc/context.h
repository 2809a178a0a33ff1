// context.h — the library's context (mm_ctx: stream, device buffers, the chain's
// control block (control.h), the loudness tail's state (loudness.h) and cached
// tables) and the helpers every host file uses: errors, device buffers, the timed
// launch.  Included by mastering.hip after the kernels, control.h and loudness.h.
#pragma once

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct PendingEvent {
    std::string name;
    hipEvent_t a, b;
};

struct KStat {
    double ms = 0.0;
    int64_t n = 0;
};

// The envelope solve kept across the queued launches (stage_compress -> comp_sweeps /
// comp_back), and what the context learnt from its last one.
struct Solve {
    bool on = false;
    CompArgs ca{};
    uint32_t stamp = 0;  // stamp of the last queued fix-up sweep
    int iters = 0, pending = 0;
    int queue = 0;     // sweeps to queue with the next solve (0: COMP_SWEEPS; then the last solve's need + 1)
    uint64_t sig = 0;  // settings and geometry of the solve `queue` was learnt on (comp_signature)
};

}  // namespace

struct mm_ctx {
    int device = 0;
    int n_cus = 256;  // compute units of the device (persistent launches)
    hipStream_t stream = nullptr;
    char err[512] = {0};
    std::map<std::string, DevBuf> bufs;
    // staged job geometry (mm_stage_chunks -> mm_hop_energies / mm_finalize; the job's
    // loudness arrays are then loud's copies)
    bool staged = false;
    mm_job job{};
    int64_t G = 0;
    short2 *mix = nullptr;
    ChainCtl ctl;  // the chain's control block and its readback (control.h)
    Solve comp;    // the envelope solve queued on it
    Loudness loud;  // what the loudness tail keeps: block programs, segment geometry, the staged job's (loudness.h)
    // timing
    bool timing = false;
    std::vector<PendingEvent> pending;
    std::vector<hipEvent_t> free_events;
    // pinned double-buffered staging for the WAV file path (mm_master_wav)
    char *pin[2] = {nullptr, nullptr};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    std::map<std::string, KStat> stats;
    std::vector<std::string> stat_order;
    // host tables already resident on the device
    uint64_t lut_key[3] = {0, 0, 0};  // content keys of the band tables on the device (0: none)
    uint64_t lut_ok_key[3] = {0, 0, 0};  // keys of the band tables last checked against their r0 (validate; 0: none)
    int64_t lut_ok_r0[3] = {0, 0, 0};
    uint64_t sat_key = 0;             // content key of the exciter table on the device (0: none)
    bool sat_codes = false;           // its correction codes are complete (no entry needs the table)
    std::map<std::string, std::vector<double>> mats_cache;
    // batch execution (mm_master_batch): child contexts, one stream each
    std::vector<mm_ctx *> children;
    // mastering report of the last master call (mm_last_meters; empty: it did not meter)
    std::vector<mm_meter> meters;
    // R 128 reports of the last master call (mm_last_r128; empty: no job asked for one)
    std::vector<mm_r128> r128s;
    // QC reports of the last master call or mm_batch_qc_* call (mm_last_qc; empty: none was made)
    std::vector<mm_qc> qcs;
    // spectrum reports of the last master call or mm_batch_spectrum_* call and their bin tables
    // (mm_last_spectrum, mm_last_spectrum_bins; empty: none was made; a table is empty for a track
    // that did not ask), and whether the kernels' tables are on the device ("spec_tab")
    std::vector<mm_spectrum> spectra;
    std::vector<std::vector<double>> spectrum_bins;
    bool spec_tab_ok = false;
    // ceilings of the last master call (mm_last_ceilings; empty: no job set one)
    std::vector<mm_ceiling> ceilings;
    // levels of the last master call (mm_last_levels; empty: its delivery set no loudness target)
    std::vector<mm_level> levels;
    // the album level of the last call (mm_last_album; empty: it levelled no album): the level and
    // the album's R 128 report; the per-track reports are r128s and ceilings above
    std::vector<mm_level> albums;
    std::vector<mm_r128> album_r128s;
    // the converter's taps on the device ("rs_taps": content key and geometry; key 0: none)
    // and the statistics of the last delivery (mm_last_resample)
    uint64_t rs_key = 0;
    int rs_L = 0, rs_M = 0, rs_K = 0;
    mm_resample resample{};
    bool resample_valid = false;
    // the FIR's taps on the device ("fir_taps": content key and length; key 0: none) and the
    // statistics of the context's last filter pass (mm_last_fir)
    uint64_t fir_key = 0;
    int fir_K = 0;
    mm_fir_result fir{};
    bool fir_valid = false;
    // rccl
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
};

static int set_err(mm_ctx *c, int code, const char *fmt, ...) {
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof(c->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(ctx, expr)                                                                    \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return set_err(ctx, MM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                              \
    } while (0)

template <typename T>
static int get_buf(mm_ctx *c, const char *name, size_t count, T **out) {
    DevBuf &b = c->bufs[name];
    size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    if (b.cap < bytes) {
        if (b.p) HIPCHK(c, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
        HIPCHK(c, hipMalloc(&b.p, bytes));
        b.cap = bytes;
    }
    *out = reinterpret_cast<T *>(b.p);
    return MM_OK;
}

static hipEvent_t take_event(mm_ctx *c) {
    if (!c->free_events.empty()) {
        hipEvent_t e = c->free_events.back();
        c->free_events.pop_back();
        return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// Launch helper: records HIP events around the kernel on the context stream
// when timing is enabled.
template <typename Kern, typename... Args>
static int launch(mm_ctx *c, const char *name, Kern k, dim3 grid, dim3 block, size_t lds, Args... args) {
    hipEvent_t a = nullptr, b = nullptr;
    if (c->timing) {
        a = take_event(c);
        b = take_event(c);
        if (a) hipEventRecord(a, c->stream);
    }
    hipLaunchKernelGGL(k, grid, block, lds, c->stream, args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(c, MM_ERR_HIP, "launch %s: %s", name, hipGetErrorString(e));
    if (c->timing && a && b) {
        hipEventRecord(b, c->stream);
        c->pending.push_back({name, a, b});
    }
    return MM_OK;
}

static void resolve_events(mm_ctx *c) {
    for (auto &p : c->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            auto it = c->stats.find(p.name);
            if (it == c->stats.end()) {
                c->stat_order.push_back(p.name);
                it = c->stats.emplace(p.name, KStat{}).first;
            }
            it->second.ms += ms;
            it->second.n += 1;
        }
        c->free_events.push_back(p.a);
        c->free_events.push_back(p.b);
    }
    c->pending.clear();
}

#define RET(expr)                  \
    do {                           \
        int r_ = (expr);           \
        if (r_ != MM_OK) return r_; \
    } while (0)

static inline unsigned blocks_for(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }
