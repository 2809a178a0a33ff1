// r128.hip — the EBU R 128 report of a delivered signal (mm_r128 in include/mastering.h):
// integrated loudness (ITU-R BS.1770-4), maximum momentary and short-term loudness and
// the loudness range (EBU Tech 3342).  No reference counterpart: the reference measures
// the channel mean through pyloudnorm (mm_meter.loudness, which the chain normalises to);
// this is what a BS.1770 meter reads, every channel K-weighted and the energies summed.
//
// The definition has one tail, mm_r128_from_hops (steps 3-7 on the 0.1 s hop energies),
// which the host restatement (mm_r128_host: the sequential filter) and the GPU path both
// end in: they differ in e[] only.  Its steps 4-7 are r128_figures, which an album's pooled
// windows end in too (album.hip).
//
// The GPU pass (AlbumPass: a single track is the pass over one track, an album or a batch the
// pass over n) is ONE launch of the K-weighting with lookback.h's carry over the workgroups of
// all its tracks, a lane per tile of R128_TILE frames, followed by a fixed-order reduction of
// the tile partials to the hops (no floating-point atomics: two runs are bit-identical), and one
// read-back of the hop energies and the look-back's error word whatever n.  A lane runs every channel of
// its tile: mono is a 4-dimensional state (lb_carry<4, 1>), stereo ONE 8-dimensional state
// of two independent 2-section cascades, L | R (lb_carry<8, 1, 2>, the block structure of
// the crossover's LP | HP).  The pass owns its geometry: the transition tables are built
// here from the caller's sections and R128_TILE and cached in the context by (sections,
// channels), so the caller gives the rate and the coefficients only.
//
// Loads: the input is interleaved in frame order, so a lane walking its own tile would
// read a cache line of its own.  Both passes therefore stage R128_CHUNK frames of every
// tile of the workgroup through LDS: consecutive threads load consecutive frames of a tile
// (whole 128-byte lines of int16 stereo) through load_frame, which decodes either kind to
// the int16 grid, and store them frame-major with a row stride of LB_THREADS + 1 dwords,
// so the stores are at most two to a bank and a lane's reads of its own frames none.
//
// Included at the end of mastering.hip (one translation unit) after meter.hip.

namespace mm {

constexpr int R128_TILE = 128;                        // frames per lane: <= 200, the shortest hop (rate 2000)
constexpr int R128_CHUNK = 32;                        // frames of a tile staged at a time
constexpr int R128_SPAN = LB_THREADS * R128_TILE;     // frames per workgroup (mm_r128_span)
constexpr int R128_ROW = LB_THREADS + 1;              // dwords per staged frame row
constexpr int R128_MIN_RATE = 2000;                   // the library's floor: hops of >= 200 frames
constexpr int64_t R128_MAX_FRAMES = (int64_t)1 << 31;
static_assert(R128_TILE <= R128_MIN_RATE / 10 && R128_TILE % R128_CHUNK == 0, "a tile touches at most two hops");
static_assert((1 << (LB_TILE_POW - 1)) * 2 == LB_THREADS, "Phi_B = (Phi_T^128)^2");

// One DF2T section in scipy.signal.lfilter's operation order, every product and sum
// rounded (the unit is built with -ffp-contract=off): the definition's filter, on the host
// and in pass 2.
__host__ __device__ __forceinline__ double r128_section(double x, double &z0, double &z1, const double *c) {
    const double y = z0 + c[0] * x;
    z0 = (z1 + x * c[1]) - y * c[3];
    z1 = x * c[2] - y * c[4];
    return y;
}

// B[i] = floor(i * R / 10) and the hop of frame f: the largest i with B[i] <= f
__host__ __device__ __forceinline__ int64_t r128_bound(int64_t i, int rate) { return i * rate / 10; }
__host__ __device__ __forceinline__ int64_t r128_hop_of(int64_t f, int rate) { return (10 * f + 9) / rate; }

struct R128Args {
    int64_t N, G;       // frames, tiles
    int rate;
    double sos[2][5];
    double *part;       // [G][2] energies of the tile's frames in its first hop and in the next
    int64_t *part_hop;  // [G]    the tile's first hop
};

// R128_CHUNK frames of every tile of the workgroup from chunk k on, decoded to the int16
// grid: a stereo frame as its packed dword, a mono one sign-extended; zeros past the end.
template <int CH, typename T>
__device__ __forceinline__ void r128_stage(uint32_t *stage, const T *__restrict__ in, int64_t N, int64_t g0, int k) {
    for (int e = threadIdx.x; e < LB_THREADS * R128_CHUNK; e += LB_THREADS) {
        const int s = e / R128_CHUNK, i = e % R128_CHUNK;
        const int64_t f = (g0 + s) * R128_TILE + k * R128_CHUNK + i;
        int v[CH] = {};
        if (f < N) load_frame<CH, T>(in, f, v);
        stage[i * R128_ROW + s] = CH == 2 ? pack_frame(v[0], v[1]) : (uint32_t)v[0];
    }
    __syncthreads();
}

// One pass over the lane's tile of `len` frames from state z (sections 2c, 2c + 1:
// channel c).  P2: the definition's filter, and the squares into e0 (frames before
// `bnd`) and e1; else the fused form, which only feeds the tile's carry map.
template <int CH, typename T, bool P2>
__device__ __forceinline__ void r128_pass(const R128Args &a, const T *__restrict__ in, uint32_t *stage, int64_t g0,
                                          int len, double (&z)[2 * CH][2], int64_t bnd, double &e0, double &e1) {
    int64_t pf = (g0 + threadIdx.x) * R128_TILE;
    for (int k = 0; k < R128_TILE / R128_CHUNK; ++k) {
        r128_stage<CH, T>(stage, in, a.N, g0, k);
        const int n = min(R128_CHUNK, max(0, len - k * R128_CHUNK));
        for (int i = 0; i < n; ++i) {
            const uint32_t d = stage[i * R128_ROW + threadIdx.x];
            double sq = 0.0;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int s = CH == 2 ? (int)(int16_t)(c ? d >> 16 : d & 0xFFFFu) : (int)d;
                const double x = (double)s * (1.0 / 32768.0);  // exact
                if constexpr (P2) {
                    double y = r128_section(x, z[2 * c][0], z[2 * c][1], a.sos[0]);
                    y = r128_section(y, z[2 * c + 1][0], z[2 * c + 1][1], a.sos[1]);
                    sq += y * y;  // (L, then R: the order of mm_r128_host)
                } else {
                    const double y = df2t(x, z[2 * c][0], z[2 * c][1], a.sos[0]);
                    df2t(y, z[2 * c + 1][0], z[2 * c + 1][1], a.sos[1]);
                }
            }
            if constexpr (P2) {
                if (pf < bnd) e0 += sq;
                else e1 += sq;
            }
            ++pf;
        }
        __syncthreads();  // the rows are free for the next chunk
    }
}

// One workgroup of the K-weighting pass on one line (a track): `blk` its logical block of the
// launch (the look-back's index), g0 its first tile counted from the line's start, a.part /
// a.part_hop the line's own partials.  The line's first tile resets the carry, so a block
// waits on predecessors back to the line's first block only, which publishes an inclusive
// prefix at once: what a workgroup computes depends on its line alone, wherever the line
// lies in the launch (the pass below puts many lines into one).
template <int CH, typename T>
__device__ __forceinline__ void r128_kweight_block(const R128Args &a, const T *__restrict__ in, const LbArgs &lb, int blk,
                                                   int64_t g0, double *smem, uint32_t *stage) {
    const int t = threadIdx.x;
    const int64_t g = g0 + t;
    const bool valid = g < a.G;
    const int len = valid ? (int)min((int64_t)R128_TILE, a.N - g * R128_TILE) : 0;
    double zs[2 * CH][2];
#pragma unroll
    for (int k = 0; k < 2 * CH; ++k) zs[k][0] = zs[k][1] = 0.0;
    double e0 = 0.0, e1 = 0.0;
    r128_pass<CH, T, false>(a, in, stage, g0, len, zs, 0, e0, e1);
    lb_carry_sections<2 * CH, 1, 2>(lb, blk, t, 0, valid, valid && g == 0, zs, smem);
    // the tile's first hop and where the next one begins
    const int64_t h0 = r128_hop_of(g * R128_TILE, a.rate);
    r128_pass<CH, T, true>(a, in, stage, g0, len, zs, r128_bound(h0 + 1, a.rate), e0, e1);
    if (!valid) return;
    a.part[2 * g] = e0;
    a.part[2 * g + 1] = e1;
    a.part_hop[g] = h0;
}

// Hop s of a line from its tile partials: lane k takes tiles g0 + k, g0 + k + 64, ..., then
// a butterfly; the order is fixed by the line's geometry alone.
__device__ __forceinline__ double r128_hop_sum(const double *part, const int64_t *part_hop, int64_t s, int rate, int lane) {
    const int64_t g0 = r128_bound(s, rate) / R128_TILE, g1 = (r128_bound(s + 1, rate) - 1) / R128_TILE;
    double acc = 0.0;
    for (int64_t g = g0 + lane; g <= g1; g += 64) {  // (g1 < G: B[s + 1] <= N)
        const int64_t ph = part_hop[g];
        acc += ph == s ? part[2 * g] : (ph == s - 1 ? part[2 * g + 1] : 0.0);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// ---- the pass: every track of a call in ONE launch of either kernel.  The tracks stay where
// they are.  Track t owns ceil(G_t / LB_THREADS) consecutive workgroups from wg0 and the
// partials of wg0 * LB_THREADS tiles on; its hops are e[hop0 .. hop0 + H_t).  Inside its track
// a workgroup is r128_kweight_block on the track's own tiles, staging and chain of
// predecessors back to the block that resets, so a track's hop energies are those of a pass
// over it alone.
struct R128Track {
    const void *pcm;
    int64_t N;     // frames
    int64_t wg0;   // first workgroup
    int64_t hop0;  // first hop
};

struct R128AlbumArgs {
    const R128Track *tracks;  // [n]
    const int *wg_track;      // [workgroups] the track a workgroup belongs to
    int n, rate;
    int64_t H;                // hops of the album
    double sos[2][5];
    double *part;             // [workgroups * LB_THREADS][2]
    int64_t *part_hop;        // [workgroups * LB_THREADS]
};

template <int CH, typename T>
__global__ void __launch_bounds__(LB_THREADS) r128_album_kweight_kernel(R128AlbumArgs al, LbArgs lb) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    uint32_t *stage = reinterpret_cast<uint32_t *>(smem + lb_lds_bytes<8, 1>() / sizeof(double));
    __shared__ int ticket_slot;
    const int blk = __builtin_amdgcn_readfirstlane(lb_ticket(lb, &ticket_slot));  // (uniform: the table reads are scalar)
    const R128Track tr = al.tracks[al.wg_track[blk]];
    R128Args a;
    a.N = tr.N;
    a.G = (tr.N + R128_TILE - 1) / R128_TILE;
    a.rate = al.rate;
#pragma unroll
    for (int k = 0; k < 10; ++k) a.sos[k / 5][k % 5] = al.sos[k / 5][k % 5];
    a.part = al.part + 2 * tr.wg0 * LB_THREADS;
    a.part_hop = al.part_hop + tr.wg0 * LB_THREADS;
    r128_kweight_block<CH, T>(a, static_cast<const T *>(tr.pcm), lb, blk, ((int64_t)blk - tr.wg0) * LB_THREADS, smem, stage);
}

// e[s] for s < H: a wave finds the track of its hop in the prefix hop0 (the last track that
// starts at or before s: a track without hops is never found); one wave a hop, so frames at or
// after a track's B[H_t] belong to no hop.
__global__ void __launch_bounds__(256) r128_album_reduce_kernel(R128AlbumArgs al, double *e) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= al.H) return;  // wave-uniform
    int lo = 0, hi = al.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (al.tracks[mid].hop0 <= s) lo = mid;
        else hi = mid - 1;
    }
    const R128Track tr = al.tracks[lo];
    const double acc = r128_hop_sum(al.part + 2 * tr.wg0 * LB_THREADS, al.part_hop + tr.wg0 * LB_THREADS, s - tr.hop0, al.rate, lane);
    if (lane == 0) e[s] = acc;
}

}  // namespace mm

// ======================================================= host side
namespace {

void r128_clear(mm_r128 *o, int64_t frames, int channels, int rate) {
    memset(o, 0, sizeof *o);
    o->frames = frames;
    o->channels = channels;
    o->rate = rate;
    o->integrated = o->relative_gate = o->momentary_max = o->short_term_max = NAN;
    o->lra = o->lra_low = o->lra_high = NAN;
}

// why a signal is refused, or null (the words of mm_last_error)
const char *r128_refusal(int channels, int64_t frames, int rate) {
    if (rate < R128_MIN_RATE) return "rate below 2000 Hz";
    return pcm_refusal(channels, frames, R128_MAX_FRAMES);
}

double r128_level(double z) { return -0.691 + 10.0 * std::log10(z); }

// z_w[j] and l_w[j] of every window of w hops (step 3)
void r128_windows(const double *e, int64_t H, int rate, int w, std::vector<double> &z, std::vector<double> &l) {
    const int64_t n = H >= w ? H - w + 1 : 0;
    z.resize((size_t)n);
    l.resize((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        double acc = e[j];
        for (int k = 1; k < w; ++k) acc += e[j + k];
        z[(size_t)j] = acc / (double)(r128_bound(j + w, rate) - r128_bound(j, rate));
        l[(size_t)j] = r128_level(z[(size_t)j]);
    }
}

// -70 LUFS absolute gate, then the relative gate `below` LU under the mean of what passed:
// the gate's level (NaN when nothing passed the absolute gate) and the passing indices
double r128_gate(const std::vector<double> &z, const std::vector<double> &l, double below, std::vector<int64_t> &keep) {
    double sum = 0.0;
    int64_t cnt = 0;
    keep.clear();
    for (size_t j = 0; j < l.size(); ++j)
        if (l[j] > -70.0) {
            sum += z[j];
            ++cnt;
        }
    if (!cnt) return NAN;
    const double gamma = r128_level(sum / (double)cnt) - below;
    for (size_t j = 0; j < l.size(); ++j)
        if (l[j] > -70.0 && l[j] > gamma) keep.push_back((int64_t)j);
    return gamma;
}

// Steps 4-7 on the momentary (w = 4) and short-term (w = 30) windows of one programme, or on
// an album's pools of them (album.hip): the one tail of every figure.  No window of a kind:
// its figures stay NaN.
void r128_figures(const std::vector<double> &z4, const std::vector<double> &l4, const std::vector<double> &z30,
                  const std::vector<double> &l30, mm_r128 *out) {
    std::vector<int64_t> keep;
    if (!l4.empty()) {  // momentary windows: the maximum and the integrated loudness
        out->momentary_blocks = (int64_t)l4.size();
        out->momentary_max = *std::max_element(l4.begin(), l4.end());
        out->relative_gate = r128_gate(z4, l4, 10.0, keep);
        double sum = 0.0;
        for (int64_t j : keep) sum += z4[(size_t)j];
        out->integrated = keep.empty() ? -INFINITY : r128_level(sum / (double)keep.size());
    }
    if (!l30.empty()) {  // short-term windows: the maximum and the loudness range
        out->short_term_blocks = (int64_t)l30.size();
        out->short_term_max = *std::max_element(l30.begin(), l30.end());
        r128_gate(z30, l30, 20.0, keep);
        std::vector<double> k;
        for (int64_t j : keep) k.push_back(l30[(size_t)j]);
        std::sort(k.begin(), k.end());
        const int64_t n = (int64_t)k.size();
        out->lra_blocks = n;
        out->lra = 0.0;
        if (n > 0) {
            out->lra_low = k[(size_t)(((n - 1) * 10 + 50) / 100)];
            out->lra_high = k[(size_t)(((n - 1) * 95 + 50) / 100)];
            out->lra = out->lra_high - out->lra_low;
        }
    }
}

// The transition tables of the pass for these sections (row-major 8 x 8; mono uses the
// leading 4 x 4, stereo the two diagonal blocks): Phi_T^(2^k), k < 8, then Phi_B^e,
// e = 0..64, with Phi_T = A^R128_TILE and Phi_B = Phi_T^LB_THREADS, in long double,
// each table rounded once.
void r128_tables(const double sos[2][5], int channels, std::vector<double> &out) {
    typedef long double M8[64];
    auto mul = [](const long double *a, const long double *b, long double *o) {
        long double t[64];
        for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c) {
                long double acc = 0.0L;
                for (int k = 0; k < 8; ++k) acc += a[r * 8 + k] * b[k * 8 + c];
                t[r * 8 + c] = acc;
            }
        memcpy(o, t, sizeof t);
    };
    M8 A = {0};
    for (int ch = 0; ch < channels; ++ch)
        for (int col = 0; col < 4; ++col) {  // one zero-input frame of the cascade from a unit state
            long double z[4] = {0, 0, 0, 0}, o[4];
            z[col] = 1.0L;
            long double u = 0.0L;
            for (int s = 0; s < 2; ++s) {
                const double *c = sos[s];
                const long double y = (long double)c[0] * u + z[2 * s];
                o[2 * s] = (long double)c[1] * u - (long double)c[3] * y + z[2 * s + 1];
                o[2 * s + 1] = (long double)c[2] * u - (long double)c[4] * y;
                u = y;
            }
            for (int r = 0; r < 4; ++r) A[(4 * ch + r) * 8 + 4 * ch + col] = o[r];
        }
    M8 P;
    memcpy(P, A, sizeof P);
    for (int t = 1; t < R128_TILE; ++t) mul(P, A, P);  // Phi_T
    out.assign((size_t)(MM_TILE_POW + MM_BLK_POW) * 64, 0.0);
    for (int k = 0; k < MM_TILE_POW; ++k) {
        for (int i = 0; i < 64; ++i) out[(size_t)k * 64 + i] = (double)P[i];
        mul(P, P, P);  // after the last table: Phi_T^256 = Phi_B
    }
    M8 E = {0};
    for (int d = 0; d < 8; ++d) E[d * 8 + d] = 1.0L;
    for (int e = 0; e < MM_BLK_POW; ++e) {
        for (int i = 0; i < 64; ++i) out[(size_t)(MM_TILE_POW + e) * 64 + i] = (double)E[i];
        mul(E, P, E);
    }
}

// the tables on the device, rebuilt only when the sections or the channel count change
int r128_upload_tables(mm_ctx *c, const double sos[2][5], int channels, LbArgs &lb) {
    std::vector<double> key(sos[0], sos[0] + 10);
    key.push_back((double)channels);
    const size_t n = (size_t)(MM_TILE_POW + MM_BLK_POW) * 64;
    double *d;
    RET(get_buf(c, "r128_tab", n, &d));
    std::vector<double> &cached = c->mats_cache["r128_tab"];
    if (cached != key) {
        std::vector<double> host;
        r128_tables(sos, channels, host);
        HIPCHK(c, hipMemcpyAsync(d, host.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // host vector is transient
        cached = key;
    }
    lb.pw_tile = d;
    lb.pw_blk = d + MM_TILE_POW * 64;
    return MM_OK;
}

// The measuring pass over n >= 1 tracks, laid out once: every track on a workgroup boundary,
// its hops at hop0[t] of the pass's.  The host table lives as long as the pass, so its upload
// needs no synchronisation of its own: album_pass_hops, which every prepared pass with a hop
// runs, ends in one.
struct AlbumPass {
    R128AlbumArgs a{};
    unsigned nblk = 0;
    int kind = 0, channels = 0;
    std::vector<int64_t> hops;  // [n] H_t
    std::vector<char> tab;      // the tracks, the track of every workgroup, the zero error word: one upload
    unsigned *d_error = nullptr;  // the look-back's error word
    bool zeroed = false;          // by the table's upload: the first measurement needs no memset
    double *d_e = nullptr;
};

// Lays the pass out and queues the upload of its table.  Arguments already checked.
int album_pass_prepare(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                       const double sos[2][5], AlbumPass &p) {
    int64_t wg = 0, hop = 0;
    p.hops.resize((size_t)n);
    std::vector<R128Track> tracks((size_t)n);
    std::vector<int> wg_track;
    for (int t = 0; t < n; ++t) {
        const int64_t G = (frames[t] + R128_TILE - 1) / R128_TILE, nwg = (G + LB_THREADS - 1) / LB_THREADS;
        tracks[(size_t)t] = R128Track{d_pcm[t], frames[t], wg, hop};
        wg_track.insert(wg_track.end(), (size_t)nwg, t);
        p.hops[(size_t)t] = 10 * frames[t] / rate;
        wg += nwg;
        hop += p.hops[(size_t)t];
    }
    p.nblk = (unsigned)wg;
    p.kind = kind;
    p.channels = channels;
    p.a.n = n;
    p.a.rate = rate;
    p.a.H = hop;
    memcpy(p.a.sos, sos, sizeof p.a.sos);
    if (hop == 0) return MM_OK;  // nothing to measure: nothing is queued
    const size_t tb = (size_t)n * sizeof(R128Track), o_err = tb + (size_t)wg * sizeof(int);
    p.tab.assign(o_err + sizeof(unsigned), 0);
    memcpy(p.tab.data(), tracks.data(), tb);
    memcpy(p.tab.data() + tb, wg_track.data(), (size_t)wg * sizeof(int));
    char *d_tab;
    RET(get_buf(c, "album_tab", p.tab.size(), &d_tab));
    RET(get_buf(c, "album_part", (size_t)wg * LB_THREADS * 2, &p.a.part));
    RET(get_buf(c, "album_part_hop", (size_t)wg * LB_THREADS, &p.a.part_hop));
    RET(get_buf(c, "album_hops", (size_t)hop, &p.d_e));
    HIPCHK(c, hipMemcpyAsync(d_tab, p.tab.data(), p.tab.size(), hipMemcpyHostToDevice, c->stream));
    p.a.tracks = reinterpret_cast<const R128Track *>(d_tab);
    p.a.wg_track = reinterpret_cast<const int *>(d_tab + tb);
    p.d_error = reinterpret_cast<unsigned *>(d_tab + o_err);
    p.zeroed = true;
    return MM_OK;
}

// One measurement: the hop energies of the pass's tracks into `e`, track after track
// (H_t = floor(10 N_t / R) of track t; none at all: nothing is launched).  Two launches, one
// read-back.  Synchronous on return.
int album_pass_hops(mm_ctx *c, AlbumPass &p, std::vector<double> &e) {
    e.assign((size_t)p.a.H, 0.0);
    if (p.a.H == 0) return MM_OK;
    LbArgs lb{};
    RET(r128_upload_tables(c, p.a.sos, p.channels, lb));
    RET(lb_prepare(c, p.nblk, 1, lb));
    lb.error = p.d_error;
    if (!p.zeroed) HIPCHK(c, hipMemsetAsync(lb.error, 0, 4, c->stream));
    p.zeroed = false;
    const size_t lds = (size_t)lb_lds_bytes<8, 1>() + (size_t)R128_CHUNK * R128_ROW * sizeof(uint32_t);
    RET(dispatch_pcm(p.kind, p.channels, [&](auto ch, auto t) {
        using T = decltype(t);
        return launch(c, "r128_album_kweight", r128_album_kweight_kernel<ch, T>, dim3(p.nblk), dim3(LB_THREADS), lds, p.a, lb);
    }));
    RET(launch(c, "r128_album_reduce", r128_album_reduce_kernel, dim3(blocks_for(p.a.H, 4)), dim3(256), 0, p.a, p.d_e));
    unsigned err = 0;
    HIPCHK(c, hipMemcpyAsync(e.data(), p.d_e, (size_t)p.a.H * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&err, lb.error, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    if (err) return set_err(c, MM_ERR_STATE, "IIR look-back timed out");
    return MM_OK;
}

}  // namespace

// The R 128 report of a device-resident signal (synchronous on return).
static int r128_device(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, int rate,
                       const double sos[2][5], mm_r128 *out) {
    if (!c || !out || !sos || (frames > 0 && !d_pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = r128_refusal(channels, frames, rate)) return set_err(c, MM_ERR_ARG, "R 128: %s", why);
    AlbumPass pass;  // (of one track: the context's other results stay as they are)
    std::vector<double> e;
    RET(album_pass_prepare(c, &d_pcm, kind, &frames, 1, channels, rate, sos, pass));
    RET(album_pass_hops(c, pass, e));
    mm_r128_from_hops(e.data(), (int64_t)e.size(), rate, out);
    out->frames = frames;
    out->channels = channels;
    return MM_OK;
}

extern "C" {

int mm_r128_span(void) { return R128_SPAN; }

int mm_r128_from_hops(const double *e, int64_t hops, int32_t rate, mm_r128 *out) {
    if (!out || hops < 0 || (hops > 0 && !e) || rate < R128_MIN_RATE) return MM_ERR_ARG;
    r128_clear(out, 0, 0, rate);
    out->hops = hops;
    std::vector<double> z4, l4, z30, l30;
    r128_windows(e, hops, rate, 4, z4, l4);
    r128_windows(e, hops, rate, 30, z30, l30);
    r128_figures(z4, l4, z30, l30, out);
    return MM_OK;
}

int mm_r128_host(const int16_t *pcm, int64_t frames, int channels, int32_t rate, const double sos[2][5],
                 double *hops_out, int64_t hops_cap, mm_r128 *out) {
    if (!out || !sos || (frames > 0 && !pcm) || hops_cap < 0 || (hops_cap > 0 && !hops_out) ||
        r128_refusal(channels, frames, rate))
        return MM_ERR_ARG;
    const int64_t H = 10 * frames / rate;
    std::vector<double> e((size_t)H, 0.0);
    double z[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    int64_t n = 0;
    for (int64_t i = 0; i < H; ++i) {  // (frames after B[H] belong to no hop and follow every one that does)
        double acc = 0.0;
        for (const int64_t end = r128_bound(i + 1, rate); n < end; ++n)
            for (int c = 0; c < channels; ++c) {
                const double x = (double)pcm[n * channels + c] / 32768.0;
                double y = r128_section(x, z[2 * c][0], z[2 * c][1], sos[0]);
                y = r128_section(y, z[2 * c + 1][0], z[2 * c + 1][1], sos[1]);
                acc += y * y;
            }
        e[(size_t)i] = acc;
    }
    for (int64_t i = 0; i < std::min(H, hops_cap); ++i) hops_out[i] = e[(size_t)i];
    mm_r128_from_hops(e.data(), H, rate, out);
    out->frames = frames;
    out->channels = channels;
    return MM_OK;
}

int mm_r128_device(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, int32_t rate,
                   const double sos[2][5], mm_r128 *out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return r128_device(c, d_pcm, kind, frames, channels, rate, sos, out);
}

int mm_r128_pcm(mm_ctx *c, const void *pcm, int kind, int64_t frames, int channels, int32_t rate,
                const double sos[2][5], mm_r128 *out) {
    if (!c) return MM_ERR_ARG;
    if (!out || !sos || (frames > 0 && !pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = r128_refusal(channels, frames, rate)) return set_err(c, MM_ERR_ARG, "R 128: %s", why);
    HIPCHK(c, hipSetDevice(c->device));
    char *din;
    RET(pcm_upload(c, "r128_in", pcm, pcm_bytes(kind, frames, channels), &din));
    return r128_device(c, din, kind, frames, channels, rate, sos, out);
}

int mm_op_r128_hops(mm_ctx *c, const void *pcm, int kind, int64_t frames, int channels, int32_t rate,
                    const double sos[2][5], double *hops_host, int64_t cap) {
    if (!c) return MM_ERR_ARG;
    if (!sos || (frames > 0 && !pcm) || cap < 0 || (cap > 0 && !hops_host)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = r128_refusal(channels, frames, rate)) return set_err(c, MM_ERR_ARG, "R 128: %s", why);
    HIPCHK(c, hipSetDevice(c->device));
    char *din;
    RET(pcm_upload(c, "r128_in", pcm, pcm_bytes(kind, frames, channels), &din));
    const void *d_pcm = din;
    AlbumPass pass;
    std::vector<double> e;
    RET(album_pass_prepare(c, &d_pcm, kind, &frames, 1, channels, rate, sos, pass));
    RET(album_pass_hops(c, pass, e));
    for (size_t i = 0; i < std::min(e.size(), (size_t)cap); ++i) hops_host[i] = e[i];
    return (int)std::min<size_t>(e.size(), (size_t)INT32_MAX);
}

int mm_last_r128(mm_ctx *c, int cap, mm_r128 *out) {
    if (!c || cap < 0 || (cap > 0 && !out)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->r128s.empty()) return set_err(c, MM_ERR_STATE, "the last master call made no R 128 report");
    const int n = (int)c->r128s.size();
    for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->r128s[(size_t)i];
    return n;
}

}  // extern "C"
