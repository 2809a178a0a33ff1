// level.hip — delivery to an R 128 loudness target under the true-peak ceiling: the static
// gain that makes the DELIVERED signal read the target on a BS.1770-4 meter with the
// ceiling held (mm_level in include/mastering.h).  No reference counterpart.  The stage is a
// short secant search on the one number a delivery spec names: every pass forms its
// candidate from the kept source (so rounding never accumulates), limits it with the ceiling
// and measures it with the R 128 meter.  This file owns what is decided and the gain's body;
// it drives nothing.  The rule (level_first, level_step, level_record / level_next,
// level_unmeasurable, level_peak_cap) is plain C++ with exactly two callers: the device's one
// pass loop, level_groups_device in tracks.hip, and the host's, level_group_host in album.hip,
// which composes mm_ceiling_host, mm_r128_host and level_gain_host the same way.  A single
// track, a batch and an album are groups of tracks to both (tracks.hip: LevelGroup).  The
// gain's launch geometry (level_gain_geom) and the kept-source layout (level_keep) are here too.
//
// The gain, level_gain_span: s' = clip((s * g + 2^15) >> 16) on the samples as one mono
// line, src -> dst (src == dst allowed).  Its kernel is tracks.hip's level_tracks_gain, which
// runs it over the spans of n tracks (n = 1 included).  It is a streaming body (2 or 4 bytes in, as
// many out, a handful of integer operations a sample), so all that matters is the width of
// its memory instructions: a lane moves 16 bytes a load and a store (8 int16 or 4 f32), a
// wave one contiguous 1 KiB run, and a workgroup LEVEL_SPAN samples in LEVEL_SPAN / (256
// lanes * samples per vector) independent vectors a lane, which are all loaded before the
// first is stored, non-temporally both ways (every byte is touched once a launch).  One
// workgroup a span: spans of 16384 samples ran 30 us on the 5-minute track where 8192 ran 35
// and 4096 more, and a persistent grid-stride form no faster.  The vectors are aligned to the DESTINATION: the up to 15 bytes before
// the first 16-byte boundary of dst and what is left after the last whole vector are
// single samples (lanes of a signal's workgroup 0), so any sample count and any sample-aligned view
// is right; when src does not share dst's offset within 16 bytes, the loads alone fall back
// to single samples (level_keep places a source copy at the delivered buffer's offset, so
// the level never takes that path).  `clipped` is summed and the peak maximised over a
// wave by shuffles and folded with at most one integer atomic a wave: no result depends on
// the launch geometry.
//
// Included at the end of mastering.hip after r128.hip and ceiling.hip and before album.hip and
// tracks.hip.

namespace mm {

constexpr int LEVEL_ONE = 1 << 16;
constexpr int LEVEL_GMIN = 1 << 8, LEVEL_GMAX = 1 << 21;  // q()'s clamp: -48.2 .. +30.1 dB
constexpr int LEVEL_THREADS = 256;
constexpr int LEVEL_SPAN = 16384;  // samples of whole vectors per workgroup (mm_level_span)

// device result block of one gain launch (zeroed on the stream before it)
struct LevelDev {
    unsigned long long clipped;  // products outside the int16 range
    unsigned peak;               // max |delivered sample|, 0..32768
    unsigned _pad;
};

// One sample by g, the definition's clip(((int64)s * g + 2^15) >> 16) in 32-bit pieces: with
// g = gh * 2^16 + gl (gh <= 32, gl < 2^16), s * g + 2^15 = (s * gh) * 2^16 + (s * gl + 2^15)
// and the first term is a multiple of 2^16, so the floor is s * gh + ((s * gl + 2^15) >> 16):
// |s * gl + 2^15| < 2^31 and |s * gh| <= 2^20, both exact in int32, the shift arithmetic.
// (mm_level_host multiplies in int64 as the definition is written.)
__device__ __forceinline__ int level_scale(int s, int gh, int gl, unsigned &clipped, int &peak) {
    const int y = s * gh + ((s * gl + (1 << 15)) >> 16);
    const int d = min(32767, max(-32768, y));
    clipped += d != y;
    peak = max(peak, abs(d));
    return d;
}

template <typename T>
struct LevelVec;
template <>
struct LevelVec<int16_t> {
    typedef short type __attribute__((ext_vector_type(8)));
};
template <>
struct LevelVec<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};

// Workgroup b takes the whole vectors [b * VPB, (b + 1) * VPB) of dst + head; workgroup 0
// also the `head` samples before them (lanes 0 ..) and the tail after the last (lanes 64 ..).
// (`blk`: the workgroup's index within the signal; tracks.hip runs the body over n signals.)
template <typename T>
__device__ __forceinline__ void level_gain_span(const T *__restrict__ src, T *__restrict__ dst, int64_t n, int head,
                                                int src_vec, int g, LevelDev *st, unsigned blk) {
    constexpr int VEC = 16 / (int)sizeof(T);                   // samples per 16-byte vector
    constexpr int VPL = LEVEL_SPAN / (LEVEL_THREADS * VEC);    // vectors per lane
    typedef typename LevelVec<T>::type V;
    static_assert(sizeof(V) == 16 && VPL * LEVEL_THREADS * VEC == LEVEL_SPAN, "a workgroup covers LEVEL_SPAN samples");
    const int tid = threadIdx.x, gh = g >> 16, gl = g & 0xFFFF;
    const int64_t nvec = (n - head) / VEC;
    const int64_t v0 = (int64_t)blk * (LEVEL_THREADS * VPL) + tid;
    unsigned clipped = 0;
    int peak = 0;
    V v[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int64_t vi = v0 + (int64_t)j * LEVEL_THREADS;
        if (vi < nvec) {
            const T *p = src + head + vi * VEC;
            if (src_vec) {
                v[j] = __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[j][k] = p[k];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int64_t vi = v0 + (int64_t)j * LEVEL_THREADS;
        if (vi < nvec) {
            V o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) o[k] = pcm_encode<T>(level_scale(pcm_decode<T>((T)v[j][k]), gh, gl, clipped, peak));
            __builtin_nontemporal_store(o, reinterpret_cast<V *>(dst + head + vi * VEC));
        }
    }
    if (blk == 0) {  // the single samples: fewer than VEC at either end
        const int64_t tail0 = head + nvec * VEC;
        int64_t i = -1;
        if (tid < head) i = tid;
        else if (tid >= 64 && tail0 + (tid - 64) < n) i = tail0 + (tid - 64);
        if (i >= 0) dst[i] = pcm_encode<T>(level_scale(pcm_decode<T>(src[i]), gh, gl, clipped, peak));
    }
    clipped = wave_sum_u32(clipped);
    peak = wave_max_i32(peak);
    // at most one atomic of either kind a wave, and none for a peak the block already holds:
    // thousands of waves on one address serialise (the maximum only grows, so a stale read
    // costs an atomic, never a result)
    if ((tid & 63) == 0) {
        if (clipped) atomicAdd(&st->clipped, (unsigned long long)clipped);
        if ((unsigned)peak > __atomic_load_n(&st->peak, __ATOMIC_RELAXED)) atomicMax(&st->peak, (unsigned)peak);
    }
}

}  // namespace mm

// ======================================================= the rule, host and device alike
namespace {

constexpr int LEVEL_PASSES = MM_LEVEL_PASSES;
constexpr double LEVEL_TOL = 0.05, LEVEL_SMIN = 0.25;

// q(G) = clamp(floor(G * 2^16 + 0.5), 2^8, 2^21) (not-a-number and anything below: 2^8)
int32_t level_q(double G) {
    const double v = std::floor(G * 65536.0 + 0.5);
    if (!(v >= (double)LEVEL_GMIN)) return LEVEL_GMIN;
    return v > (double)LEVEL_GMAX ? LEVEL_GMAX : (int32_t)v;
}

double level_db(int32_t g) { return 20.0 * std::log10((double)g / 65536.0); }

void level_clear(mm_level *o, int64_t frames, int channels, int rate, int32_t clu, int32_t C, int32_t W) {
    memset(o, 0, sizeof *o);
    o->frames = frames;
    o->channels = channels;
    o->rate = rate;
    o->target_clu = clu;
    o->ceiling_q28 = C;
    o->window = W;
    o->status = MM_LEVEL_OFF;
    o->gain_q16 = LEVEL_ONE;
    o->min_gain_q16 = LEVEL_ONE;
    o->source_lufs = o->loudness = NAN;
    for (double &v : o->pass_lufs) v = NAN;
}

// g_0 of step 2
int32_t level_first(const mm_level *o) {
    return level_q(std::pow(10.0, ((double)o->target_clu / 100.0 - o->source_lufs) / 20.0));
}

// Steps 4 and 5 after pass k = o->passes - 1 was measured (pass_gain_q16[k] the gain it ran
// with, pass_lufs[k] its loudness): sets the status and returns 0 when the pass is
// delivered, else returns the next gain.
int32_t level_next(mm_level *o, bool capped) {
    const int k = o->passes - 1;
    const double T = (double)o->target_clu / 100.0, Ik = o->pass_lufs[k], dk = level_db(o->pass_gain_q16[k]);
    bool have_m = false;
    double m = 1.0;
    if (k >= 1) {
        const double dp = level_db(o->pass_gain_q16[k - 1]);
        if (dk != dp) {
            have_m = true;
            m = (Ik - o->pass_lufs[k - 1]) / (dk - dp);
        }
    }
    if (std::fabs(T - Ik) <= LEVEL_TOL) o->status = MM_LEVEL_REACHED;
    else if (capped) o->status = MM_LEVEL_CAPPED;
    else if (have_m && m < LEVEL_SMIN) o->status = MM_LEVEL_SATURATED;
    else if (k == LEVEL_PASSES - 1) o->status = MM_LEVEL_PASSES_SPENT;
    if (o->status != MM_LEVEL_OFF) {
        o->gain_q16 = o->pass_gain_q16[k];
        o->loudness = Ik;
        return 0;
    }
    const double slope = have_m ? std::min(m, 1.0) : 1.0;
    return level_q(((double)o->pass_gain_q16[k] / 65536.0) * std::pow(10.0, (T - Ik) / (20.0 * slope)));
}

// the boost branch's cap and inner ceiling (step 3, C != 0 and g > ONE)
int32_t level_boost_cap(int32_t C) { return (int32_t)((((int64_t)C - CEIL_GUARD) << 16) >> 24); }
int32_t level_inner_ceiling(int32_t C, int32_t g) { return (int32_t)((((int64_t)C - CEIL_GUARD) << 16) / g); }

// the clip-free gain of a signal of sample peak `peak` (step 3, C == 0)
int32_t level_peak_cap(int32_t peak) {
    return peak > 0 ? (int32_t)std::min<int64_t>(((int64_t)32767 << 16) / peak, LEVEL_GMAX) : LEVEL_GMAX;
}

// Step 3 for the candidate g of a pass: the gain the pass runs with, whether a cap held it,
// and for a boost behind the limiter (C != 0 and g > ONE) the inner ceiling of that gain.
// g_peak: level_peak_cap of the source, which caps a level without a ceiling.
struct LevelStep {
    int32_t g, C_inner;
    bool capped, boost;
};

LevelStep level_step(int32_t C, int32_t g, int32_t g_peak) {
    LevelStep s{g, 0, false, C != 0 && g > LEVEL_ONE};
    if (C && !s.boost) return s;  // a cut under a ceiling: plain gain
    const int32_t cap = C ? level_boost_cap(C) : g_peak;
    if (s.g > cap) s.g = cap, s.capped = true;
    if (s.boost) s.C_inner = level_inner_ceiling(C, s.g);  // the limiter before the boost, so that the boost cannot clip first
    return s;
}

// what the limiter did over n ceilings (one a track): the frames summed, the smallest gain
void level_limited(mm_level *o, const mm_ceiling *ce, int n) {
    o->limited_frames = 0;
    o->min_gain_q16 = LEVEL_ONE;
    for (int t = 0; t < n; ++t) {
        o->limited_frames += ce[t].limited_frames;
        o->min_gain_q16 = std::min(o->min_gain_q16, ce[t].min_gain_q16);
    }
}

// The record after a pass ran with s and was measured at `lufs`, then steps 4 and 5: returns
// level_next.  ce [n]: the pass's ceilings at C; ce_in [n]: its inner ceilings, which a boost
// reports as the limiter's work (else the ceilings at C are the limiter).  n == 0: no ceiling.
int32_t level_record(mm_level *o, const LevelStep &s, double lufs, int64_t clipped, const mm_ceiling *ce,
                     const mm_ceiling *ce_in, int n) {
    const int k = o->passes++;
    o->pass_gain_q16[k] = s.g;
    o->pass_lufs[k] = lufs;
    o->clipped = clipped;
    if (n) level_limited(o, s.boost ? ce_in : ce, n);
    return level_next(o, s.capped);
}

// no gain to find (fewer than 4 hops, or silence): the signal only got its n ceilings
void level_unmeasurable(mm_level *o, const mm_ceiling *ce, int n) {
    o->status = MM_LEVEL_UNMEASURABLE;
    if (n) level_limited(o, ce, n);
}

// gain(x, g) as the definition writes it, in int64: from -> to (from == to allowed), the
// products outside the int16 range added to `clipped`
void level_gain_host(const int16_t *from, int16_t *to, size_t n, int32_t g, int64_t &clipped) {
    for (size_t i = 0; i < n; ++i) {
        const int64_t v = (int64_t)from[i] * g + (1 << 15);
        const int64_t y = v >= 0 ? v >> 16 : -((-v + 65535) >> 16);  // floor(v / 2^16): the arithmetic shift
        const int64_t d = std::min<int64_t>(32767, std::max<int64_t>(-32768, y));
        clipped += d != y;
        to[i] = (int16_t)d;
    }
}

// why the arguments are not a levelling job, or null (C == 0: no ceiling, W is then ignored)
const char *level_bad_args(int64_t frames, int channels, int rate, int32_t clu, int32_t C, int32_t W) {
    if (clu < -4000 || clu > -500) return "level_clu out of range [-4000, -500] (-40 .. -5 LUFS)";
    if (const char *why = r128_refusal(channels, frames, rate)) return why;
    return C ? ceiling_bad_args(frames, channels, C, W) : nullptr;
}

// The geometry of one gain launch of n samples: the single samples before dst's first 16-byte
// boundary, whether src shares dst's offset within 16 bytes (whole-vector loads), and the
// workgroups (one a LEVEL_SPAN of whole vectors, at least one; none for no samples).
struct LevelGeom {
    int head, src_vec;
    int64_t wgs;
};

LevelGeom level_gain_geom(const void *src, const void *dst, int kind, int64_t n) {
    const int64_t sb = (int64_t)pcm_sample_bytes(kind);
    const int head = (int)std::min<int64_t>(n, (int64_t)((16 - ((uintptr_t)dst & 15)) & 15) / sb);
    const int src_vec = ((((uintptr_t)src) ^ ((uintptr_t)dst)) & 15) == 0;
    const int64_t nvec = (n - head) / (16 / sb), vpb = LEVEL_SPAN / (16 / sb);
    return LevelGeom{head, src_vec, n ? std::max<int64_t>(1, (nvec + vpb - 1) / vpb) : 0};
}

// The kept sources of n tracks in the one context buffer `name`: src[t] lies at its delivered
// buffer's offset within 16 bytes, so that a pass from it loads whole vectors.
int level_keep(mm_ctx *c, const char *name, void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
               std::vector<char *> &src) {
    auto room = [&](int t) { return ((pcm_bytes(kind, frames[t], channels) + 15) & ~(size_t)15) + 16; };
    size_t total = 0;
    for (int t = 0; t < n; ++t) total += room(t);
    char *keep;
    RET(get_buf(c, name, total, &keep));
    src.resize((size_t)n);
    for (int t = 0; t < n; ++t) {
        src[(size_t)t] = keep + ((uintptr_t)d_pcm[t] & 15);
        keep += room(t);
    }
    return MM_OK;
}

}  // namespace

extern "C" {

int mm_level_span(void) { return LEVEL_SPAN; }

int mm_last_levels(mm_ctx *c, int cap, mm_level *out) {
    if (!c || cap < 0 || (cap > 0 && !out)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->levels.empty()) return set_err(c, MM_ERR_STATE, "the last master call set no loudness target");
    const int n = (int)c->levels.size();
    for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->levels[(size_t)i];
    return n;
}

}  // extern "C"
