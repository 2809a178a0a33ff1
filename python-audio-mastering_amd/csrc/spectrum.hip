// spectrum.hip — the spectrum report of a delivered signal (mm_spectrum in include/mastering.h):
// Welch's long-term spectrum of both channels and their cross-spectrum's real part on frames of
// 8192 samples, and from that bin table the 1/3-octave bands.  No reference counterpart.  The
// FFT is float arithmetic, so the report is not bit-equal between its restatements; it is
// between two runs, between a batch and single calls and between a master call and
// mm_spectrum_pcm on what it delivered.  The bins end in mm_spectrum_from_bins, the one tail
// of the host restatement (mm_spectrum_host: its own radix-2 FFT in double) and the GPU path.
//
// The GPU path is two launches on the context's stream, with no atomic.  spec_tracks: a
// workgroup of 256 threads owns a group of G consecutive frames of one track (spectrum.h) and
// runs, a frame, ONE complex 8192-point FFT on z = w * (L + iR) with 32 points a thread:
//   n = 256 a + t, k = k1 + 32 (p + 16 q), t = 16 b + c
//   pass 1  thread t        DFT-32 over a, times W_8192^(t k1)          -> y[k1][t]
//   pass 2  thread (k1, c)  DFT-16 over b, times W_256^(c p)    (twice) -> u[k1][p][c]
//   pass 3  thread (k1, p)  DFT-16 over c                       (twice) -> Z[k1 + 32 p + 512 q]
// The samples are loaded straight into registers (thread t the frames 256 a + t: whole lines,
// a dword a stereo frame, at any frame offset of an allocation) and windowed in fp32.  Between
// the passes the points cross LDS one component at a time (34 KiB static, so four workgroups
// share a CU's LDS and no opt-in is needed): [k1][16][16] with the rows of 16 padded to 17 and
// the k1 planes to 272 floats, which leaves every strided read and write of the two exchanges
// free of bank conflicts (a 32-lane group meets 16 consecutive banks twice, 16 apart).  A third
// exchange brings Z to natural order (k + k / 32) for the unpacking X_L[k] = (Z[k] + conj
// Z[N - k]) / 2, X_R[k] = (Z[k] - conj Z[N - k]) / 2i: thread t owns the bins t + 256 m, and
// thread 0 bin N/2 too, and adds |X_L|^2, |X_R|^2 and Re(X_L conj X_R), squared and summed in
// double, into 51 float64 registers that live across the group's frames.  Then it writes the
// group's record [N/2 + 1][3] with plain stores.  The twiddles of the passes' seams and the
// window are tables computed once a context on the host in double and rounded to fp32; the
// butterflies inside a thread take W_32's powers as literals.  No device sincos.
// spec_fold: one thread a (track, bin, column) sums the track's records in group order and
// divides by F (no frame: NaN); stream order gives it the records.
//
// The frames launch lies over the groups of all tracks of a call (tracks.h's prefix sums): a
// single signal is a call of one track.  Included at the end of mastering.hip after qc.hip.

#include "spectrum.h"

namespace mm {

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_PLANE = 272;                  // floats of a k1 plane: 16 rows of 17
constexpr int SPEC_LDS = 32 * SPEC_PLANE;        // floats of the exchange buffer
constexpr int SPEC_MIN_RATE = 2000;              // the library's floor
constexpr int64_t SPEC_MAX_FRAMES = (int64_t)1 << 31;
static_assert(SPEC_N == 32 * SPEC_THREADS && SPEC_N == 32 * 16 * 16, "32 points a thread, passes of 32 * 16 * 16");
static_assert(SPEC_N - 1 + (SPEC_N - 1) / 32 < SPEC_LDS, "the natural-order exchange fits the buffer");
static_assert(SPEC_LDS * sizeof(float) <= 65536, "static LDS");

// cos(j pi / 16), j = 0 .. 8: W_32^j = e^(-2 pi i j / 32) = (cos, -sin), sin(j pi / 16) = cos((8 - j) pi / 16)
__host__ __device__ constexpr float spec_cos16(int j) {
    constexpr float C[9] = {1.0f,
                            0.98078528040323044913f,
                            0.92387953251128675613f,
                            0.83146961230254523708f,
                            0.70710678118654752440f,
                            0.55557023301960222474f,
                            0.38268343236508977173f,
                            0.19509032201612826785f,
                            0.0f};
    return j <= 8 ? C[j] : -C[16 - j];
}
__host__ __device__ constexpr float spec_sin16(int j) { return j <= 8 ? spec_cos16(8 - j) : spec_cos16(j - 8); }

__host__ __device__ constexpr int spec_bitrev(int k, int bits) {
    int r = 0;
    for (int i = 0; i < bits; ++i) r |= ((k >> i) & 1) << (bits - 1 - i);
    return r;
}

// In-place radix-2 decimation in frequency over R register points: X[k] lands at index
// spec_bitrev(k).  Every index and every twiddle is a constant once the loops are unrolled.
template <int R, int LEN>
__device__ __forceinline__ void spec_dif(float (&re)[R], float (&im)[R]) {
    if constexpr (LEN >= 2) {
        constexpr int HALF = LEN / 2;
#pragma unroll
        for (int b = 0; b < R; b += LEN) {
#pragma unroll
            for (int j = 0; j < HALF; ++j) {
                const float ur = re[b + j], ui = im[b + j], vr = re[b + j + HALF], vi = im[b + j + HALF];
                re[b + j] = ur + vr;
                im[b + j] = ui + vi;
                const float dr = ur - vr, di = ui - vi;
                const int j32 = j * (32 / LEN);  // W_LEN^j = W_32^j32, 0 <= j32 < 16
                if (j32 == 0) {
                    re[b + j + HALF] = dr;
                    im[b + j + HALF] = di;
                } else if (j32 == 8) {  // times -i
                    re[b + j + HALF] = di;
                    im[b + j + HALF] = -dr;
                } else {
                    const float c = spec_cos16(j32), s = spec_sin16(j32);
                    re[b + j + HALF] = dr * c + di * s;
                    im[b + j + HALF] = di * c - dr * s;
                }
            }
        }
        spec_dif<R, LEN / 2>(re, im);
    }
}

// the tables of a context: the seam twiddles of passes 1 and 2 and the window
struct SpecTables {
    const float2 *tw1;  // [32][256]: W_8192^(t k1) at k1 * 256 + t
    const float2 *tw2;  // [16][16]:  W_256^(c p) at p * 16 + c
    const float *win;   // [8192]
};
constexpr size_t SPEC_TABLE_FLOATS = 2 * 32 * 256 + 2 * 16 * 16 + SPEC_N;

// one track of a launch
struct SpecTrack {
    const void *pcm;
    int64_t F;  // frames
};

struct SpecLaunch {
    const SpecTrack *tr;     // [n]
    const uint32_t *first;   // [n + 1] prefix sums of the tracks' groups (tracks.h)
    double *rec;             // [first[n]][SPEC_REC] a track's records at first[t]
    double *out;             // [n][SPEC_REC]
    SpecTables tab;
    int n;
};

// Group `group` of a track of F frames: its record into rec[SPEC_REC].
template <int CH, typename T>
__device__ __forceinline__ void spec_frames_group(const T *__restrict__ in, int64_t F, int64_t group, const SpecTables &tab,
                                                  double *__restrict__ rec) {
    __shared__ float lds[SPEC_LDS];
    const int t = threadIdx.x, hi = t >> 4, lo = t & 15;
    int64_t f0;
    const int nf = (int)spec_group_frames(F, group, &f0);
    double acc[17][3];
#pragma unroll
    for (int m = 0; m < 17; ++m) acc[m][0] = acc[m][1] = acc[m][2] = 0.0;

    for (int f = 0; f < nf; ++f) {
        const int64_t base = (f0 + f) * SPEC_HOP;
        float re[32], im[32];
#pragma unroll
        for (int a = 0; a < 32; ++a) {
            const int n = 256 * a + t;
            const float w = tab.win[n];
            if constexpr (CH == 2) {
                const uint32_t d = load_frame_packed<T>(in, base + n);
                re[a] = w * ((float)(int)(int16_t)(d & 0xFFFFu) * (1.0f / 32768.0f));
                im[a] = w * ((float)(int)(int16_t)(d >> 16) * (1.0f / 32768.0f));
            } else {
                int s[1];
                load_frame<1, T>(in, base + n, s);
                re[a] = w * ((float)s[0] * (1.0f / 32768.0f));
                im[a] = 0.0f;
            }
        }
        // pass 1: y[k1][t] at index bitrev(k1), times W_8192^(t k1)
        spec_dif<32, 32>(re, im);
#pragma unroll
        for (int k1 = 1; k1 < 32; ++k1) {
            const float2 w = tab.tw1[k1 * 256 + t];
            const int i = spec_bitrev(k1, 5);
            const float r = re[i] * w.x - im[i] * w.y, q = re[i] * w.y + im[i] * w.x;
            re[i] = r;
            im[i] = q;
        }
        // exchange 1: thread t = 16 b + c gives y[k1][b][c]; thread (k1 = hi + 16 j, c = lo) takes its b
        float re2[2][16], im2[2][16];
#pragma unroll
        for (int k1 = 0; k1 < 32; ++k1) lds[k1 * SPEC_PLANE + hi * 17 + lo] = re[spec_bitrev(k1, 5)];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int b = 0; b < 16; ++b) re2[j][b] = lds[(hi + 16 * j) * SPEC_PLANE + b * 17 + lo];
        __syncthreads();
#pragma unroll
        for (int k1 = 0; k1 < 32; ++k1) lds[k1 * SPEC_PLANE + hi * 17 + lo] = im[spec_bitrev(k1, 5)];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int b = 0; b < 16; ++b) im2[j][b] = lds[(hi + 16 * j) * SPEC_PLANE + b * 17 + lo];
        __syncthreads();
        // pass 2: u[k1][p][c] at index bitrev(p), times W_256^(c p)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            spec_dif<16, 16>(re2[j], im2[j]);
#pragma unroll
            for (int p = 1; p < 16; ++p) {
                const float2 w = tab.tw2[p * 16 + lo];
                const int i = spec_bitrev(p, 4);
                const float r = re2[j][i] * w.x - im2[j][i] * w.y, q = re2[j][i] * w.y + im2[j][i] * w.x;
                re2[j][i] = r;
                im2[j][i] = q;
            }
        }
        // exchange 2: thread (k1, c = lo) gives u[k1][p][c]; thread (k1, p = lo) takes its c
        float re3[2][16], im3[2][16];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < 16; ++p) lds[(hi + 16 * j) * SPEC_PLANE + p * 17 + lo] = re2[j][spec_bitrev(p, 4)];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int c = 0; c < 16; ++c) re3[j][c] = lds[(hi + 16 * j) * SPEC_PLANE + lo * 17 + c];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < 16; ++p) lds[(hi + 16 * j) * SPEC_PLANE + p * 17 + lo] = im2[j][spec_bitrev(p, 4)];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int c = 0; c < 16; ++c) im3[j][c] = lds[(hi + 16 * j) * SPEC_PLANE + lo * 17 + c];
        __syncthreads();
        // pass 3: Z[k1 + 32 p + 512 q] at index bitrev(q)
#pragma unroll
        for (int j = 0; j < 2; ++j) spec_dif<16, 16>(re3[j], im3[j]);
        // exchange 3: natural order, k at k + k / 32; thread t takes Z[k] and Z[N - k] of its bins
        float ar[17], ai[17], br[17], bi[17];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int k = (hi + 16 * j) + 32 * lo + 512 * q;
                lds[k + (k >> 5)] = re3[j][spec_bitrev(q, 4)];
            }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 17; ++m) {
            const int k = m < 16 ? t + 256 * m : SPEC_N / 2, kn = (SPEC_N - k) & (SPEC_N - 1);
            ar[m] = lds[k + (k >> 5)];
            br[m] = lds[kn + (kn >> 5)];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int k = (hi + 16 * j) + 32 * lo + 512 * q;
                lds[k + (k >> 5)] = im3[j][spec_bitrev(q, 4)];
            }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 17; ++m) {
            const int k = m < 16 ? t + 256 * m : SPEC_N / 2, kn = (SPEC_N - k) & (SPEC_N - 1);
            ai[m] = lds[k + (k >> 5)];
            bi[m] = lds[kn + (kn >> 5)];
        }
        __syncthreads();  // (the buffer is free for the next frame)
        // X_L = (Z[k] + conj Z[N - k]) / 2, X_R = (Z[k] - conj Z[N - k]) / 2i; the powers in double
#pragma unroll
        for (int m = 0; m < 17; ++m) {
            const double lr = (double)(0.5f * (ar[m] + br[m])), li = (double)(0.5f * (ai[m] - bi[m]));
            acc[m][0] += lr * lr + li * li;
            if constexpr (CH == 2) {
                const double rr = (double)(0.5f * (ai[m] + bi[m])), ri = (double)(0.5f * (br[m] - ar[m]));
                acc[m][1] += rr * rr + ri * ri;
                acc[m][2] += lr * rr + li * ri;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        double *o = rec + (size_t)(t + 256 * m) * 3;
        o[0] = acc[m][0];
        o[1] = acc[m][1];
        o[2] = acc[m][2];
    }
    if (t == 0) {
        double *o = rec + (size_t)(SPEC_N / 2) * 3;
        o[0] = acc[16][0];
        o[1] = acc[16][1];
        o[2] = acc[16][2];
    }
}

// spec_frames_group over the groups of all tracks: a record lands among its track's own, and
// every frame index is the track's
template <int CH, typename T>
__global__ void __launch_bounds__(SPEC_THREADS) spec_tracks_kernel(SpecLaunch L) {
    const int t = tracks_find(L.first, L.n, blockIdx.x);
    const SpecTrack tr = L.tr[t];
    spec_frames_group<CH, T>(static_cast<const T *>(tr.pcm), tr.F, (int64_t)(blockIdx.x - L.first[t]), L.tab,
                             L.rec + (size_t)blockIdx.x * SPEC_REC);
}

// Thread (blockIdx.y = track, i = bin * 3 + column) sums the track's records in group order and
// divides by its frames.
__global__ void __launch_bounds__(SPEC_THREADS) spec_fold_kernel(SpecLaunch L) {
    const int i = (int)blockIdx.x * SPEC_THREADS + (int)threadIdx.x, t = (int)blockIdx.y;
    if (i >= SPEC_REC) return;
    const int64_t F = L.tr[t].F;
    const uint32_t g0 = L.first[t], g1 = L.first[t + 1];
    double s = 0.0;
    for (uint32_t g = g0; g < g1; ++g) s += L.rec[(size_t)g * SPEC_REC + i];
    L.out[(size_t)t * SPEC_REC + i] = F > 0 ? s / (double)F : __builtin_nan("");
}

}  // namespace mm

// ======================================================= host side
namespace {

const double SPEC_PI = 3.14159265358979323846;

// edge m of the 1/3-octave bands: band m is [edge(m), edge(m + 1)) around 1000 * 10^(m / 10)
double spec_edge(int m) { return 1000.0 * std::pow(10.0, (2 * m - 1) / 20.0); }
constexpr int SPEC_BAND0 = -17;  // the 20 Hz band

int spec_n_bands(int rate) {
    int n = 0;
    while (n < MM_SPECTRUM_MAX_BANDS && spec_edge(SPEC_BAND0 + n) < 0.5 * rate) ++n;
    return n;
}

// why a signal is refused, or null (the words of mm_last_error)
const char *spectrum_refusal(int channels, int64_t frames, int rate) {
    if (rate < SPEC_MIN_RATE) return "rate below 2000 Hz";
    return pcm_refusal(channels, frames, SPEC_MAX_FRAMES);
}

// in-place radix-2 FFT of SPEC_N complex doubles (decimation in time; the host restatement's own)
void spec_fft_host(std::vector<double> &re, std::vector<double> &im) {
    static const std::vector<double> tw = [] {
        std::vector<double> v((size_t)SPEC_N);  // cos, -sin of 2 pi j / N, j < N / 2
        for (int j = 0; j < SPEC_N / 2; ++j) {
            v[(size_t)(2 * j)] = std::cos(2.0 * SPEC_PI * j / SPEC_N);
            v[(size_t)(2 * j + 1)] = -std::sin(2.0 * SPEC_PI * j / SPEC_N);
        }
        return v;
    }();
    for (int i = 0; i < SPEC_N; ++i) {
        const int j = spec_bitrev(i, 13);
        if (j > i) {
            std::swap(re[(size_t)i], re[(size_t)j]);
            std::swap(im[(size_t)i], im[(size_t)j]);
        }
    }
    for (int len = 2; len <= SPEC_N; len <<= 1) {
        const int half = len / 2, step = SPEC_N / len;
        for (int b = 0; b < SPEC_N; b += len)
            for (int j = 0; j < half; ++j) {
                const double c = tw[(size_t)(2 * j * step)], s = tw[(size_t)(2 * j * step + 1)];
                const size_t u = (size_t)(b + j), v = u + (size_t)half;
                const double xr = re[v] * c - im[v] * s, xi = re[v] * s + im[v] * c;
                re[v] = re[u] - xr;
                im[v] = im[u] - xi;
                re[u] += xr;
                im[u] += xi;
            }
    }
}

// the tables of the kernels on the device, once a context
int spec_tables(mm_ctx *c, SpecTables *tab) {
    float *d;
    RET(get_buf(c, "spec_tab", SPEC_TABLE_FLOATS, &d));
    if (!c->spec_tab_ok) {
        std::vector<float> h(SPEC_TABLE_FLOATS);
        float *tw1 = h.data(), *tw2 = tw1 + 2 * 32 * 256, *win = tw2 + 2 * 16 * 16;
        for (int k1 = 0; k1 < 32; ++k1)
            for (int t = 0; t < 256; ++t) {
                const double a = 2.0 * SPEC_PI * ((t * k1) % SPEC_N) / SPEC_N;
                tw1[2 * (k1 * 256 + t)] = (float)std::cos(a);
                tw1[2 * (k1 * 256 + t) + 1] = (float)-std::sin(a);
            }
        for (int p = 0; p < 16; ++p)
            for (int q = 0; q < 16; ++q) {
                const double a = 2.0 * SPEC_PI * ((q * p) % 256) / 256.0;
                tw2[2 * (p * 16 + q)] = (float)std::cos(a);
                tw2[2 * (p * 16 + q) + 1] = (float)-std::sin(a);
            }
        for (int n = 0; n < SPEC_N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * SPEC_PI * n / SPEC_N));
        HIPCHK(c, hipMemcpyAsync(d, h.data(), SPEC_TABLE_FLOATS * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host vector is transient)
        c->spec_tab_ok = true;
    }
    tab->tw1 = reinterpret_cast<const float2 *>(d);
    tab->tw2 = reinterpret_cast<const float2 *>(d + 2 * 32 * 256);
    tab->win = d + 2 * 32 * 256 + 2 * 16 * 16;
    return MM_OK;
}

// The reports of n checked device-resident tracks into out[n], their bin tables into bins[n]
// (synchronous on return): one upload of the track table, the frames launch, the fold launch
// and one read-back, then the tail.  The host tables live until the synchronisation.
int spectrum_run(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                 mm_spectrum *out, std::vector<std::vector<double>> &bins) {
    const size_t N = (size_t)n;
    std::vector<SpecTrack> tr(N);
    std::vector<int64_t> wgs(N);
    std::vector<uint32_t> first(N + 1);
    for (int t = 0; t < n; ++t) {
        tr[(size_t)t] = SpecTrack{d_pcm[t], spec_frames(frames[t])};
        wgs[(size_t)t] = spec_groups(tr[(size_t)t].F);
    }
    const uint32_t grid = tracks_prefix(wgs.data(), n, first.data());
    const size_t tab_bytes = N * sizeof(SpecTrack) + (N + 1) * sizeof(uint32_t);
    std::vector<char> tab(tab_bytes);
    memcpy(tab.data(), tr.data(), N * sizeof(SpecTrack));
    memcpy(tab.data() + N * sizeof(SpecTrack), first.data(), (N + 1) * sizeof(uint32_t));
    std::vector<double> back(N * SPEC_REC);
    char *d_tab;
    SpecLaunch L{};
    RET(spec_tables(c, &L.tab));
    RET(get_buf(c, "spec_trk", tab_bytes, &d_tab));
    RET(get_buf(c, "spec_out", N * SPEC_REC, &L.out));
    RET(get_buf(c, "spec_rec", std::max<size_t>((size_t)grid * SPEC_REC, 1), &L.rec));
    L.tr = reinterpret_cast<const SpecTrack *>(d_tab);
    L.first = reinterpret_cast<const uint32_t *>(d_tab + N * sizeof(SpecTrack));
    L.n = n;
    HIPCHK(c, hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    if (grid)
        RET(dispatch_pcm(kind, channels, [&](auto ch, auto t) {
            using T = decltype(t);
            return launch(c, "spec_tracks", spec_tracks_kernel<ch, T>, dim3(grid), dim3(SPEC_THREADS), 0, L);
        }));
    RET(launch(c, "spec_fold", spec_fold_kernel, dim3(blocks_for(SPEC_REC, SPEC_THREADS), (unsigned)n), dim3(SPEC_THREADS), 0, L));
    HIPCHK(c, hipMemcpyAsync(back.data(), L.out, N * SPEC_REC * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    bins.resize(N);
    for (int t = 0; t < n; ++t) {
        bins[(size_t)t].assign(back.begin() + (ptrdiff_t)((size_t)t * SPEC_REC), back.begin() + (ptrdiff_t)((size_t)(t + 1) * SPEC_REC));
        mm_spectrum_from_bins(bins[(size_t)t].data(), frames[t], channels, rate, &out[t], nullptr);
    }
    return MM_OK;
}

// an entry of a master call's results for a track that did not ask
void spectrum_clear(mm_spectrum *o, int channels) {
    *o = mm_spectrum{};
    o->channels = channels;
    o->n_fft = SPEC_N;
    o->hop = SPEC_HOP;
    o->total_ms[0] = o->total_ms[1] = NAN;
}

// Refuses what is not a batch to take the spectra of, as batch_qc_check does.
int batch_spectrum_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                         const mm_spectrum *out) {
    return batch_check(c, pcm, kind, frames, n, channels, out != nullptr,
                       [&](int t) { return spectrum_refusal(channels, frames[t], rate); });
}

// The spectrum reports of n checked device-resident tracks (synchronous on return).  Only
// c->spectra and the bin tables are set: the other results of the context's last call stay.
int batch_spectrum_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels, int rate,
                          mm_spectrum *out) {
    std::vector<std::vector<double>> bins;
    RET(spectrum_run(c, d_pcm, kind, frames, n, channels, rate, out, bins));
    c->spectra.assign(out, out + n);
    c->spectrum_bins.swap(bins);
    return MM_OK;
}

}  // namespace

// The spectrum report of a device-resident signal (synchronous on return), a call of one track
// that leaves the context's results as they are; the bin table into *bins.
static int spectrum_device(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, int rate, mm_spectrum *out,
                           std::vector<double> *bins) {
    if (!c || !out || (frames > 0 && !d_pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = spectrum_refusal(channels, frames, rate)) return set_err(c, MM_ERR_ARG, "spectrum: %s", why);
    std::vector<std::vector<double>> all;
    RET(spectrum_run(c, &d_pcm, kind, &frames, 1, channels, rate, out, all));
    if (bins) bins->swap(all[0]);
    return MM_OK;
}

// what the single entries do with the table: the bands and the caller's copy
static void spectrum_outputs(const std::vector<double> &bins, int64_t frames, int channels, int rate, mm_spectrum *out,
                             double *bands, double *bins_out) {
    if (bands) mm_spectrum_from_bins(bins.data(), frames, channels, rate, out, bands);
    if (bins_out) memcpy(bins_out, bins.data(), SPEC_REC * sizeof(double));
}

extern "C" {

int mm_spectrum_bands(int32_t rate, int cap, double *edges) {
    if (rate < SPEC_MIN_RATE || cap < 0 || (cap > 0 && !edges)) return MM_ERR_ARG;
    const int n = spec_n_bands(rate);
    for (int b = 0; b < std::min(n, cap); ++b) {
        edges[3 * b] = spec_edge(SPEC_BAND0 + b);
        edges[3 * b + 1] = 1000.0 * std::pow(10.0, (SPEC_BAND0 + b) / 10.0);
        edges[3 * b + 2] = std::min(spec_edge(SPEC_BAND0 + b + 1), 0.5 * rate);
    }
    return n;
}

int mm_spectrum_from_bins(const double *bins, int64_t frames, int channels, int32_t rate, mm_spectrum *out, double *bands) {
    if (!bins || !out || spectrum_refusal(channels, frames, rate)) return MM_ERR_ARG;
    const double df = (double)rate / SPEC_N, nyq = 0.5 * rate, norm = (double)SPEC_N * (3.0 * SPEC_N / 8.0);
    out->frames = frames;
    out->channels = channels;
    out->rate = rate;
    out->n_fft = SPEC_N;
    out->hop = SPEC_HOP;
    out->n_frames = spec_frames(frames);
    out->n_bands = spec_n_bands(rate);
    out->_pad = 0;
    for (int ch = 0; ch < 2; ++ch) {
        double s = 0.0;
        for (int k = 0; k <= SPEC_N / 2; ++k) s += (k == 0 || k == SPEC_N / 2 ? 1.0 : 2.0) * bins[3 * k + ch];
        out->total_ms[ch] = s / norm;
    }
    if (!bands) return MM_OK;
    for (int b = 0; b < out->n_bands; ++b) {
        const double lo = spec_edge(SPEC_BAND0 + b), hi = std::min(spec_edge(SPEC_BAND0 + b + 1), nyq);
        const int k0 = std::max(0, (int)std::floor(lo / df + 0.5) - 1), k1 = std::min(SPEC_N / 2, (int)std::floor(hi / df + 0.5) + 1);
        double s[3] = {0.0, 0.0, 0.0}, width = 0.0;
        for (int k = k0; k <= k1; ++k) {
            const double bl = std::max(0.0, (k - 0.5) * df), bh = std::min(nyq, (k + 0.5) * df);
            const double ov = std::min(bh, hi) - std::max(bl, lo);
            if (!(ov > 0.0)) continue;
            const double frac = ov / (bh - bl), ck = k == 0 || k == SPEC_N / 2 ? 1.0 : 2.0;
            for (int q = 0; q < 3; ++q) s[q] += frac * ck * bins[3 * k + q];
            width += 0.5 * frac * ck;
        }
        for (int q = 0; q < 3; ++q) bands[4 * b + q] = s[q] / norm;
        bands[4 * b + 3] = width;
    }
    return MM_OK;
}

int mm_spectrum_host(const int16_t *pcm, int64_t frames, int channels, int32_t rate, mm_spectrum *out, double *bands,
                     double *bins_out) {
    if (!out || (frames > 0 && !pcm) || spectrum_refusal(channels, frames, rate)) return MM_ERR_ARG;
    const int64_t F = spec_frames(frames);
    std::vector<double> bins((size_t)SPEC_REC, 0.0), re((size_t)SPEC_N), im((size_t)SPEC_N), win((size_t)SPEC_N);
    for (int n = 0; n < SPEC_N; ++n) win[(size_t)n] = 0.5 - 0.5 * std::cos(2.0 * SPEC_PI * n / SPEC_N);
    for (int64_t f = 0; f < F; ++f) {
        const int16_t *x = pcm + f * SPEC_HOP * channels;
        for (int n = 0; n < SPEC_N; ++n) {
            re[(size_t)n] = win[(size_t)n] * (x[(size_t)n * channels] / 32768.0);
            im[(size_t)n] = channels == 2 ? win[(size_t)n] * (x[(size_t)n * 2 + 1] / 32768.0) : 0.0;
        }
        spec_fft_host(re, im);
        for (int k = 0; k <= SPEC_N / 2; ++k) {
            const size_t a = (size_t)k, b = (size_t)((SPEC_N - k) & (SPEC_N - 1));
            const double lr = 0.5 * (re[a] + re[b]), li = 0.5 * (im[a] - im[b]);
            bins[3 * a] += lr * lr + li * li;
            if (channels == 2) {
                const double rr = 0.5 * (im[a] + im[b]), ri = 0.5 * (re[b] - re[a]);
                bins[3 * a + 1] += rr * rr + ri * ri;
                bins[3 * a + 2] += lr * rr + li * ri;
            }
        }
    }
    for (double &v : bins) v = F > 0 ? v / (double)F : NAN;
    mm_spectrum_from_bins(bins.data(), frames, channels, rate, out, bands);
    if (bins_out) memcpy(bins_out, bins.data(), SPEC_REC * sizeof(double));
    return MM_OK;
}

int mm_spectrum_device(mm_ctx *c, const void *d_pcm, int kind, int64_t frames, int channels, int32_t rate, mm_spectrum *out,
                       double *bands, double *bins_out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<double> bins;
    RET(spectrum_device(c, d_pcm, kind, frames, channels, rate, out, &bins));
    spectrum_outputs(bins, frames, channels, rate, out, bands, bins_out);
    return MM_OK;
}

int mm_spectrum_pcm(mm_ctx *c, const void *pcm, int kind, int64_t frames, int channels, int32_t rate, mm_spectrum *out,
                    double *bands, double *bins_out) {
    if (!c) return MM_ERR_ARG;
    if (!out || (frames > 0 && !pcm)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    if (const char *why = spectrum_refusal(channels, frames, rate)) return set_err(c, MM_ERR_ARG, "spectrum: %s", why);
    HIPCHK(c, hipSetDevice(c->device));
    char *din;
    RET(pcm_upload(c, "spec_in", pcm, pcm_bytes(kind, frames, channels), &din));
    std::vector<double> bins;
    RET(spectrum_device(c, din, kind, frames, channels, rate, out, &bins));
    spectrum_outputs(bins, frames, channels, rate, out, bands, bins_out);
    return MM_OK;
}

int mm_batch_spectrum_device(mm_ctx *c, const void *const *d_pcm, int kind, const int64_t *frames, int n, int channels,
                             int32_t rate, mm_spectrum *out) {
    if (!c) return MM_ERR_ARG;
    RET(batch_spectrum_check(c, d_pcm, kind, frames, n, channels, rate, out));
    HIPCHK(c, hipSetDevice(c->device));
    return batch_spectrum_device(c, d_pcm, kind, frames, n, channels, rate, out);
}

int mm_batch_spectrum_pcm(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                          int32_t rate, mm_spectrum *out) {
    if (!c) return MM_ERR_ARG;
    RET(batch_spectrum_check(c, pcm, kind, frames, n, channels, rate, out));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<void *> d;
    RET(album_upload(c, "batch_spec_in", pcm, kind, frames, n, channels, d));
    return batch_spectrum_device(c, d.data(), kind, frames, n, channels, rate, out);
}

int mm_last_spectrum(mm_ctx *c, int cap, mm_spectrum *out) {
    if (!c || cap < 0 || (cap > 0 && !out)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->spectra.empty()) return set_err(c, MM_ERR_STATE, "the last call made no spectrum report");
    const int n = (int)c->spectra.size();
    for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->spectra[(size_t)i];
    return n;
}

int mm_last_spectrum_bins(mm_ctx *c, int track, int cap, double *bins) {
    if (!c || cap < 0 || (cap > 0 && !bins)) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (c->spectra.empty()) return set_err(c, MM_ERR_STATE, "the last call made no spectrum report");
    if (track < 0 || track >= (int)c->spectra.size()) return set_err(c, MM_ERR_ARG, "track %d out of range", track);
    const std::vector<double> &b = c->spectrum_bins[(size_t)track];
    for (int i = 0; i < std::min(cap, SPEC_BINS) * 3; ++i) bins[i] = b.empty() ? NAN : b[(size_t)i];
    return SPEC_BINS;
}

}  // extern "C"
