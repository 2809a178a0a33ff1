// decode.hip — integer PCM above 16 bits (no reference counterpart: the reference
// decodes such files and then wraps them on the way out): packed 24-bit
// (MM_IN_I24) and 32-bit (MM_IN_I32) little-endian samples to the f32 the chain
// takes as MM_IN_F32.  With v the sample left-justified in an int32 (s << 8 for a
// sign-extended 24-bit s), x = RN_f32(v) * 2^-31: one round-to-nearest-even
// conversion (exact for 24-bit samples, where it equals float(s) * 2^-23), then an
// exact power-of-two scale.  The kernel, its launch, the host restatement and the
// entry points; included from mastering.hip after context.h (stage_front calls
// pcm_decode).

namespace mm {

// A workgroup pass ("span") decodes DEC_SPAN samples: the span's bytes are staged in
// LDS with 16-byte aligned loads, then every thread turns DEC_QUADS quads of four
// samples into one 16-byte store each.  A packed 24-bit input has no alignment (a
// slice of a caller's tensor, a fused timeline's track at a multiple of 3 or 6
// bytes), and neither input nor output bounds are multiples of anything, so:
//  - samples are counted from a virtual origin `hs` (0..3) samples before out[0], at
//    which the output is 16-byte aligned: quad Q covers virtual samples 4Q..4Q+3, a
//    quad inside [hs, hs + n) is one float4 store, the (at most two) quads on the
//    ends store their valid elements one by one;
//  - a quad is 4 * BPS bytes = whole dwords, so every quad of a launch starts at the
//    same byte phase p of an aligned dword; a thread reads BPS + 1 dwords of LDS
//    (odd dword stride for 24-bit: no bank conflicts) and resolves p with
//    v_alignbyte in registers;
//  - global loads are aligned uint4 where all 16 bytes lie in [lo, hi), the aligned
//    dwords that hold at least one input byte, and single aligned dwords of that
//    range on its two ends; nothing outside [lo, hi) is read, so no load can touch a
//    page the input does not touch.  (LDS past the input holds zeros; what is
//    decoded from it is never stored.)
constexpr int DEC_THREADS = 256;
constexpr int DEC_QUADS = 4;
constexpr int DEC_SPAN = DEC_THREADS * DEC_QUADS * 4;  // samples per span (mm_pcm_decode_span)
constexpr int DEC_MAX_GRID = 2048;                     // 256 CUs x 8 workgroups; spans beyond: grid-stride

typedef uint32_t dec_u32x4 __attribute__((ext_vector_type(4)));

template <int BPS>  // bytes per sample: 3 (MM_IN_I24) or 4 (MM_IN_I32, input 4-byte aligned: p == 0)
__global__ void __launch_bounds__(DEC_THREADS) pcm_decode_kernel(const unsigned char *in, int64_t n, float *out) {
    // up to 3 dwords from the span's 16-byte chunk to its first byte, the span, and
    // the dword a phase p != 0 makes the last quad reach into
    constexpr int DWORDS = 3 + BPS * (DEC_SPAN / 4) + 1;
    constexpr int CHUNKS = (DWORDS + 3) / 4;
    __shared__ uint4 stage[CHUNKS];
    const uint32_t *lds = reinterpret_cast<const uint32_t *>(stage);

    const int64_t ia = (int64_t) reinterpret_cast<uintptr_t>(in);
    const int64_t hs = (int64_t)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);
    const int64_t lo = ia & ~(int64_t)3, hi = (ia + n * BPS + 3) & ~(int64_t)3;
    const int64_t vb = ia - BPS * hs;  // byte address of virtual sample 0 (never dereferenced below lo)
    const int p = (int)(vb & 3);
    const int64_t spans = (hs + n + DEC_SPAN - 1) / DEC_SPAN;

    for (int64_t s = blockIdx.x; s < spans; s += gridDim.x) {
        const int64_t b0 = vb + s * (int64_t)(DEC_SPAN * BPS);
        const int64_t a0 = b0 & ~(int64_t)15;
        for (int k = threadIdx.x; k < CHUNKS; k += DEC_THREADS) {
            const int64_t a = a0 + 16 * (int64_t)k;
            const unsigned char *g = in + (a - ia);  // (formed from the argument: a global address)
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (a >= lo && a + 16 <= hi) {  // (read once: non-temporal)
                const dec_u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const dec_u32x4 *>(g));
                v = make_uint4(t.x, t.y, t.z, t.w);
            } else {  // an end of the input: only the dwords that hold input bytes
                if (a >= lo && a + 4 <= hi) v.x = *reinterpret_cast<const uint32_t *>(g);
                if (a + 4 >= lo && a + 8 <= hi) v.y = *reinterpret_cast<const uint32_t *>(g + 4);
                if (a + 8 >= lo && a + 12 <= hi) v.z = *reinterpret_cast<const uint32_t *>(g + 8);
                if (a + 12 >= lo && a + 16 <= hi) v.w = *reinterpret_cast<const uint32_t *>(g + 12);
            }
            stage[k] = v;
        }
        __syncthreads();
        const int dw = (int)((b0 - a0) >> 2);
#pragma unroll
        for (int q = 0; q < DEC_QUADS; ++q) {
            const int ql = q * DEC_THREADS + (int)threadIdx.x;
            const uint32_t *w = lds + dw + BPS * ql;
            int32_t v[4];  // left-justified samples
            if constexpr (BPS == 3) {
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
                // the quad's 12 bytes at phase 0
                const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, p), d1 = __builtin_amdgcn_alignbyte(w2, w1, p),
                               d2 = __builtin_amdgcn_alignbyte(w3, w2, p);
                v[0] = (int32_t)(d0 << 8);                                     // bytes 0..2
                v[1] = (int32_t)(__builtin_amdgcn_alignbyte(d1, d0, 3) << 8);  // bytes 3..5
                v[2] = (int32_t)(__builtin_amdgcn_alignbyte(d2, d1, 2) << 8);  // bytes 6..8
                v[3] = (int32_t)(d2 & 0xFFFFFF00u);                            // bytes 9..11
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (int32_t)w[e];
            }
            float f[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = __fmul_rn(__int2float_rn(v[e]), 0x1p-31f);
            const int64_t i = s * DEC_SPAN + 4 * (int64_t)ql - hs;  // index of the quad's first sample
            if (i >= 0 && i + 4 <= n) {
                *reinterpret_cast<float4 *>(out + i) = make_float4(f[0], f[1], f[2], f[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i + e >= 0 && i + e < n) out[i + e] = f[e];
            }
        }
        __syncthreads();  // (the next span overwrites the stage)
    }
}

}  // namespace mm

// Bytes of one input sample of an mm_job.in_kind (0: not a kind).
static inline size_t in_sample_bytes(int kind) {
    switch (kind) {
        case MM_IN_I16: return 2;
        case MM_IN_F32: return 4;
        case MM_IN_I24: return 3;
        case MM_IN_I32: return 4;
        default: return 0;
    }
}

// Queue the decode of n samples of `kind` at d_in (any byte address for MM_IN_I24,
// 4-byte aligned for MM_IN_I32) into n floats at d_out on the context's stream.
static int pcm_decode(mm_ctx *c, int kind, const void *d_in, int64_t n, float *d_out) {
    if (kind != MM_IN_I24 && kind != MM_IN_I32) return set_err(c, MM_ERR_ARG, "pcm decode: kind %d (MM_IN_I24 | MM_IN_I32)", kind);
    if (n < 0 || (n > 0 && (!d_in || !d_out))) return set_err(c, MM_ERR_ARG, "pcm decode: bad arguments");
    if (n >= (int64_t)1 << 40) return set_err(c, MM_ERR_ARG, "pcm decode: %lld samples", (long long)n);
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return set_err(c, MM_ERR_ARG, "pcm decode: output not 4-byte aligned");
    if (kind == MM_IN_I32 && (reinterpret_cast<uintptr_t>(d_in) & 3))
        return set_err(c, MM_ERR_ARG, "pcm decode: 32-bit input not 4-byte aligned");
    if (n == 0) return MM_OK;
    const int64_t hs = (int64_t)((reinterpret_cast<uintptr_t>(d_out) >> 2) & 3);
    const unsigned grid = (unsigned)std::min<int64_t>((hs + n + DEC_SPAN - 1) / DEC_SPAN, DEC_MAX_GRID);
    const unsigned char *in = static_cast<const unsigned char *>(d_in);
    if (kind == MM_IN_I24)
        return launch(c, "pcm_decode", pcm_decode_kernel<3>, dim3(grid), dim3(DEC_THREADS), 0, in, n, d_out);
    return launch(c, "pcm_decode", pcm_decode_kernel<4>, dim3(grid), dim3(DEC_THREADS), 0, in, n, d_out);
}

extern "C" {

int mm_pcm_decode_device(mm_ctx *c, int kind, const void *d_in, int64_t n_samples, float *d_out) {
    if (!c) return MM_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    RET(pcm_decode(c, kind, d_in, n_samples, d_out));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    return MM_OK;
}

int mm_op_pcm_decode(mm_ctx *c, int kind, const void *in, int64_t n, float *out) {
    if (!c) return MM_ERR_ARG;
    const size_t bps = (kind == MM_IN_I24 || kind == MM_IN_I32) ? in_sample_bytes(kind) : 0;
    if (!bps || n < 0 || (n > 0 && (!in || !out))) return set_err(c, MM_ERR_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    char *din;
    float *dout;
    RET(get_buf(c, "op_in", std::max<size_t>((size_t)n * bps, 1), &din));
    RET(get_buf(c, "op_out", (size_t)std::max<int64_t>(n, 1), &dout));
    if (n) HIPCHK(c, hipMemcpyAsync(din, in, (size_t)n * bps, hipMemcpyHostToDevice, c->stream));
    RET(pcm_decode(c, kind, din, n, dout));
    if (n) HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    return MM_OK;
}

int mm_pcm_decode_host(int kind, const void *in, int64_t n, float *out) {
    if ((kind != MM_IN_I24 && kind != MM_IN_I32) || n < 0 || (n > 0 && (!in || !out))) return MM_ERR_ARG;
    const unsigned char *b = static_cast<const unsigned char *>(in);
    for (int64_t i = 0; i < n; ++i) {
        if (kind == MM_IN_I24) {
            const unsigned char *q = b + 3 * i;
            const int32_t s = (int32_t)q[0] | (int32_t)q[1] << 8 | (int32_t)(int8_t)q[2] * 65536;
            out[i] = (float)s * 0x1p-23f;
        } else {
            const unsigned char *q = b + 4 * i;
            const uint32_t u = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
            int32_t s;
            memcpy(&s, &u, 4);
            out[i] = (float)s * 0x1p-31f;  // int -> f32 rounds to nearest even
        }
    }
    return MM_OK;
}

int mm_pcm_decode_span(void) { return DEC_SPAN; }

}  // extern "C"
