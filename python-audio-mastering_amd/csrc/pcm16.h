// pcm16.h — the delivered signal on the int16 grid, once for the stages that work on it
// (meter.hip, ceiling.hip, resample.hip): a buffer of kind MM_OUT_I16 holds int16, one of
// kind MM_OUT_F32 holds int16 / 32768 exactly, interleaved, with 1 or 2 channels.  Device:
// a sample and a frame decoded to ints and encoded back, and the wave reductions of the
// stages' statistics.  Host: the bytes of a sample, the refusal of a (kind, channels,
// frames), the choice of a kernel's instantiation, and for the stages' entries over n tracks
// the tracks' way to the device and back and the refusal of a batch.  Included by
// mastering.hip after ops.hip and before meter.hip.
#pragma once

namespace mm {

template <typename T>
__device__ __forceinline__ int pcm_decode(T v) {
    if constexpr (sizeof(T) == 2) {
        return (int)v;
    } else {  // an MM_OUT_F32 buffer holds int16 / 32768 exactly
        int k = (int)rintf(v * 32768.0f);
        return min(32767, max(-32768, k));
    }
}

// y on the int16 grid (already clipped)
template <typename T>
__device__ __forceinline__ T pcm_encode(int y) {
    if constexpr (sizeof(T) == 2) return (T)y;
    else return (float)y * (1.0f / 32768.0f);
}

// both channels of a stereo frame as one dword, left in the low half
__device__ __forceinline__ uint32_t pack_frame(int l, int r) { return ((uint32_t)l & 0xFFFFu) | ((uint32_t)r << 16); }

// Frame f of an interleaved buffer, its channels as ints (a stereo frame is one aligned
// 4- or 8-byte access); load_frame_packed gives a stereo frame as its dword.
template <int CH, typename T>
__device__ __forceinline__ void load_frame(const T *in, int64_t f, int (&s)[CH]) {
    if constexpr (CH == 2 && sizeof(T) == 2) {
        const uint32_t d = reinterpret_cast<const uint32_t *>(in)[f];
        s[0] = (int16_t)(d & 0xFFFFu);
        s[1] = (int16_t)(d >> 16);
    } else if constexpr (CH == 2) {
        const float2 d = reinterpret_cast<const float2 *>(in)[f];
        s[0] = pcm_decode<float>(d.x);
        s[1] = pcm_decode<float>(d.y);
    } else {
        s[0] = pcm_decode<T>(in[f]);
    }
}

template <typename T>
__device__ __forceinline__ uint32_t load_frame_packed(const T *in, int64_t f) {
    if constexpr (sizeof(T) == 2) return reinterpret_cast<const uint32_t *>(in)[f];
    int s[2];
    load_frame<2, T>(in, f, s);
    return pack_frame(s[0], s[1]);
}

template <int CH, typename T>
__device__ __forceinline__ void store_frame(T *out, int64_t n, const int (&y)[CH]) {
    if constexpr (CH == 2 && sizeof(T) == 2) {
        reinterpret_cast<uint32_t *>(out)[n] = pack_frame(y[0], y[1]);
    } else if constexpr (CH == 2) {
        reinterpret_cast<float2 *>(out)[n] = make_float2(pcm_encode<float>(y[0]), pcm_encode<float>(y[1]));
    } else {
        out[n] = pcm_encode<T>(y[0]);
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int wave_max_i32(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

}  // namespace mm

namespace {

// (as the chain writes it: whatever is not MM_OUT_I16 is float)
size_t pcm_sample_bytes(int kind) { return kind == MM_OUT_I16 ? 2 : 4; }

size_t pcm_bytes(int kind, int64_t frames, int channels) { return (size_t)frames * channels * pcm_sample_bytes(kind); }

bool pcm_kind_ok(int kind) { return kind == MM_OUT_I16 || kind == MM_OUT_F32; }

#define PCM_BAD_KIND "kind %d (MM_OUT_I16 | MM_OUT_F32)"  // (the one reason that prints its argument)

// why (channels, frames) is not a signal a stage takes, or null: frames in [0, limit), the
// caller's own bound, refused in the caller's own words
const char *pcm_refusal(int channels, int64_t frames, int64_t limit, const char *range = "frames out of range") {
    if (channels != 1 && channels != 2) return "channels must be 1 or 2";
    return frames < 0 || frames >= limit ? range : nullptr;
}

// A host signal into the context buffer `name`, queued on the stream; and back, synchronous.
int pcm_upload(mm_ctx *c, const char *name, const void *pcm, size_t bytes, char **d) {
    RET(get_buf(c, name, std::max<size_t>(bytes, 1), d));
    if (bytes) HIPCHK(c, hipMemcpyAsync(*d, pcm, bytes, hipMemcpyHostToDevice, c->stream));
    return MM_OK;
}

int pcm_download(mm_ctx *c, void *pcm, const char *d, size_t bytes) {
    if (bytes) HIPCHK(c, hipMemcpyAsync(pcm, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

// n host tracks into one context buffer, each on a 16-byte boundary: their device pointers
// (pcm null: laid out, nothing copied)
int album_upload(mm_ctx *c, const char *name, const void *const *pcm, int kind, const int64_t *frames, int n, int channels,
                 std::vector<void *> &d) {
    size_t total = 0;
    for (int t = 0; t < n; ++t) total += (pcm_bytes(kind, frames[t], channels) + 15) & ~(size_t)15;
    char *base;
    RET(get_buf(c, name, std::max<size_t>(total, 1), &base));
    d.resize((size_t)n);
    for (int t = 0; t < n; ++t) {
        const size_t bytes = pcm_bytes(kind, frames[t], channels);
        d[(size_t)t] = base;
        if (bytes && pcm) HIPCHK(c, hipMemcpyAsync(base, pcm[t], bytes, hipMemcpyHostToDevice, c->stream));
        base += (bytes + 15) & ~(size_t)15;
    }
    return MM_OK;
}

// d[t] back into pcm[t] for the tracks `pick` names (null: all), synchronous
int batch_download(mm_ctx *c, void *const *pcm, const std::vector<void *> &d, int kind, const int64_t *frames, int n,
                   int channels, const char *pick) {
    for (int t = 0; t < n; ++t) {
        const size_t bytes = pcm_bytes(kind, frames[t], channels);
        if (bytes && (!pick || pick[t])) HIPCHK(c, hipMemcpyAsync(pcm[t], d[(size_t)t], bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MM_OK;
}

// Refuses what is not a batch of n tracks for a stage (MM_ERR_ARG, the sentence in mm_last_error
// names the track), before anything is queued.  rest: the stage's other pointers are there;
// bad(t): why the stage refuses track t, or null.  Every segmented stage counts frames in 32
// bits over the whole launch.
template <typename Bad>
int batch_check(mm_ctx *c, const void *const *pcm, int kind, const int64_t *frames, int n, int channels, bool rest, Bad &&bad) {
    if (n < 1 || n > MM_ALBUM_TRACKS) return set_err(c, MM_ERR_ARG, "batch: %d tracks out of range [1, %d]", n, MM_ALBUM_TRACKS);
    if (!pcm || !frames || !rest) return set_err(c, MM_ERR_ARG, "bad arguments");
    if (!pcm_kind_ok(kind)) return set_err(c, MM_ERR_ARG, PCM_BAD_KIND, kind);
    int64_t total = 0;
    for (int t = 0; t < n; ++t) {
        if (const char *why = bad(t)) return set_err(c, MM_ERR_ARG, "batch: track %d: %s", t, why);
        if (frames[t] > 0 && !pcm[t]) return set_err(c, MM_ERR_ARG, "batch: track %d: null pointer", t);
        total += frames[t];
        if (total >= (int64_t)1 << 31) return set_err(c, MM_ERR_ARG, "batch: track %d: 2^31 frames or more in all", t);
    }
    return MM_OK;
}

// The instantiation of a stage's kernel for a checked (kind, channels): f(ch, t) with the
// channel count as a std::integral_constant and a value of the sample type.
template <typename F>
int dispatch_pcm(int kind, int channels, F &&f) {
    const std::integral_constant<int, 1> mono;
    const std::integral_constant<int, 2> stereo;
    if (kind == MM_OUT_I16) return channels == 2 ? f(stereo, int16_t{}) : f(mono, int16_t{});
    return channels == 2 ? f(stereo, float{}) : f(mono, float{});
}

}  // namespace
