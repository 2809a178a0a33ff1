// wav.hip — the WAV file path of the C-ABI: mm_wav_probe, and the RIFF codec and pinned
// double-buffered staging (wav_job, wav_stream_in, wav_stream_out) that mm_master_wav and
// mm_deliver_wav run around the chain (master_wav in resample.hip).  Included from
// mastering.hip (its context helpers).

extern "C" {

// ------------------------------------------------------------ WAV files
// RIFF/WAVE codec of the file path (replaces pydub/ffmpeg decode, AME:43, and the
// stdlib `wave` export, AME:98), mirroring mastering_amd/wavio.py: integer PCM of
// 16, 24 (packed) or 32 bits or IEEE float32 (WAVE_FORMAT_EXTENSIBLE resolved through
// its subformat; its valid-bits are ignored, samples are left-justified in the
// container; the two wide PCM formats must carry their own block align), the
// last fmt/data chunk wins, a data chunk running past the end of the file is
// truncated to whole frames.
static uint32_t le32(const unsigned char *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }
static uint16_t le16(const unsigned char *p) { return (uint16_t)(p[0] | p[1] << 8); }

static int wav_parse(mm_ctx *c, FILE *f, const char *path, mm_wav_info *info) {
    unsigned char h[40];
    if (fseeko(f, 0, SEEK_END) != 0) return set_err(c, MM_ERR_ARG, "%s: cannot seek", path);
    const int64_t fsize = (int64_t)ftello(f);
    if (fseeko(f, 0, SEEK_SET) != 0 || fread(h, 1, 12, f) != 12 || memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4))
        return set_err(c, MM_ERR_ARG, "%s: not a RIFF/WAVE file", path);
    int64_t pos = 12, data_off = -1, data_size = 0;
    int tag = -1, ch = 0, rate = 0, bits = 0, align = 0;
    while (pos + 8 <= fsize) {
        if (fseeko(f, pos, SEEK_SET) != 0 || fread(h, 1, 8, f) != 8) break;
        const int64_t size = le32(h + 4);
        if (!memcmp(h, "fmt ", 4)) {
            const size_t nb = (size_t)std::min<int64_t>(std::min<int64_t>(size, 40), fsize - pos - 8);
            unsigned char b[40] = {0};
            if (nb < 16 || fread(b, 1, nb, f) != nb) return set_err(c, MM_ERR_ARG, "%s: short fmt chunk", path);
            tag = le16(b);
            ch = le16(b + 2);
            rate = (int)le32(b + 4);
            align = le16(b + 12);
            bits = le16(b + 14);
            if (tag == 0xFFFE && nb >= 26) tag = le16(b + 24);
        } else if (!memcmp(h, "data", 4)) {
            data_off = pos + 8;
            data_size = std::min<int64_t>(size, fsize - data_off);
        }
        pos += 8 + size + (size & 1);
    }
    if (tag < 0 || data_off < 0) return set_err(c, MM_ERR_ARG, "%s: missing fmt or data chunk", path);
    const bool wide = tag == 1 && (bits == 24 || bits == 32);  // decoded by pcm_decode_kernel
    if (!((tag == 1 && bits == 16) || (tag == 3 && bits == 32) || wide))
        return set_err(c, MM_ERR_ARG, "%s: unsupported WAV format tag=%d bits=%d", path, tag, bits);
    if (ch < 1 || rate < 1) return set_err(c, MM_ERR_ARG, "%s: bad fmt chunk (channels %d, rate %d)", path, ch, rate);
    if (wide && align != ch * bits / 8)
        return set_err(c, MM_ERR_ARG, "%s: unsupported WAV format tag=%d bits=%d with block align %d (not %d)", path, tag,
                       bits, align, ch * bits / 8);
    info->frames = data_size / (ch * bits / 8);
    info->data_offset = data_off;
    info->rate = rate;
    info->channels = ch;
    info->format = tag;
    info->bits = bits;
    return MM_OK;
}

int mm_wav_probe(mm_ctx *c, const char *path, mm_wav_info *info) {
    if (!path || !info) return set_err(c, MM_ERR_ARG, "null argument");
    FILE *f = fopen(path, "rb");
    if (!f) return set_err(c, MM_ERR_ARG, "%s: cannot open", path);
    const int rc = wav_parse(c, f, path, info);
    fclose(f);
    return rc;
}

constexpr size_t PIN_CHUNK = (size_t)8 << 20;  // bytes per staging buffer

static int ensure_pinned(mm_ctx *c) {
    for (int b = 0; b < 2; ++b) {
        if (!c->pin[b]) HIPCHK(c, hipHostMalloc((void **)&c->pin[b], PIN_CHUNK, hipHostMallocDefault));
        if (!c->pin_ev[b]) HIPCHK(c, hipEventCreateWithFlags(&c->pin_ev[b], hipEventDisableTiming));
    }
    return MM_OK;
}

namespace {
struct FileCloser {
    FILE *f;
    ~FileCloser() {
        if (f) fclose(f);
    }
};
}  // namespace

// The job of a WAV run: the caller's job with in_kind taken from the parsed file, checked
// against the file's geometry and validated.
static int wav_job(mm_ctx *c, FILE *f, const char *in_path, const mm_job *jin, mm_job *j, mm_wav_info *wi) {
    RET(wav_parse(c, f, in_path, wi));
    *j = *jin;
    j->in_kind = wi->format != 1 ? MM_IN_F32 : wi->bits == 16 ? MM_IN_I16 : wi->bits == 24 ? MM_IN_I24 : MM_IN_I32;
    if (j->frames_in != wi->frames || j->channels != wi->channels || j->rate != wi->rate)
        return set_err(c, MM_ERR_ARG, "%s: job built for %lld frames x %d ch @ %d Hz, file has %lld x %d @ %d", in_path,
                       (long long)j->frames_in, j->channels, j->rate, (long long)wi->frames, wi->channels, wi->rate);
    return validate(c, j);
}

// file -> pinned -> HBM ("host_in"): chunk k is read while chunk k-1 is in flight
static int wav_stream_in(mm_ctx *c, FILE *f, const char *in_path, const mm_job *j, const mm_wav_info *wi, char **d_in_out) {
    // (the packed bytes as they lie in the file: a staging boundary may split a sample)
    const size_t in_bytes = (size_t)wi->frames * wi->channels * in_sample_bytes(j->in_kind);
    char *d_in;
    RET(get_buf(c, "host_in", std::max<size_t>(in_bytes, 1), &d_in));
    RET(ensure_pinned(c));
    if (fseeko(f, wi->data_offset, SEEK_SET) != 0) return set_err(c, MM_ERR_ARG, "%s: cannot seek", in_path);
    size_t k = 0;
    for (size_t off = 0; off < in_bytes; ++k) {
        const int b = (int)(k & 1);
        const size_t n = std::min(PIN_CHUNK, in_bytes - off);
        if (k >= 2) HIPCHK(c, hipEventSynchronize(c->pin_ev[b]));
        if (fread(c->pin[b], 1, n, f) != n) return set_err(c, MM_ERR_ARG, "%s: short read", in_path);
        HIPCHK(c, hipMemcpyAsync(d_in + off, c->pin[b], n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->pin_ev[b], c->stream));
        off += n;
    }
    *d_in_out = d_in;
    return MM_OK;
}

// The 44-byte header, then HBM -> pinned -> file: chunk k is written while chunk k+1 is
// copied back.  Synchronous on return.
static int wav_stream_out(mm_ctx *c, const char *out_path, int out_kind, int channels, int rate, const char *d_out,
                          size_t out_bytes) {
    FileCloser out{fopen(out_path, "wb")};
    if (!out.f) return set_err(c, MM_ERR_ARG, "%s: cannot create", out_path);
    const int tag = out_kind == MM_OUT_I16 ? 1 : 3, bits = out_kind == MM_OUT_I16 ? 16 : 32;
    const int ba = channels * bits / 8;
    unsigned char hdr[44];
    auto put32 = [&](int at, uint32_t v) {
        for (int i = 0; i < 4; ++i) hdr[at + i] = (unsigned char)(v >> (8 * i));
    };
    auto put16 = [&](int at, uint32_t v) {
        hdr[at] = (unsigned char)v;
        hdr[at + 1] = (unsigned char)(v >> 8);
    };
    memcpy(hdr, "RIFF", 4);
    put32(4, (uint32_t)(36 + out_bytes));
    memcpy(hdr + 8, "WAVEfmt ", 8);
    put32(16, 16);
    put16(20, tag);
    put16(22, channels);
    put32(24, rate);
    put32(28, (uint32_t)rate * ba);
    put16(32, ba);
    put16(34, bits);
    memcpy(hdr + 36, "data", 4);
    put32(40, (uint32_t)out_bytes);
    if (fwrite(hdr, 1, 44, out.f) != 44) return set_err(c, MM_ERR_ARG, "%s: write failed", out_path);
    size_t prev_n = 0, k = 0;
    for (size_t off = 0; off < out_bytes; ++k) {
        const int b = (int)(k & 1);
        const size_t n = std::min(PIN_CHUNK, out_bytes - off);
        HIPCHK(c, hipMemcpyAsync(c->pin[b], d_out + off, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(c->pin_ev[b], c->stream));
        if (k >= 1) {
            HIPCHK(c, hipEventSynchronize(c->pin_ev[b ^ 1]));
            if (fwrite(c->pin[b ^ 1], 1, prev_n, out.f) != prev_n) return set_err(c, MM_ERR_ARG, "%s: write failed", out_path);
        }
        prev_n = n;
        off += n;
    }
    if (k >= 1) {
        const int b = (int)((k - 1) & 1);
        HIPCHK(c, hipEventSynchronize(c->pin_ev[b]));
        if (fwrite(c->pin[b], 1, prev_n, out.f) != prev_n) return set_err(c, MM_ERR_ARG, "%s: write failed", out_path);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    return MM_OK;
}

}  // extern "C"
