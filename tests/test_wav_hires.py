"""24- and 32-bit integer PCM on the CPU (no GPU needed): the RIFF parsing of
mm_wav_probe and mastering_amd.wavio.read_wav against scipy.io.wavfile.read, an
independent decoder, on files built here byte by byte, what both refuse, the 16-bit and
float32 behaviour that must not have moved, and mm_pcm_decode_host (the definition of
MM_IN_I24 / MM_IN_I32 restated on the host) against numpy in float64."""
import ctypes
import os
import struct

import numpy as np
import pytest

I24_EDGES = [0x7FFFFF, 0x800000, 0xFFFFFF, 0x000001, 0]           # raw 24-bit words
I32_EDGES = [2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, 2 ** 24 + 3, 0, 1, -1, 0x7FFFFF00, -0x80000000 + 0x100]
GUID_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"


def _probe(path):
    from mastering_amd import native
    lib = native.load()
    info = native.MMWavInfo()
    rc = lib.mm_wav_probe(None, os.fsencode(str(path)), ctypes.byref(info))
    return rc, info


def _sext24(w):
    w = np.asarray(w, dtype=np.int64) & 0xFFFFFF
    return np.where(w >= 0x800000, w - 0x1000000, w)


def _pack24(s):
    """sign-extended 24-bit values -> packed little-endian bytes"""
    u = (np.asarray(s, dtype=np.int64) & 0xFFFFFF).astype(np.uint32).reshape(-1)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


def _wav(path, payload, tag, ch, rate, bits, extensible=False, list_chunk=False, align=None, valid_bits=None,
         data_size=None):
    """A RIFF/WAVE file from raw bytes: a plain 16-byte fmt chunk or a 40-byte
    EXTENSIBLE one, optionally a LIST chunk (odd size, padded) ahead of the data.
    Returns the byte offset of the samples."""
    ba = ch * bits // 8 if align is None else align
    if extensible:
        fmt = struct.pack("<HHIIHH", 0xFFFE, ch, rate, rate * ba, ba, bits)
        fmt += struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, 3 if ch == 2 else 4)
        fmt += struct.pack("<H", tag) + GUID_TAIL
    else:
        fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * ba, ba, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if list_chunk:
        body += b"LIST" + struct.pack("<I", 3) + b"abc\x00"
    body += b"data" + struct.pack("<I", len(payload) if data_size is None else data_size)
    off = 8 + len(body)
    body += payload
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return off


def _samples(bits, n, ch, seed):
    """left-justified int32 samples [n] or [n, ch]: the edge values first, then random"""
    rng = np.random.default_rng(seed)
    if bits == 24:
        s = _sext24(rng.integers(0, 1 << 24, n * ch))
        s[:len(I24_EDGES)] = _sext24(I24_EDGES)
        payload, left = _pack24(s), (s << 8).astype(np.int32)
    else:
        s = rng.integers(-2 ** 31, 2 ** 31, n * ch, dtype=np.int64)
        s[:len(I32_EDGES)] = I32_EDGES
        left = s.astype(np.int32)
        payload = left.astype("<i4").tobytes()
    return payload, (left.reshape(n, ch) if ch > 1 else left)


CASES = [(bits, ch, ext, lst) for bits in (24, 32) for ch in (1, 2) for ext, lst in ((False, False), (True, True))]


@pytest.mark.parametrize("bits,ch,ext,lst", CASES)
def test_read_and_probe_match_scipy(tmp_path, bits, ch, ext, lst):
    from scipy.io import wavfile
    from mastering_amd import wavio
    n = 257
    payload, want = _samples(bits, n, ch, seed=bits + ch)
    p = tmp_path / "x.wav"
    off = _wav(str(p), payload, 1, ch, 48000, bits, extensible=ext, list_chunk=lst)
    got, rate = wavio.read_wav(str(p))
    assert rate == 48000 and got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    r2, ref = wavfile.read(str(p))
    assert r2 == 48000 and ref.dtype == np.int32 and np.array_equal(got, ref)
    rc, info = _probe(p)
    assert rc == 0
    assert (info.format, info.bits, info.frames, info.rate, info.channels) == (1, bits, n, 48000, ch)
    assert info.data_offset == off == 12 + 8 + (40 if ext else 16) + (12 if lst else 0) + 8


def test_extensible_valid_bits_are_ignored(tmp_path):
    """20 valid bits in a 24-bit container: the samples are left-justified in the
    container, which is decoded whole."""
    from mastering_amd import wavio
    payload, want = _samples(24, 64, 2, seed=5)
    p = tmp_path / "v20.wav"
    _wav(str(p), payload, 1, 2, 44100, 24, extensible=True, valid_bits=20)
    got, _ = wavio.read_wav(str(p))
    assert np.array_equal(got, want)
    rc, info = _probe(p)
    assert rc == 0 and (info.format, info.bits, info.frames) == (1, 24, 64)


@pytest.mark.parametrize("bits,ch", [(24, 1), (24, 2), (32, 2)])
def test_data_chunk_cut_mid_frame_is_truncated(tmp_path, bits, ch):
    from mastering_amd import wavio
    n = 100
    payload, want = _samples(bits, n, ch, seed=9)
    fb = ch * bits // 8
    # the chunk claims n frames, the file ends 2 bytes into frame n - 3
    p = tmp_path / "cut.wav"
    _wav(str(p), payload[:(n - 3) * fb + 2], 1, ch, 44100, bits, data_size=n * fb)
    got, _ = wavio.read_wav(str(p))
    assert got.shape[0] == n - 3 and np.array_equal(got, want[:n - 3])
    rc, info = _probe(p)
    assert rc == 0 and info.frames == n - 3
    # and a chunk whose own size is no whole number of frames
    q = tmp_path / "odd.wav"
    _wav(str(q), payload[:10 * fb + 1] + b"\x00", 1, ch, 44100, bits, data_size=10 * fb + 1)
    got, _ = wavio.read_wav(str(q))
    assert got.shape[0] == 10 and np.array_equal(got, want[:10])
    rc, info = _probe(q)
    assert rc == 0 and info.frames == 10


def _rejected(path):
    from mastering_amd import wavio
    assert _probe(path)[0] < 0, path
    with pytest.raises(ValueError):
        wavio.read_wav(str(path))


def test_rejections(tmp_path):
    pay24 = bytes(3 * 2 * 10)
    p = tmp_path / "r.wav"
    for ch, align in ((2, 4), (2, 8), (1, 4), (1, 2)):  # 24-bit with a block align that is not ch * 3
        _wav(str(p), pay24, 1, ch, 44100, 24, align=align)
        _rejected(p)
        _wav(str(p), pay24, 1, ch, 44100, 24, align=align, extensible=True)
        _rejected(p)
    _wav(str(p), bytes(4 * 2 * 10), 1, 2, 44100, 32, align=4)  # 32-bit PCM with the 16-bit block align
    _rejected(p)
    _wav(str(p), bytes(20), 1, 2, 44100, 8)    # 8-bit PCM
    _rejected(p)
    _wav(str(p), pay24, 3, 2, 44100, 24)       # "float" of 24 bits
    _rejected(p)
    _wav(str(p), bytes(8 * 2 * 10), 3, 2, 44100, 64)  # float64
    _rejected(p)
    _wav(str(p), bytes(8 * 2 * 10), 3, 2, 44100, 64, extensible=True)
    _rejected(p)
    for bits in (24, 32):                      # no channels
        _wav(str(p), pay24, 1, 0, 44100, bits, align=bits // 8)
        _rejected(p)
        _wav(str(p), pay24, 1, 0, 44100, bits, align=0)
        _rejected(p)


def test_pcm16_and_float32_read_as_before(tmp_path):
    """The two formats the engine always took: same samples, same probe, and no
    block-align check on them (a wrong nBlockAlign is accepted, as it always was)."""
    from mastering_amd import wavio
    rng = np.random.default_rng(2)
    x16 = rng.integers(-32768, 32768, (301, 2)).astype(np.int16)
    xf = rng.uniform(-1, 1, (301, 2)).astype(np.float32)
    m16 = rng.integers(-32768, 32768, 77).astype(np.int16)
    for x, tag, bits in ((x16, 1, 16), (xf, 3, 32), (m16, 1, 16)):
        ch = 1 if x.ndim == 1 else x.shape[1]
        for kw in ({}, {"align": 1}, {"align": 6}, {"extensible": True, "list_chunk": True},
                   {"extensible": True, "align": 3}):
            p = tmp_path / "old.wav"
            off = _wav(str(p), x.tobytes(), tag, ch, 22050, bits, **kw)
            got, rate = wavio.read_wav(str(p))
            assert rate == 22050 and got.dtype == x.dtype and np.array_equal(got, x), kw
            rc, info = _probe(p)
            assert rc == 0, kw
            assert (info.format, info.bits, info.frames, info.rate, info.channels, info.data_offset) == \
                (tag, bits, x.shape[0], 22050, ch, off), kw
    # written by the package's own writer: the canonical 44-byte header
    p = tmp_path / "w.wav"
    wavio.write_wav(str(p), x16, 48000)
    rc, info = _probe(p)
    assert rc == 0 and (info.format, info.bits, info.frames, info.data_offset) == (1, 16, 301, 44)
    assert np.array_equal(wavio.read_wav(str(p))[0], x16)
    with pytest.raises(TypeError):
        wavio.write_wav(str(p), x16.astype(np.int32), 48000)  # writing wide PCM stays out of scope


def _decode_host(kind, raw, n):
    from mastering_amd import native
    lib = native.load()
    raw = np.ascontiguousarray(raw)
    out = np.full(n + 8, np.nan, np.float32)
    rc = lib.mm_pcm_decode_host(kind, raw.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    assert np.isnan(out[n:]).all()
    return out[:n]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_decode_host_is_the_numpy_definition():
    from mastering_amd import native
    rng = np.random.default_rng(11)
    n = 1 << 20
    # I32: (s / 2^31) rounded once to f32
    s32 = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64)
    s32[:len(I32_EDGES)] = I32_EDGES
    s32[100:200] = (1 << 24) + np.arange(100)          # ties and near-ties of the int -> f32 conversion
    s32[200:300] = -(1 << 25) - np.arange(100)
    s32 = s32.astype(np.int32)
    want = (s32.astype(np.float64) / 2 ** 31).astype(np.float32)
    got = _decode_host(native.MM_IN_I32, s32, n)
    assert np.array_equal(_bits(got), _bits(want))
    assert got[0] == 1.0 and got[1] == -1.0            # INT32_MAX, INT32_MIN
    assert _bits(got[2:4]).tolist() == _bits(np.float32([2.0 ** -7, (2.0 ** 24 + 4) / 2.0 ** 31])).tolist()
    # I24: s / 2^23, exact
    s24 = _sext24(rng.integers(0, 1 << 24, n))
    s24[:len(I24_EDGES)] = _sext24(I24_EDGES)
    raw = np.frombuffer(_pack24(s24), np.uint8)
    want24 = (s24.astype(np.float64) / 2 ** 23).astype(np.float32)
    assert np.array_equal(want24.astype(np.float64) * 2 ** 23, s24)  # (exact: every 24-bit integer is an f32)
    got24 = _decode_host(native.MM_IN_I24, raw, n)
    assert np.array_equal(_bits(got24), _bits(want24))
    assert got24[:5].tolist() == [(2 ** 23 - 1) / 2 ** 23, -1.0, -(2.0 ** -23), 2.0 ** -23, 0.0]
    # the same samples left-justified in an int32 decode to the same floats
    left = (s24 << 8).astype(np.int32)
    assert np.array_equal(_bits(_decode_host(native.MM_IN_I32, left, n)), _bits(got24))
    # packed bytes at an odd address
    odd = np.empty(raw.size + 1, np.uint8)
    odd[1:] = raw
    assert np.array_equal(_bits(_decode_host(native.MM_IN_I24, odd[1:], 4099)), _bits(want24[:4099]))


def test_decode_host_arguments():
    from mastering_amd import native
    lib = native.load()
    out = np.zeros(4, np.float32)
    po = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.mm_pcm_decode_host(native.MM_IN_I24, None, 0, None) == 0      # n = 0
    assert lib.mm_pcm_decode_host(native.MM_IN_I32, None, 0, po) == 0
    assert lib.mm_pcm_decode_host(native.MM_IN_I32, None, 1, po) == native.MM_ERR_ARG
    assert lib.mm_pcm_decode_host(native.MM_IN_I16, po, 1, po) == native.MM_ERR_ARG  # not a wide kind
    assert lib.mm_pcm_decode_host(native.MM_IN_I24, po, -1, po) == native.MM_ERR_ARG
    assert lib.mm_pcm_decode_span() >= 64 and lib.mm_pcm_decode_span() % 4 == 0
    assert (native.MM_IN_I24, native.MM_IN_I32) == (2, 3)


def test_engine_input_kinds():
    """master_pcm takes int32 (left-justified wide PCM); the meter and the ceiling stay
    on the int16 grid and refuse it, as does every other dtype everywhere."""
    from mastering_amd import engine, native
    x = np.zeros((8, 2), np.int32)
    assert engine._device_input(x, wide=True)[1] == native.MM_IN_I32
    assert engine._device_input(x.astype(np.int16), wide=True)[1] == native.MM_IN_I16
    assert engine._device_input(x.astype(np.float32), wide=True)[1] == native.MM_IN_F32
    with pytest.raises(TypeError):
        engine._device_input(x)
    with pytest.raises(TypeError):
        engine._device_input(x.astype(np.int64), wide=True)
    with pytest.raises(TypeError):
        engine.meter_pcm(x, 44100)
    with pytest.raises(TypeError):
        engine.ceiling_pcm(x, 44100, -1.0)
