"""The pointwise operators (pointwise_kernel, csrc/ops.hip) past one trip of their
grid-stride loop, with the special values in it.  Their grid is capped at 4096 blocks
of 256 threads, so 4096 * 256 + 257 elements (frames for the width) send 257 threads
round a second time; the rest of the suite passes at most 16384 elements.  Every
result is compared bit for bit with the oracle's numpy expression (NaN equal to NaN,
the sign of zero through np.signbit); the f32 exciter is bit-exact on the int16 grid
(the table holds numpy's own values) and within 2 ulp off it (device tanhf against
numpy's f32 tanh, as tests/test_ops.py).

The special values sit at the start, at index 4096 * 256 (the first element of the
second trip) and up to the last element: +-0, the smallest subnormal, +-1, +-(1 + ulp),
+-inf, NaN and the limiter's threshold 0.98 (as f32 and as f64) with its neighbours."""
import numpy as np
import pytest

from conftest import record_exact

pytestmark = pytest.mark.gpu

TRIP = 4096 * 256
N = TRIP + 257


def _specials(dtype):
    t = np.dtype(dtype).type
    one, thr = t(1.0), t(0.98)
    tiny = np.nextafter(t(0.0), one)
    up, dn = np.nextafter(thr, one), np.nextafter(thr, t(0.0))
    vals = [0.0, -0.0, tiny, -tiny, one, -one, np.nextafter(one, t(2.0)), -np.nextafter(one, t(2.0)), np.inf, -np.inf,
            np.nan, thr, -thr, up, -up, dn, -dn]
    thr32 = np.float32(0.98)  # the f32 threshold is also an f64 value (and the reverse, rounded, an f32 one)
    vals += [t(thr32), -t(thr32), np.nextafter(t(thr32), one), np.nextafter(t(thr32), t(0.0))]
    return np.array(vals, dtype)


def _sprinkle(flat, spec):
    """spec at the start, from `TRIP` on (scaled to flat's elements per item of the
    operator) and reversed up to the last element."""
    k = len(spec)
    flat[:k] = spec
    at = TRIP * (flat.size // N)
    flat[at:at + k] = spec
    flat[-k:] = spec[::-1]
    flat[flat.size // 2:flat.size // 2 + k] = np.roll(spec, 1)  # shifted: other left/right pairings
    return flat


def _noise(dt, shape, seed):
    """Uniform noise in (-1.2, 1.2), one element in four on the int16 grid, and the
    special values."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.2, 1.2, shape).astype(dt)
    grid = rng.random(shape) < 0.25
    x[grid] = (rng.integers(-32768, 32768, int(grid.sum())).astype(np.float32) / 32768).astype(dt)
    _sprinkle(x.reshape(-1), _specials(dt))
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def samples(request):
    """[N] of the dtype for the elementwise operators."""
    return _noise(request.param, N, 31)


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["f32", "f64"])
def stereo(request):
    """[N, 2] of the dtype for the width: the special values meet each other and
    ordinary samples as left / right pairs."""
    return _noise(request.param, (N, 2), 34)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8]
    assert np.array_equal(np.signbit(got) & (got == 0), np.signbit(want) & (want == 0))  # the sign of zero


def test_pcm_to_float(oracle):
    from mastering_amd import ops
    rng = np.random.default_rng(32)
    q = rng.integers(-32768, 32768, N).astype(np.int16)
    edge = np.array([-32768, 32767, 0, -1, 1], np.int16)
    q[:5], q[TRIP:TRIP + 5], q[-5:] = edge, edge, edge[::-1]
    _same(ops.audio_segment_to_float_array(q), oracle.pcm_to_float(q))


def test_quantize(samples, oracle):
    from mastering_amd import ops
    x = samples.copy()
    with np.errstate(invalid="ignore"):  # NaN -> int16 (0 on the device and here)
        want = oracle.quantize(x)
    got = ops._quantize(x, 0)
    assert got.dtype == np.int16 and np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_stereo_width(stereo, oracle):
    from mastering_amd import ops
    with np.errstate(invalid="ignore", over="ignore"):  # inf - inf
        want = oracle.stereo_width(stereo, 1.3)
    _same(ops.apply_stereo_width(stereo, 1.3), np.ascontiguousarray(want))


def test_soft_limiter(samples, oracle):
    from mastering_amd import ops
    x = samples.copy()
    with np.errstate(invalid="ignore", over="ignore"):  # inf / inf
        want = oracle.soft_limiter(x)
    assert ops.soft_limiter(x) is x
    _same(x, want)
    k = np.abs(want) > 0.98
    assert k.sum() > N // 10 and (~k).sum() > N // 10  # both sides of the knee


def test_gain(samples):
    from mastering_amd import native, ops
    import ctypes
    x = samples.copy()
    g = 10.0 ** (-3.7 / 20.0)
    out = np.empty(x.shape, np.float64)
    ctx = native.context(0)
    dt = native.MM_F32 if x.dtype == np.float32 else native.MM_F64
    ctx.check(ctx.lib.mm_op_gain(ctx.ptr, dt, ops._ptr(x), x.size, float(g), out.ctypes.data_as(ctypes.c_void_p)),
              "mm_op_gain")
    with np.errstate(invalid="ignore", under="ignore"):
        want = x * np.float64(g)
    _same(out, want)


def test_saturation_f32(oracle):
    """apply_saturation on f32: table values on the int16 grid, tanhf off it, and the
    edges of sat_lookup's float -> int conversion: x = 1.0 (k = 32768, past the table:
    tanhf), x = -1.0 (k = -32768, the table's first entry), +-inf, NaN and 1e30 (no
    int holds them: the expression itself)."""
    from mastering_amd import design, ops
    rng = np.random.default_rng(33)
    x = rng.uniform(-1.2, 1.2, N).astype(np.float32)
    grid = rng.random(N) < 0.5
    x[grid] = rng.integers(-32768, 32768, int(grid.sum())).astype(np.float32) / 32768
    edge = np.array([1.0, -1.0, np.inf, -np.inf, np.nan, 1e30, -1e30, 0.0, -0.0, 32767 / 32768, 1.0 + 2.0 ** -23],
                    np.float32)
    _sprinkle(x, edge)
    for pct in (30, 100):
        with np.errstate(invalid="ignore", over="ignore"):
            ref = oracle.saturation(x, pct)
        y = ops.apply_saturation(x, pct)
        assert y.dtype == ref.dtype == np.float32 and y.shape == ref.shape
        on = (x * 32768 == np.trunc(x * 32768)) & (x >= -1) & (x < 1)
        assert 0.4 < on.mean() < 0.6 and on[x == -1.0].all() and not on[x == 1.0].any()
        assert np.array_equal(y[on], ref[on]), np.flatnonzero(on & (y != ref))[:8]
        k = (x[on] * 32768).astype(np.int32)  # the table's own bits (-0.0 is k = 0: the table's +0.0)
        assert np.array_equal(y[on].view(np.uint32), design.saturation_table(pct)[0][k + 32768].view(np.uint32))
        record_exact(np.mean((y == ref) | (np.isnan(y) & np.isnan(ref))), "f32")
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(y), np.isnan(ref)) and np.array_equal(y[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
        ulp = np.spacing(np.abs(ref[fin]))
        d = np.abs(y[fin].astype(np.float64) - ref[fin].astype(np.float64))
        assert np.all(d <= 2 * ulp.astype(np.float64)), float(np.max(d / ulp))
