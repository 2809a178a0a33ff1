"""mm_op_sosfilt (iir_op_kernel over csrc/lookback.h's tile carry) across tile,
transpose and workgroup seams, at f64 resolution, against tests/iir_model.py's
long-double reference.  The tile T is the test's own: with T = 1, 3, 4 a workgroup
(B = T * 256 / channels frames) is short, so sizes 1, T-1, T, T+1, 16T, 16T+1 (the
transposes' OPS_TILES seam), B-1, B, B+1 (a second workgroup holding one one-frame
tile), 2B+T+1 and 65B+3 are cheap; T = 125, the product's tile, runs B-1, B+1, 3B+5.

What cannot be forced: how deep a block looks back depends on which predecessors
had published when it asked.  65B+3 puts a block more than one look-back window (64
blocks) from the line start, so the second window and the Pw <- Pw * Phi_B^64 update
are reachable; it does not prove they were taken.  Nothing here spins, sleeps or
sets an environment switch to force it.

Exact assertions: a silent channel comes out as exactly 0.0 at every size, whatever
the other channel holds; inside one workgroup (n <= B) the output of x[:n] is the
first n samples of the output of x[:B], bit for bit, and two runs of the same input
are bit-identical.  Neither of the last two is asserted across workgroups: the
look-back's summation order depends on which predecessors had published.

Tolerance without the f32 write-back: the kernel's max-abs error against the
reference may be 8 x the larger of the two modelled extremes' own errors
(iir_model.tolerance; floor 64 ulp of the reference's peak).  error / allowed-base
of every case is recorded ("lbx": the largest over its sizes and signals, gate 8).
With the write-back (R32) a last-bit difference of a carry can move an f32 rounding:
at most 1e-3 of a case's samples may differ from the reference (a cap), none by more
than R32_ULP_BOUND f32 ulps of the reference's peak; the identical share is recorded
("f32").  A rounded cascade runs one section per launch (csrc/ops.hip iir_in_place);
tests/test_iir_model.py shows why one launch cannot meet the cap.

Measured on an MI355X (largest error / model error per filter over all tiles, sizes,
signals and channel counts): techno EQ 1 section 1.29, 2 sections 1.31, 3 sections
1.32, 4 sections 1.77, K-weighting 2.48, 20 Hz shelf 3.22 (the three largest at T = 3,
n = 48 or 49, DC, where the model's own error is 2e-14 to 3e-14); at T = 125 all are
1.00 to 1.12.  R32 identical shares: K-weighting 0.99966 to 0.99994, techno EQ
0.99997 to 1; every differing sample 1.0 f32 ulp of the peak or less.
"""
import ctypes

import numpy as np
import pytest

import iir_model as im
from conftest import record_exact

pytestmark = pytest.mark.gpu

PATHS = ("inclusive", "aggregates")
# Largest deviation of a differing R32 sample, in f32 ulps of the reference's peak:
# measured 1.0 on the first MI355X run (a differing sample is the neighbouring f32
# value, and no case's peak sits just above a power of two), allowed 4 x that.
R32_ULP_BOUND = 4.0


def _filled(sections, T, ch):
    from mastering_amd import native
    from mastering_amd.engine import Job
    iir = native.MMIir()
    Job._fill_iir(iir, sections, [len(sections)], T, im.LB_THREADS // ch)
    return iir


def _call(x, iir, round_f32=False, mix=None):
    """mm_op_sosfilt (or _mix) on contiguous f32/f64 samples [n] or [n, 2]: status, out."""
    from mastering_amd import native
    assert x.flags.c_contiguous and x.dtype in (np.float32, np.float64)
    dt = native.MM_F32 if x.dtype == np.float32 else native.MM_F64
    ch = 2 if x.ndim == 2 else 1
    out = np.full(x.shape, np.nan)
    ctx = native.context(0)
    vp = ctypes.c_void_p
    args = (ctx.ptr, dt, x.ctypes.data_as(vp), x.shape[0], ch, ctypes.byref(iir))
    if mix is None:
        rc = ctx.lib.mm_op_sosfilt(*args, int(round_f32), out.ctypes.data_as(vp))
    else:
        rc = ctx.lib.mm_op_sosfilt_mix(*args, float(mix[0]), float(mix[1]), out.ctypes.data_as(vp))
    return rc, out, ctx


def sosfilt(x, iir, round_f32=False, mix=None):
    rc, out, ctx = _call(x, iir, round_f32, mix)
    ctx.check(rc, "mm_op_sosfilt")
    return out


def _ulp32(v):
    return float(np.spacing(np.float32(v)))


@pytest.mark.parametrize("case", im.seam_cases(), ids=im.case_id)
def test_seams(case):
    name, r32, T, ch = case
    sections = im.filters()[name]
    iir = _filled(sections, T, ch)
    B = im.block_frames(T, ch)
    worst = 0.0
    for sig, f32 in im.runs(case):
        full = im.signal(sig, T, ch, f32)
        x = np.ascontiguousarray(full.astype(np.float32) if f32 else full)
        assert np.array_equal(x.astype(np.float64), full)  # f32 inputs are f32 values
        ref = im.reference(name, r32, sig, T, ch, f32)
        models = [] if r32 else [im.model(name, p, sig, T, ch, f32) for p in PATHS]
        in_block = sosfilt(x[:B], iir, r32)
        differing = total = 0
        for n in im.sizes(T, ch):
            y = sosfilt(x[:n], iir, r32)
            assert y.shape == x[:n].shape and not np.isnan(y).any(), (sig, n)
            if n <= B:  # one workgroup: a prefix of the full block's bits, and reproducible
                assert np.array_equal(y, in_block[:n]), (sig, n)
                assert np.array_equal(y, sosfilt(x[:n], iir, r32)), (sig, n)
            if sig == "noise_silence":
                assert np.all(y[:, 1] == 0.0), (sig, n)
            if sig == "impulse" and n < B - 1:
                assert np.all(y == 0.0), (sig, n)
            r = ref[:n]
            if r32:
                d = np.abs(y.astype(np.longdouble) - r).astype(np.float64)
                differing += int(np.count_nonzero(d))
                total += d.size
                dev = float(d.max()) / _ulp32(np.max(np.abs(r))) if n and float(np.max(np.abs(r))) > 0 else 0.0
                if dev:
                    print(f"{im.case_id(case)} {sig} f32={f32} n={n}: {np.count_nonzero(d)} differ, max {dev:.2f} ulp")
                assert dev <= R32_ULP_BOUND, (sig, n, dev)
            else:
                e = im.err(y, r)
                e_model = max(im.err(m[:n], r) for m in models)
                tol = im.tolerance(r, e_model)
                if tol == 0.0:  # nothing but zeros so far (before the impulse): exact
                    assert e == 0.0, (sig, n)
                    continue
                ratio = e / (tol / 8.0)
                worst = max(worst, ratio)
                if ratio > 2.0:
                    print(f"{im.case_id(case)} {sig} f32={f32} n={n}: error {e:.3e}, model {e_model:.3e}, "
                          f"ratio {ratio:.2f}")
                assert e <= tol, (sig, f32, n, e, e_model, ratio)
        if r32:
            share = differing / total
            print(f"{im.case_id(case)} {sig} f32={f32}: {differing} of {total} samples differ")
            record_exact(1.0 - share, "f32")
            assert share <= 1e-3, (sig, f32, differing, total)
    if not r32:
        print(f"{im.case_id(case)}: largest error / model error {worst:.3f}")
        record_exact(worst, "lbx")


@pytest.mark.parametrize("a,c", im.MIX, ids=["x+c*f", "a*x+c*f"])
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
def test_mix(a, c, f32):
    """mm_op_sosfilt_mix = a * x + c * sosfilt(x), the a * x product in f32 for f32
    samples (mix_a_f32; a == 1.0 takes x itself), against the same expression on the
    reference; the model's paths go through the same expression."""
    T, name = 4, "techno4"
    iir = _filled(im.filters()[name], T, 1)
    B = im.block_frames(T, 1)
    full = im.signal("noise", T, 1, f32)
    x = np.ascontiguousarray(full.astype(np.float32) if f32 else full)
    if a == 1.0:
        ax = full
    elif f32:
        ax = (np.float32(a) * x).astype(np.float64)
        assert ax.dtype == np.float64 and (np.float32(a) * x).dtype == np.float32
    else:
        ax = a * full
    ref = ax.astype(np.longdouble) + np.longdouble(c) * im.reference(name, False, "noise", T, 1, f32)
    models = [ax + im.model(name, p, "noise", T, 1, f32) * c for p in PATHS]
    worst = 0.0
    for n in (B - 1, B + 1, 2 * B + T + 1):
        y = sosfilt(x[:n], iir, mix=(a, c))
        e = im.err(y, ref[:n])
        tol = im.tolerance(ref[:n], max(im.err(m[:n], ref[:n]) for m in models))
        worst = max(worst, e / (tol / 8.0))
        assert e <= tol, (n, e, tol)
    record_exact(worst, "lbx")


@pytest.mark.parametrize("T,ch", [(255, 2), (511, 1)], ids=["T255-stereo", "T511-mono"])
def test_largest_tiles_run(T, ch):
    """The largest tiles whose transposes fit 64 KiB of LDS (16 * (T * ch + 1) * 8
    bytes: 65408 and 65536), at n = 16T + 1, under the seam tests' rule."""
    sections = im.filters()["techno4"]
    n = 16 * T + 1
    x = im.signal("noise", 4, ch, False)[:n].copy()
    ref = im.sos_reference(x, sections)
    e_model = max(im.err(im.lookback_model(x, sections, T, im.LB_THREADS // ch, p), ref) for p in PATHS)
    tol = im.tolerance(ref, e_model)
    y = sosfilt(x, _filled(sections, T, ch))
    e = im.err(y, ref)
    record_exact(e / (tol / 8.0), "lbx")
    assert e <= tol, (e, e_model)


@pytest.mark.parametrize("T,ch", [(256, 2), (512, 1)], ids=["T256-stereo", "T512-mono"])
def test_tiles_past_the_lds_limit_are_refused(T, ch):
    """A tile whose transposes would need more than 64 KiB of LDS is an argument
    error that names the tile, raised before anything is launched; the context stays
    usable."""
    from mastering_amd import native
    sections = im.filters()["techno4"]
    x = im.signal("noise", 4, ch, False)[:16 * T + 1].copy()
    rc, out, ctx = _call(x, _filled(sections, T, ch))
    assert rc == native.MM_ERR_ARG
    msg = ctx.lib.mm_last_error(ctx.ptr).decode()
    assert f"tile {T}" in msg and "LDS" in msg, msg
    assert np.isnan(out).all()  # nothing was written
    ok = _filled(sections, 4, ch)
    y = sosfilt(x, ok)
    assert im.err(y, im.sos_reference(x, sections)) <= 1e-12


def test_loudness_operator_refuses_the_same_tile():
    """mm_op_loudness transposes its mono line with the K-weighting tables' tile: 512
    is refused like mm_op_sosfilt's, 511 runs and gives the product tile's loudness
    (4e-4 LU, the suite's bound between K-weighting tiles)."""
    from mastering_amd import design, native, ops
    from mastering_amd.engine import Job
    rate = 48000
    x = np.ascontiguousarray(im.base_signals()[:rate, 0].astype(np.float32) * np.float32(0.25))
    want = float(ops.integrated_loudness(x, rate))
    ctx = native.context(0)

    def run(tile):
        job = Job(x.shape[0], rate, 1, {"lufs": 0.0}, single_chunk=True)
        Job._fill_iir(job.job.kweight, design.kweight_sections(rate), [2], tile, design.LB_THREADS)
        out = np.zeros(2)
        rc = ctx.lib.mm_op_loudness(ctx.ptr, ctypes.byref(job.job), native.MM_F32, x.ctypes.data_as(ctypes.c_void_p),
                                    out.ctypes.data_as(native.c_double_p))
        return rc, float(out[0])

    rc, _ = run(512)
    assert rc == native.MM_ERR_ARG and "tile 512" in ctx.lib.mm_last_error(ctx.ptr).decode()
    rc, got = run(511)
    ctx.check(rc, "mm_op_loudness")
    assert abs(got - want) <= 4e-4, (got, want)
