"""The reference and the model that tests/test_gpu_iir_seams.py holds the look-back
IIR operator against (tests/iir_model.py), checked on the CPU: the reference against
scipy, both model paths and the plain f64 recurrence against the tolerance rule on
every GPU case, the rule against deliberately wrong models, the f32 write-back's
inputs, and design.lookback_tables against long-double powers."""
import numpy as np
import pytest

import iir_model as im

PATHS = ("inclusive", "aggregates")
OFF_CASES = [c for c in im.seam_cases() if not c[1]]
ON_CASES = [c for c in im.seam_cases() if c[1]]


def test_reference_matches_scipy_on_the_preset_eqs():
    """sos_reference (long double) against scipy.signal.sosfilt (f64) on 8192 frames
    of noise, within scipy's own f64 error.  Its scale: a section commits about five
    roundings of half an ulp of its values per frame, four sections, remembered over
    the filters' memory of some hundred frames as a random walk, times the EQs' gain
    of up to 3: sqrt(5 * 4 * 100) / 2 * 3 = 67 ulp of the peak; 256 are allowed
    (measured: techno 30, rock 36, 96 kHz dubstep 65).  And the f64 instance of the
    same loop is scipy's recurrence bit for bit, so that error is scipy's."""
    from scipy.signal import sosfilt

    from mastering_amd import EQ_PRESETS, design
    x = im.base_signals()[:8192, 2:4]
    for rate, preset in [(44100, "techno"), (44100, "rock"), (96000, "dubstep")]:
        sec = design.eq_sections(rate, EQ_PRESETS[preset])
        sos = np.array([[b0, b1, b2, 1.0, a1, a2] for b0, b1, b2, a1, a2 in sec])
        want = sosfilt(sos, x, axis=0)
        ref = im.sos_reference(x, sec)
        assert ref.dtype == np.longdouble and ref.shape == x.shape
        e = im.err(want, ref)
        ulp = 2.0 ** -52 * float(np.max(np.abs(ref)))
        print(f"{preset} {rate}: scipy vs long double {e:.3e} = {e / ulp:.0f} ulp of the peak")
        assert e <= 256 * ulp
        assert np.array_equal(im.sos_reference(x, sec, dtype=np.float64), want)


def test_reference_rounds_every_section_to_f32():
    sec = im.filters()["kweight"]
    x = im.base_signals()[:4096, 0]
    y1 = im.sos_reference(x, sec[:1], round_f32=True)
    assert np.array_equal(y1, y1.astype(np.float32).astype(np.longdouble))
    y = im.sos_reference(x, sec, round_f32=True)
    assert np.array_equal(y, im.sos_reference(y1, sec[1:], round_f32=True))  # two write-back passes
    assert np.array_equal(y, im.reference("kweight", True, "noise", 4, 1, True)[:4096])  # the cached loop
    assert np.array_equal(im.sos_reference(x, sec), im.reference("kweight", False, "noise", 4, 1, True)[:4096])
    assert np.array_equal(im.sos_reference(x, sec, True, np.float64),
                          im.reference("kweight", True, "noise", 4, 1, True, dtype=np.float64)[:4096])
    assert not np.array_equal(y, im.sos_reference(x, sec).astype(np.float32).astype(np.longdouble))


@pytest.mark.parametrize("case", OFF_CASES, ids=im.case_id)
def test_model_paths_and_f64_recurrence_meet_the_rule(case):
    """On every R32-off GPU case and size: each model path is inside the rule (they
    define it), the two paths agree to within it, and so does the sequential f64
    recurrence, i.e. the rule asks nothing f64 arithmetic does not deliver."""
    name, _, T, ch = case
    for sig, f32 in im.runs(case):
        ref = im.reference(name, False, sig, T, ch, f32)
        ms = [im.model(name, p, sig, T, ch, f32) for p in PATHS]
        seq = im.reference(name, False, sig, T, ch, f32, dtype=np.float64)
        for n in im.sizes(T, ch):
            es = [im.err(m[:n], ref[:n]) for m in ms]
            tol = im.tolerance(ref[:n], max(es))
            assert max(es) <= tol
            assert im.err(ms[0][:n], ms[1][:n].astype(np.longdouble)) <= tol, (sig, n)
            assert im.err(seq[:n], ref[:n]) <= tol, (sig, n, im.err(seq[:n], ref[:n]), tol)


def test_model_is_causal():
    """The cached evaluations at the longest size serve the shorter ones: the model of
    x[:n] is the first n samples of the model of x, bit for bit, on both paths."""
    sec = im.filters()["kweight"]
    x = im.signal("noise", 4, 2, False)[:2 * 512 + 5]
    for p in PATHS:
        full = im.lookback_model(x, sec, 4, 128, p)
        for n in (1, 3, 511, 512, 513, 1024 + 4):
            assert np.array_equal(im.lookback_model(x[:n], sec, 4, 128, p), full[:n]), (p, n)


@pytest.mark.parametrize("name", im.R32_OFF)
@pytest.mark.parametrize("ch", [1, 2])
def test_wrong_models_exceed_the_rule_100_times(name, ch):
    """The gate discriminates: Phi_B^(i+1) for Phi_B^i, the two channels' carries
    swapped and t taken as t + 1 each miss the rule by at least 100 x at the sizes
    past one workgroup (measured: 1e5 x for the 20 Hz shelf, 1e9 x and more for the
    others).  The mutations live in the model only."""
    T = 4
    B = im.block_frames(T, ch)
    sec = im.filters()[name]
    for sig, f32 in [("noise", True), ("dc", False), ("impulse", True)]:
        for n in (B + 1, 2 * B + T + 1):
            x = im.signal(sig, T, ch, f32)[:n]
            ref = im.reference(name, False, sig, T, ch, f32)[:n]
            e_model = max(im.err(im.model(name, p, sig, T, ch, f32)[:n], ref) for p in PATHS)
            tol = im.tolerance(ref, e_model)
            for mut in ("blk_pow", "swap", "t_plus_1"):
                if mut == "swap" and ch == 1:
                    continue
                for p in PATHS:
                    e = im.err(im.lookback_model(x, sec, T, im.LB_THREADS // ch, p, mutate=mut), ref)
                    assert e >= 100 * tol, (sig, n, mut, p, e / tol)


@pytest.mark.parametrize("case", ON_CASES, ids=im.case_id)
def test_f32_write_back_inputs_are_unambiguous(case):
    """The R32 cases' inputs: the sequential recurrence with the f32 write-back gives
    the same samples in f64 and in long double, bit for bit, so a GPU sample that
    differs is a carry that moved an f32 rounding, not an ambiguity of the reference."""
    name, _, T, ch = case
    for sig, f32 in im.runs(case):
        n = max(im.sizes(T, ch))
        a = im.reference(name, True, sig, T, ch, f32)[:n]
        b = im.reference(name, True, sig, T, ch, f32, dtype=np.float64)[:n]
        assert np.array_equal(a, b.astype(np.longdouble)), (sig, float(np.mean(a != b)))


def test_one_launch_cannot_carry_the_write_back_but_one_per_section_can():
    """Why a rounded cascade runs one section per launch (csrc/ops.hip iir_in_place):
    with the write-back a later section's input depends non-linearly on the earlier
    sections' carried states, so the tile maps of the whole cascade leave some 5 % of
    the samples one f32 step off (modelled: 7.6 % at T = 4, 4.6 % at T = 125), while
    section-by-section passes leave under 1e-3 (modelled: 7.5e-5)."""
    sec = im.filters()["kweight"]
    n = max(im.sizes(4, 1))
    x = im.signal("noise", 4, 1, True)[:n]
    ref = im.reference("kweight", True, "noise", 4, 1, True)[:n]
    whole = im.lookback_model(x, sec, 4, 256, "inclusive", round_f32=True)
    assert np.mean(whole != ref) > 0.01
    y = x
    for s in sec:
        y = im.lookback_model(y, [s], 4, 256, "aggregates", round_f32=True)
    assert np.mean(y != ref) <= 1e-3


# measured relative errors (max-norm of the difference over max-norm of the long-double
# power) per (filter, T, tpb): tile_pow (largest over k), blk_pow[1], [2], [63], [64];
# None: the power is below 1e-300 (it underflows in f64) and the table holds < 1e-290
TABLE_ERRORS = {
    ("techno1", 125, 256): (2.03e-10, None, None, None, None),
    ("techno1", 125, 128): (2.03e-10, 2.03e-10, None, None, None),
    ("techno1", 4, 256): (3.84e-12, 1.11e-11, 2.04e-11, None, None),
    ("techno1", 4, 128): (3.84e-12, 3.84e-12, 1.11e-11, None, None),
    ("techno2", 125, 256): (2.03e-10, None, None, None, None),
    ("techno2", 125, 128): (2.03e-10, 2.03e-10, None, None, None),
    ("techno2", 4, 256): (3.84e-12, 1.11e-11, 2.04e-11, None, None),
    ("techno2", 4, 128): (3.84e-12, 3.84e-12, 1.11e-11, None, None),
    ("techno3", 125, 256): (2.03e-10, None, None, None, None),
    ("techno3", 125, 128): (2.03e-10, 2.03e-10, None, None, None),
    ("techno3", 4, 256): (3.84e-12, 1.11e-11, 2.04e-11, None, None),
    ("techno3", 4, 128): (3.84e-12, 3.84e-12, 1.11e-11, None, None),
    ("techno4", 125, 256): (2.03e-10, None, None, None, None),
    ("techno4", 125, 128): (2.03e-10, 2.03e-10, None, None, None),
    ("techno4", 4, 256): (3.84e-12, 1.11e-11, 2.04e-11, None, None),
    ("techno4", 4, 128): (3.84e-12, 3.84e-12, 1.11e-11, None, None),
    ("kweight", 125, 256): (2.22e-06, 1.47e-05, 9.31e-05, None, None),
    ("kweight", 125, 128): (2.22e-06, 2.22e-06, 1.47e-05, None, None),
    ("kweight", 4, 256): (3.27e-11, 1.02e-10, 1.94e-09, 1.40e-06, 1.44e-06),
    ("kweight", 4, 128): (3.27e-11, 3.27e-11, 1.02e-10, 1.36e-06, 1.40e-06),
    ("shelf20", 125, 256): (6.35e-07, 7.63e-07, 3.53e-06, None, None),
    ("shelf20", 125, 128): (6.35e-07, 6.35e-07, 7.63e-07, 5.13e-05, 1.60e-04),
    ("shelf20", 4, 256): (1.71e-10, 6.38e-10, 2.73e-09, 1.06e-06, 1.01e-07),
    ("shelf20", 4, 128): (1.71e-10, 1.71e-10, 6.38e-10, 4.22e-07, 7.88e-07),
}


def _ld_pow(M, n):
    out = np.eye(M.shape[0], dtype=np.longdouble)
    sq = M.copy()
    while n:
        if n & 1:
            out = out @ sq
        n >>= 1
        if n:
            sq = sq @ sq
    return out


def _table_errors(name, T, tpb):
    from mastering_amd import design
    sec = im.filters()[name]
    A = design.transition_matrix(list(sec), [len(sec)])
    tabs = design.lookback_tables(A, T, tpb)
    phi = _ld_pow(A.astype(np.longdouble), T)

    def rel(tab, ref):
        m = float(np.max(np.abs(ref)))
        if m < 1e-300:
            assert float(np.max(np.abs(tab))) < 1e-290
            return None
        return float(np.max(np.abs(tab - ref))) / m

    tile = [rel(tabs["tile_pow"][k], _ld_pow(phi, 1 << k)) for k in range(design.TILE_POW)]
    assert all(t is not None for t in tile)
    pb = _ld_pow(phi, tpb)
    return (max(tile),) + tuple(rel(tabs["blk_pow"][e], _ld_pow(pb, e)) for e in (1, 2, 63, 64))


@pytest.mark.parametrize("key", sorted(TABLE_ERRORS), ids=lambda k: f"{k[0]}-T{k[1]}-tpb{k[2]}")
def test_lookback_tables_against_long_double_powers(key):
    """design.lookback_tables (f64 matrix_power and running products) against powers of
    the same one-frame matrix by repeated squaring in long double.  Each entry group
    may be 8 x its measured error (numpy's matmul order may differ between builds).
    Measured, relative to the group's max-norm (techno1..3 are leading blocks of
    techno4 and measure the same; "-" is a power below 1e-300):

    filter   T    tpb  tile_pow  blk_pow[1] blk_pow[2] blk_pow[63] blk_pow[64]
    techno4  125  256  2.0e-10    -          -          -          -
    techno4  125  128  2.0e-10    2.0e-10    -          -          -
    techno4  4    256  3.8e-12    1.1e-11    2.0e-11    -          -
    techno4  4    128  3.8e-12    3.8e-12    1.1e-11    -          -
    kweight  125  256  2.2e-06    1.5e-05    9.3e-05    -          -
    kweight  125  128  2.2e-06    2.2e-06    1.5e-05    -          -
    kweight  4    256  3.3e-11    1.0e-10    1.9e-09    1.4e-06    1.4e-06
    kweight  4    128  3.3e-11    3.3e-11    1.0e-10    1.4e-06    1.4e-06
    shelf20  125  256  6.3e-07    7.6e-07    3.5e-06    -          -
    shelf20  125  128  6.3e-07    6.3e-07    7.6e-07    5.1e-05    1.6e-04
    shelf20  4    256  1.7e-10    6.4e-10    2.7e-09    1.1e-06    1.0e-07
    shelf20  4    128  1.7e-10    1.7e-10    6.4e-10    4.2e-07    7.9e-07

    The large relative figures belong to powers that have decayed to 1e-31 and below
    (K-weighting, T = 125) or sit on poles next to 1 (the 20 Hz shelf): their absolute
    error is what the seam tests see."""
    got = _table_errors(*key)
    want = TABLE_ERRORS[key]
    for g, w in zip(got, want):
        assert (g is None) == (w is None), (got, want)
        if g is not None:
            assert g <= 8 * w, (got, want)
