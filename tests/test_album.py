"""An album levelled as one programme, on CPU: the pooled R 128 figures (mm_r128_album_from_hops)
and the host restatement of the album level (mm_album_level_host) against fifty lines of numpy
written from the definition in include/mastering.h on top of the single-track definitions of
test_level.py and test_r128.py, the properties of the pooling, and the Python refusals that
need no GPU.  Samples and integers are compared for equality; loudness within 1e-6 LU."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_ceiling import GUARD, ONE, q28
from test_level import PASSES, SMIN, STATUS, TOL, pink, q, ref_gain, ref_pass
from test_r128 import FIGURES, design_rate, from_hops, level, ref_hops, same, stepped_noise, windows

RATE = 44100
COUNTS = ("hops", "momentary_blocks", "short_term_blocks", "lra_blocks")


# ------------------------------------------------------------ the definition, in numpy
def ref_album_r128(es, rate):
    """The album R 128 figures of the tracks' hop energies `es`: the windows of every track on
    its own, pooled in track order, then mm_r128's gates and percentiles on the pools.  Also
    the pooled block levels and the gates, for the tests' margins."""
    r = {f: math.nan for f in FIGURES}
    r.update(hops=sum(len(e) for e in es), lra_blocks=0, levels=[], gates=[])
    pool = {}
    for w in (4, 30):
        zl = [windows(np.asarray(e, np.float64), rate, w) for e in es]
        pool[w] = np.concatenate([z for z, _ in zl]), np.concatenate([l for _, l in zl])
    (z, l), (zs, ls) = pool[4], pool[30]
    r.update(momentary_blocks=len(l), short_term_blocks=len(ls), levels=list(l) + list(ls))
    if len(l):
        r["momentary_max"], r["integrated"] = l.max(), -math.inf
        if (l > -70).any():
            gate = r["relative_gate"] = level(z[l > -70].mean()) - 10.0
            r["integrated"] = level(z[(l > -70) & (l > gate)].mean())
            r["gates"].append(gate)
    if len(ls):
        r["short_term_max"], r["lra"] = ls.max(), 0.0
        if (ls > -70).any():
            gate = level(zs[ls > -70].mean()) - 20.0
            r["gates"].append(gate)
            k = np.sort(ls[(ls > -70) & (ls > gate)])
            n = r["lra_blocks"] = len(k)
            r["lra_low"], r["lra_high"] = k[((n - 1) * 10 + 50) // 100], k[((n - 1) * 95 + 50) // 100]
            r["lra"] = r["lra_high"] - r["lra_low"]
    return r


def album_margin(r):
    """The smallest distance of a finite pooled block level from -70 or from a relative gate."""
    l = np.array([v for v in r["levels"] if math.isfinite(v)])
    return min(np.abs(l - g).min() for g in [-70.0] + r["gates"]) if len(l) else math.inf


def ref_album_level(tracks, rate, T, C, W, gains=None):
    """The album level: (delivered tracks, stats).  `gains`: replay exactly these pass gains
    without deciding anything (the last pass is delivered)."""
    tracks = [np.asarray(t) for t in tracks]

    def measure(ts):
        return ref_album_r128([ref_hops(t, rate) for t in ts], rate)

    src = measure(tracks)
    st = dict(status="unmeasurable", passes=0, gain_q16=ONE, pass_gain_q16=[], pass_lufs=[], loudness=math.nan,
              source_lufs=float(src["integrated"]), clipped=0, min_gain_q16=ONE, limited_frames=0, margins=[], slopes=[],
              gate_margins=[album_margin(src)], frames=sum(len(t) for t in tracks))
    if not math.isfinite(st["source_lufs"]):
        out = [t.copy() for t in tracks]
        if C:
            done = [ref_pass(t, ONE, C, W) for t in tracks]  # (gain by ONE is the identity: the ceiling alone)
            out = [d[0] for d in done]
            st.update(min_gain_q16=min(d[4]["min_gain_q16"] for d in done),
                      limited_frames=sum(d[4]["limited_frames"] for d in done))
        return out, st
    peak = max(int(np.abs(t.astype(np.int64)).max()) for t in tracks if len(t))
    g, st["status"] = q(10.0 ** ((T - st["source_lufs"]) / 20.0)), None
    for k in range(PASSES if gains is None else len(gains)):
        g, capped = g if gains is None else gains[k], False
        cap = min((32767 << 16) // peak, 1 << 21) if not C else ((C - GUARD) << 16) >> 24 if g > ONE else g
        g, capped = (cap, True) if g > cap else (g, False)
        done = [ref_pass(t, g, C, W) for t in tracks]  # (g is under every track's own cap: none caps again)
        assert all(d[1] == g and not d[2] for d in done)
        out, r = [d[0] for d in done], None
        r = measure(out)
        st["pass_gain_q16"].append(g)
        st["pass_lufs"].append(float(r["integrated"]))
        st["gate_margins"].append(album_margin(r))
        st.update(passes=k + 1, gain_q16=g, loudness=st["pass_lufs"][k], clipped=sum(d[3] for d in done), r128=r)
        if C:
            st.update(min_gain_q16=min(d[4]["min_gain_q16"] for d in done),
                      limited_frames=sum(d[4]["limited_frames"] for d in done))
        if gains is not None:
            continue
        I, d = st["pass_lufs"], [20.0 * math.log10(v / 65536.0) for v in st["pass_gain_q16"]]
        m = (I[k] - I[k - 1]) / (d[k] - d[k - 1]) if k >= 1 and d[k] != d[k - 1] else None
        st["margins"].append(abs(abs(T - I[k]) - TOL))
        st["slopes"] += [] if m is None else [abs(m - SMIN)]
        st["status"] = ("reached" if abs(T - I[k]) <= TOL else "capped" if capped else
                        "saturated" if m is not None and m < SMIN else "passes" if k == PASSES - 1 else None)
        if st["status"]:
            break
        g = q((g / 65536.0) * 10.0 ** ((T - I[k]) / (20.0 * (1.0 if m is None else min(m, 1.0)))))
    return out, st


# ------------------------------------------------------------ the library
def album_from_hops(es, rate):
    from mastering_amd import native
    e = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64) for x in es]) if es else np.zeros(0))
    th = (ctypes.c_int64 * len(es))(*[len(x) for x in es])
    m = native.MMR128()
    assert native.load().mm_r128_album_from_hops(e.ctypes.data_as(native.c_double_p), th, len(es), rate, ctypes.byref(m)) == 0
    return m


def host_album_level(tracks, rate, T, C, W):
    """(delivered tracks, mm_level, album mm_r128, per-track mm_r128s, per-track mm_ceilings) of
    mm_album_level_host."""
    from mastering_amd import design, engine, native
    xs = [np.array(t, np.int16, order="C") for t in tracks]  # copies: the call works in place
    n = len(xs)
    I16P = ctypes.POINTER(ctypes.c_int16)
    ptrs = (I16P * n)(*[x.ctypes.data_as(I16P) for x in xs])
    frames = (ctypes.c_int64 * n)(*[x.shape[0] for x in xs])
    m, alb, tr, ce = native.MMLevel(), native.MMR128(), (native.MMR128 * n)(), (native.MMCeiling * n)()
    rc = native.load().mm_album_level_host(ptrs, frames, n, 1 if xs[0].ndim == 1 else xs[0].shape[1], rate,
                                           engine.kweight_sos(design_rate(rate)), design.level_clu(T), C, W,
                                           ctypes.byref(m), ctypes.byref(alb), tr, ce)
    assert rc == 0
    return xs, m, alb, list(tr), list(ce)


# ------------------------------------------------------------ the albums
def album_q(ch):
    return [pink(2, ch, -20, 1), pink(1.5, ch, -30, 2), ref_gain(stepped_noise(int(1.7 * RATE), RATE, ch), 1 << 15)[0],
            pink(0.3, ch, -18, 5)]


def album_l():
    return [pink(2, 2, -12, 1), pink(1.5, 2, -24, 2), stepped_noise(int(1.7 * RATE), RATE, 2), pink(0.3, 2, -10, 5)]


def album_h():
    return [stepped_noise(3 * RATE, RATE, 2), pink(2, 2, -9, 1), pink(0.3, 2, -10, 5), pink(1.5, 2, -24, 2)]


def album_fates():
    """(tracks, rate, target, C, W): a stereo album at 8 kHz that boosts, with tracks of different
    fates in one pass: 2 s that the inner ceiling limits, 2 s that it does not touch, a track
    three frames longer than one span of the ceiling, 0.3 s (no window of its own) and an empty
    track.  test_the_fates_album_is_what_its_name_says asserts all of that on the host."""
    from mastering_amd import native
    from mastering_amd.synth import pink_noise_pcm16
    rate, n = 8000, native.load().mm_ceiling_span() + 3
    tracks = [pink(2, 2, -14, 31, rate), pink(2, 2, -40, 32, rate), pink_noise_pcm16(n, rate, 2, track=33, level_dbfs=-16.0),
              pink(0.3, 2, -14, 34, rate), np.zeros((0, 2), np.int16)]
    return tracks, rate, -10.0, q28(-1.0), 40


def case_inputs():
    """name -> (tracks, target, C, W, status, passes): the outcomes are those of the rule's numpy
    prototype on these albums (asserted on ref_album_level itself in `refs`)."""
    C = q28(-1.0)
    return {
        "cut": (album_l(), -15.0, C, 220, "reached", 1),
        "hot-cut": (album_h(), -9.0, C, 220, "saturated", 3),
        "boost-2": (album_q(2), -12.0, C, 220, "reached", 2),
        "boost-3": (album_q(2), -11.0, C, 220, "reached", 3),
        "saturated": (album_q(2), -8.0, C, 220, "saturated", 2),
        "mono": (album_q(1), -13.0, C, 220, "reached", 3),
        "no-ceiling": (album_q(2), -8.0, 0, 220, "capped", 1),
        "unmeasurable": ([pink(0.3, 2, -10, 5), pink(0.39, 2, -12, 1)], -14.0, C, 220, "unmeasurable", 0),
    }


NAMES = ["cut", "hot-cut", "boost-2", "boost-3", "saturated", "mono", "no-ceiling", "unmeasurable"]


@pytest.fixture(scope="module")
def cases():
    return case_inputs()


@pytest.fixture(scope="module")
def refs(cases):
    """ref_album_level of every case (shared, read-only), with the conditions that keep every
    decision of the rule and every gate stable against the 1e-6 LU by which two correct meters
    may differ."""
    out = {}
    for name, (tracks, T, C, W, status, passes) in cases.items():
        y, st = ref_album_level(tracks, RATE, T, C, W)
        print(name, st["status"], st["passes"], st["pass_gain_q16"], [round(v, 4) for v in st["pass_lufs"]],
              "source", round(st["source_lufs"], 4), "margins", st["margins"], st["slopes"], min(st["gate_margins"]))
        assert st["status"] == status and st["passes"] == passes, name
        assert min(st["margins"], default=1.0) >= 1e-3, name
        assert min(st["slopes"], default=1.0) >= 0.01, name
        assert min(st["gate_margins"]) >= 1e-3, name
        assert min(len(t) for t in tracks) < 0.4 * RATE, name  # every album holds a track without a window
        out[name] = (y, st)
    return out


# ------------------------------------------------------------ the pooled figures
def test_one_track_is_from_hops_bit_for_bit():
    for n, rate in ((0, 48000), (3, 48000), (4, 44100), (29, 44100), (30, 2000), (400, 44100)):
        e = ref_hops(stepped_noise(n * rate // 10 + 7, rate, 2), rate) if n else np.zeros(0)
        assert len(e) == n
        assert bytes(album_from_hops([e], rate)) == bytes(from_hops(e, rate)), n


def test_against_the_numpy_definition():
    es = [ref_hops(t, RATE) for t in album_h()] + [np.zeros(0), ref_hops(stepped_noise(5 * RATE, RATE, 1, seed=5), RATE)]
    m, r = album_from_hops(es, RATE), ref_album_r128(es, RATE)
    assert album_margin(r) >= 1e-3
    for f in COUNTS:
        assert getattr(m, f) == r[f], f
    for f in FIGURES:
        assert math.isfinite(r[f]) and same(getattr(m, f), r[f], 1e-9), f
    assert m.frames == 0 and m.channels == 0 and m.rate == RATE


def test_no_window_spans_two_tracks():
    e = ref_hops(stepped_noise(4 * RATE, RATE, 2), RATE)
    assert len(e) == 40
    m = album_from_hops([e[:7], e[7:]], RATE)
    assert (m.hops, m.momentary_blocks, m.short_term_blocks) == (40, 4 + 30, 0 + 4)
    whole = from_hops(e, RATE)
    assert (whole.momentary_blocks, whole.short_term_blocks) == (37, 11)
    r = ref_album_r128([e[:7], e[7:]], RATE)
    for f in FIGURES:
        assert same(getattr(m, f), r[f], 1e-9), f


def test_order_and_pooling():
    a = ref_hops(stepped_noise(4 * RATE, RATE, 2), RATE)
    b = ref_hops(pink(3.5, 2, -20, 3), RATE)
    short = ref_hops(pink(0.3, 2, -3, 4), RATE)
    assert len(short) == 3
    ab, asb = album_from_hops([a, b], RATE), album_from_hops([a, short, b], RATE)
    assert asb.hops == ab.hops + 3
    asb.hops = ab.hops
    assert bytes(asb) == bytes(ab)  # a track without a window changes nothing but `hops`
    one, twice = from_hops(a, RATE), album_from_hops([a, a], RATE)
    assert abs(twice.integrated - one.integrated) <= 1e-12 and abs(twice.lra - one.lra) <= 1e-12
    assert (twice.momentary_blocks, twice.lra_blocks) == (2 * one.momentary_blocks, 2 * one.lra_blocks)
    ba = album_from_hops([b, a], RATE)
    for f in FIGURES:
        assert abs(getattr(ba, f) - getattr(ab, f)) <= 1e-12, f
    for f in COUNTS:
        assert getattr(ba, f) == getattr(ab, f), f


def test_nothing_to_pool():
    m = album_from_hops([np.ones(3), np.zeros(0), np.ones(2)], RATE)
    assert m.hops == 5 and m.momentary_blocks == 0 and all(math.isnan(getattr(m, f)) for f in FIGURES)
    m = album_from_hops([np.zeros(10), np.zeros(4)], RATE)  # silence: windows, none above -70
    assert m.momentary_blocks == 8 and m.integrated == -math.inf and math.isnan(m.relative_gate)


def test_from_hops_refusals():
    from mastering_amd import native
    lib, m = native.load(), native.MMR128()
    e = np.ones(8)
    p, ok = e.ctypes.data_as(native.c_double_p), (ctypes.c_int64 * 2)(4, 4)
    assert lib.mm_r128_album_from_hops(p, ok, 2, RATE, ctypes.byref(m)) == 0
    assert lib.mm_r128_album_from_hops(p, ok, 0, RATE, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_album_from_hops(p, (ctypes.c_int64 * 257)(), 257, RATE, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_album_from_hops(p, (ctypes.c_int64 * 2)(4, -1), 2, RATE, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_album_from_hops(None, ok, 2, RATE, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_album_from_hops(p, None, 2, RATE, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_album_from_hops(p, ok, 2, 1999, ctypes.byref(m)) == native.MM_ERR_ARG
    assert lib.mm_r128_album_from_hops(p, ok, 2, RATE, None) == native.MM_ERR_ARG


def test_from_hops_is_what_it_was():
    """mm_r128_from_hops on the inputs of test_r128.py (the stepped noises of its hop cases
    and the EBU sines): the bytes of the struct recorded before its tail moved into the helper
    the album shares."""
    with open(os.path.join(GOLDEN, "r128_from_hops.json")) as f:
        d = json.load(f)
    assert len(d) == 14
    for name, rec in d.items():
        m = from_hops(np.array([float.fromhex(v) for v in rec["hops"]]), rec["rate"])
        assert bytes(m).hex() == rec["mm_r128"], name


# ------------------------------------------------------------ the album level
@pytest.mark.parametrize("name", NAMES)
def test_host_restatement(cases, refs, name):
    from test_meter import ref_meter
    tracks, T, C, W, _, _ = cases[name]
    want, st = refs[name]
    got, m, alb, tr, ce = host_album_level(tracks, RATE, T, C, W)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert m.status == STATUS[st["status"]] and m.passes == st["passes"]
    for k in range(m.passes):
        assert abs(m.pass_gain_q16[k] - st["pass_gain_q16"][k]) <= 1, k
    ch = tracks[0].reshape(len(tracks[0]), -1).shape[1]
    assert (m.frames, m.channels, m.rate, m.target_clu, m.ceiling_q28, m.window) == (st["frames"], ch, RATE, round(100 * T), C, W)
    # the reference again with the library's recorded gains: the same bytes and figures
    gains = [int(m.pass_gain_q16[k]) for k in range(m.passes)]
    again, rst = ref_album_level(tracks, RATE, T, C, W, gains)
    assert all(np.array_equal(g, a) for g, a in zip(got, again))
    for k in range(m.passes):
        assert abs(m.pass_lufs[k] - rst["pass_lufs"][k]) <= 1e-6, k
    assert all(math.isnan(m.pass_lufs[k]) and m.pass_gain_q16[k] == 0 for k in range(m.passes, PASSES))
    assert same(m.source_lufs, rst["source_lufs"], 1e-6) and same(m.loudness, rst["loudness"], 1e-6)
    assert (m.clipped, m.min_gain_q16, m.limited_frames) == (rst["clipped"], rst["min_gain_q16"], rst["limited_frames"])
    if m.passes:
        assert m.gain_q16 == gains[-1] and m.loudness == m.pass_lufs[m.passes - 1]
    if st["status"] == "reached":
        assert abs(m.loudness - T) <= TOL
    # the reports describe what was delivered: the album's, and every track's own
    r = ref_album_r128([ref_hops(g, RATE) for g in got], RATE)
    assert (alb.frames, alb.channels, alb.rate) == (st["frames"], ch, RATE)
    for f in COUNTS:
        assert getattr(alb, f) == r[f], f
    for f in FIGURES:
        assert same(getattr(alb, f), r[f], 1e-6), f
    if m.passes:
        assert alb.integrated == m.loudness
    from test_r128 import host_r128
    for t, g in enumerate(got):
        assert bytes(tr[t]) == bytes(host_r128(g, RATE)[1]), t
        if C:  # every track's true peak is mm_ceiling's own guarantee, and the struct is the final call's
            tp = max(ref_meter(g)["true_peak_q28"])
            assert tp <= C and ce[t].tp_out_q28 == tp and ce[t].ceiling_q28 == C and ce[t].frames == len(g), t
    if not C:
        assert m.clipped == 0 and all(np.array_equal(g, ref_gain(t, int(m.gain_q16))[0]) for g, t in zip(got, tracks))


def test_the_library_takes_every_branch(cases, refs):
    """The branches on mm_album_level_host's own results (the reference's, which `refs` pins to
    the table, agree with them pass by pass in test_host_restatement).  "hot-cut" is a cut whose
    limiter bites so hard that the secant steps past ONE on its third pass: two passes on the
    g <= ONE branch, the delivered one behind the limiter."""
    lib = {name: host_album_level(*[cases[name][0], RATE, *cases[name][1:4]])[1] for name in NAMES}
    for name, m in lib.items():
        assert (m.status, m.passes) == (STATUS[refs[name][1]["status"]], refs[name][1]["passes"]), name
    assert lib["cut"].gain_q16 < ONE and lib["cut"].limited_frames == 0
    hot = lib["hot-cut"]
    assert hot.pass_gain_q16[0] <= ONE and hot.pass_gain_q16[1] <= ONE < hot.pass_gain_q16[2]
    assert hot.limited_frames > 0 and hot.loudness < -9.0 - TOL
    assert lib["boost-2"].gain_q16 > ONE and lib["boost-3"].gain_q16 > ONE and lib["mono"].gain_q16 > ONE
    assert lib["saturated"].loudness < -8.0 - TOL
    assert lib["no-ceiling"].gain_q16 == 108477 and lib["no-ceiling"].loudness < -8.0 - TOL and lib["no-ceiling"].clipped == 0
    assert math.isnan(lib["unmeasurable"].source_lufs) and lib["unmeasurable"].limited_frames > 0
    for name, want in (("boost-2", -19.172), ("mono", -22.172), ("cut", -11.532), ("hot-cut", -8.196)):
        assert abs(lib[name].source_lufs - want) <= 2e-3, name


def test_one_track_is_mm_level_host(cases):
    from test_level import host_level
    from mastering_amd import native
    for pcm, T, C in ((cases["cut"][0][0], -15.0, q28(-1.0)), (cases["boost-2"][0][0], -12.0, q28(-1.0)),
                      (cases["boost-2"][0][0], -8.0, 0), (cases["cut"][0][3], -14.0, q28(-1.0))):
        ce1 = native.MMCeiling()
        want, m1 = host_level(pcm, RATE, T, C, 220, ce1)
        got, m, alb, tr, ce = host_album_level([pcm], RATE, T, C, 220)
        assert np.array_equal(got[0], want) and bytes(m) == bytes(m1)
        assert (bytes(ce[0]) == bytes(ce1)) if C else True
        assert bytes(alb) == bytes(tr[0])


def test_the_fates_album_is_what_its_name_says():
    """Every pass boosts behind the limiter; the inner ceiling of every pass lies under the true
    peaks of tracks 0, 2 and 3 and above that of track 1; and no decision of the rule is nearer
    than 1e-3 LU to its threshold."""
    from test_meter import ref_meter
    from mastering_amd import native
    tracks, rate, T, C, W = album_fates()
    got, m, alb, tr, ce = host_album_level(tracks, rate, T, C, W)
    assert (m.status, m.passes) == (STATUS["reached"], 3) and m.limited_frames > 0
    assert [len(t) for t in tracks] == [2 * rate, 2 * rate, native.load().mm_ceiling_span() + 3, 3 * rate // 10, 0]
    tp = [max(ref_meter(t)["true_peak_q28"]) for t in tracks[:4]]
    for k in range(m.passes):
        g = m.pass_gain_q16[k]
        inner = ((C - GUARD) << 16) // g
        assert g > ONE and tp[1] <= inner < min(tp[0], tp[2], tp[3]), k
        assert abs(abs(T - m.pass_lufs[k]) - TOL) >= 1e-3, k
        if k:
            d = [20.0 * math.log10(m.pass_gain_q16[j] / 65536.0) for j in (k - 1, k)]
            assert abs((m.pass_lufs[k] - m.pass_lufs[k - 1]) / (d[1] - d[0]) - SMIN) >= 0.01, k
    assert all(c.tp_out_q28 <= C for c in ce) and ce[4].frames == 0 and math.isnan(tr[3].integrated)


def test_host_refusals():
    from mastering_amd import engine, native
    lib = native.load()
    I16P = ctypes.POINTER(ctypes.c_int16)
    xs = [np.zeros((100, 2), np.int16), np.zeros((50, 2), np.int16)]
    ptrs = (I16P * 2)(*[x.ctypes.data_as(I16P) for x in xs])
    fr = (ctypes.c_int64 * 2)(100, 50)
    m, alb, sos, C = native.MMLevel(), native.MMR128(), engine.kweight_sos(RATE), q28(-1.0)

    def call(p=ptrs, f=fr, n=2, ch=2, rate=RATE, s=sos, clu=-1400, c=C, w=220, out=ctypes.byref(m), al=ctypes.byref(alb)):
        return lib.mm_album_level_host(p, f, n, ch, rate, s, clu, c, w, out, al, None, None)

    assert call() == 0 and m.status == STATUS["unmeasurable"] and m.frames == 150
    for bad in (dict(n=0), dict(n=257), dict(ch=3), dict(rate=1999), dict(s=None), dict(clu=-400), dict(clu=0),
                dict(c=2 ** 24 - 1), dict(w=0), dict(w=1025), dict(p=None), dict(f=None), dict(out=None), dict(al=None),
                dict(f=(ctypes.c_int64 * 2)(100, -1)), dict(f=(ctypes.c_int64 * 2)(2 ** 30, 2 ** 30), c=0),
                dict(p=(I16P * 2)(xs[0].ctypes.data_as(I16P), None))):
        assert call(**bad) == native.MM_ERR_ARG, bad


# ------------------------------------------------------------ structure and plumbing
def test_the_header_constants_match(tmp_path):
    from mastering_amd import native
    prog = tmp_path / "album.c"
    prog.write_text('#include <stdio.h>\n#include "mastering.h"\nint main(void){printf("%d %zu %zu %zu %d\\n", '
                    'MM_ALBUM_TRACKS, sizeof(mm_level), sizeof(mm_r128), sizeof(mm_ceiling), MM_ABI_VERSION);return 0;}')
    exe = tmp_path / "album"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [native.ALBUM_TRACKS, ctypes.sizeof(native.MMLevel), ctypes.sizeof(native.MMR128),
                   ctypes.sizeof(native.MMCeiling), native.ABI_VERSION]
    assert native.ALBUM_TRACKS == 256 and native.ABI_VERSION == 5


def test_python_refusals_need_no_gpu(tmp_path, monkeypatch):
    from mastering_amd import album_level_pcm, album_r128_pcm, engine, master_album, native, process_album, wavio

    def no_context(device=0):
        raise AssertionError("a refused album must not reach the device")

    monkeypatch.setattr(native, "context", no_context)
    st, mono, f32 = np.zeros((100, 2), np.int16), np.zeros(100, np.int16), np.zeros((100, 2), np.float32)
    for fn, tail in ((album_level_pcm, (RATE, -14.0)), (album_r128_pcm, (RATE,))):
        with pytest.raises(ValueError, match="1 to 256 tracks, not 0"):
            fn([], *tail)
        with pytest.raises(ValueError, match="1 to 256 tracks, not 257"):
            fn([st] * 257, *tail)
        with pytest.raises(ValueError, match="one channel count"):
            fn([st, mono], *tail)
        with pytest.raises(ValueError, match="one sample type"):
            fn([st, f32], *tail)
    with pytest.raises(ValueError, match=r"loudness target -4.0 LUFS outside \[-40, -5\]"):
        album_level_pcm([st], RATE, -4.0)
    with pytest.raises(ValueError, match="ceiling"):
        album_level_pcm([st], RATE, -14.0, ceiling_dbtp=1.0)
    # master_album: the jobs of an album
    p = {"lufs": -14.0}
    job = lambda **kw: engine.Job(kw.pop("n", 44100), kw.pop("rate", 44100), kw.pop("ch", 2), p, **kw)  # noqa: E731
    for jobs, words in (([], "1 to 256 tracks, not 0"), ([job(), job(ceiling_dbtp=-1.0)], "without ceiling_dbtp"),
                        ([job(deliver_lufs=-14.0)], "without a delivery"), ([job(output_rate=48000)], "without a delivery"),
                        ([job(), job(report=True)], "without report or r128"), ([job(r128=True)], "without report or r128"),
                        ([job(), job(rate=48000)], "one sample rate"), ([job(), job(ch=1)], "one channel count"),
                        ([job(), job(out_kind=native.MM_OUT_F32)], "one output kind")):
        with pytest.raises(ValueError, match=words):
            master_album(None, jobs, [0] * len(jobs), [0] * len(jobs), -14.0, -1.0)
    with pytest.raises(ValueError, match="outside"):
        master_album(None, [job()], [0], [0], -4.0)
    # process_album: the keys and the files
    a, b, m = str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), str(tmp_path / "m.wav")
    wavio.write_wav(a, np.zeros((44100, 2), np.int16), 44100)
    wavio.write_wav(b, np.zeros((48000, 2), np.int16), 48000)
    wavio.write_wav(m, np.zeros(44100, np.int16), 44100)
    with pytest.raises(ValueError, match="deliver_lufs"):
        process_album([a], [a + ".out"], {"lufs": -14.0})
    with pytest.raises(ValueError, match=r"delivery at another rate \(output_rate\) is not available for a batch"):
        process_album([a], [a + ".out"], {"deliver_lufs": -14.0, "output_rate": 48000})
    for key in ("report", "r128"):
        with pytest.raises(ValueError, match=f"takes no params\\['{key}'\\]"):
            process_album([a], [a + ".out"], {"deliver_lufs": -14.0, key: True})
    with pytest.raises(ValueError, match="one output path"):
        process_album([a, b], [a + ".out"], {"deliver_lufs": -14.0})
    with pytest.raises(ValueError, match="one sample rate"):
        process_album([a, b], [a + ".out", b + ".out"], {"deliver_lufs": -14.0})
    with pytest.raises(ValueError, match="the tracks of an album must have one channel count"):
        process_album([a, m], [a + ".out", m + ".out"], {"deliver_lufs": -14.0})
    # master_batch still refuses a job planned with deliver_lufs
    with pytest.raises(ValueError, match="deliver_lufs"):
        engine.master_batch(None, [job(deliver_lufs=-14.0)], [0], [0])

